"""The C++ binding of farthest-point sampling (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::FarthestPoints) over the C ABI:
compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_fps.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fps_mirror.cpp")
f32 = np.float32


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "fps_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_fps_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]
    sym = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    assert "pcgx_kdtree_fps" in sym  # the mirror's call reaches the ABI


@pytest.mark.gpu
def test_cpp_fps_matches_python(tmp_path):
    from pcgol_amd import kdtree, synth
    exe = _build(tmp_path)
    pts = synth.uniform_cloud(3000, 1.0, 71)
    t = kdtree.New(pts)
    blocks = [(100, -1), (100, 1234), (4000, -1)]
    lines = ["P %d" % len(pts)] + ["%r %r %r" % tuple(map(float, p)) for p in pts]
    lines += ["Q %d %d" % b for b in blocks]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert [w[0] for w in rows] == ["K", "D", "C", "O"] * len(blocks)
    for k, (count, start) in enumerate(blocks):
        ids, dsq, cover, owner = t.FarthestPoints(count, Start=start, Owner=True)
        assert len(ids) == min(count, len(pts))
        assert np.array_equal(np.array(rows[4 * k][1:], np.int64), ids)
        assert [int(w, 16) for w in rows[4 * k + 1][1:]] == dsq.view(np.uint32).tolist()
        assert int(rows[4 * k + 2][1], 16) == int(np.array([cover], f32).view(np.uint32)[0])
        assert np.array_equal(np.array(rows[4 * k + 3][1:], np.int64), owner)
