"""The C++ binding of keypoint detection (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::LocalMaxima and ::ISSKeypoints) over
the C ABI: compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against
the Python binding's results, which tests/test_gpu_keypoints.py compares with the oracle."""
import os
import subprocess

import numpy as np
import pytest

from pcgol_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "keypoints_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "keypoints_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_keypoints_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_keypoints_match_python(tmp_path):
    from pcgol_amd import kdtree
    exe = _build(tmp_path)
    base = synth.surface_cloud(3000, 2.0, 21)[0]
    score = np.random.default_rng(3).integers(0, 8, len(base)).astype(np.float32)
    lines = ["P %d" % len(base)]
    lines += ["%r %r %r %r" % tuple(map(float, np.append(p, s))) for p, s in zip(base, score)]
    lines += ["M 0.1", "I 0.15 0.1"]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.strip().split("\n")]
    assert len(rows) == 2 + len(base) and rows[0][0] == "M" and rows[1][0] == "I"
    t = kdtree.New(base)
    assert np.array_equal(np.array(rows[0][1:], np.int64), t.LocalMaxima(0.1, score))
    ids, eig, sal = t.ISSKeypoints(0.15, 0.1)
    assert np.array_equal(np.array(rows[1][1:], np.int64), ids) and len(ids) > 10
    got = np.array([[float(x) for x in w] for w in rows[2:]], np.float32)
    assert np.array_equal(got[:, :3].view(np.uint32), eig.view(np.uint32))
    assert np.array_equal(got[:, 3].view(np.uint32), sal.view(np.uint32))
