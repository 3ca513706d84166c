"""The C++ binding of consistent normal orientation (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::OrientNormals) over the C
ABI: compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the
Python binding's results, which tests/test_gpu_orient.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "orient_mirror.cpp")
f32 = np.float32


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "orient_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_orient_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]
    sym = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    assert "pcgx_kdtree_orient_normals" in sym  # the mirror's call reaches the ABI


@pytest.mark.gpu
def test_cpp_orient_matches_python(tmp_path):
    from pcgol_amd import kdtree, synth
    exe = _build(tmp_path)
    pts = synth.uniform_cloud(2500, 1.0, 71)
    rng = np.random.default_rng(72)
    v = rng.normal(size=(len(pts), 3))
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    nrm[::97] = 0
    t = kdtree.New(pts)
    blocks = [(0.1, 0, (0.0, 0.0, 0.0)), (0.1, 1, (0.0, 0.5, 1.0)), (0.12, 2, (0.5, 0.5, 3.0))]
    lines = ["P %d" % len(pts)] + ["%r %r %r %r %r %r" % tuple(map(float, np.concatenate([p, m]))) for p, m in zip(pts, nrm)]
    lines += ["Q %r %d %r %r %r" % ((r, mode) + ref) for r, mode, ref in blocks]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert [w[0] for w in rows] == ["F", "C", "N", "S"] * len(blocks)
    for k, (rad, mode, ref) in enumerate(blocks):
        kw = dict(Direction=ref) if mode == 1 else dict(Viewpoint=ref) if mode == 2 else {}
        out, flipped, ncomp, comp = t.OrientNormals(rad, nrm, Component=True, **kw)
        assert np.array_equal(np.array(rows[4 * k][1:], np.uint8), flipped) and 500 < flipped.sum() < 2000
        assert np.array_equal(np.array(rows[4 * k + 1][1:], np.int64), comp) and (comp[::97] == -1).all()
        assert int(rows[4 * k + 2][1]) == ncomp
        assert np.array_equal(np.array(rows[4 * k + 3][1:], np.int64).reshape(-1, 3), np.signbit(out).astype(np.int64))
