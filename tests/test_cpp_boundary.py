"""The C++ binding of boundary detection (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::Boundary) over the C ABI: compiled
with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python binding's
results, which tests/test_gpu_boundary.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_scenes as BS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "boundary_mirror.cpp")
TAGS = ["I", "G", "M", "C"]


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "boundary_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_boundary_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]
    sym = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    assert "pcgx_kdtree_boundary" in sym  # the mirror's call reaches the ABI


@pytest.mark.gpu
def test_cpp_boundary_matches_python(tmp_path):
    from pcgol_amd import kdtree
    exe = _build(tmp_path)
    pts = BS.plate()[:3000]
    t = kdtree.New(pts)
    nrm = t.Normals(BS.PLATE_RADIUS, Viewpoint=(40.0, 40.0, 500.0))[0]
    nrm[::100] = 0.0
    calls = [(3.0, 16, 1), (2.0, 8, 12), (3.0, 64, 1)]
    lines = ["P %d" % len(pts)] + ["%r %r %r %r %r %r" % tuple(map(float, np.concatenate([p, m]))) for p, m in zip(pts, nrm)]
    lines += ["B %r %d %d" % c for c in calls]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert [w[0] for w in rows] == TAGS * len(calls)
    for k, (radius, gap, mn) in enumerate(calls):
        want = t.Boundary(radius, nrm, gap, mn)
        got = [np.array(w[1:], np.uint64 if w[0] == "M" else np.int64) for w in rows[4 * k:4 * k + 4]]
        for g, w in zip(got, want):
            assert np.array_equal(g, w.astype(g.dtype)), (k, radius, gap, mn)
    assert len(t.Boundary(3.0, nrm, 16, 1)[0]) > 50
