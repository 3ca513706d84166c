"""The C++ binding of the Generalized ICP extension (pcgol_amd/host/pcgx.hpp, pcgx::GeneralizedICP) over the C ABI:
compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the
Python binding's Fit, which tests/test_gpu_icp_gicp.py compares with the oracle."""
import os
import subprocess

import numpy as np
import pytest

from pcgol_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gicp_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "gicp_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_gicp_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


def _xyz(p):
    return ["%r %r %r" % tuple(map(float, r)) for r in np.asarray(p, np.float32)]


@pytest.mark.gpu
def test_cpp_gicp_matches_python(tmp_path):
    from pcgol_amd import icp, kdtree
    exe = _build(tmp_path)
    c = synth.c4_plane(5000, base_seed=81, perm_seed=82)
    k, eps, iters = 16, 1e-3, 6
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(["B %d" % len(c["base"])] + _xyz(c["base"]) + ["T %d" % len(c["target"])] + _xyz(c["target"])
                             + ["F %d %r %r %d" % (k, eps, c["max_dist"], iters)]) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [np.array([float(x) for x in w.split()]) for w in r.stdout.strip().split("\n")]
    assert len(rows) == 2
    t = kdtree.New(c["base"])
    bc = t.Covariances(k, Epsilon=eps)[0]
    tc = kdtree.New(c["target"]).Covariances(k, Epsilon=eps)[0]
    reg = icp.GeneralizedICP(icp.GeneralizedICPEvaluator(icp.NearestPointCorresponder(c["max_dist"]), bc, tc, 6),
                             icp.GaussNewtonUpdaterFactory(Threshold=np.full(6, -1, np.float32), MaxIteration=iters))
    trans, stat = reg.Fit(t, c["target"])
    for row in rows:  # (Fit, FitKNN: the same bits)
        assert int(row[0]) == stat.NumIteration == iters and int(row[1]) == stat.Evaluated.NumPairs
        assert np.float32(row[2]) == stat.Evaluated.Value
        assert np.array_equal(np.float32(row[3:19]), trans)
        assert np.array_equal(np.float32(row[19:55]), stat.Evaluated.Hessian)
