"""The C++ binding of k-NN covariances (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::Covariances) over the C ABI: compiled
with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_covariances.py compares with the oracle."""
import os
import subprocess

import numpy as np
import pytest

from pcgol_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "covariances_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "covariances_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_covariances_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


def _xyz(p):
    return ["%r %r %r" % tuple(map(float, r)) for r in np.asarray(p, np.float32)]


@pytest.mark.gpu
def test_cpp_covariances_match_python(tmp_path):
    from pcgol_amd import _lib as L
    from pcgol_amd import kdtree
    exe = _build(tmp_path)
    base = synth.surface_cloud(3000, 2.0, 71)[0]
    q = synth.uniform_cloud(200, 2.0, 72)
    vp = (1.0, 1.0, 50.0)
    cases = [(20, 1e30, L.PCGX_COV_PLANE, 1e-3, None), (8, 0.2, L.PCGX_COV_RAW, 1e-3, q),
             (16, 1e30, L.PCGX_COV_PLANE, 0.5, q)]  # (1e30: max_range^2 is +inf)
    lines = ["P %d" % len(base)] + _xyz(base)
    for k, r, mode, eps, qq in cases:
        lines += ["C %d %r %d %r %r %r %r %d" % (k, r, mode, eps, *vp, 0 if qq is None else len(qq))]
        lines += [] if qq is None else _xyz(qq)
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.strip().split("\n")]
    t = kdtree.New(base)
    at = 0
    for k, rr, mode, eps, qq in cases:
        cov, normals, counts = t.Covariances(k, rr, Mode=mode, Epsilon=eps, Queries=qq, Viewpoint=vp)
        got = rows[at:at + len(counts)]
        at += len(counts)
        assert np.array_equal(np.int32([int(w[0]) for w in got]), counts)
        assert np.array_equal(np.float32([[float(x) for x in w[1:7]] for w in got]), cov)
        assert np.array_equal(np.float32([[float(x) for x in w[7:10]] for w in got]), normals)
    assert at == len(rows)
