"""The C++ binding of moving-least-squares smoothing (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::MLS) over the C ABI:
compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the
Python binding's results, which tests/test_gpu_mls.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mls_oracle as MO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mls_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "mls_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_mls_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


def _xyz(p):
    return ["%r %r %r" % tuple(map(float, r)) for r in np.asarray(p, np.float32)]


@pytest.mark.gpu
def test_cpp_mls_match_python(tmp_path):
    from pcgol_amd import kdtree
    exe = _build(tmp_path)
    base = MO.noisy_surface()[0]
    q = MO.surface_queries(base, 200, 20)
    vp = (1.0, 1.0, 50.0)
    lines = ["P %d" % len(base)] + _xyz(base)
    lines += ["M 0.15 0 2 3 %r %r %r 0" % vp]                                      # sigma <= 0: the radius
    lines += ["M 0.15 0.075 2 40 %r %r %r %d" % (*vp, len(q))] + _xyz(q)
    lines += ["M 0.15 0.15 1 3 %r %r %r %d" % (*vp, len(q))] + _xyz(q)
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.strip().split("\n")]
    assert len(rows) == len(base) + 2 * len(q)
    got_p = np.array([[float(x) for x in w[:3]] for w in rows], np.float32)
    got_n = np.array([[float(x) for x in w[3:6]] for w in rows], np.float32)
    got_kind = np.array([int(w[6]) for w in rows], np.int32)
    got_k = np.array([int(w[7]) for w in rows], np.int32)
    t = kdtree.New(base)
    a = t.MLS(0.15, Viewpoint=vp)
    b = t.MLS(0.15, Sigma=0.075, MinNeighbors=40, Viewpoint=vp, Queries=q)
    c = t.MLS(0.15, Order=1, Viewpoint=vp, Queries=q)
    want = [np.concatenate(x) for x in zip(a, b, c)]
    assert np.array_equal(got_k, want[3]) and np.array_equal(got_kind, want[2])
    assert np.array_equal(got_p.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got_n.view(np.uint32), want[1].view(np.uint32))
    assert set(got_kind.tolist()) == {0, 1, 2}
