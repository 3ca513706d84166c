"""The C++ binding of normal estimation (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::Normals) over the C ABI: compiled
with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_normals.py compares with the oracle."""
import os
import subprocess

import numpy as np
import pytest

from pcgol_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "normals_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "normals_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_normals_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


def _xyz(p):
    return ["%r %r %r" % tuple(map(float, r)) for r in np.asarray(p, np.float32)]


@pytest.mark.gpu
def test_cpp_normals_match_python(tmp_path):
    from pcgol_amd import kdtree
    exe = _build(tmp_path)
    base = synth.surface_cloud(3000, 2.0, 21)[0]
    q = synth.uniform_cloud(200, 2.0, 22)
    q[:, 2] = base[:200, 2]
    vp = (1.0, 1.0, 50.0)
    lines = ["P %d" % len(base)] + _xyz(base)
    lines += ["N 0.15 %r %r %r 3 0" % vp]
    lines += ["N 0.15 %r %r %r 5 %d" % (*vp, len(q))] + _xyz(q)
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.strip().split("\n")]
    assert len(rows) == len(base) + len(q)
    got_n = np.array([[float(x) for x in w[:3]] for w in rows], np.float32)
    got_c = np.array([float(w[3]) for w in rows], np.float32)
    got_k = np.array([int(w[4]) for w in rows], np.int32)
    t = kdtree.New(base)
    n1, c1, k1 = t.Normals(0.15, Viewpoint=vp)
    n2, c2, k2 = t.Normals(0.15, Viewpoint=vp, MinNeighbors=5, Queries=q)
    assert np.array_equal(got_k, np.concatenate([k1, k2]))
    assert np.array_equal(got_n, np.concatenate([n1, n2]))
    assert np.array_equal(np.isnan(got_c), np.isnan(np.concatenate([c1, c2])))
    want_c = np.concatenate([c1, c2])
    assert np.array_equal(got_c[~np.isnan(got_c)], want_c[~np.isnan(want_c)])
    assert (~np.isnan(want_c)).sum() > len(base) // 2
