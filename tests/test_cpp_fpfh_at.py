"""The C++ binding of FPFH at chosen points (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::FPFHAt) over the C ABI: compiled
with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_fpfh_at.py compares with the oracle and with the full call."""
import os
import subprocess

import numpy as np
import pytest

from pcgol_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fpfh_at_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "fpfh_at_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_fpfh_at_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_fpfh_at_matches_python(tmp_path):
    from pcgol_amd import kdtree
    exe = _build(tmp_path)
    base, normals = synth.surface_cloud(3000, 2.0, 21)
    ids = np.random.default_rng(3).choice(len(base), 70, replace=False).astype(np.int64)
    ids[5] = ids[0]  # a repeat
    lines = ["P %d" % len(base)]
    lines += ["%r %r %r %r %r %r" % tuple(map(float, np.concatenate([p, n]))) for p, n in zip(base, normals)]
    lines += ["A 0.15 %d" % len(ids), " ".join(str(int(i)) for i in ids)]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.strip().split("\n")]
    assert len(rows) == len(ids) + 1 and all(len(w) == 70 for w in rows[:-1]) and rows[-1][0] == "n_spfh"
    got_f = np.array([[float(x) for x in w[:33]] for w in rows[:-1]], np.float32)
    got_x = np.array([[float(x) for x in w[33:36]] for w in rows[:-1]], np.float32)
    got_c = np.array([[int(x) for x in w[36:69]] for w in rows[:-1]], np.int32)
    got_m = np.array([int(w[69]) for w in rows[:-1]], np.int32)
    f, x, c, m, n_spfh = kdtree.New(base).FPFHAt(0.15, normals, ids)
    assert np.array_equal(got_f.view(np.uint32), f.view(np.uint32))
    assert np.array_equal(got_x.view(np.uint32), x.view(np.uint32)) and np.array_equal(x, base[ids])
    assert np.array_equal(got_c, c.reshape(-1, 33)) and np.array_equal(got_m, m)
    assert int(rows[-1][1]) == n_spfh and len(set(ids.tolist())) <= n_spfh < len(base)
    assert m.min() > 0 and np.allclose(f.reshape(-1, 3, 11).sum(axis=2), 200.0, rtol=1e-5)
