"""The C++ binding of the FPFH descriptors (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::FPFH) over the C ABI: compiled with
g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python binding's
results, which tests/test_gpu_fpfh.py compares with the oracle."""
import os
import subprocess

import numpy as np
import pytest

from pcgol_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fpfh_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "fpfh_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_fpfh_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_fpfh_matches_python(tmp_path):
    from pcgol_amd import kdtree
    exe = _build(tmp_path)
    base, normals = synth.surface_cloud(3000, 2.0, 21)
    lines = ["P %d" % len(base)]
    lines += ["%r %r %r %r %r %r" % tuple(map(float, np.concatenate([p, n]))) for p, n in zip(base, normals)]
    lines += ["F 0.15"]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.strip().split("\n")]
    assert len(rows) == len(base) and all(len(w) == 67 for w in rows)
    got_f = np.array([[float(x) for x in w[:33]] for w in rows], np.float32)
    got_c = np.array([[int(x) for x in w[33:66]] for w in rows], np.int32)
    got_m = np.array([int(w[66]) for w in rows], np.int32)
    f, c, m = kdtree.New(base).FPFH(0.15, normals)
    assert np.array_equal(got_f.view(np.uint32), f.view(np.uint32))
    assert np.array_equal(got_c, c.reshape(-1, 33)) and np.array_equal(got_m, m)
    assert m.min() > 0 and np.allclose(f.reshape(-1, 3, 11).sum(axis=2), 200.0, rtol=1e-5)
