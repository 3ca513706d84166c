"""The C++ binding of NDT registration (pcgol_amd/host/pcgx.hpp, pcgx::NDTMap / pcgx::NDT) over the C ABI: compiled
with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_ndt.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ndt_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "ndt_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_ndt_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


def _xyz(p):
    return ["%r %r %r" % tuple(map(float, r)) for r in np.asarray(p, np.float32)]


@pytest.mark.gpu
def test_cpp_ndt_match_python(tmp_path):
    from pcgol_amd import ndt, segmentation
    from test_ndt_oracle import prototype
    exe = _build(tmp_path)
    sc = prototype()
    g = sc["grid"]
    lines = ["G %r %d %d %d %r %r %r" % (float(g.resolution), *map(int, g.size), *map(float, g.origin))]
    lines += ["B %d" % len(sc["base"])] + _xyz(sc["base"]) + ["T %d" % len(sc["target"])] + _xyz(sc["target"]) + ["F 7 5"]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.strip().split("\n")]
    vg = segmentation.StorageVoxelGrid(float(g.resolution), g.size, g.origin)
    vg.AddAll(sc["base"])
    m = ndt.NDTMap(vg, sc["base"])
    cells = m.Cells()
    assert [int(x) for x in rows[0][1:]] == list(m.Counts())
    v = np.array([[int(x) for x in w[1:]] for w in rows if w[0] == "V"], np.int64)
    assert np.array_equal(v[:, 0], cells["addr"]) and np.array_equal(v[:, 1], cells["count"])
    assert np.array_equal(v[:, 2], cells["valid"])
    s = np.array([float(x) for x in [w for w in rows if w[0] == "S"][0][1:]])
    assert np.array_equal(s, m.Evaluate(sc["target"]))
    p = [w for w in rows if w[0] == "P"][0]
    trans, stat = ndt.NDT(m, Threshold=np.full(6, -1, np.float32), MaxIteration=5).Fit(sc["target"])
    assert np.array_equal(np.array([float(x) for x in p[1:17]], np.float32).view(np.uint32), trans.view(np.uint32))
    assert int(p[17]) == stat.NumIteration == 5
