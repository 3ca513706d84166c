"""The C++ binding of the group footprints (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::GroupHulls) over the C ABI: compiled
with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_group_hulls.py compares with the oracle."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "group_hulls_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "group_hulls_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_group_hulls_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_group_hulls_match_python(tmp_path):
    from pcgol_amd import kdtree, synth
    exe = _build(tmp_path)
    pts = synth.uniform_cloud(4000, 1.0, 78)
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(["P %d" % len(pts)] + ["%r %r %r" % tuple(map(float, p)) for p in pts] + ["C 0.06"]) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert [w[0] for w in rows] == ["H", "I", "S", "R"]
    t = kdtree.New(pts)
    _, sizes, ids = t.Clusters(0.06)
    want = t.GroupHulls(ids, sizes)
    assert len(sizes) > 100 and want.hull_sizes.max() > 3
    assert np.array_equal(np.array(rows[0][1:], np.int64), want.hull_sizes)
    assert np.array_equal(np.array(rows[1][1:], np.int64), want.hull_ids)
    for w, a in zip(rows[2:], (want.area, want.rect)):
        got = np.array([int(x, 16) for x in w[1:]], np.uint64)
        assert np.array_equal(got, a.ravel().view(np.uint64)), w[0]
