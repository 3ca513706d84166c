"""The C++ binding of density clustering and radius outlier removal (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::DBSCAN,
pcgx::RadiusOutlierRemoval) over the C ABI: compiled with g++ everywhere (CPU check: it builds and links against
libpcgx.so), run on the GPU box against the Python binding's results, which tests/test_gpu_dbscan.py and
tests/test_gpu_ror.py compare with the oracle."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dbscan_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "dbscan_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_dbscan_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_dbscan_matches_python(tmp_path):
    from pcgol_amd import kdtree, outlier, synth
    exe = _build(tmp_path)
    pts = synth.uniform_cloud(4000, 1.0, 78)
    calls = [(0.06, 1, 1, 0), (0.06, 4, 1, 0), (0.06, 4, 3, 40), (0.06, 6, 1, 0), (0.06, 4, 5000, 0)]
    rors = [(0.06, 1, 0), (0.06, 4, 0), (0.06, 4, 1)]
    lines = ["P %d" % len(pts)] + ["%r %r %r" % tuple(map(float, p)) for p in pts]
    lines += ["D %r %d %d %d" % c for c in calls] + ["R %r %d %d" % c for c in rors]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert len(rows) == 5 * len(calls) + len(rors)
    assert [w[0] for w in rows] == ["L", "S", "I", "K", "M"] * len(calls) + ["F"] * len(rors)
    t = kdtree.New(pts)
    counts, borders = [], []
    for k, (rad, min_pts, lo, hi) in enumerate(calls):
        labels, sizes, ids, kind = t.DBSCAN(rad, min_pts, MinSize=lo, MaxSize=hi)
        got = [np.array(w[1:], np.int64) for w in rows[5 * k:5 * k + 5]]
        assert np.array_equal(got[0], labels) and np.array_equal(got[1], sizes) and np.array_equal(got[2], ids), k
        assert np.array_equal(got[3], kind), k
        assert np.array_equal(got[4], ids[len(ids) - sizes[-1]:] if len(sizes) else ids[:0]), k
        counts.append(len(sizes))
        borders.append(int(np.sum(kind == 1)))
    assert counts[1] > counts[2] > 1 and counts[3] > 1 and counts[4] == 0  # the scene does what it is for
    assert borders[0] == 0 and borders[1] > 100 and borders[1] == borders[2] == borders[4]
    for k, (rad, mn, neg) in enumerate(rors):
        want = outlier.RadiusOutlierRemoval(rad, mn, outlier.WithNegative(bool(neg))).Filter(pts).Data
        got = np.array(rows[5 * len(calls) + k][1:], np.int64).astype(np.uint32)
        assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint32)), k
        if mn == 1:
            assert len(got) == 3 * len(pts)
