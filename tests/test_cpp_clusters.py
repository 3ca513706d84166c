"""The C++ binding of cluster extraction (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::Clusters) over the C ABI: compiled
with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_clusters.py compares with the oracle."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cluster_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "cluster_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_cluster_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_clusters_match_python(tmp_path):
    from pcgol_amd import kdtree, synth
    exe = _build(tmp_path)
    pts = synth.uniform_cloud(4000, 1.0, 78)
    rng = np.random.default_rng(79)
    table = np.array([(1, 0, 0), (0.75, 0.5, 0), (0, 1, 0), (0, 0, 0), (-1, 0, 0)], np.float32)
    nrm = table[rng.integers(0, len(table), len(pts))]
    cur = rng.choice(np.array([0.0, 0.125, 0.5], np.float32), len(pts))
    calls = [(0.06, 0, 0.0, 0, 0, 0.0, 1, 0), (0.06, 0, 0.0, 0, 0, 0.0, 3, 40), (0.08, 1, 0.75, 0, 0, 0.0, 1, 0),
             (0.08, 1, 0.75, 1, 1, 0.125, 2, 0), (0.08, 0, 0.0, 0, 1, 0.125, 5000, 0)]
    lines = ["P %d" % len(pts)] + ["%r %r %r %r %r %r %r" % tuple(map(float, (*p, *n, c))) for p, n, c in zip(pts, nrm, cur)]
    lines += ["C %r %d %r %d %d %r %d %d" % c for c in calls]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert len(rows) == 4 * len(calls) and [w[0] for w in rows] == ["L", "S", "I", "M"] * len(calls)
    t = kdtree.New(pts)
    counts = []
    for k, (rad, use_n, mc, ori, use_c, xc, lo, hi) in enumerate(calls):
        labels, sizes, ids = t.Clusters(rad, Normals=nrm if use_n else None, MinCos=mc, Oriented=bool(ori),
                                        Curvature=cur if use_c else None, MaxCurvature=xc, MinSize=lo, MaxSize=hi)
        got = [np.array(w[1:], np.int64) for w in rows[4 * k:4 * k + 4]]
        assert np.array_equal(got[0], labels) and np.array_equal(got[1], sizes) and np.array_equal(got[2], ids), k
        assert np.array_equal(got[3], ids[len(ids) - sizes[-1]:] if len(sizes) else ids[:0]), k
        counts.append(len(sizes))
    assert counts[0] > counts[1] > 1 and counts[2] > 1 and counts[3] > 1 and counts[4] == 0  # the scene does what it is for
