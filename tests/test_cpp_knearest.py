"""The C++ bindings of k nearest neighbours and statistical outlier removal (pcgol_amd/host/pcgx.hpp,
pcgx::KDTree::KNearestBatch, pcgx::StatisticalOutlierRemoval) over the C ABI: compiled with g++ everywhere (CPU
check: it builds and links against libpcgx.so), run on the GPU box against the Python binding's results, which
tests/test_gpu_knearest.py and tests/test_gpu_sor.py compare with the oracles."""
import os
import subprocess

import numpy as np
import pytest

from pcgol_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "knearest_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "knearest_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_knearest_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


def _xyz(p):
    return ["%r %r %r" % tuple(map(float, r)) for r in np.asarray(p, np.float32)]


@pytest.mark.gpu
def test_cpp_knearest_and_sor_match_python(tmp_path):
    from pcgol_amd import kdtree, outlier
    exe = _build(tmp_path)
    base = synth.uniform_cloud(3000, 2.0, 71)
    base[:20] = base[20:40]  # twins: ties by id
    q = synth.uniform_cloud(200, 2.0, 72)
    lines = ["P %d" % len(base)] + _xyz(base)
    lines += ["K 8 0.3 0", "K 16 0.2 %d" % len(q)] + _xyz(q)
    lines += ["S 8 1.5 0", "S 8 1.5 1"]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = r.stdout.strip().split("\n")
    t = kdtree.New(base)
    at = 0
    for k, rr, qq in ((8, 0.3, None), (16, 0.2, q)):
        ids, dsq, counts = t.KNearestBatch(qq, k, rr)
        for j in range(len(counts)):
            w = rows[at].split()
            at += 1
            assert int(w[0]) == counts[j]
            assert [int(x) for x in w[1::2]] == ids[j, :counts[j]].tolist()
            assert np.array_equal(np.float32([float(x) for x in w[2::2]]), dsq[j, :counts[j]])
    for neg in (False, True):
        f = outlier.New(8, 1.5, outlier.WithNegative(neg))
        out = f.Filter(base)
        w = rows[at].split()
        at += 1
        assert int(w[0]) == out.Points
        assert tuple(float(x) for x in w[1:]) == f.Stats
        got = np.float32([[float(x) for x in rows[at + i].split()] for i in range(out.Points)])
        at += out.Points
        assert np.array_equal(got.reshape(-1, 3), out.Vec3())
    assert at == len(rows)
