"""csrc/fps_plan.h, the one place that decides how a farthest-point call is cut up, compiled with g++ as plain C++
(tests/cpp/fps_plan_host.cpp) and walked over its input space: Len() 1, a tile +- 1, 20 000, 1M and 2^26; count 0, 1
and Len().  Every pick is one wide launch (the one-workgroup form of the late picks lost its measurement and is not in
the tree: DESIGN.md 3.28), so what the plan decides is the tiles, a pick workgroup's share of them, the number of
launches and the temporaries."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pcgol_amd", "csrc")
BUFS = ["xyz", "perm", "rec", "dist", "owner", "cand", "pos", "box", "key", "best"]
PER_POINT = dict(xyz=12, perm=4, rec=16, dist=4, owner=4, cand=1, pos=4)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fps_plan") / "libfps_plan_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fps_plan_host.cpp")])
    lib = ctypes.CDLL(so)
    rows = (ctypes.c_int32 * 2)()
    lib.fps_plan_rows(rows)
    assert list(rows) == [5 + len(BUFS), len(BUFS)]
    return lib


def facts(lib):
    out = (ctypes.c_int64 * 4)()
    lib.fps_plan_facts(out)
    return dict(tile=out[0], waves=out[1], max_workgroups=out[2], wave=out[3])


def plans(lib, lens, counts):
    lens, counts = np.ascontiguousarray(lens, np.int64), np.ascontiguousarray(counts, np.int64)
    out = np.zeros((5 + len(BUFS), len(lens)), np.int64)
    lib.fps_plan_cases(lens.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p),
                       ctypes.c_int64(len(lens)), out.ctypes.data_as(ctypes.c_void_p))
    names = ["picks", "tile", "tiles", "wg_tiles", "workgroups"] + BUFS
    return {k: out[i] for i, k in enumerate(names)}


def _lens(f):
    t = f["tile"]
    return [1, 2, t - 1, t, t + 1, 4 * t - 1, 4 * t, 4 * t + 1, 20_000, 1_000_000, t * 4 * f["max_workgroups"],
            t * 4 * f["max_workgroups"] + 1, 2 ** 26]


def test_the_plan_over_its_input_space(host):
    f = facts(host)
    assert f["tile"] % 64 == 0 and f["waves"] >= 1
    lens, counts = [], []
    for n in _lens(f):
        for c in (0, 1, 2, 64, n - 1, n, n + 1, 2 ** 31 - 1):
            if c >= 0:
                lens.append(n)
                counts.append(c)
    lens, counts = np.array(lens, np.int64), np.array(counts, np.int64)
    p = plans(host, lens, counts)
    none = counts == 0
    for k in p:
        assert np.all(p[k][none] == 0), k  # count 0: nothing is launched, nothing allocated
    some = ~none
    n, c = lens[some], counts[some]
    q = {k: v[some] for k, v in p.items()}
    assert np.array_equal(q["picks"], np.minimum(c, n))  # a launch per pick, and no more picks than points
    assert np.all(q["tile"] == f["tile"]) and np.array_equal(q["tiles"], -(-n // f["tile"]))
    assert np.all(q["wg_tiles"] % f["waves"] == 0) and np.all(q["wg_tiles"] >= f["waves"])
    assert np.array_equal(q["workgroups"], -(-q["tiles"] // q["wg_tiles"]))
    # a lane tests one tile: a wave never takes more tiles than it has lanes; the launch stays within the bound until
    # then, and grows beyond it only at that cap
    cap = f["waves"] * f["wave"]
    assert np.all(q["wg_tiles"] <= cap) and np.all(q["workgroups"] >= 1)
    assert np.all((q["workgroups"] <= f["max_workgroups"]) | (q["wg_tiles"] == cap))
    at_cap = q["workgroups"] > f["max_workgroups"]
    assert at_cap.any() and np.all(n[at_cap] > f["tile"] * cap * f["max_workgroups"])
    # a workgroup takes more tiles only where the launch would be too large otherwise
    grew = q["wg_tiles"] > f["waves"]
    assert np.all(-(-q["tiles"][grew] // (q["wg_tiles"][grew] // 2)) > f["max_workgroups"])
    assert grew.any() and (~grew).any() and np.all(grew == (-(-q["tiles"] // f["waves"]) > f["max_workgroups"]))
    for k, b in PER_POINT.items():
        assert np.array_equal(q[k], n * b), k
    assert np.array_equal(q["box"], q["tiles"] * 32) and np.array_equal(q["key"], q["tiles"] * 8)
    assert np.array_equal(q["best"], (q["picks"] + 1) * 8)


def test_temporaries_never_shrink_as_the_cloud_grows(host):
    f = facts(host)
    lens = np.unique(np.concatenate([np.arange(1, 3 * f["tile"] + 2), _lens(f), np.geomspace(1, 2 ** 26, 400).astype(np.int64)]))
    for c in (1, 64, 2 ** 26):
        p = plans(host, lens, np.full(len(lens), c, np.int64))
        for k in BUFS + ["tiles", "picks"]:
            assert np.all(np.diff(p[k]) >= 0), (c, k)


def test_the_library_reports_the_same_plan(host):
    """pcgx_fps_plan, what the GPU tests read their sizes from, is this header's plan (needs the built library)"""
    from pcgol_amd import _lib as L
    f = facts(host)
    lens = np.array(_lens(f), np.int64)
    p = plans(host, lens, np.full(len(lens), 10, np.int64))
    for i, n in enumerate(lens):
        out = np.zeros(4, np.int64)
        L.check(L.lib().pcgx_fps_plan(int(n), 10, L.ptr(out)))
        assert out.tolist() == [p["tile"][i], p["tiles"][i], p["wg_tiles"][i], p["workgroups"][i]], n
