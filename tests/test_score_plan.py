"""What pcgx_kdtree_score_poses_dev allocates and launches (csrc/pose_score_plan.h): the header is compiled for the host
with g++ (tests/cpp/score_plan_host.cpp; it needs neither HIP nor the library) and its plan is walked over the sizes at
which it takes another turn: n across a tile, K across a chunk, every kind of handle, a forced chunk.  Every temporary
must cover its worst case -- every pair of a round left to the walk -- and the rounds must cover [0, K) exactly once."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pcgol_amd", "csrc")
BUFS = ("counts", "sums", "box", "keys0", "keys1", "vals0", "vals1", "sort_ws", "src4", "partials", "masks", "walk_q",
        "walk_list", "walk_ids", "walk_dsq", "walk_count", "plain_q", "plain_ids", "plain_dsq")
IN = ("n", "K", "grid", "deletions", "empty", "forced", "sort_ws", "have_counts", "have_sums")
NOTHING, EMPTY, FUSED, PLAIN = range(4)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("score_plan") / "libscore_plan_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "score_plan_host.cpp")])
    lib = ctypes.CDLL(so)
    rows = (ctypes.c_int32 * 3)()
    lib.score_plan_rows(rows)
    assert list(rows) == [len(IN), 5 + len(BUFS), len(BUFS)]
    return lib


def facts(lib):
    out = (ctypes.c_int64 * 5)()
    lib.score_plan_facts(out)
    return dict(zip(("tile", "wave", "budget", "max_chunk", "partial_rec"), out))


def plan(lib, cases):
    rows = np.ascontiguousarray(np.array([[int(c[k]) for c in cases] for k in IN], np.int64))
    n = rows.shape[1]
    out = np.empty((5 + len(BUFS), n), np.int64)
    lib.score_plan_cases(rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(n), out.ctypes.data_as(ctypes.c_void_p))
    names = ("path", "tiles", "chunk", "nchunks", "order") + BUFS
    return [dict(zip(names, (int(v) for v in out[:, i]))) for i in range(n)]


HANDLES = {"grid": dict(grid=1, deletions=0, empty=0), "walk only": dict(grid=0, deletions=0, empty=0),
           "deletions": dict(grid=1, deletions=1, empty=0), "deletions, walk only": dict(grid=0, deletions=1, empty=0),
           "every point deleted": dict(grid=1, deletions=1, empty=1)}


def cases_for(f):
    tile = f["tile"]
    out = []
    for n in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 5, 3000, 1 << 20, (1 << 22) + 1, 2 ** 31 - 1):
        chunk = max(1, f["budget"] // n) if n else 1
        for K in sorted({0, 1, 2, 6, chunk, chunk + 1, 16, 65535, 65536}):
            if n * K > 2 ** 45:
                continue
            for hname, h in HANDLES.items():
                for forced in (0, 1, 4, 100000, 2 ** 40):
                    for have in (0, 1):
                        out.append(dict(n=n, K=K, forced=forced, sort_ws=4096 + n // 8, have_counts=have, have_sums=have,
                                        handle=hname, **h))
    return out


def test_the_facts(host):
    f = facts(host)
    assert f == dict(tile=256, wave=64, budget=1 << 22, max_chunk=65535, partial_rec=16)


def test_plan_covers_its_worst_case(host):
    f = facts(host)
    cases = cases_for(f)
    plans = plan(host, cases)
    seen = set()
    for c, p in zip(cases, plans):
        n, K, tile = c["n"], c["K"], f["tile"]
        why = (c, p)
        seen.add(p["path"])
        # the outputs the caller did not give
        assert p["counts"] == (0 if c["have_counts"] else 4 * max(K, 1)), why
        assert p["sums"] == (0 if c["have_sums"] else 8 * max(K, 1)), why
        if n == 0 or K == 0:
            assert p["path"] == NOTHING and p["nchunks"] == 0, why
        elif c["empty"]:
            assert p["path"] == EMPTY and p["nchunks"] == 0, why
        elif c["deletions"] or not c["grid"]:
            assert p["path"] == PLAIN, why
        else:
            assert p["path"] == FUSED, why
        if p["path"] in (NOTHING, EMPTY):
            assert all(p[b] == 0 for b in BUFS[2:]), why
            continue
        tiles = -(-n // tile)
        assert p["tiles"] == tiles and tiles * tile >= n > (tiles - 1) * tile, why
        # the rounds cover [0, K) exactly once: round r takes [r chunk, min(K, (r + 1) chunk))
        chunk, rounds = p["chunk"], p["nchunks"]
        assert 1 <= chunk <= max(K, 1) and (rounds - 1) * chunk < K <= rounds * chunk, why
        assert p["partials"] >= chunk * tiles * f["partial_rec"], why
        if p["path"] == PLAIN:
            assert chunk == 1 and rounds == K and not p["order"], why
            assert p["plain_q"] >= 12 * n and p["plain_ids"] >= 4 * n and p["plain_dsq"] >= 4 * n, why
            assert all(p[b] == 0 for b in BUFS[2:9] + BUFS[10:16]), why
            continue
        # fused: a slot index is an int32, the grid's y extent holds a chunk, the forced chunk is taken where it may be
        assert chunk * n <= 2 ** 31 - 1 and chunk <= f["max_chunk"], why
        want = c["forced"] if c["forced"] > 0 else max(1, f["budget"] // n)
        assert chunk == max(1, min(want, K, f["max_chunk"], (2 ** 31 - 1) // n)), why
        if c["forced"] <= 0 and chunk > 1:
            assert chunk * n <= f["budget"], why
        # the worst case: every pair of a round goes to the walk
        assert p["walk_q"] >= 12 * chunk * n and p["walk_list"] >= 4 * chunk * n, why
        assert p["walk_ids"] >= 4 * chunk * n and p["walk_dsq"] >= 4 * chunk * n, why
        assert p["masks"] >= 8 * chunk * tiles * (tile // f["wave"]) and p["walk_count"] >= 4 * rounds, why
        assert p["src4"] >= 16 * n, why
        assert p["order"] == (1 if n > 1 else 0), why
        if p["order"]:
            assert all(p[b] >= 4 * n for b in ("keys0", "keys1", "vals0", "vals1")), why
            assert p["sort_ws"] >= c["sort_ws"] and p["box"] >= 24, why
        assert all(p[b] == 0 for b in ("plain_q", "plain_ids", "plain_dsq")), why
    assert seen == {NOTHING, EMPTY, FUSED, PLAIN}


def test_default_bound_of_the_contract(host):
    """include/pcgx.h: the per-round temporaries of the default chunk stay within max(96 MiB, 24 n bytes) plus 48 bytes
    per workgroup"""
    f = facts(host)
    cases = [dict(n=n, K=K, forced=0, sort_ws=0, have_counts=1, have_sums=1, grid=1, deletions=0, empty=0)
             for n in (1, 255, 3000, 1 << 20, (1 << 22) - 1, 1 << 22, 1 << 24) for K in (1, 16, 4096)]
    for c, p in zip(cases, plan(host, cases)):
        per_pair = p["walk_q"] + p["walk_list"] + p["walk_ids"] + p["walk_dsq"]
        assert per_pair <= max(96 << 20, 24 * c["n"]), (c, p)
        assert p["partials"] + p["masks"] == 48 * p["chunk"] * p["tiles"], (c, p)
