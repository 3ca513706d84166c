"""The NumPy restatement of farthest-point sampling (tests/fps_oracle.py) against a pure-Python double loop, its own
properties (the prefix property, dist_sq non-increasing, cover_sq the final largest d, owners the argmin over (DistSq,
pick position)), and a NumPy simulation of what csrc/fps.hip does -- the points in some order, tiles with their box and
largest d, a pick skipping every tile whose box is at least that far away -- which gives the plain oracle's d, owners
and picks bit for bit in Morton order and in row-major cell order.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_oracle as FO  # noqa: E402

f32, u32 = np.float32, np.uint32
inf = np.inf


def _python_fps(P, count, start, deleted):
    """the contract, one float32 operation at a time"""
    n = len(P)
    ok = [all(np.isfinite(P[i])) and not (deleted is not None and deleted[i]) for i in range(n)]
    d = [f32(inf)] * n
    owner = [-1] * n
    picked = [False] * n
    ids, dsq = [], []
    cur = start if start >= 0 else next((i for i in range(n) if ok[i]), -1)
    cur_d = f32(inf)
    while cur >= 0 and len(ids) < count:
        ids.append(cur)
        dsq.append(cur_d)
        picked[cur] = True
        for i in range(n):
            if not ok[i]:
                continue
            dx, dy, dz = f32(P[i][0] - P[cur][0]), f32(P[i][1] - P[cur][1]), f32(P[i][2] - P[cur][2])
            nd = f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz))
            if nd < d[i]:
                d[i], owner[i] = nd, cur
        cur, cur_d = -1, f32(-1)
        for i in range(n):
            if ok[i] and not picked[i] and (cur < 0 or d[i] > cur_d):
                cur, cur_d = i, d[i]
    return ids, dsq, (cur_d if ids and cur >= 0 else f32(-1)), owner


def _scenes():
    rng = np.random.default_rng(3)
    uni = rng.random((60, 3), dtype=f32)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    lattice = (g[rng.permutation(len(g))] * f32(0.25)).astype(f32)
    heaps = np.concatenate([np.tile(f32([0.1, 0.2, 0.3]), (20, 1)), np.tile(f32([0.9, 0.2, 0.3]), (15, 1)), rng.random((10, 3), dtype=f32)])
    heaps = heaps[rng.permutation(len(heaps))]
    holes = uni.copy()
    holes[::7, 1] = np.nan
    holes[3] = inf
    return dict(uniform=uni, lattice=lattice, coincident=heaps, holes=holes)


@pytest.mark.parametrize("scene", ["uniform", "lattice", "coincident", "holes"])
def test_the_oracle_is_the_double_loop(scene):
    with np.errstate(all="ignore"):
        P = _scenes()[scene]
        n = len(P)
        deleted = np.zeros(n, bool)
        deleted[[1, 8]] = True
        for count, start, dele in ((n + 3, -1, None), (7, 5, None), (n, -1, deleted), (0, -1, None)):
            ids, dsq, cover, owner = _python_fps(P, count, start, dele)
            got = FO.fps(P, count, start, dele)
            m = got["n_ids"]
            assert m == len(ids) and got["ids"][:m].tolist() == ids and np.all(got["ids"][m:] == -1), (scene, count)
            assert np.array_equal(FO.bits(got["dist_sq"][:m]), FO.bits(dsq)) and np.all(got["dist_sq"][m:] == -1.0)
            assert FO.bits(got["cover_sq"])[0] == FO.bits(cover)[0]
            assert (got["owner"].tolist() == owner) if count > 0 else np.all(got["owner"] == -1)


def test_properties():
    P = np.random.default_rng(5).random((3000, 3), dtype=f32)
    P[100:140] = P[7]  # a heap
    big = FO.fps(P, 400)
    for k in (1, 2, 50, 399):
        small = FO.fps(P, k)
        assert np.array_equal(small["ids"], big["ids"][:k]) and np.array_equal(FO.bits(small["dist_sq"]), FO.bits(big["dist_sq"][:k]))
        assert FO.bits(small["cover_sq"])[0] == FO.bits(big["dist_sq"][k])[0]  # read off the larger call
    d = big["dist_sq"]
    assert np.isinf(d[0]) and np.all(np.diff(d[1:]) <= 0) and len(np.unique(big["ids"])) == 400
    # the final largest d among the unpicked is cover_sq, and every point lies within it of a pick
    assert big["cover_sq"] == big["d"][~big["picked"]].max() and np.all(big["d"] <= big["cover_sq"])
    # owners: the argmin over (DistSq, pick position), by brute force
    picks = big["ids"]
    D = np.stack([FO.dist_sq(P, P[s]) for s in picks], axis=1)
    assert np.array_equal(big["owner"], picks[np.argmin(D, axis=1)])  # (the first minimum: the earlier pick)
    assert np.array_equal(big["d"], D.min(axis=1))
    heap = np.concatenate([[7], np.arange(100, 140)])
    assert len(np.unique(big["owner"][heap])) == 1  # coincident points share their owner
    everything = FO.fps(P, len(P) + 5)
    assert everything["n_ids"] == len(P) and everything["cover_sq"] == -1.0 and np.all(everything["dist_sq"][-5:] == -1.0)
    tail = everything["ids"][everything["dist_sq"] == 0]
    assert len(tail) == 40 and np.all(np.diff(tail) > 0)  # coincident points come last, in id order


# ------------------------------------------------------------------------------------------------ the pruned form

def _morton(P, bits=5):
    lo, hi = P.min(axis=0), P.max(axis=0)
    c = np.clip(((P - lo) * (f32(1 << bits) / (hi - lo))).astype(np.int64), 0, (1 << bits) - 1)
    key = np.zeros(len(P), np.int64)
    for b in range(bits):
        for k in range(3):
            key |= ((c[:, k] >> b) & 1) << (3 * b + k)
    return np.argsort(key, kind="stable")


def _row_major(P, cells=24):
    lo, hi = P.min(axis=0), P.max(axis=0)
    c = np.clip(((P - lo) * (f32(cells) / (hi - lo))).astype(np.int64), 0, cells - 1)
    return np.argsort((c[:, 2] * cells + c[:, 1]) * cells + c[:, 0], kind="stable")


def _pruned(P, count, order, tile=64):
    """fps.hip's scheme in NumPy: -> (ids, dist_sq bits, owner by id, d by id, touched tiles per pick)"""
    n = len(P)
    Q = P[order]
    tiles = -(-n // tile)
    pad = tiles * tile - n
    idx = np.concatenate([np.arange(n), np.full(pad, -1)]).reshape(tiles, tile)
    real = idx >= 0
    X = np.where(real[..., None], Q[np.maximum(idx, 0)], f32(np.nan))
    lo, hi = np.nanmin(X, axis=1).astype(f32), np.nanmax(X, axis=1).astype(f32)
    d = np.full(n, inf, f32)
    owner = np.full(n, -1, np.int64)
    cand = np.ones(n, bool)
    ident = order.astype(np.int64)

    def tile_key(t):  # (largest d, smallest id) among the tile's candidates, or None
        m = idx[t][real[t]]
        m = m[cand[m]]
        if len(m) == 0:
            return None
        best = np.lexsort((ident[m], -d[m].astype(np.float64)))[0]
        return d[m[best]], ident[m[best]], m[best]

    keys = [tile_key(t) for t in range(tiles)]
    cur = int(np.argmin(ident))  # position of id 0
    cur_d = f32(inf)
    ids, dsq, touched = [], [], []
    for j in range(count):
        ids.append(int(ident[cur]))
        dsq.append(cur_d)
        s = Q[cur]
        c = np.clip(s, lo, hi)
        with np.errstate(over="ignore"):
            lower = FO.dist_sq(c, s)
        tmax = np.array([k[0] if k else f32(0) for k in keys], f32)
        touch = ~(lower >= tmax)
        touch[cur // tile] = True
        touched.append(int(touch.sum()))
        cand[cur] = False  # the pick leaves the candidates; its own d and owner are still updated below
        for t in np.flatnonzero(touch):
            m = idx[t][real[t]]
            m = m[cand[m] | (m == cur)]
            nd = FO.dist_sq(Q[m], s)
            u = nd < d[m]
            d[m[u]] = nd[u]
            owner[m[u]] = ident[cur]
            keys[t] = tile_key(t)
        live = [k for k in keys if k]
        if not live:
            break
        best = max(live, key=lambda k: (k[0], -k[1]))
        cur, cur_d = int(best[2]), best[0]
    by_id = np.empty(n, np.int64)
    by_id[ident] = np.arange(n)
    return np.array(ids), FO.bits(dsq), owner[by_id], d[by_id], touched


def test_the_pruned_form_gives_the_plain_oracles_bits():
    from pcgol_amd import synth
    P = np.ascontiguousarray(synth.surface_cloud(20_000, 5.0, 6)[0], f32)
    want = FO.fps(P, 512)
    shares = {}
    for name, order in (("morton", _morton(P)), ("row-major", _row_major(P))):
        ids, dbits, owner, d, touched = _pruned(P, 512, order)
        assert np.array_equal(ids, want["ids"]), name
        assert np.array_equal(dbits, FO.bits(want["dist_sq"])), name
        assert np.array_equal(owner, want["owner"]) and np.array_equal(FO.bits(d), FO.bits(want["d"])), name
        shares[name] = np.mean(touched[64:]) / -(-len(P) // 64)
    # the pruning prunes: late picks touch a small share of the tiles, Morton order fewer than row-major order
    assert shares["morton"] < 0.1 and shares["morton"] < shares["row-major"], shares
