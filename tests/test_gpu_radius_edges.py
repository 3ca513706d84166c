"""Radius neighbourhoods (csrc/range_enum.h) where the shared enumeration branches: grid rows of 4095 / 4096 / 4097
and more records (kRangeFatRow: rows the whole wave scans, two per lane, a third one the lane's own), several owners
of different fat rows in one wave and one in a partial last wave, heaps at exactly DistSq == r*r, long runs of exact
ties on a tree deep enough for the high word of the walk's place (range.hip, pcgx_kdtree_range_fill), runs of
127 / 128 / 129 ties, and batches either side of the Morton presort (16384).  Range (count + fill), Normals /
NormalsDev and RegionGrowing.Components are checked against references that share no code with the kernels: float32
brute force for sets and counts, the C oracle's walk for the order, float64 normals from the brute-force lists, and a
union-find in NumPy for the components."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle as O
from pcgol_amd import _lib as L
from pcgol_amd import kdtree, segmentation, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_oracle as NO  # noqa: E402
from test_gpu_normals import _check_against_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32

# ------------------------------------------------------------------------------------------------ scenes

# Four coincident heaps round HC, each alone in its grid row (y, z): they differ by 1.0 in y or z, and the grid's
# cells are below 0.5 (asserted).  4095 records are one lane's row, 4096 and more a fat row.  Every coordinate is a
# multiple of 1/4, so distances between heaps and the special queries are exact in float32.
HC = np.array([8.0, 8.0, 12.0], f32)
HEAPS = [(HC + np.array(o, f32), m) for o, m in (((0.0, -0.5, -0.5), 4095), ((0.25, 0.5, -0.5), 4096),
                                                  ((-0.25, -0.5, 0.5), 4097), ((0.5, 0.5, 0.5), 6000))]
BOX = 16.0  # the scene's bounding box is [0, 16]^3 (two corner points), so the grid is a cube of cells


def _heap_scene(n_slab=50_000):
    rng = np.random.default_rng(2024)
    slab = synth.uniform_cloud(n_slab, 1.0, 31) * np.array([BOX, BOX, 4.0], f32)  # background, z in [0, 4)
    s = (rng.uniform(6.0, 10.0, (6000, 3)) + np.array([0.0, 0.0, 4.0])).astype(f32)  # sparse round the heaps...
    far = np.ones(len(s), bool)
    for h, _ in HEAPS:  # ... but never in a heap's row
        far &= (np.abs(s[:, 1] - h[1]) >= 0.5) | (np.abs(s[:, 2] - h[2]) >= 0.5)
    parts = [slab, s[far][:3000], np.array([[0.0, 0.0, 0.0], [BOX, BOX, BOX]], f32)]
    parts += [np.repeat(h[None, :], m, axis=0) for h, m in HEAPS]
    pts = np.concatenate(parts).astype(f32)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


_SCENE = {}


def _scene(name, make):
    if name not in _SCENE:
        _SCENE[name] = make()
    return _SCENE[name]


def _heap_queries(seed):
    """Queries at the heaps: the centre (all four within 1.0; two at exactly 0.75), a heap at exactly 1.0 (r = 1) from
    one side or another, jittered points that see two, three or four heaps -- shuffled with queries in the slab and
    among the sparse points, so the lanes of one wave own different fat rows."""
    rng = np.random.default_rng(seed)
    special = [HC]
    for h, _ in HEAPS:
        for a in range(3):
            for sgn in (1.0, -1.0):
                e = np.zeros(3, f32)
                e[a] = sgn
                special.append(h + e)  # the heap at DistSq 1.0 exactly
                special.append(h + e * f32(0.75))  # at 0.5625 == 0.75 * 0.75
    special = np.array(special, f32)
    jitter = (HC + np.concatenate([rng.uniform(-1.0, 1.0, (120, 3)), rng.uniform(-0.4, 0.4, (100, 3))])).astype(f32)
    sparse = rng.uniform([6.0, 6.0, 10.0], [10.0, 10.0, 14.0], (120, 3)).astype(f32)
    slab = rng.uniform([0.5, 0.5, 0.5], [15.5, 15.5, 3.5], (300, 3)).astype(f32)
    q = np.concatenate([special, jitter, sparse, slab])
    return np.ascontiguousarray(q[rng.permutation(len(q))])


# ------------------------------------------------------------------------------------------------ references

def _bf_points(pts, deleted=None):
    """points for the brute force: a deleted point becomes NaN (never DistSq < bound), ids stay"""
    p = np.array(pts, f32)
    if deleted is not None:
        p[np.asarray(deleted)] = np.nan
    return p


def _oracle_tree(pts, deleted=None):
    o = O.KDTree(pts)
    for i in (deleted if deleted is not None else []):
        o.delete_point(int(i))
    return o


def _host_walks():
    v = C.c_int64()
    L.check(L.lib().pcgx_debug_host_walks(C.byref(v), 0))
    return v.value


def _grid_on(t):
    out = (C.c_int64 * 14)()
    L.check(L.lib().pcgx_debug_grid_stats(t._h, None, 0, 1.0, out))
    return list(out)


def _assert_heap_grid(t):
    """the grid is on and its cells are under 0.5 wide: every heap has a grid row of its own"""
    st = _grid_on(t)
    assert st[3] == 1, st
    d = int(round(st[1] ** (1.0 / 3.0)))
    assert d ** 3 == st[1], st  # nx = ny = nz = d = int(16 / h) + 1
    assert BOX / (d - 1) < 0.5, d


def _range_count(t, q, r):
    c = np.zeros(len(q), np.int64)
    L.check(L.lib().pcgx_kdtree_range_count(t._h, L.ptr(q), len(q), float(r), L.ptr(c)))
    return c


def _check_range(t, q, r, bf_pts, otree, what, order=None, cap=1 << 16):
    """counts and sets against the brute force, every DistSq recomputed, and the order of the queries `order`
    (default: all) against the oracle's walk, ids and DistSq bits"""
    hw = _host_walks()
    offs, ids, dsq = t.RangeBatch(q, r)
    assert _host_walks() == hw, what  # the device answered (batches above 32 queries)
    bo, bi = NO.brute_force_lists(bf_pts, q, r)
    assert np.array_equal(offs, bo), (what, np.nonzero(np.diff(offs) != np.diff(bo))[0][:10])
    qi = np.repeat(np.arange(len(q)), np.diff(offs))
    assert np.array_equal(ids[np.lexsort((ids, qi))], bi), what
    p, qq = bf_pts[ids], q[qi]
    d = ((p[:, 0] - qq[:, 0]) * (p[:, 0] - qq[:, 0]) + (p[:, 1] - qq[:, 1]) * (p[:, 1] - qq[:, 1])) + \
        (p[:, 2] - qq[:, 2]) * (p[:, 2] - qq[:, 2])
    assert np.array_equal(d.view(np.uint32), dsq.view(np.uint32)), what
    for i in (range(len(q)) if order is None else order):
        oi, od = otree.range(q[i], r, cap=cap)
        s, e = offs[i], offs[i + 1]
        assert np.array_equal(ids[s:e], oi), (what, i)
        assert np.array_equal(dsq[s:e].view(np.uint32), od.view(np.uint32)), (what, i)
    return offs, ids, dsq


def _check_normals(t, q, r, bf_pts, what, vp=(0.3, -2.0, 25.0)):
    got = t.Normals(r, Viewpoint=vp, Queries=q)
    assert np.array_equal(got[2].astype(np.int64), _range_count(t, q, r)), what
    ref = NO.normals_from_lists(bf_pts, q, *NO.brute_force_lists(bf_pts, q, r), vp, 3)
    _check_against_oracle(got, ref, q, vp, what)
    return got


def _handles(pts, monkeypatch, deleted=None, rows=True):
    """(name, tree, deleted ids) on the grid (PCGX_GRID=2: the heaps crowd it), the forced walk, and -- given
    `deleted` -- a handle that has seen DeletePoints (the patched tree's walk)"""
    monkeypatch.setenv("PCGX_GRID", "2")
    t = kdtree.New(pts)
    if rows:
        _assert_heap_grid(t)
    else:
        assert _grid_on(t)[3] == 1
    yield "grid", t, None
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    yield "walk", t, None
    monkeypatch.delenv("PCGX_RANGE_WALK")
    if deleted is not None:
        td = kdtree.New(pts)
        td.DeletePoints(deleted)
        yield "deleted", td, deleted


def _heap_deleted(pts):
    """2 % of the points, a few of every heap's among them"""
    return np.random.default_rng(9).choice(len(pts), len(pts) // 50, replace=False)


# ------------------------------------------------------------------------------------------------ tests

@pytest.mark.parametrize("r", [1.0, 0.75])
def test_range_and_normals_at_fat_grid_rows(r, monkeypatch):
    """Counts, sets, the walk's order and normals where queries see two, three or four heaps of 4095 / 4096 / 4097 /
    6000 records in rows of their own (a third fat row: the lane's own work), with heaps at exactly DistSq == r*r
    (left out: the bound is strict on grid rows, fat rows and walks alike)."""
    pts = _scene("heaps", _heap_scene)
    q = _heap_queries(1)
    dele = _heap_deleted(pts)
    for name, t, gone in _handles(pts, monkeypatch, dele):
        bf = _bf_points(pts, gone)
        o = _oracle_tree(pts, gone)
        offs, _, _ = _check_range(t, q, r, bf, o, (name, r))
        _check_normals(t, q, r, bf, (name, r))
        if name == "grid":  # the scene does what it is for: heaps at the bound, queries with three fat rows
            bound = f32(r) * f32(r)
            hd = np.stack([NO.dist_sq_f32(q, h) for h, _ in HEAPS], axis=1)
            assert np.sum(hd == bound) >= 24, int(np.sum(hd == bound))
            if r == 1.0:
                assert np.sum(np.all(hd[:, 1:] < bound, axis=1)) >= 5
                assert np.max(np.diff(offs)) >= sum(m for _, m in HEAPS)


def test_many_fat_row_owners_in_one_wave_and_a_partial_last_wave(monkeypatch):
    """Batches of 97 and 150 queries (caller order: below the presort): the lanes of a wave own different fat rows,
    and the last query -- the only one at the heaps in one case -- sits alone in a partial wave whose other lanes
    stay to the end without a query.  Range fill, counts and normals; NormalsDev gives the host entry's bits."""
    import torch
    pts = _scene("heaps", _heap_scene)
    rng = np.random.default_rng(3)
    slab = rng.uniform([0.5, 0.5, 0.5], [15.5, 15.5, 3.5], (96, 3)).astype(f32)
    q97a = np.concatenate([slab, HC[None, :]]).astype(f32)  # one owner, index 96 (lane 32 of the second wave)
    q97b = np.concatenate([_heap_queries(5)[:96], (HC + np.array([0.0, 0.0, 0.25], f32))[None, :]]).astype(f32)
    near = (HC + rng.uniform(-0.6, 0.6, (150, 3))).astype(f32)  # every lane of two waves and a half at the heaps
    for name, t, gone in _handles(pts, monkeypatch, _heap_deleted(pts)):
        bf = _bf_points(pts, gone)
        o = _oracle_tree(pts, gone)
        # (near at 0.75: mostly two heaps or one, a line or a point -- no normal to compare)
        for q, radii in ((q97a, (1.0, 0.75)), (q97b, (1.0, 0.75)), (near, (1.0,))):
            for r in radii:
                _check_range(t, q, r, bf, o, (name, len(q), r))
                n, c, k = _check_normals(t, q, r, bf, (name, len(q), r))
                dev = torch.device("cuda", 0)
                dq = torch.from_numpy(q).to(dev)
                dn = torch.empty((len(q), 3), dtype=torch.float32, device=dev)
                dc = torch.empty(len(q), dtype=torch.float32, device=dev)
                dk = torch.empty(len(q), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                t.NormalsDev(r, dn.data_ptr(), dc.data_ptr(), dk.data_ptr(), d_q=dq.data_ptr(), nq=len(q),
                             Viewpoint=(0.3, -2.0, 25.0), stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert np.array_equal(dn.cpu().numpy().view(np.uint32), n.view(np.uint32)), name
                assert np.array_equal(dc.cpu().numpy().view(np.uint32), c.view(np.uint32)), name
                assert np.array_equal(dk.cpu().numpy(), k), name


def test_presort_boundary_batches(monkeypatch):
    """Batches of 16383 (caller order), 16384 and 16385 (Morton order) queries: count, fill and normals agree bit for
    bit on the shared prefix, and with the references on a sample.  NaN, inf and far-outside queries (some in the
    prefix, the two extra ones of the largest batch) give count 0, normal 0 and curvature NaN."""
    pts = _scene("heaps", _heap_scene)
    rng = np.random.default_rng(11)
    r = 1.0
    base_q = np.concatenate([_heap_queries(7),
                             rng.uniform([0.0, 0.0, 0.0], [16.0, 16.0, 4.5], (16_385, 3)).astype(f32)])[:16_385]
    base_q = np.ascontiguousarray(base_q[rng.permutation(16_385)])
    odd = {100: [np.nan, 1.0, 1.0], 5000: [1.0e30, -1.0e30, 5.0], 9000: [-np.inf, 8.0, 12.0],
           16_383: [np.nan, np.nan, np.nan], 16_384: [np.inf, 8.0, 12.0]}
    for i, v in odd.items():
        base_q[i] = v
    odd_idx = np.array(sorted(odd))
    sample = np.unique(np.concatenate([rng.choice(16_383, 250, replace=False), odd_idx[:3],
                                       np.nonzero(np.linalg.norm(base_q[:16_383] - HC, axis=1) < 1.2)[0][:40]]))
    for name, t, gone in _handles(pts, monkeypatch, _heap_deleted(pts)):
        bf = _bf_points(pts, gone)
        o = _oracle_tree(pts, gone)
        res = []
        for nq in (16_383, 16_384, 16_385):
            q = base_q[:nq]
            hw = _host_walks()
            offs, ids, dsq = t.RangeBatch(q, r)
            cnt = _range_count(t, q, r)
            nrm = t.Normals(r, Viewpoint=(0.3, -2.0, 25.0), Queries=q)
            assert _host_walks() == hw
            assert np.array_equal(np.diff(offs), cnt) and np.array_equal(nrm[2].astype(np.int64), cnt), (name, nq)
            ok = odd_idx[odd_idx < nq]
            assert np.all(cnt[ok] == 0) and np.all(nrm[0][ok] == 0) and np.all(np.isnan(nrm[1][ok])), (name, nq)
            res.append((offs, ids, dsq, nrm))
        p = 16_383
        offs0, ids0, dsq0, nrm0 = res[0]
        for offs, ids, dsq, nrm in res[1:]:
            assert np.array_equal(offs[:p + 1], offs0), name
            assert np.array_equal(ids[:offs0[-1]], ids0) and np.array_equal(dsq[:offs0[-1]].view(np.uint32), dsq0.view(np.uint32)), name
            for a, b in zip(nrm, nrm0):
                assert np.array_equal(a[:p].view(np.uint32), b.view(np.uint32)), name
        offs, ids, dsq, nrm = res[2]
        qs = base_q[sample]
        bo, bi = NO.brute_force_lists(bf, qs, r)
        assert np.array_equal(np.diff(offs)[sample], np.diff(bo)), name
        for j, i in enumerate(sample):
            assert np.array_equal(np.sort(ids[offs[i]:offs[i + 1]]), bi[bo[j]:bo[j + 1]]), (name, i)
            if j % 4 == 0 or np.linalg.norm(base_q[i] - HC) < 1.2:
                oi, od = o.range(base_q[i], r)
                assert np.array_equal(ids[offs[i]:offs[i + 1]], oi) and np.array_equal(dsq[offs[i]:offs[i + 1]], od), (name, i)
        ref = NO.normals_from_lists(bf, qs, bo, bi, (0.3, -2.0, 25.0), 3)
        _check_against_oracle(tuple(x[sample] for x in nrm), ref, qs, (0.3, -2.0, 25.0), name)


def _deep_scene():
    """1.1M points (a tree of depth 21: the walk's place has 3^21 values, more than 32 bits) with heaps of 150 to 300
    coincident points: pairs equally far from a query on the two sides of the root's split (x ~ 5) and of the split
    below it on the far side (y ~ 5), and one heap alone"""
    base = synth.uniform_cloud(1_100_000, 10.0, 41)
    heaps = [((4.0, 5.0, 5.0), 150), ((6.0, 5.0, 5.0), 150),        # DistSq 1 from (5, 5, 5)
             ((5.5, 4.0, 5.0), 200), ((5.5, 6.0, 5.0), 200),        # DistSq 3.25 from (4, 5, 5)
             ((2.5, 7.5, 2.5), 300)]
    pts = np.concatenate([base] + [np.repeat(np.array([h], f32), m, axis=0) for h, m in heaps]).astype(f32)
    return np.ascontiguousarray(pts[np.random.default_rng(12).permutation(len(pts))])


def test_long_tie_runs_on_a_tree_deeper_than_32_place_bits(monkeypatch):
    """Runs of 300 and 400 exact ties (beyond kTieRunLimit: the four-pass sort) whose slots lie on both sides of the
    root, so their walk places differ in the high word: Range fill in the oracle walk's order on the default grid,
    and the same arrays with PCGX_RANGE_WALK=1."""
    pts = _scene("deep", _deep_scene)
    t = kdtree.New(pts)
    assert t.MaxDepth() >= 21
    assert _grid_on(t)[3] == 1
    o = _scene("deep_oracle", lambda: O.KDTree(pts))
    root = int(o.dump()[0][0])
    assert 4.0 < pts[root, 0] < 5.5, pts[root]  # the heap pairs straddle the root's split
    rng = np.random.default_rng(13)
    special = np.array([[5.0, 5.0, 5.0], [4.0, 5.0, 5.0], [2.5, 7.5, 2.5], [2.75, 7.5, 2.5], [5.0, 5.0, 5.25]], f32)
    q = np.concatenate([special, rng.uniform(0.0, 10.0, (60, 3)).astype(f32)])
    r = 1.875  # (3.515625 exactly)
    cap = 1 << 17
    offs, ids, dsq = _check_range(t, q, r, pts, o, "deep grid", cap=cap)
    for i, key, m in ((0, 1.0, 300), (1, 3.25, 400), (3, 0.0625, 300)):
        run = dsq[offs[i]:offs[i + 1]] == f32(key)
        assert run.sum() == m, (i, int(run.sum()))
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    ow, iw, dw = t.RangeBatch(q, r)
    monkeypatch.delenv("PCGX_RANGE_WALK")
    assert np.array_equal(offs, ow) and np.array_equal(ids, iw) and np.array_equal(dsq.view(np.uint32), dw.view(np.uint32))


def _tie_scene():
    """50k points with heaps of 127, 128 and 129 coincident points, and pairs of heaps (64 + 64, 64 + 65) equally far
    from a query between them; no other point within 1.1 of a heap or a pair's centre, so the queries beside them
    (r = 0.75) see the heaps alone, and a run of ties is a query's whole list"""
    base = synth.uniform_cloud(50_000, 10.0, 51)
    keep = np.ones(len(base), bool)
    for c in list(TIE_HEAPS) + [(5.0, 5.0, 8.0), (5.0, 2.0, 5.0)]:
        keep &= np.linalg.norm(base - np.array(c, f32), axis=1) > 1.1
    pts = np.concatenate([base[keep]] + [np.repeat(np.array([h], f32), m, axis=0) for h, m in TIE_HEAPS.items()])
    return np.ascontiguousarray(pts.astype(f32)[np.random.default_rng(52).permutation(len(pts))])


TIE_HEAPS = {(2.0, 2.0, 2.0): 127, (2.0, 8.0, 2.0): 128, (8.0, 2.0, 2.0): 129,
             (4.5, 5.0, 8.0): 64, (5.5, 5.0, 8.0): 64,   # 128 at DistSq 0.25 from (5, 5, 8)
             (5.0, 1.5, 5.0): 64, (5.0, 2.5, 5.0): 65}   # 129 at DistSq 0.25 from (5, 2, 5)


def test_runs_of_127_128_and_129_ties(monkeypatch):
    """Runs of at most 128 ties in a batch are ordered slot by slot, a batch with one of 129 by sorting
    (range.hip, kTieRunLimit).  Both, and runs of equal DistSq in adjacent queries (the same key, another query),
    in the oracle walk's order on the grid and on the walk."""
    pts = _scene("ties", _tie_scene)
    t = kdtree.New(pts)
    assert t.MaxDepth() <= 20  # the place fits 32 bits
    assert _grid_on(t)[3] == 1
    o = _scene("ties_oracle", lambda: O.KDTree(pts))
    rng = np.random.default_rng(53)
    fill = rng.uniform(0.0, 10.0, (40, 3)).astype(f32)
    e = np.array([0.25, 0.0, 0.0], f32)
    h127, h128, h129 = (np.array(h, f32) for h in ((2.0, 2.0, 2.0), (2.0, 8.0, 2.0), (8.0, 2.0, 2.0)))
    # (query, DistSq, ties): queries 0 / 1 of each batch have runs of one key back to back, and so do 2 / 3
    short = (((h127 + e, 0.0625, 127), (h127 - e, 0.0625, 127), (h128 + e, 0.0625, 128), (h128 - e, 0.0625, 128),
              (h128 + e[[1, 0, 2]], 0.0625, 128), ((5.0, 5.0, 8.0), 0.25, 128)))
    long_ = (((h129 + e, 0.0625, 129), (h129 - e, 0.0625, 129), (h127 + e, 0.0625, 127), (h128 - e, 0.0625, 128),
              ((5.0, 2.0, 5.0), 0.25, 129), ((5.0, 5.0, 8.0), 0.25, 128)))
    for name in ("grid", "walk"):
        if name == "walk":
            monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        for runs in (short, long_):
            q = np.ascontiguousarray(np.concatenate([np.array([x[0] for x in runs], f32), fill]), f32)
            offs, ids, dsq = _check_range(t, q, 0.75, pts, o, (name, len(runs)))
            for i, (_, key, m) in enumerate(runs):
                assert offs[i + 1] - offs[i] == m and np.all(dsq[offs[i]:offs[i + 1]] == f32(key)), (name, i)
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)


def _components_reference(pts, labels, r):
    """comp[i] = smallest id of i's component: points joined when DistSq < r*r (float32) and their labels are equal.
    Coincident points of one label are one site; the sites' pairs by brute force; a union-find by pointer jumping."""
    key = np.concatenate([pts.view(np.uint32), labels[:, None].astype(np.uint32)], axis=1)
    _, first, site = np.unique(key, axis=0, return_index=True, return_inverse=True)
    site = site.reshape(-1)
    sp, sl = pts[first], labels[first]
    bound = f32(r) * f32(r)
    a_list, b_list = [], []
    for s0 in range(0, len(sp), 512):
        blk = sp[s0:s0 + 512]
        dx = blk[:, None, 0] - sp[None, :, 0]
        dy = blk[:, None, 1] - sp[None, :, 1]
        dz = blk[:, None, 2] - sp[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        a, b = np.nonzero((d < bound) & (sl[s0:s0 + 512, None] == sl[None, :]))
        a_list.append(a + s0)
        b_list.append(b)
    a, b = np.concatenate(a_list), np.concatenate(b_list)
    parent = np.arange(len(sp))
    while True:
        m = np.minimum(parent[a], parent[b])
        new = parent.copy()
        np.minimum.at(new, parent[a], m)
        np.minimum.at(new, parent[b], m)
        while True:  # pointer jumping
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, parent):
            break
        parent = new
    low = np.full(len(sp), len(pts), np.int64)
    np.minimum.at(low, parent[site], np.arange(len(pts)))
    return low[parent[site]]


def test_region_growing_on_a_grid_with_coincident_heaps(monkeypatch):
    """Components on the heap scene's grid (PCGX_GRID=2; segment.hip's grid kernel has no fat-row path) and on the
    walk, three label values (a fifth of the background, for the brute force's sake).  r = 0.5 keeps every heap apart
    from everything else; r = 1.5 joins the heaps (two pairs at exactly 1.5 do not join directly).  Equal to a
    union-find over the brute-force pairs, every component named by its smallest id; a few seeds against the oracle's
    Segment."""
    pts = _scene("heaps_rg", lambda: _heap_scene(10_000))
    labels = np.random.default_rng(21).integers(0, 3, len(pts)).astype(np.uint32)
    o = O.KDTree(pts)
    seeds = [HEAPS[0][0], HEAPS[3][0], HC, np.array([3.0, 3.0, 2.0], f32), np.array([7.0, 9.5, 12.0], f32)]
    for r in (0.5, 1.5):
        want = _components_reference(pts, labels, r)
        for lab in range(3):  # the scene does what it is for
            heap_ids = [np.nonzero(np.all(pts == h, axis=1) & (labels == lab))[0] for h, _ in HEAPS]
            names = {int(want[ids[0]]) for ids in heap_ids}
            assert all(np.all(want[ids] == want[ids[0]]) for ids in heap_ids)
            if r == 0.5:
                assert len(names) == 4 and all(np.sum(want == want[ids[0]]) == len(ids) for ids in heap_ids)
            else:
                assert len(names) == 1
        for name, t, _ in _handles(pts, monkeypatch, rows=False):
            rg = segmentation.RegionGrowing(t, labels)
            got = rg.Components(r)
            assert np.array_equal(got, want), (name, r, int(np.sum(got != want)))
            for p in (seeds if r == 0.5 else seeds[3:4]):  # (the oracle's BFS through a heap at 1.5 takes minutes)
                exact = O.region_growing_segment(o, labels, p, r)
                assert np.array_equal(rg.Segment(p, r, order="id"), np.sort(exact)), (name, r, p)
