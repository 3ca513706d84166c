"""GPU parity: pcgx KD-tree (through the C ABI) vs the CPU oracle and the
reference's known-answer tables.  Bit-exact ids and float32 DistSq."""
import numpy as np
import pytest

import oracle as O
from pcgol_amd import kdtree, synth

pytestmark = pytest.mark.gpu
f32 = np.float32


def test_tree_shape_golden(golden):
    g = golden("ref_kdtree.json")
    t = kdtree.New(np.array(g["test_cloud"]["points"], f32))
    assert t.InOrder().tolist() == [5, 4, 1, 3, 2, 0, 6]  # == expected_tree in-order
    assert t.MaxDepth() == 3
    assert t.Len() == 7
    assert t.Vec3At(6).tolist() == [6, 2, 1]
    for c in g["max_depth"]["cases"]:
        assert kdtree.New(np.array(c["points"], f32)).MaxDepth() == c["expected"]


def test_nearest_table_golden(golden):
    g = golden("ref_kdtree.json")
    base = kdtree.New(np.array(g["test_cloud"]["points"], f32))
    for md in g["nearest"]["min_dist"]:
        t = base.With(MinDistSq=float(f32(md) * f32(md)))
        for c in g["nearest"]["cases"]:
            nb = t.Nearest(c["p"], c["max_range"])
            assert nb.ID == c["id"], (md, c)
            assert abs(float(nb.DistSq) - c["dist_sq"]) <= g["nearest"]["eps"]


@pytest.mark.parametrize("n,ties", [(1, False), (2, False), (3, False), (6, False), (100, False),
                                    (1000, True), (4097, False), (50000, True)])
def test_build_matches_oracle(n, ties):
    """Only the 50 000-point case is built on the device; test_gpu_tree_build.py forces the device build at sizes from 2
    points up (PCGX_BUILD=gpu) and compares it with the host build and the oracle there."""
    rng = np.random.default_rng(n)
    if ties:  # integer grid coordinates: many equal split keys -> exercises the stable order
        pts = rng.integers(0, 8, size=(n, 3)).astype(f32)
    else:
        pts = rng.random((n, 3), dtype=f32) * f32(10)
    t = kdtree.New(pts)
    o = O.KDTree(pts)
    assert np.array_equal(t.InOrder(), o.inorder())
    assert t.MaxDepth() == o.max_depth()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_nearest_equals_naive_property(golden, seed):
    """kdtree_test.go:794-834 through the C ABI: == brute force on ID and DistSq."""
    g = golden("ref_kdtree.json")["random_property"]
    rng = np.random.default_rng(seed)
    w = f32(g["width"])
    pts = rng.random((g["n_points"], 3), dtype=f32) * w
    t = kdtree.New(pts)
    for _ in range(g["n_queries"]):
        p = rng.random(3, dtype=f32) * w
        mr = float(rng.random(dtype=f32) * w)
        nb = t.Nearest(p, mr)
        assert (nb.ID, nb.DistSq) == O.naive_nearest(pts, p, mr)


@pytest.mark.parametrize("n,nq,max_range,min_dist_sq", [
    (1, 50, 10.0, 0.0), (2, 50, 10.0, 0.0), (5, 200, 3.0, 0.0), (1000, 5000, 10.0, 0.0),
    (20000, 20000, 0.3, 0.0), (20000, 20000, 10.0, 0.01), (20000, 20000, 0.5, 0.1),
    (200000, 100000, 10.0, 0.0), (200000, 100000, 0.05, 0.0), (200000, 50000, 10.0, 0.001),
])
def test_nearest_batch_vs_oracle(n, nq, max_range, min_dist_sq):
    base = synth.uniform_cloud(n, 10.0, 100 + n)
    q = synth.uniform_cloud(nq, 10.0, 200 + nq)
    t = kdtree.New(base, MinDistSq=min_dist_sq)
    ids, dsq = t.NearestBatch(q, max_range)
    o = O.KDTree(base, min_dist_sq=min_dist_sq)
    oi, od = o.nearest_batch(q, max_range)
    assert np.array_equal(ids, oi)
    assert np.array_equal(dsq.view(np.uint32), od.view(np.uint32))


def test_nearest_with_ties_and_duplicates():
    """Integer lattice: exact distance ties everywhere; the id chosen depends on the
    reference's visit order, which the device walk reproduces."""
    rng = np.random.default_rng(7)
    base = rng.integers(0, 6, size=(3000, 3)).astype(f32)
    q = rng.integers(0, 12, size=(4000, 3)).astype(f32) * f32(0.5)
    for md in (0.0, 0.3):
        t = kdtree.New(base, MinDistSq=md)
        ids, dsq = t.NearestBatch(q, 2.0)
        oi, od = O.KDTree(base, min_dist_sq=md).nearest_batch(q, 2.0)
        assert np.array_equal(ids, oi)
        assert np.array_equal(dsq, od)


def test_not_found_and_empty():
    base = synth.uniform_cloud(100, 1.0, 3)
    t = kdtree.New(base)
    nb = t.Nearest([50, 50, 50], 0.25)
    assert nb.ID == -1 and nb.DistSq == f32(0.25) * f32(0.25)  # kdtree.go:100-103
    ids, dsq = t.NearestBatch(np.zeros((0, 3), f32), 1.0)
    assert len(ids) == 0
    from pcgol_amd import ErrNoPoint
    with pytest.raises(ErrNoPoint):
        kdtree.New(np.zeros((0, 3), f32))


def test_c2_full_size_vs_oracle():
    """BASELINE config C2: 1M base, 1M queries, maxRange 10: ids and DistSq bit-exact."""
    c = synth.c2_knn()
    t = kdtree.New(c["base"])
    ids, dsq = t.NearestBatch(c["queries"], c["max_range"])
    o = O.KDTree(c["base"])
    assert np.array_equal(t.InOrder(), o.inorder())
    oi, od, visits, dists = o.nearest_batch(c["queries"], c["max_range"], stats=True)
    assert np.array_equal(ids, oi)
    assert np.array_equal(dsq.view(np.uint32), od.view(np.uint32))
    # V(q) is the figure the roofline's algorithmic bytes are built on
    assert 35.0 < visits / len(ids) < 55.0


def test_range_table_golden(golden):
    """kdtree_test.go:281-386 through the C ABI."""
    g = golden("ref_kdtree.json")["range"]
    t = kdtree.New(np.array(g["points"], f32))
    for c in g["cases"]:
        nb = t.Range(c["p"], c["max_range"])
        assert [n.ID for n in nb] == [x[0] for x in c["neighbors"]]
        for n, x in zip(nb, c["neighbors"]):
            assert abs(float(n.DistSq) - x[1]) <= g["eps"]


@pytest.mark.parametrize("n,nq,max_range", [(100, 100, 3.0), (5000, 2000, 1.0), (200000, 20000, 0.2),
                                            (3000, 500, 20.0)])
def test_range_batch_vs_oracle(n, nq, max_range):
    """kdtree_test.go:887-924 at scale: same set, sorted by DistSq; ties in the walk's discovery
    order (the oracle's order), so the arrays are identical."""
    base = synth.uniform_cloud(n, 10.0, 300 + n)
    q = synth.uniform_cloud(nq, 10.0, 400 + nq)
    if n == 3000:  # lattice: many exact distance ties
        base = np.random.default_rng(1).integers(0, 8, size=(n, 3)).astype(f32)
        q = np.random.default_rng(2).integers(0, 16, size=(nq, 3)).astype(f32) * f32(0.5)
        max_range = 1.6
    t = kdtree.New(base)
    offs, ids, dsq = t.RangeBatch(q, max_range)
    o = O.KDTree(base)
    assert offs[0] == 0 and offs[-1] == len(ids)
    for i in range(0, nq, max(1, nq // 300)):
        oi, od = o.range(q[i], max_range)
        s, e = offs[i], offs[i + 1]
        assert np.array_equal(ids[s:e], oi), i
        assert np.array_equal(dsq[s:e], od), i
    # every count agrees with brute force on a sample
    for i in range(0, nq, max(1, nq // 50)):
        d = base - q[i]
        dn = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert offs[i + 1] - offs[i] == int(np.sum(dn < f32(max_range) * f32(max_range)))


@pytest.mark.parametrize("n", [40_000, 70_001, 300_000, 1_000_000])
def test_build_with_the_lower_levels_in_lds_equals_radix_passes_all_the_way(n, monkeypatch):
    """kdtree.New on the device sorts a level's sub-slices with radix passes over the whole array until every
    sub-slice fits LDS, then one launch carries out all remaining levels there (csrc/kdtree_build_gpu.hip).
    PCGX_BUILD_LDS=0 keeps the radix passes all the way down: the in-order ids must be the same -- on a lattice
    (every split coordinate tied many times over: stability is what decides), with -0.0 / +0.0 mixed (equal under <)
    and at sizes whose sub-slices are ragged."""
    rng = np.random.default_rng(n)
    clouds = [synth.uniform_cloud(n, 10.0, n % 97),
              rng.integers(0, 12, size=(n, 3)).astype(f32),
              np.stack([rng.uniform(-5, 5, n), rng.choice([0.0, -0.0, 1.0], n), rng.normal(0, 0.01, n)], axis=1).astype(f32)]
    for c in clouds[:3 if n <= 300_000 else 1]:
        monkeypatch.delenv("PCGX_BUILD_LDS", raising=False)
        a = kdtree.New(c).InOrder()
        monkeypatch.setenv("PCGX_BUILD_LDS", "0")
        b = kdtree.New(c).InOrder()
        monkeypatch.delenv("PCGX_BUILD_LDS", raising=False)
        assert np.array_equal(a, b)


def test_a_nan_in_a_large_cloud_takes_the_host_build(monkeypatch):
    """A packed cloud of device-build size is on its way to the GPU before the host has looked for NaNs
    (csrc/knn.hip, build_tree); when it finds one, the device's work is dropped and the host builds, as for any cloud
    with a NaN coordinate (no consistent order under <): the same tree and the same answers as with the host build
    asked for from the start (PCGX_BUILD=host)."""
    n = 50_000
    base = synth.uniform_cloud(n, 10.0, 21)
    base[12_345, 1] = np.nan
    base[40_000] = [np.nan, np.nan, 0.5]
    q = synth.uniform_cloud(2000, 10.0, 22)
    t = kdtree.New(base)
    monkeypatch.setenv("PCGX_BUILD", "host")
    h = kdtree.New(base)
    monkeypatch.delenv("PCGX_BUILD")
    assert np.array_equal(t.InOrder(), h.InOrder())
    a, b = t.NearestBatch(q, 1.0), h.NearestBatch(q, 1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    clean = np.delete(base, [12_345, 40_000], axis=0)  # and every answer is a real nearest neighbour
    for i in range(0, len(q), 97):
        d = clean - q[i]
        dn = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        best = dn.min()
        assert (a[0][i] < 0 and not best < f32(1.0)) or a[1][i] == best, i


def test_range_with_a_run_of_a_hundred_thousand_exact_ties(monkeypatch):
    """One point taken 100 000 times (and a few more runs of 300): every neighbour of a query there is tied with all the
    others.  The grid path puts a run of ties into the walk's order afterwards; a slot that scans its run to find its
    place is quadratic in the run (ADVICE round 3 / VERDICT round 5: 1e10 steps here) -- runs beyond 128 slots are
    ordered by sorting instead, and a grid row of thousands of records is scanned by the whole wave (csrc/range.hip).
    The grid is forced (PCGX_GRID=2: a cloud this crowded is normally left to the tree walk, where ONE lane visits the
    hundred thousand nodes).  Ids and DistSq are the reference walk's (PCGX_RANGE_WALK=1, itself checked against the
    oracle above), and the call is quick."""
    import time
    rng = np.random.default_rng(5)
    base = np.concatenate([synth.uniform_cloud(50_000, 10.0, 9),
                           np.repeat(np.array([[5.0, 5.0, 5.0]], f32), 100_000, axis=0),
                           np.repeat(synth.uniform_cloud(40, 10.0, 10), 300, axis=0)]).astype(f32)
    base = np.ascontiguousarray(base[rng.permutation(len(base))])
    q = np.concatenate([np.array([[5.0, 5.0, 5.0], [5.01, 5.0, 4.99]], f32), synth.uniform_cloud(500, 10.0, 11)]).astype(f32)
    monkeypatch.setenv("PCGX_GRID", "2")
    t = kdtree.New(base)
    t.RangeBatch(q, 0.3)
    t0 = time.perf_counter()
    offs, ids, dsq = t.RangeBatch(q, 0.3)
    dt = time.perf_counter() - t0
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    offs_w, ids_w, dsq_w = t.RangeBatch(q, 0.3)
    monkeypatch.delenv("PCGX_RANGE_WALK")
    assert offs[1] - offs[0] >= 100_000
    assert np.array_equal(offs, offs_w) and np.array_equal(dsq, dsq_w) and np.array_equal(ids, ids_w)
    assert dt < 0.05, dt


@pytest.mark.parametrize("kind", ["uniform", "lattice", "surface"])
def test_range_on_the_grid_equals_the_walk(kind, monkeypatch):
    """Range collects the neighbours from the handle's uniform grid and puts equal DistSq of one query into the
    walk's discovery order afterwards (csrc/range.hip); PCGX_RANGE_WALK=1 runs the reference's walk
    (kdtree.go:148-197) instead.  Every offset, id and DistSq of the two must agree -- clouds with thousands of
    exact ties and repeated points included -- and so must odd queries (NaN, inf, far outside, radius 0 / huge)."""
    rng = np.random.default_rng(77)
    n, nq = 120_000, 30_000
    if kind == "uniform":
        base = synth.uniform_cloud(n, 10.0, 5)
        q = synth.uniform_cloud(nq, 10.0, 6)
        radii = [0.25, 0.0, 1.0e-3]
    elif kind == "lattice":  # integer lattice, every site several times: ties everywhere
        base = rng.integers(0, 24, size=(n, 3)).astype(f32)
        q = (rng.integers(0, 48, size=(nq, 3)).astype(f32) * f32(0.5))
        radii = [1.6, 1.0]
    else:  # a thin sheet: crowded cells, empty cells
        base = np.stack([rng.uniform(0, 10, n), rng.uniform(0, 10, n), rng.normal(0, 0.01, n)], axis=1).astype(f32)
        q = np.stack([rng.uniform(-1, 11, nq), rng.uniform(-1, 11, nq), rng.normal(0, 0.05, nq)], axis=1).astype(f32)
        radii = [0.1, 3.0e38]
    q[0] = [np.nan, 1.0, 1.0]
    q[1] = [np.inf, 0.0, 0.0]
    q[2] = [1.0e30, -1.0e30, 5.0]
    q[3] = base[17]
    t = kdtree.New(base)
    for r in radii:
        if r > 1.0e30:
            qq = q[:40]  # (every point is a neighbour)
        else:
            qq = q
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)
        og, ig, dg = t.RangeBatch(qq, r)
        monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        ow, iw, dw = t.RangeBatch(qq, r)
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)
        assert np.array_equal(og, ow), (kind, r)
        assert np.array_equal(dg.view(np.uint32), dw.view(np.uint32)), (kind, r)
        assert np.array_equal(ig, iw), (kind, r, int(np.sum(ig != iw)))
        if kind == "lattice":
            assert len(ig) > 10 * len(qq)  # (the case is about ties: make sure there are neighbours at all)


def test_range_fill_rejects_wrong_offsets():
    import ctypes as C
    from pcgol_amd import _lib as L
    base = synth.uniform_cloud(2000, 1.0, 8)
    q = synth.uniform_cloud(50, 1.0, 9)
    t = kdtree.New(base)
    offs, ids, dsq = t.RangeBatch(q, 0.2)
    bad = offs.copy()
    bad[1:] += 3  # claims more neighbours than exist
    ids2 = np.empty(int(bad[-1]), np.int64)
    dsq2 = np.empty(int(bad[-1]), np.float32)
    rc = L.lib().pcgx_kdtree_range_fill(t._h, L.ptr(q), len(q), 0.2, L.ptr(bad), L.ptr(ids2), L.ptr(dsq2))
    assert rc == L.PCGX_E_INVALID
