"""The k-NN and SOR oracles (tests/knn_oracle.py, tests/sor_oracle.py) against hand-computed cases: ties by id,
coincident heaps, the max_range boundary, NaN points and queries, deletions, m == mean_k.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_oracle as KO  # noqa: E402
import sor_oracle as SO  # noqa: E402

LINE = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [-1, 0, 0], [0, 2, 0]])


def test_line_by_distance_then_id():
    ids, dsq = KO.knearest_one(LINE, [0, 0, 0], 4, np.inf)
    # 0 at 0; 1 and 4 at 1 (tie: id 1 first); 2 and 5 at 4 (tie: id 2 first)
    assert ids.tolist() == [0, 1, 4, 2]
    assert dsq.tolist() == [0, 1, 1, 4]
    ids, dsq = KO.knearest_one(LINE, [0, 0, 0], 6, np.inf)
    assert ids.tolist() == [0, 1, 4, 2, 5, 3]


def test_max_range_is_strict_and_pads():
    ids, dsq, counts = KO.knearest(LINE, [[0, 0, 0]], 4, 1.0)  # DistSq 1 == max_range^2: out
    assert counts.tolist() == [1]
    assert ids.tolist() == [[0, -1, -1, -1]] and dsq.tolist() == [[0, 1, 1, 1]]
    ids, dsq, counts = KO.knearest(LINE, [[0, 0, 0]], 3, 0.0)
    assert counts.tolist() == [0] and ids.tolist() == [[-1, -1, -1]] and dsq.tolist() == [[0, 0, 0]]


def test_k_beyond_len_and_inf_range():
    ids, dsq, counts = KO.knearest(LINE, [[10, 0, 0]], 8, np.inf)
    assert counts.tolist() == [6]
    assert ids[0, :6].tolist() == [3, 2, 1, 0, 5, 4] or ids[0, :6].tolist() == [3, 2, 1, 0, 4, 5]
    d = KO.dist_sq_f32(LINE, np.float32([10, 0, 0]))
    assert np.all(np.diff(dsq[0, :6]) >= 0) and sorted(d.tolist()) == dsq[0, :6].tolist()
    assert ids[0, 6:].tolist() == [-1, -1] and np.all(np.isinf(dsq[0, 6:]))


def test_coincident_heap_takes_smallest_ids():
    pts = np.concatenate([np.tile(np.float32([1, 1, 1]), (50, 1)), np.float32([[1, 1, 1.5]])])
    perm = np.random.default_rng(1).permutation(len(pts))
    pts = pts[perm]
    ids, dsq = KO.knearest_one(pts, [1, 1, 1], 5, np.inf)
    heap_ids = np.sort(np.nonzero(perm != 50)[0])
    assert ids.tolist() == heap_ids[:5].tolist() and np.all(dsq == 0)


def test_nan_points_and_queries_and_exclusions():
    pts = LINE.copy()
    pts[1] = np.nan
    ids, dsq, counts = KO.knearest(pts, [[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]], 3, np.inf, exclude=[4])
    assert counts.tolist() == [3, 0, 0]
    assert ids[0].tolist() == [0, 2, 5]
    assert ids[1].tolist() == [-1, -1, -1] and ids[2].tolist() == [-1, -1, -1]


def test_batched_equals_lexsort_on_a_tied_lattice():
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pts = np.repeat(g, rng.integers(1, 4, len(g)), axis=0)
    pts = pts[rng.permutation(len(pts))]
    q = np.concatenate([g[:40], g[:40] + np.float32(0.5)])
    for k in (1, 8, 27):
        ids, dsq, counts = KO.knearest(pts, q, k, 1.8, chunk=4096)
        for j, qq in enumerate(q):
            oi, od = KO.knearest_one(pts, qq, k, 1.8)
            assert counts[j] == len(oi)
            assert ids[j, :len(oi)].tolist() == oi.tolist() and np.array_equal(dsq[j, :len(oi)], od)


def test_sor_hand_computed():
    # a unit square's corners and one far point; mean_k = 1: each corner's nearest other is at 1, the far point's at 9
    pts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [10, 1, 0]])
    r = SO.sor(pts, 1, 1.0)
    assert r["mean_dist"].tolist() == [1, 1, 1, 1, 9]
    mu = 13 / 5
    sigma = np.sqrt((4 * (1 - mu) ** 2 + (9 - mu) ** 2) / 4)
    assert r["mu"] == pytest.approx(mu, rel=1e-15) and r["sigma"] == pytest.approx(sigma, rel=1e-15)
    assert r["keep"].tolist() == [True, True, True, True, False]
    assert SO.sor(pts, 1, 1.0, negative=True)["keep"].tolist() == [False] * 4 + [True]


def test_sor_duplicates_count_and_self_does_not():
    # three coincident points and one at distance 2: mean_k = 2 -> the coincident ones have two others at 0
    pts = np.float32([[0, 0, 0], [0, 0, 0], [0, 0, 0], [2, 0, 0]])
    r = SO.sor(pts, 2, 0.0)
    assert r["mean_dist"].tolist() == [0, 0, 0, 2]
    # four coincident points, mean_k = 2, k = 3: point 3 is not among its own 3 nearest (ids 0, 1, 2 come first)
    pts = np.float32([[0, 0, 0]] * 4 + [[1, 0, 0]])
    r = SO.sor(pts, 2, 0.0)
    assert r["mean_dist"].tolist() == [0, 0, 0, 0, 1]


def test_sor_nan_dropped_and_m_equal_mean_k():
    pts = np.float32([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0, np.inf, 0], [3, 0, 0]])
    r = SO.sor(pts, 1, 1.0)
    assert np.isnan(r["mean_dist"][[1, 3]]).all()
    assert r["mean_dist"][[0, 2, 4]].tolist() == [1, 1, 2]
    assert not r["keep"][[1, 3]].any() and not SO.sor(pts, 1, 1.0, negative=True)["keep"][[1, 3]].any()
    with pytest.raises(SO.NoPoint):
        SO.sor(pts, 3, 1.0)  # m == mean_k
    SO.sor(pts, 2, 1.0)
