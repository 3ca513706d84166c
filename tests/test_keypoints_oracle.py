"""tests/keypoints_oracle.py against cases worked by hand, its three statements of the suppression against one another,
and the pin on pose_oracle.moved_clouds(): 51 ISS keypoints on each cloud, with the same ids."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_oracle as KO  # noqa: E402
import pose_oracle as PO  # noqa: E402

f32 = np.float32
nan, inf = np.nan, np.inf


def _all_forms(pts, score, r, deleted=None):
    pts = np.asarray(pts, f32).reshape(-1, 3)
    score = np.asarray(score, f32)
    a = KO.local_maxima_direct(pts, score, r, deleted)
    b = KO.maxima_from_lists(score, *KO.brute_lists(pts, r, deleted))
    c = KO.maxima_from_lists(score, *KO.brute_lists(pts, r), deleted=deleted)
    d = KO.maxima_from_sites(score, KO.sites(pts, r, deleted=deleted))
    e = KO.maxima_from_sites(score, KO.sites(pts, r, only=KO.candidate(score), deleted=deleted))
    f = e if deleted is None else KO.maxima_from_sites(score, KO.sites_without(KO.sites(pts, r), deleted, len(pts)))
    for x in (b, c, d, e, f):
        assert np.array_equal(a, x), (a, x)
    return a.tolist()


def test_ties_go_to_the_smaller_id():
    pts = [[0, 0, 0], [0.5, 0, 0]]
    assert _all_forms(pts, [1, 1], 1.0) == [0]
    assert _all_forms(pts, [1, 2], 1.0) == [1]
    assert _all_forms(pts, [2, 1], 1.0) == [0]
    # coincident points with equal scores leave the smallest id; the far one stands alone
    assert _all_forms([[1, 1, 1]] * 3 + [[9, 9, 9]], [4, 4, 4, 4], 1.0) == [0, 3]
    assert _all_forms([[1, 1, 1]] * 3, [4, 4, 5], 1.0) == [2]


def test_the_bound_is_strict():
    # DistSq == r * r exactly (dyadic coordinates): not a neighbour, so both are maxima
    assert _all_forms([[0, 0, 0], [0.75, 0, 0]], [1, 2], 0.75) == [0, 1]
    assert _all_forms([[0, 0, 0], [0.75, 0, 0]], [1, 2], 0.7500001) == [1]
    assert _all_forms([[0.25, 0.5, 0], [0.25, 0.5, 1.0]], [3, 3], 1.0) == [0, 1]


def test_nan_zero_negative_and_inf_scores():
    pts = [[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0]]
    assert _all_forms(pts, [1, nan, 0.5], 1.0) == [0]      # a NaN neighbour beats nobody, and never qualifies
    assert _all_forms(pts, [nan, nan, nan], 1.0) == []
    assert _all_forms(pts, [0, -0.0, -1], 1.0) == []       # 0 or below never qualifies
    assert _all_forms(pts, [0, -1, 1e-45], 1.0) == [2]     # ... the smallest denormal does
    assert _all_forms(pts, [inf, 5, inf], 1.0) == [0]      # +inf qualifies; equal infinities tie by id
    assert _all_forms(pts, [-inf, 0, 0], 1.0) == []


def test_a_point_that_is_not_its_own_neighbour():
    # a NaN coordinate is never a maximum and nobody's neighbour
    assert _all_forms([[nan, 0, 0], [0, 0, 0], [0.1, 0, 0]], [9, 1, 2], 1.0) == [2]
    assert _all_forms([[0, nan, 0]], [9], 1.0) == []
    # a deleted id neither wins nor suppresses
    assert _all_forms([[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0]], [1, 9, 2], 1.0, deleted=[1]) == [2]


def test_random_clouds_three_statements_agree():
    rng = np.random.default_rng(5)
    for n, r in ((1, 0.3), (2, 0.3), (150, 0.2), (400, 0.12)):
        pts = (rng.integers(0, 16, (n, 3)) / 16.0).astype(f32)  # a lattice: coincident points, DistSq == r * r
        s = rng.integers(0, 4, n).astype(f32)
        s[rng.random(n) < 0.05] = nan
        s[rng.random(n) < 0.05] = -1
        s[rng.random(n) < 0.02] = inf
        for rr in (r, 0.25):
            _all_forms(pts, s, rr)
            _all_forms(pts, s, rr, deleted=rng.choice(n, n // 5, replace=False))


def test_saliency_thresholds_are_strict_float32_products():
    below = np.nextafter(f32(0.5), f32(0))
    eig = np.array([[0.1, 0.5, 1.0],      # l1 == g21 * l2 exactly: not salient
                    [0.1, below, 1.0],    # one ulp below: salient
                    [0.25, 0.5, 2.0],     # l0 == g32 * l1 exactly: not salient
                    [0.0, 0.5, 2.0],      # l0 == 0: not salient
                    [0.0, 0.0, 0.0],      # degenerate
                    [nan, 0.5, 2.0], [0.1, nan, 2.0], [0.1, 0.2, nan]], f32)
    got = KO.saliency(eig, 0.5, 0.5)
    assert got.dtype == f32 and got.tolist()[:5] == [0.0, float(f32(0.1)), 0.0, 0.0, 0.0] and not got[5:].any()
    # the product is rounded to float32 before the comparison: 0.975f * 3 rounds up to a value l1 may equal
    g, l2 = f32(0.975), f32(3.0)
    t = g * l2
    assert float(t) != float(g) * 3.0  # (the float64 product differs: the float32 one decides)
    assert KO.saliency([[0.1, t, l2]], g, g)[0] == 0.0 and KO.saliency([[0.1, np.nextafter(t, f32(0)), l2]], g, g)[0] == f32(0.1)


def test_iss_degenerate_neighbourhoods_give_zero_eigenvalues():
    pts = np.array([[0, 0, 0]] * 6 + [[5, 5, 5], [5.01, 5, 5]], f32)  # six coincident points; two that are too few
    got = KO.iss_keypoints(pts, 0.5, 0.5, min_neighbors=5)
    assert not got["eigenvalues"].any() and not got["saliency"].any() and len(got["ids"]) == 0


def test_moved_clouds_pin():
    P, P2 = PO.moved_clouds()
    a = KO.iss_keypoints(P, 0.15, 0.1)
    b = KO.iss_keypoints(P2, 0.15, 0.1)
    assert len(a["ids"]) == 51 and np.array_equal(a["ids"], b["ids"])
    assert abs(a["counts"].mean() - 70.1) < 0.05 and int((a["saliency"] == 0).sum()) == 14
    assert np.array_equal(a["saliency"] == 0, b["saliency"] == 0)
