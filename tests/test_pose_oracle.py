"""tests/pose_oracle.py, the NumPy restatement of "pose from correspondences" (include/pcgx.h), on cases worked by hand
and on scene M (the moved clouds, 1500 pairs of which 40 % name a wrong partner, 4096 hypotheses), which the GPU tests
(tests/test_gpu_pose.py) and the host test of csrc/pose_terms.h (tests/test_pose_terms_host.py) compare the library
with.  No GPU, no library."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_oracle as PO  # noqa: E402

f32, f64, u32 = np.float32, np.float64, np.uint32


def word_for(i, m):
    """the smallest sample word that names pair i of m"""
    u = -((-i << 32) // m)
    assert 0 <= u < 2 ** 32 and (u * m) >> 32 == i
    return u


def words(idx, m):
    return np.array([[word_for(i, m) for i in row] for row in idx], u32).reshape(-1, 3)


TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)


def hand_cases():
    """name -> dict(P, Q, src, dst, samples, es, status): one hypothesis each unless said otherwise"""
    ids3 = np.arange(3, dtype=np.int64)
    s012 = words([[0, 1, 2]], 3)
    c = {}
    c["translation"] = dict(P=TRI, Q=TRI + np.array([1, 2, 3], f32), src=ids3, dst=ids3, samples=s012, es=0.9, status=[0],
                            pose=np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 2, 3, 1], f32))
    c["repeated index"] = dict(P=TRI, Q=TRI, src=ids3, dst=ids3, samples=words([[0, 0, 1], [2, 1, 2], [1, 0, 1]], 3), es=0.9,
                               status=[1, 1, 1])
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], f32)
    c["collinear source"] = dict(P=line, Q=TRI, src=ids3, dst=ids3, samples=s012, es=0.0, status=[2])
    c["collinear target"] = dict(P=TRI, Q=line, src=ids3, dst=ids3, samples=s012, es=0.0, status=[2])
    c["coincident points"] = dict(P=TRI[[0, 0, 1]], Q=TRI, src=ids3, dst=ids3, samples=s012, es=0.0, status=[2])
    near = np.array([[0, 0, 0], [1.05, 0, 0], [0, 1, 0]], f32)   # edge (0,1): 1 against 1.05, 1 >= 0.9 * 1.05
    far = np.array([[0, 0, 0], [1.25, 0, 0], [0, 1, 0]], f32)    # 1 against 1.25: 1 < 0.9 * 1.25
    c["stretched edge inside"] = dict(P=TRI, Q=near, src=ids3, dst=ids3, samples=s012, es=0.9, status=[0])
    c["stretched edge outside"] = dict(P=TRI, Q=far, src=ids3, dst=ids3, samples=s012, es=0.9, status=[3])
    c["shrunk edge outside"] = dict(P=far, Q=TRI, src=ids3, dst=ids3, samples=s012, es=0.9, status=[3])
    c["stretched edge, test off"] = dict(P=TRI, Q=far, src=ids3, dst=ids3, samples=s012, es=0.0, status=[0])
    nanp = TRI.copy()
    nanp[1, 0] = np.nan
    c["NaN point"] = dict(P=nanp, Q=TRI, src=ids3, dst=ids3, samples=s012, es=0.9, status=[2])
    infp = TRI.copy()
    infp[2, 1] = np.inf
    c["inf point"] = dict(P=TRI, Q=infp, src=ids3, dst=ids3, samples=s012, es=0.9, status=[2])
    c["m = 0"] = dict(P=TRI, Q=TRI, src=ids3[:0], dst=ids3[:0], samples=np.array([[0, 1 << 31, 0xffffffff]], u32), es=0.9,
                      status=[1])
    c["m = 2"] = dict(P=TRI, Q=TRI, src=ids3[:2], dst=ids3[:2], samples=np.array([[0, 1 << 31, 0xffffffff]], u32), es=0.9,
                      status=[1])
    c["m = 3"] = dict(P=TRI, Q=TRI, src=ids3, dst=ids3, samples=np.array([[0, 1 << 31, 0xffffffff]], u32), es=0.9,
                      status=[0], pose=np.eye(4, dtype=f32).reshape(-1))
    return c


def line_scene():
    """A hypothesis whose own three pairs are NOT inliers (the target triangle is the source's, twice as large: the best
    rigid fit is the identity, with residuals over 1), and five pairs on a line that are: an inlier set that cannot be
    refitted."""
    tri = np.array([[2, 0, 0], [-1, 1, 0], [-1, -1, 0]], f32)
    on_line = np.array([[0.25 * k, 5, 1] for k in range(5)], f32)
    P = np.concatenate([tri, on_line])
    Q = np.concatenate([2 * tri, on_line])
    ids = np.arange(8, dtype=np.int64)
    return dict(P=P, Q=Q, src=ids, dst=ids, samples=words([[0, 1, 2]], 8), es=0.0, max_dist_sq=1e-4)


def lower_refit_scene():
    """An exact hypothesis (identity, seven inliers) and four more pairs of one and the same source point, one moved
    0.0099 along -x and three along +x: no rigid motion serves both, the refit over the seven moves that point towards
    +x and loses the pair on the other side: the refined count is 6 < 7 and the hypothesis's pose is kept."""
    P = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, 0], [1, 1, 0], [1, 1, 0], [1, 1, 0]], f32)
    Q = P.copy()
    Q[3, 0] -= f32(0.0099)
    Q[4:, 0] += f32(0.0099)
    ids = np.arange(7, dtype=np.int64)
    return dict(P=P, Q=Q, src=ids, dst=ids, samples=words([[0, 1, 2]], 7), es=0.9, max_dist_sq=1e-4)


@functools.lru_cache(maxsize=None)
def scene_m_reference(es=0.9):
    """scene M and the oracle's whole answer on it (computed once per process, shared, never changed)"""
    s = PO.scene_m()
    r = PO.estimate(s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], es, True)
    for v in list(s.values()) + [x for x in r.values() if isinstance(x, np.ndarray)]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s, r


def test_sample_index():
    assert PO.sample_index(np.array([0, 1, 0x7fffffff, 0x80000000, 0xffffffff], u32), 3).tolist() == [0, 0, 1, 1, 2]
    assert PO.sample_index(np.array([0xffffffff], u32), 2 ** 31 - 1).tolist() == [2 ** 31 - 2]
    for m in (3, 7, 1500):
        for i in (0, 1, m - 1):
            assert PO.sample_index(np.array([word_for(i, m)], u32), m)[0] == i
            assert i == 0 or PO.sample_index(np.array([word_for(i, m) - 1], u32), m)[0] == i - 1


def test_hand_cases():
    for name, c in hand_cases().items():
        st, poses, _ = PO.hypotheses(c["P"], c["Q"], c["src"], c["dst"], c["samples"], c["es"])
        assert st.tolist() == c["status"], name
        assert not poses[st != 0].any(), name
        if "pose" in c:
            assert PO.pose_close(poses[0], c["pose"])[0], (name, poses[0])
            assert poses[0][[3, 7, 11, 15]].tolist() == [0, 0, 0, 1]


def test_triangle_boundary():
    """sin^2 on either side of 1e-12"""
    for h, deg in ((0.9e-6, True), (1.1e-6, False)):
        X = np.array([[0, 0, 0], [1, 0, 0], [1, h, 0]], f32)
        assert bool(PO.triangle_degenerate(X)) is deg


def test_out_of_range_ids():
    ids = np.arange(4, dtype=np.int64)
    P = np.concatenate([TRI, [[5, 5, 5]]]).astype(f32)
    for bad_src, bad_dst in ((-1, 3), (4, 3), (3, -1), (3, 4)):
        src, dst = ids.copy(), ids.copy()
        src[3], dst[3] = bad_src, bad_dst
        st, _, _ = PO.hypotheses(P, P, src, dst, words([[0, 1, 2], [0, 1, 3]], 4), 0.9)
        assert st.tolist() == [0, 1]
        r = PO.estimate(P, P, src, dst, words([[0, 1, 2], [0, 1, 3]], 4), 1e-4, 0.9, False)
        assert r["counts"].tolist() == [3, 0] and r["inliers"].tolist() == [0, 1, 2]


def test_strict_less_than():
    """DistSq < max_dist_sq, not <=: a pair exactly 0.5 off under the identity has DistSq = 0.25"""
    P = np.concatenate([TRI, [[3, 3, 3]]]).astype(f32)
    Q = P.copy()
    Q[3, 2] += f32(0.5)
    ids = np.arange(4, dtype=np.int64)
    for mds, n in ((0.25, 3), (float(np.nextafter(f32(0.25), f32(1))), 4)):
        r = PO.estimate(P, Q, ids, ids, words([[0, 1, 2]], 4), mds, 0.9, False)
        assert r["best_count"] == n and r["found"]


def test_line_inliers_are_not_refitted():
    s = line_scene()
    r = PO.estimate(s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], s["es"], True)
    assert r["status"].tolist() == [0] and r["found"] and r["best_count"] == 5
    assert r["inliers"].tolist() == [3, 4, 5, 6, 7] and r["refit_pose"] is None and not r["refined"]
    A, B, _ = PO.pair_points(s["P"], s["Q"], s["src"], s["dst"])
    assert PO.refit(A, B, np.array([3, 4])) is None  # fewer than three
    assert PO.refit(A, B, np.array([0, 3, 4])) is not None


def test_lower_refit_keeps_the_hypothesis():
    s = lower_refit_scene()
    r = PO.estimate(s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], s["es"], True)
    assert r["found"] and r["best_count"] == 7 and r["refit_pose"] is not None and not r["refined"]
    A, B, _ = PO.pair_points(s["P"], s["Q"], s["src"], s["dst"])
    assert PO.inlier_mask(r["refit_pose"], A, B, s["max_dist_sq"]).sum() == 6
    assert np.array_equal(r["pose"], r["poses"][0]) and r["inliers"].tolist() == list(range(7))


def test_scene_m_is_decisive():
    s, r = scene_m_reference()
    true = s["dst"] == s["src"]
    n_true = int(true.sum())
    st = r["status"]
    print("scene M: %d true pairs of %d; status counts %s; best %d with count %d, reached by %d hypotheses"
          % (n_true, len(true), np.bincount(st, minlength=4).tolist(), r["best"], r["best_count"],
             int((r["counts"] == r["best_count"]).sum())))
    assert 800 < n_true < 1000
    assert all((st == k).any() for k in (0, 1, 2, 3))  # every status occurs
    A, B, _ = PO.pair_points(s["P"], s["Q"], s["src"], s["dst"])
    # the best count: the true pairs plus whatever the oracle itself counts among the wrong ones
    mask = PO.inlier_mask(r["poses"][r["best"]], A, B, s["max_dist_sq"])
    assert mask[true].all() and r["best_count"] == n_true + int(mask[~true].sum()) and r["found"]
    assert r["best"] == int(np.nonzero((st == 0) & (r["counts"] == r["counts"].max()))[0][0])
    # the best pose maps every true pair within max_dist
    d = np.sqrt(PO.dist_sq(r["poses"][r["best"]], A[true], B[true]).astype(f64))
    assert d.max() < s["max_dist"]
    # the hypotheses the pose comparisons leave out are few
    well = PO.well_conditioned(s["P"], s["Q"], s["src"], s["dst"], r["idx"])
    ok = st == 0
    assert (ok & ~well).sum() <= 0.05 * ok.sum()
    print("scene M: %d of %d status-0 hypotheses have sin^2 < 1e-4 (%.2f %%)"
          % ((ok & ~well).sum(), ok.sum(), 100.0 * (ok & ~well).sum() / ok.sum()))
    # the refit over the best's inliers is kept, and still maps every true pair within max_dist
    assert r["refined"] and len(r["inliers"]) >= r["best_count"]
    assert np.sqrt(PO.dist_sq(r["pose"], A[true], B[true]).astype(f64)).max() < s["max_dist"]
