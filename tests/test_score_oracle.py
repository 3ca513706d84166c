"""tests/score_oracle.py, the NumPy restatement of "score poses" and pcgx_pose_select (include/pcgx.h), on cases worked by
hand and on the decoy scene: a wrong pose that collects more correspondences than the right one, which the whole clouds
tell apart.  The GPU tests (tests/test_gpu_score_poses.py) compare the library with it.  No GPU, no library."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_oracle as PO  # noqa: E402
import score_oracle as SO  # noqa: E402

f32, f64 = np.float32, np.float64
EYE = np.eye(4, dtype=f32).reshape(-1)


@functools.lru_cache(maxsize=None)
def decoy_reference():
    """the decoy scene, the estimator's oracle on it and the whole-cloud scores of its four hypotheses (computed once per
    process, shared, never changed)"""
    s = SO.decoy_scene()
    est = PO.estimate(s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], s["es"], True)
    sc = SO.score(s["Q"], s["P"], est["poses"], s["max_dist"])
    for r in (est, sc):
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return s, est, sc


@functools.lru_cache(maxsize=None)
def main_reference(max_dist=0.02):
    """the main scene of the GPU tests (tree over the decoy scene's Q, source P, six poses) by brute force"""
    s = SO.decoy_scene()
    poses = SO.main_poses()
    r = SO.score(s["Q"], s["P"], poses, max_dist)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def test_dead_and_live():
    assert not SO.pose_live(np.zeros(16, f32))
    z = np.zeros(16, f32)
    z[3] = -0.0
    assert not SO.pose_live(z)
    z[7] = np.nan
    assert SO.pose_live(z)
    assert SO.pose_live(EYE)


def test_hand_scores():
    T = np.array([[0, 0, 0], [10, 0, 0]], f32)
    P = np.array([[0.5, 0, 0], [9, 0, 0], [5, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]], f32)
    shift = EYE.copy()
    shift[12] = 0.25
    r = SO.score(T, P, np.stack([EYE, np.zeros(16, f32), shift]), 1.5)
    assert r["counts"].tolist() == [2, 0, 2] and r["fragile"].tolist() == [0, 0, 0]
    assert r["sums"].tolist() == [0.25 + 1.0, 0.0, 0.5625 + 0.5625]
    assert r["best"] == 0 and r["n_live"] == 2 and np.array_equal(r["pose"], EYE)
    # strictly below max_dist^2: a pair exactly at the distance is not found, and is reported
    r = SO.score(T, P[:2], EYE[None], 1.0)
    assert r["counts"].tolist() == [1] and r["fragile"].tolist() == [1]
    # no live pose; no pose; no point; no tree point
    r = SO.score(T, P, np.zeros((2, 16), f32), 1.0)
    assert r["best"] == -1 and not r["pose"].any() and r["counts"].tolist() == [0, 0]
    assert SO.score(T, P, np.zeros((0, 16), f32), 1.0)["best"] == -1
    r = SO.score(T, P[:0], EYE[None], 1.0)
    assert r["best"] == 0 and r["counts"].tolist() == [0]
    assert SO.score(T[:0], P, EYE[None], 1.0)["counts"].tolist() == [0]
    # equal counts: the smaller k
    assert SO.score(T, P, np.stack([np.zeros(16, f32), shift, EYE]), 1.5)["best"] == 1


def test_hand_selection():
    status = np.array([0, 0, 1, 0, 0, 0], np.int32)
    counts = np.array([5, 9, 50, 9, 2, 3], np.int64)
    poses = np.arange(96, dtype=f32).reshape(6, 16) + 1
    ids, out, n = SO.select(status, counts, poses, 3)
    assert ids.tolist() == [1, 3, 0] and n == 3 and np.array_equal(out, poses[[1, 3, 0]])
    ids, out, n = SO.select(status, counts, poses, 6)
    assert ids.tolist() == [1, 3, 0, 5, -1, -1] and n == 4 and not out[4:].any()
    ids, out, n = SO.select(status, counts, poses, 0)
    assert len(ids) == 0 and n == 0
    ids, out, n = SO.select(status[:0], counts[:0], poses[:0], 2)
    assert ids.tolist() == [-1, -1] and n == 0


def test_decoy_scene_is_pinned():
    s, est, sc = decoy_reference()
    assert len(s["Q"]) == 3014 and len(s["pairs"]) == 24
    assert est["status"].tolist() == [0, 0, 0, 0]
    assert est["counts"].tolist() == [14, 10, 14, 10]
    assert est["best"] == 0 and est["best_count"] == 14 and est["found"] and est["refined"]
    assert len(est["inliers"]) == 14
    ids, _, n = SO.select(est["status"], est["counts"], est["poses"], 4)
    assert ids.tolist() == [0, 2, 1, 3] and n == 4
    print("decoy scene: whole-cloud counts %s, fragile %s" % (sc["counts"].tolist(), sc["fragile"].tolist()))
    assert sc["counts"][1] == 3000 and sc["counts"][3] == 3000
    assert sc["counts"][0] < 300 and sc["counts"][2] < 300
    assert not sc["fragile"].any()
    assert sc["best"] == 1
    # in selection order the verified best is slot 2
    sel = SO.score(s["Q"], s["P"], est["poses"][ids], s["max_dist"])
    assert sel["best"] == 2 and sel["counts"][2] == 3000


def test_decoy_pose_by_float64_brute_force():
    """105 of the 3000 points of P lie within 0.02 of Q under the decoy pose W itself, in float64"""
    s = SO.decoy_scene()
    W = s["W"].astype(f64).reshape(4, 4).T
    X = s["P"].astype(f64) @ W[:3, :3].T + W[:3, 3]
    Q = s["Q"].astype(f64)
    d2 = np.min(((X[:, None, :] - Q[None, :, :]) ** 2).sum(axis=2), axis=1)
    assert int((d2 < 0.02 ** 2).sum()) == 105


def test_main_scene_has_no_fragile_pair():
    for md in (0.02, 10.0):
        r = main_reference(md)
        print("main scene, max_dist %g: counts %s sums %s" % (md, r["counts"].tolist(), r["sums"].tolist()))
        assert not r["fragile"].any()
        assert r["counts"][4] == 0 and r["counts"][5] == 0 and r["n_live"] == 5
    r = main_reference(0.02)
    assert r["counts"][0] == 3000 and r["counts"][1] < 300 and r["counts"][2] == 0 and r["counts"][3] == 3000
    assert r["sums"][3] > 0 and r["best"] == 0
