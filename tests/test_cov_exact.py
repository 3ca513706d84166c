"""The exact covariance reference (tests/cov_exact.py) pinned before anything is compared with it: it equals the
float64 oracle (tests/cov_oracle.py) where that one is well conditioned, reproduces the analytic plane, and on a query
far from a tight neighbourhood it stays put under a permutation of the list while the float64 formula moves, by far
more than the 1e-9 of the trace tests/test_gpu_covariances.py allows it but inside the derived bound B."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_exact as CE  # noqa: E402
import cov_oracle as CO  # noqa: E402
import knn_oracle as KO  # noqa: E402


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _plane_cloud():
    r = _rng(0)
    nrm = np.array([1.0, -2.0, 2.0]) / 3.0
    e1 = np.array([2.0, 1.0, 0.0]) / np.sqrt(5.0)
    e2 = np.cross(nrm, e1)
    ab = r.random((3000, 2))
    return (ab[:, :1] * e1 + ab[:, 1:] * e2).astype(np.float32), nrm


def test_equals_the_float64_oracle_where_it_is_well_conditioned():
    r = _rng(1)
    pts = r.random((2000, 3)).astype(np.float32)
    q = r.random((50, 3)).astype(np.float32)
    plane = _plane_cloud()[0]
    for P, Q, k in ((pts, q, 20), (pts, q, 3), (pts, q, 64), (plane, plane[:200], 16)):
        ids, _, counts = KO.knearest(P, Q, k, np.inf)
        o = CO.covariances(P, Q, ids, counts, CO.RAW)
        e = CE.from_lists(P, Q, CE.knn_lists(ids, counts))
        assert not e["degenerate"].any() and np.array_equal(e["n"], counts)
        assert np.max(np.abs(o["cov6"] - e["cov6"]) / e["trace"][:, None]) <= 1e-12
        assert np.max(np.abs(o["trace"] - e["trace"]) / e["trace"]) <= 1e-12
        assert np.all(np.abs(o["cov6"] - e["cov6"]) <= e["B"][:, None])  # the float64 formula within its bound
        assert np.max(np.abs(o["lam"] / o["trace"][:, None] - e["lam"])) <= 1e-12
        assert np.all(e["S"] >= e["trace"]) and np.allclose(e["lam"].sum(1), 1.0, rtol=0, atol=1e-14)


def test_plane_points_give_the_plane_normal():
    """tests/test_cov_oracle.py's analytic case: the float32 points lie on the plane to ~1e-8"""
    pts, nrm = _plane_cloud()
    q = pts[:200]
    ids, _, counts = KO.knearest(pts, q, 16, np.inf)
    e = CE.from_lists(pts, q, CE.knn_lists(ids, counts))
    u = e["vec"][:, :, 0]
    u = u * np.sign(u @ nrm)[:, None]
    assert np.max(np.abs(u - nrm[None, :])) <= 1e-6
    assert np.max(e["lam"][:, 0]) <= 1e-12 and np.min(e["lam"][:, 1]) > 1e-3


def test_multiplicities_and_degenerates():
    P = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    q = np.float32([0.25, 0.5, -1.0])
    a = CE.one(np.repeat(P, [5, 1, 4097, 2], axis=0), q)
    b = CE.one(P, q, [5, 1, 4097, 2])
    assert a["n"] == b["n"] == 4105 and np.array_equal(a["cov6"], b["cov6"]) and a["S"] == b["S"]
    c = CE.from_lists(np.repeat(P, [5, 1, 4097, 2], axis=0), q[None], [np.arange(4105)])  # merged above 64
    assert np.array_equal(c["cov6"][0], a["cov6"]) and c["n"][0] == 4105
    # the unit simplex corners once each: C = I / 4 - 1 1^T / 16, exactly
    u = CE.one(P, q)
    assert np.array_equal(u["cov6"], [3 / 16, -1 / 16, -1 / 16, 3 / 16, -1 / 16, 3 / 16]) and u["trace"] == 9 / 16
    for pts in (P[:2], np.tile(P[1], (9, 1)), P[:0]):
        d = CE.one(pts, q)
        assert d["degenerate"] and d["trace"] == 0.0 and not d["cov6"].any()
    assert CE.one(P, np.float32([np.nan, 0, 0]))["degenerate"]


def test_far_query_the_float64_formula_moves_the_exact_one_does_not():
    """neighbours within 1e-3 of (1, 1, 1), the query 1e3 away: sum d d^T / n - m m^T cancels 12 digits.  The float64
    oracle is off by far more than 1e-9 of the trace and changes with the order of the list; it stays inside B, the
    bound derived for that formula, and the exact reference is the same bits in any order."""
    r = _rng(2)
    off_trace, off_B, moved = 0.0, 0.0, 0
    for _ in range(100):
        n = int(r.integers(3, 65))
        P = (1.0 + 1e-3 * r.uniform(-1, 1, (n, 3))).astype(np.float32)
        u = r.normal(size=3)
        q = (1.0 + 1e3 * u / np.linalg.norm(u)).astype(np.float32)
        e = CE.one(P, q)
        assert not e["degenerate"] and e["B"] > 1e3 * 1e-9 * e["trace"]
        ids, cnt = np.arange(n)[None, :], np.int64([n])
        o = CO.covariances(P, q[None], ids, cnt, CO.RAW)["cov6"][0]
        perm = r.permutation(n)
        o2 = CO.covariances(P[perm], q[None], ids, cnt, CO.RAW)["cov6"][0]
        e2 = CE.one(P[perm], q)
        assert np.array_equal(e2["cov6"], e["cov6"]) and e2["trace"] == e["trace"] and e2["S"] == e["S"]
        err = np.max(np.abs(o - e["cov6"]))
        off_trace = max(off_trace, err / e["trace"])
        off_B = max(off_B, err / e["B"])
        moved += not np.array_equal(o, o2)
    print("float64 oracle, far query: worst error %.3g of the trace, %.3g of B; %d of 100 moved when permuted"
          % (off_trace, off_B, moved))
    assert off_trace > 1e3 * 1e-9 and moved >= 50
    assert off_B <= 1.0
