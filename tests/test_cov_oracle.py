"""The float64 covariance oracle (tests/cov_oracle.py) on analytic cases: it is the contract the GPU kernel
(csrc/knearest.hip, covariance mode) is compared with, so it is pinned here first."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_oracle as CO  # noqa: E402
import knn_oracle as KO  # noqa: E402


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def test_plane_points_give_the_plane_covariance():
    """points on a tilted plane: PLANE = I - (1 - eps) n n^T with n the plane's normal, turned to the viewpoint"""
    r = _rng(0)
    nrm = np.array([1.0, -2.0, 2.0]) / 3.0
    e1 = np.array([2.0, 1.0, 0.0]) / np.sqrt(5.0)
    e2 = np.cross(nrm, e1)
    ab = r.random((3000, 2))
    pts = (ab[:, :1] * e1 + ab[:, 1:] * e2).astype(np.float32)
    q = pts[:200]
    ids, _, counts = KO.knearest(pts, q, 16, np.inf)
    for eps in (1e-3, 0.5, 1.0):
        o = CO.covariances(pts, q, ids, counts, CO.PLANE, eps, viewpoint=(0.0, 0.0, 10.0))
        assert not o["degenerate"].any()
        f = 1.0 - float(np.float32(eps))
        want = np.eye(3) - f * np.outer(nrm, nrm)
        want6 = np.array([want[i, j] for i, j in CO.UPPER])
        # (the float32 points lie on the plane to ~1e-8: their covariance's smallest eigenvector to about as much)
        assert np.max(np.abs(o["cov6"] - want6[None, :])) <= 1e-6
        assert np.max(np.abs(o["normals"] - nrm[None, :])) <= 1e-6  # nrm . (v - q) > 0 for every q here


def test_raw_is_the_biased_covariance_of_the_knn_list():
    r = _rng(1)
    pts = r.random((2000, 3)).astype(np.float32)
    q = r.random((50, 3)).astype(np.float32)
    ids, _, counts = KO.knearest(pts, q, 20, np.inf)
    o = CO.covariances(pts, q, ids, counts, CO.RAW)
    for j in range(len(q)):
        want = np.cov(pts[ids[j]].astype(np.float64).T, bias=True)
        got = np.array([[o["cov6"][j][CO.UPPER.index((min(a, b), max(a, b)))] for b in range(3)] for a in range(3)])
        assert np.allclose(got, want, rtol=0, atol=1e-12 * np.trace(want))
    assert np.allclose(o["trace"], [np.trace(np.cov(pts[i].T.astype(np.float64), bias=True)) for i in ids])


def test_degenerate_neighbourhoods():
    pts = np.concatenate([np.tile(np.float32([[0.3, 0.2, 0.1]]), (50, 1)), np.float32([[5, 5, 5], [5, 6, 5]])])
    q = np.float32([[0.3, 0.2, 0.1], [0.31, 0.2, 0.1], [5, 5.5, 5], [50, 50, 50]])
    ids, _, counts = KO.knearest(pts, q, 8, 2.0)
    assert counts.tolist() == [8, 8, 2, 0]  # a heap, beside the heap, two neighbours, none
    for mode, diag in ((CO.PLANE, 1.0), (CO.RAW, 0.0)):
        o = CO.covariances(pts, q, ids, counts, mode)
        assert o["degenerate"].all()
        assert np.array_equal(o["cov6"], np.tile([diag, 0, 0, diag, 0, diag], (4, 1)))
        assert np.array_equal(o["normals"], np.zeros((4, 3)))
