"""The float64 normal-estimation oracle (tests/normals_oracle.py) on analytic cases: it is the contract the GPU
kernels (csrc/normals.hip) are compared with, so it is pinned here first."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_oracle as NO  # noqa: E402


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _plane(n=2000, z=0.5, seed=0):
    xy = _rng(seed).random((n, 2)).astype(np.float32)
    return np.ascontiguousarray(np.column_stack([xy, np.full(n, z, np.float32)]), dtype=np.float32)


def test_plane_gives_ez_and_zero_curvature():
    p = _plane()
    q = p[:50]
    o = NO.normals(p, q, 0.1, viewpoint=(0.5, 0.5, 10.0))
    assert not o["degenerate"].any()
    assert np.all(o["counts"] >= 3)
    assert np.array_equal(o["normals"], np.tile(np.float32([0, 0, 1]), (50, 1)))
    assert np.all(np.abs(o["curvature"]) <= 1e-12)


def test_orientation_follows_the_viewpoint():
    p = _plane()
    q = p[:50]
    up = NO.normals(p, q, 0.1, viewpoint=(0.5, 0.5, 10.0))["normals"]
    down = NO.normals(p, q, 0.1, viewpoint=(0.5, 0.5, -10.0))["normals"]
    assert np.array_equal(up, -down)
    # the default viewpoint is the origin, below the plane z = 0.5
    assert np.array_equal(NO.normals(p, q, 0.1)["normals"], down)


def test_sphere_gives_radial_normals():
    u = _rng(1).normal(size=(20000, 3))
    p = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    q = p[:100]
    o = NO.normals(p, q, 0.15)  # viewpoint at the centre: the normals point inwards
    assert not o["degenerate"].any()
    cosang = np.sum(o["normals"].astype(np.float64) * -q.astype(np.float64), axis=1) / np.linalg.norm(q, axis=1)
    assert np.all(cosang > np.cos(np.radians(3.0))), np.degrees(np.arccos(cosang.min()))
    assert np.all((o["curvature"] > 0) & (o["curvature"] < 0.05))


def test_queries_off_the_cloud_and_tree_points_count_themselves():
    p = _plane(200)
    o = NO.normals(p, np.float32([[5, 5, 5], p[3]]), 0.05)
    assert o["counts"][0] == 0 and o["degenerate"][0]
    offs, ids = NO.brute_force_lists(p, p[3:4], 0.05)
    assert 3 in ids


def test_min_neighbors():
    p = np.float32([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [0.01, 0.01, 0.001], [0.005, 0.002, 0]])
    q = np.float32([[0.004, 0.004, 0]])
    o = NO.normals(p, q, 0.1, min_neighbors=5)
    assert o["counts"][0] == 5 and not o["degenerate"][0]
    o = NO.normals(p, q, 0.1, min_neighbors=6)
    assert o["counts"][0] == 5 and o["degenerate"][0]
    assert np.array_equal(o["normals"][0], np.zeros(3, np.float32)) and np.isnan(o["curvature"][0])
    # below 3 counts as 3: two neighbours are never enough
    o = NO.normals(p[:2], q, 0.1, min_neighbors=0)
    assert o["counts"][0] == 2 and o["degenerate"][0] and np.isnan(o["curvature"][0])


def test_all_coincident_is_degenerate():
    p = np.tile(np.float32([[0.3, 0.2, 0.1]]), (50, 1))
    for q in (p[:1], np.float32([[0.31, 0.2, 0.1]])):  # on the heap and beside it
        o = NO.normals(p, q, 0.1)
        assert o["counts"][0] == 50 and o["degenerate"][0]
        assert np.array_equal(o["normals"][0], np.zeros(3, np.float32)) and np.isnan(o["curvature"][0])


def test_collinear_gives_a_perpendicular_unit_normal():
    t = np.linspace(0, 1, 101, dtype=np.float32)
    d = np.float32([1, 2, 2]) / np.float32(3)
    p = np.ascontiguousarray(t[:, None] * d[None, :], dtype=np.float32)
    o = NO.normals(p, p[40:60], 0.1, viewpoint=(0, 0, 5))
    assert not o["degenerate"].any()
    n = o["normals"].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    assert np.all(np.abs(n @ d.astype(np.float64)) < 1e-6)
    assert np.all(np.abs(o["curvature"]) < 1e-6)
    assert np.all(n @ np.array([0, 0, 5.0]) - np.sum(n * p[40:60], axis=1) >= 0)  # towards the viewpoint


def test_range_lists_and_brute_force_agree_on_counts_shape():
    p = _plane(500, seed=3)
    offs, ids = NO.brute_force_lists(p, p[:20], 0.1)
    o = NO.normals_from_lists(p, p[:20], offs, ids, chunk=64)  # chunked: several passes
    o2 = NO.normals(p, p[:20], 0.1)
    assert np.array_equal(o["counts"], o2["counts"]) and np.array_equal(o["normals"], o2["normals"])
