"""tests/group_oracle.py, the NumPy restatement of the group geometry contract (include/pcgx.h, "group geometry"), on
cases worked by hand: two points, the eight corners of a 1 x 2 x 4 cuboid, a group of coincident points, and the list
layout (clamped sizes, the clip at cap_ids, dead slots)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_oracle as GO  # noqa: E402

f32 = np.float32


def test_two_points():
    P = f32([[1, 1, 1], [3, 1, 1]])
    S, info = GO.group_stats(P, [0, 1], [2])
    assert S.count.tolist() == [2]
    assert S.aabb[0].tolist() == [1, 1, 1, 3, 1, 1]
    assert S.centroid[0].tolist() == [2, 1, 1]
    assert S.cov[0].tolist() == [1, 0, 0, 0, 0, 0]  # ((-1)^2 + 1^2) / 2
    assert S.eig[0].tolist() == [1, 0, 0]
    assert S.axes[0, 0].tolist() == [1, 0, 0]
    assert np.allclose(S.axes[0] @ S.axes[0].T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(S.axes[0]), 1.0)
    assert np.allclose(S.obb[0], [2, 1, 1, 1, 0, 0], atol=1e-15)
    assert info["D"][0] == 2.0 and info["cov_bound"][0] == 8 * 2.0 ** -53 * 4


def test_cuboid_corners():
    P = f32([[x, y, z] for x in (0, 1) for y in (0, 2) for z in (0, 4)])
    S, _ = GO.group_stats(P, np.arange(8), [8])
    assert S.count.tolist() == [8]
    assert S.aabb[0].tolist() == [0, 0, 0, 1, 2, 4]
    assert S.centroid[0].tolist() == [0.5, 1, 2]
    assert S.cov[0].tolist() == [0.25, 0, 0, 1, 0, 4]
    assert S.eig[0].tolist() == [4, 1, 0.25]
    # axes z, y, x: axis 2 = z x y = -x keeps the frame right-handed
    assert S.axes[0].tolist() == [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]
    assert S.obb[0].tolist() == [0.5, 1, 2, 2, 1, 0.5]


def test_coincident_points():
    P = f32([[5, -2, 7], [0, 0, 0]])
    S, info = GO.group_stats(P, [0, 0, 0, 0, 0], [5])
    assert S.count.tolist() == [5]
    assert S.aabb[0].tolist() == [5, -2, 7, 5, -2, 7]
    assert S.centroid[0].tolist() == [5, -2, 7]
    assert not S.cov.any() and not S.eig.any()
    assert np.array_equal(S.axes[0], np.eye(3))
    assert S.obb[0].tolist() == [5, -2, 7, 0, 0, 0]
    assert info["D"][0] == 0.0


def test_sign_rule():
    assert GO.sign([-0.6, 0.0, 0.8]).tolist() == [-0.6, 0.0, 0.8]  # the largest component is positive already
    assert GO.sign([0.6, 0.0, -0.8]).tolist() == [-0.6, -0.0, 0.8]
    s = np.sqrt(0.5)
    assert GO.sign([-s, s, 0.0]).tolist() == [s, -s, -0.0]  # a tie: the first such component decides
    assert GO.sign([s, -s, 0.0]).tolist() == [s, -s, 0.0]


def test_layout():
    P = f32([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [4, 4, 4]])
    assert GO.live(P, [-1, 0, 2, 3, 4, 5]).tolist() == [False, True, False, False, True, False]
    assert GO.slices([2, -3, 0, 4, 1], 5, 6) == [(0, 2), (2, 2), (2, 2), (2, 6), (6, 6)]  # clamped, clipped at 6
    assert GO.slices([2, 2, 2], 1, 10) == [(0, 2), (2, 2), (2, 2)]  # groups >= G own nothing
    ids = [0, 1, -1, 2, 3, 4, 7, 4]
    S, _ = GO.group_stats(P, ids, [2, 3, 3, 1], n_groups=3, cap_ids=7)
    assert S.count.tolist() == [2, 0, 1, 0]  # {0, 1}; {-1, NaN, inf}; {4, 7, (clipped)}; beyond G
    assert S.centroid[0].tolist() == [0.5, 0, 0] and S.centroid[2].tolist() == [4, 4, 4]
    assert not S.aabb[1].any() and not S.axes[1].any() and not S.axes[3].any()
