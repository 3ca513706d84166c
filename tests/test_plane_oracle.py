"""The NumPy restatement of pcgx_kdtree_planes' contract (tests/plane_oracle.py) on cases small enough to write down, and
on the room the GPU tests use: it finds four planes there and stops."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_oracle as PO  # noqa: E402
import plane_scenes as SC  # noqa: E402

f32 = np.float32


def test_three_points():
    P = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], f32)
    r = PO.segment(P, SC.words([(0, 1, 2), (2, 1, 0), (1, 1, 2)], 3), 0.01, 3, refine=False)
    assert r.n_planes == 1 and r.status[0].tolist() == [0, 0, 1] and r.counts[0].tolist() == [3, 3, 0]
    assert r.hyp_planes[0, 0].tolist() == [0, 0, 1, -1] and r.hyp_planes[0, 1].tolist() == [0, 0, 1, -1]  # either winding
    assert r.best.tolist() == [0] and r.sizes.tolist() == [3] and r.labels.tolist() == [0, 0, 0] and r.ids.tolist() == [0, 1, 2]
    # two points, or two rounds over three: the round cannot run
    assert PO.segment(P[:2], SC.samples(4, 1, 0), 0.01, 4).status.tolist() == [[-1] * 4]
    r = PO.segment(P, np.tile(SC.words([(0, 1, 2)], 3), (2, 1)), 0.01, 1, max_planes=2, refine=False)
    assert r.n_planes == 1 and r.status.tolist() == [[0], [-1]] and r.best.tolist() == [0, -1]


def test_collinear_triple_and_min_inliers():
    P = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 1, 0]], f32)
    r = PO.segment(P, SC.words([(0, 1, 2)], 4), 0.01, 1)
    assert r.status.tolist() == [[2]] and r.n_planes == 0 and r.best.tolist() == [-1] and np.all(r.labels == -1)
    r = PO.segment(P, SC.words([(0, 1, 3)], 4), 0.01, 1, min_inliers=5)
    assert r.status.tolist() == [[0]] and r.counts.tolist() == [[4]] and r.n_planes == 0 and np.all(r.planes == 0)


def test_lattice_layer_at_max_dist_and_duplicated_triple():
    P = SC.lattice(0.125)
    tri = [(0, 9, 60), (3, 40, 21), (64, 73, 124), (3, 40, 21), (0, 64, 9)]
    r = PO.segment(P, SC.words(tri, 128), 0.125, 5, refine=False)
    assert r.status[0].tolist() == [0] * 5
    assert r.counts[0].tolist() == [64, 64, 64, 64, 44]  # a layer at exactly max_dist is not in; x = y takes |i - j| <= 1 of both
    assert r.best.tolist() == [0] and np.array_equal(r.ids, np.arange(64))
    assert r.hyp_planes[0, 0].tolist() == [0, 0, 1, 0] and r.hyp_planes[0, 2].tolist() == [0, 0, 1, -0.125]
    r = PO.segment(P, SC.words(tri[4:] + tri[1:4], 128), np.nextafter(f32(0.125), f32(1)), 4, refine=False)
    assert r.counts[0].tolist() == [44, 128, 128, 128] and r.best.tolist() == [1]  # equal counts: the smaller h


def test_both_sign_rules():
    P = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1]], f32)
    w = SC.words([(0, 2, 1)], 4)  # e1 x e2 = -x
    assert PO.segment(P, w, 0.01, 1, refine=False).planes[0].tolist() == [1, 0, 0, 0]
    assert PO.segment(P, w, 0.01, 1, refine=False, axis=(-2, 0, 0)).planes[0].tolist() == [-1, 0, 0, 0]
    assert PO.segment(P, w, 0.01, 1, refine=False, axis=(0, 3, 0)).planes[0].tolist() == [1, 0, 0, 0]  # the dot is 0
    assert PO.segment(P, w, 0.01, 1, refine=False, axis=(0, 3, 0), min_axis_cos=0.1).status.tolist() == [[3]]


def test_refinement_rules():
    P, w = SC.refit_loses()
    off = PO.segment(P, w, 0.02, 1, refine=False)
    on = PO.segment(P, w, 0.02, 1, refine=True)
    assert off.sizes.tolist() == [14] and on.sizes.tolist() == [14] and on.refined.tolist() == [0]
    assert np.array_equal(on.planes, off.planes) and on.pre_ids[0].tolist() == list(range(14))
    ok, pl = PO.refit(*PO.lstsq_frame(P)(np.arange(14)))
    assert ok and PO.inlier_mask(pl, P, 0.02).sum() == 13  # the refit loses the low point: the hypothesis is kept
    Q = P.copy()
    Q[13, 2] = 0.019  # ... and with that point on the others' side it loses nobody: the refit is kept
    on = PO.segment(Q, w, 0.02, 1, refine=True)
    assert on.refined.tolist() == [1] and on.sizes.tolist() == [14] and -0.019 < on.planes[0, 3] < -0.005
    assert not PO.refit(np.zeros(3), np.array([0, 0, 1.0]), 0.0)[0]  # the degenerate frame


@pytest.mark.parametrize("n_hyp", [128, 256])
def test_room_four_planes_then_stop(n_hyp):
    P = SC.room()
    r = PO.segment(P, SC.samples(n_hyp, 6, 11), 0.02, n_hyp, max_planes=6, min_inliers=600)
    assert r.n_planes == 4 and np.all(r.status[4] >= 0) and np.all(r.status[5] == -1)
    assert 0 < r.counts[4].max() < 200
    want = (6000, 3000, 2000, 1200)
    assert all(abs(int(s) - w) < 0.06 * w for s, w in zip(r.sizes, want)), r.sizes
    assert r.sizes[4:].tolist() == [0, 0] and r.best[4:].tolist() == [-1, -1] and np.all(r.planes[4:] == 0)
    assert len(r.ids) == r.sizes.sum() and len(np.unique(r.ids)) == len(r.ids)
    assert all(np.all(np.diff(r.ids[a:b]) > 0) for a, b in zip(np.cumsum(r.sizes) - r.sizes, np.cumsum(r.sizes)))
    assert np.array_equal(np.bincount(r.labels[r.labels >= 0], minlength=6), r.sizes)
    assert abs(abs(r.planes[0, 2]) - 1) < 1e-3 and abs(abs(r.planes[1, 0]) - 1) < 1e-3 and abs(abs(r.planes[2, 1]) - 1) < 1e-3
