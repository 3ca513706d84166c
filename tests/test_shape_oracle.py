"""The NumPy oracle of cylinder and sphere segmentation (tests/shape_oracle.py) on cases small enough to write down, and
on the yard (tests/shape_scenes.py): it finds what the scene holds, then a round that finds none, with a wide gap about
min_inliers; and the refit's derived tolerance is one float32 ulp there."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_oracle as SO  # noqa: E402
import shape_scenes as SC  # noqa: E402

f32, f64 = np.float32, np.float64
S2 = float(np.sqrt(0.5))


def test_two_points_give_the_unit_sphere_and_cylinder_exactly():
    st, rec = SO.hypothesis(SO.SPHERE, True, (1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 1, 0))
    assert st == SO.OK and rec.tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    st, rec = SO.hypothesis(SO.SPHERE, True, (3, 2, 5), (2, 0, 0), (2, 2, 6), (0, 0, -0.5))  # normals of any length or sign
    assert st == SO.OK and rec.tolist() == [2, 2, 5, 1, 0, 0, 0, 0]
    st, rec = SO.hypothesis(SO.CYLINDER, True, (1, 0, 0), (1, 0, 0), (0, 1, 0.5), (0, 1, 0))
    assert st == SO.OK and rec.tolist() == [0, 0, 0, 1, 0, 0, 1, 0]
    # the axis through (2, 3, z): q is its point nearest the origin, (2, 3, 0); a turned so that its lead is positive
    st, rec = SO.hypothesis(SO.CYLINDER, True, (2, 4, 7), (0, 1, 0), (3, 3, -4), (1, 0, 0))
    assert st == SO.OK and rec.tolist() == [2, 3, 0, 1, 0, 0, 1, 0]
    st, rec = SO.hypothesis(SO.CYLINDER, True, (2, 4, 7), (0, 1, 0), (3, 3, -4), (1, 0, 0), SO.Axis((0, 0, -1), 0.9))
    assert st == SO.OK and rec.tolist() == [2, 3, 0, 1, 0, 0, -1, 0]
    assert SO.hypothesis(SO.SPHERE, False, (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0))[0] == SO.NO_PARTNER


def test_parallel_normals_axis_and_radius_at_equality():
    for kind in (SO.SPHERE, SO.CYLINDER):
        for n1 in ((1, 0, 0), (-2, 0, 0), (1, 1e-7, 0)):
            st, rec = SO.hypothesis(kind, True, (1, 0, 0), (1, 0, 0), (0, 1, 0), n1)
            assert st == SO.DEGENERATE and np.all(rec == 0)
        assert SO.hypothesis(kind, True, (1, 0, 0), (1, 0, 0), (0, 1, 0), (np.nan, 1, 0))[0] == SO.DEGENERATE
        # r == 1 exactly: inside [1, 1], [1, 2] and [0.5, 1]; outside the next float32 either way
        up, dn = float(np.nextafter(f32(1), f32(2))), float(np.nextafter(f32(1), f32(0)))
        for lo, hi, want in ((1, 1, SO.OK), (1, 2, SO.OK), (0.5, 1, SO.OK), (up, 2, SO.RADIUS), (0, dn, SO.RADIUS),
                             (0, np.inf, SO.OK)):
            assert SO.hypothesis(kind, True, (1, 0, 0), (1, 0, 0), (0, 1, 0.5 * kind), (0, 1, 0), None, lo, hi)[0] == want
    # the axis test at equality: a = z, |a . (0, 3, 4)| = 4 = 0.8 * 5 with the float64 0.8 ... the bound is the float32's
    pair = ((1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 1, 0))
    assert SO.hypothesis(SO.CYLINDER, True, *pair, SO.Axis((0, 3, 4), 0.5))[0] == SO.OK
    assert SO.hypothesis(SO.CYLINDER, True, *pair, SO.Axis((0, 4, 3), 0.75))[0] == SO.AXIS      # 3 < 3.75
    assert SO.hypothesis(SO.CYLINDER, True, *pair, SO.Axis((0, 4, 3), 0.5))[0] == SO.OK        # 3 >= 2.5
    assert SO.hypothesis(SO.CYLINDER, True, *pair, SO.Axis((0, 0, 8), 1.0))[0] == SO.OK        # 8 >= 8: equality holds
    assert SO.hypothesis(SO.CYLINDER, True, *pair, SO.Axis((0, 3, 4), 0.8))[0] == SO.AXIS      # 4 < float32(0.8) * 5
    assert SO.hypothesis(SO.CYLINDER, True, *pair, SO.Axis((3, 0, 0), 0.0))[0] == SO.OK        # 0 >= 0
    assert SO.hypothesis(SO.SPHERE, True, *pair, SO.Axis((3, 0, 0), 1.0))[0] == SO.OK          # a sphere has no axis


def test_the_band_is_strict_and_lo_may_be_negative():
    rec = np.array([0, 0, 0, 1, 0, 0, 1, 0], f32)
    M = np.tile([1.0, 0, 0], (6, 1)).astype(f32)
    for kind in (SO.SPHERE, SO.CYLINDER):
        # max_dist 0.25: lo2 = 0.5625 and hi2 = 1.5625 exactly, reached exactly at x = 0.75 and 1.25
        lo2, hi2 = SO.band(1.0, 0.25)
        assert (float(lo2), float(hi2)) == (0.5625, 1.5625)
        x = np.array([0.75, np.nextafter(f32(0.75), f32(1)), 1.0, np.nextafter(f32(1.25), f32(1)), 1.25, np.nan], f32)
        P = np.column_stack([x, np.zeros(6), np.zeros(6)]).astype(f32)  # (z = 0: along the axis d2 would round)
        assert SO.inlier_mask(kind, rec, P, 0.25, M).tolist() == [False, True, True, True, False, False]
        # lo <= 0: lo2 = -1, the centre itself (d2 == 0) is an inlier; lo == 0 exactly is lo <= 0
        for md in (1.0, 1.5):
            lo2, hi2 = SO.band(1.0, md)
            assert float(lo2) == -1.0
            P0 = np.array([[0, 0, 4 * kind], [1 + md, 0, 0], [np.nextafter(f32(1 + md), f32(0)), 0, 0]], f32)
            assert SO.inlier_mask(kind, rec, P0, md, M[:3]).tolist() == [True, False, True]
    # the normal test: g g >= c2 d2, with d2 == 0 any normal agrees; a NaN normal never does
    P = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]], f32)
    Mn = np.array([[S2, S2, 0], [0.5, 0.8660254, 0], [np.nan, 0, 0], [0, 1, 0]], f32)
    assert SO.inlier_mask(SO.SPHERE, rec, P, 1.5, Mn, 0.7).tolist() == [True, False, False, True]
    assert SO.inlier_mask(SO.SPHERE, rec, P, 1.5, Mn, 0.0).tolist() == [True, True, True, True]
    # the cylinder takes the axis' part out of both: a normal along the axis agrees with nothing
    Pc = np.array([[1, 0, 5], [1, 0, 5]], f32)
    Mc = np.array([[0, 0, 1], [S2, 0, S2]], f32)
    assert SO.inlier_mask(SO.CYLINDER, rec, Pc, 0.25, Mc, 0.5).tolist() == [False, True]


def test_partner_rule_on_a_hand_made_neighbourhood():
    # ids 0..5 on a line; the seed is id 1, radius 2.5: Range's set is {0, 1, 2, 3} (3 is at distance 2 < 2.5, 4 at 3)
    P = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [1, 2.5, 0]], f32)
    assert np.flatnonzero(SO.range_set(P, P[1], 2.5)).tolist() == [0, 1, 2, 3]  # the bound is strict: id 5 is at 2.5
    for u1 in (0, 1, 77, 0xdeadbeef, 0xffffffff):
        x = {i: int(SO.mix(u1, [i])[0]) for i in range(6)}
        assert SO.partner(u1, [0, 2, 3]) == min((0, 2, 3), key=lambda i: (x[i], i))
        assert SO.partner(u1, [0, 3]) == min((0, 3), key=lambda i: (x[i], i))  # id 2 taken by an earlier round
        assert SO.partner(u1, [3, 0, 2]) == SO.partner(u1, [2, 0, 3])          # a property of the set
    assert SO.partner(5, []) == -1
    assert int(SO.mix(1, [0])[0]) == 0x514E28B7  # fmix32(1)
    # in segment: the seed itself and a deleted point are no candidates; a seed alone in its radius has no partner
    M = np.tile([0.0, 1.0, 0.0], (6, 1)).astype(f32)
    M[::2] = (1, 0, 0)
    deleted = np.zeros(6, bool)
    deleted[2] = True
    w = np.array([[SC.word_for(k, 5), 9] for k in range(5)], np.uint32)  # R = 5 live points: seeds 0, 1, 3, 4, 5
    r = SO.segment(P, M, SO.SPHERE, w, 0.5, 5, sample_radius=1.2, deleted=deleted)
    assert r.partners[0].tolist() == [1, 0, 4, 3, -1] and r.status[0, 4] == SO.NO_PARTNER
    x = {i: int(SO.mix(9, [i])[0]) for i in range(6)}
    r = SO.segment(P, M, SO.SPHERE, w, 0.5, 5, sample_radius=2.2, deleted=deleted)
    assert r.partners[0, 1] == min((0, 3), key=lambda i: (x[i], i)) and r.partners[0, 4] == -1
    # sample_radius 0: the second word names the partner among all that is left; the seed again is status 1
    w0 = np.array([[SC.word_for(0, 5), SC.word_for(3, 5)], [SC.word_for(2, 5), SC.word_for(2, 5)]], np.uint32)
    r = SO.segment(P, M, SO.SPHERE, w0, 0.5, 2, deleted=deleted)
    assert r.partners[0].tolist() == [4, -1] and r.status[0, 1] == SO.NO_PARTNER


@pytest.mark.parametrize("kind", (SO.SPHERE, SO.CYLINDER))
def test_both_outcomes_of_the_refit(kind):
    P, M, w = SC.refit_loses(kind)
    off = SO.segment(P, M, kind, w, 0.02, 1, refine=False)
    on = SO.segment(P, M, kind, w, 0.02, 1, refine=True)
    unit = [0, 0, 0, 1, 0, 0, kind, 0]
    assert off.sizes.tolist() == [13] and off.shapes[0].tolist() == unit and np.array_equal(off.ids, np.arange(13))
    f = on.refits[0]
    assert f.ok and 1.005 < f.rec[3] < 1.019 and SO.inlier_mask(kind, f.rec, P, 0.02, M).sum() == 12  # the low one is lost
    assert on.refined.tolist() == [0] and on.sizes.tolist() == [13] and on.shapes[0].tolist() == unit
    Q, M, w = SC.refit_loses(kind, low=1.019)
    on = SO.segment(Q, M, kind, w, 0.02, 1, refine=True)
    assert on.refined.tolist() == [1] and on.sizes.tolist() == [13] and 1.01 < on.shapes[0, 3] < 1.019
    assert np.array_equal(on.shapes[0], on.refits[0].rec) and on.shapes[0, 4:].tolist() == unit[4:]
    if kind == SO.CYLINDER:
        assert abs(float(on.shapes[0, :3].astype(f64) @ on.shapes[0, 4:7].astype(f64))) < 1e-7  # q canonical again
    # no refit: every inlier the same point (a pivot of the factorisation is 0), the radius window, and k + |u|^2 <= 0
    assert not SO.refit(kind, unit, np.tile([1.0, 0, 0], (5, 1))).ok
    assert SO.refit(kind, unit, Q[:13]).ok and not SO.refit(kind, unit, Q[:13], 0.0, 1.0).ok
    assert not SO.refit_from_sums(kind, np.array(unit, f32), 4, [0, 0, 0, 1, 0, 0, 1, 0, 1 - kind, 0, 0, 0, -4.0])[0]


@pytest.mark.parametrize("n_hyp", [128, 256])
@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("call", sorted(SC.CALLS))
def test_yard_finds_what_it_holds_and_stops(call, refine, n_hyp):
    P, M, part = SC.yard()
    kind, kw, want = SC.CALLS[call]
    for seed in SC.SEEDS:
        r = SO.segment(P, M, kind, SC.samples(n_hyp, 5, seed), n_hyp=n_hyp, max_shapes=5, refine=refine, **SC.YARD, **kw)
        assert r.n_shapes == len(want), (seed, r.sizes)
        # a wide gap about min_inliers = 600: every shape found has over 800 inliers, the round after fewer than 550
        assert r.sizes[:r.n_shapes].min() > 800 and r.counts[r.n_shapes].max() < 550, (seed, r.sizes, r.counts[r.n_shapes].max())
        assert np.all(r.status[r.n_shapes + 1:] == -1) and np.all(r.sizes[r.n_shapes:] == 0)
        found = [int(np.bincount(part[g], minlength=6).argmax()) for g in np.split(r.ids, np.cumsum(r.sizes[:r.n_shapes])[:-1])]
        assert sorted(found) == sorted(want), (seed, found)
        for g, k in zip(np.split(r.ids, np.cumsum(r.sizes[:r.n_shapes])[:-1]), found):
            assert (part[g] == k).mean() > 0.97  # the shape's own points
        for f in r.refits:
            if refine:
                # the derived tolerance: the term of the sums' order lies below one float32 ulp at the record's scale
                assert f.ok and f.n * f.kappa * 2.0 ** -52 * np.abs(f.rec[:4]).max() < np.spacing(f32(np.abs(f.rec[:4]).max()))
                assert f.tol == np.spacing(f32(np.abs(f.rec[:4]).max()))
