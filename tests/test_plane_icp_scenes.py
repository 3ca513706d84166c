"""tests/plane_icp_scenes.py against the oracle alone (no GPU): every group of the scene does what it is for, the
NumPy / fsum restatement of the 30 sums agrees with oracle/plane_oracle.c, and the host's evaluate tail and Gauss-Newton
update (pcgx_icp_plane_finish_evaluate, pcgx_icp_gauss_newton_update) equal the oracle's bit for bit on the inputs the
GPU tests compare the device's update with."""
import os
import sys

import numpy as np
import pytest

import oracle as O
from pcgol_amd import icp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_icp_scenes as S  # noqa: E402

f32 = np.float32


def _dist_sq(base, p):
    """the reference's float32 expression (mat/vec3.go:18-20,38-40) from p to every base point"""
    d = base - p.astype(f32)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


@pytest.fixture(scope="module")
def sc():
    s = S.scene()
    return s, O.KDTree(s.base)


def test_the_base_and_its_normals(sc):
    s, _ = sc
    assert len(s.base) == 2977 and len(s.lattice_ids) == 576 and len(s.target) == S.N_TARGETS
    lat = s.base[s.lattice_ids]
    assert np.array_equal(lat * 16, np.round(lat * 16)) and np.abs(lat).max() < 8  # multiples of 2^-4
    n = s.normals.astype(np.float64)
    assert np.all(np.abs(np.sqrt((n * n).sum(axis=1)) - 1.0) < 1e-6)
    # unrelated to the neighbours': the mean |cos| between a point's normal and its nearest neighbour's is that of
    # random directions (1/2), not 1
    near = np.array([np.argsort(_dist_sq(s.base, s.base[i]))[1] for i in range(0, len(s.base), 37)])
    cos = np.abs((n[::37] * n[near]).sum(axis=1))
    assert 0.35 < cos.mean() < 0.65


def test_every_group_does_what_it_is_for(sc):
    s, ot = sc
    ids, dsq = np.full(len(s.target), -1, np.int64), np.full(len(s.target), np.nan, f32)
    ok = S.finite_rows(s.target)
    ids[ok], dsq[ok] = ot.nearest_batch(s.target[ok], s.max_dist)
    md2 = f32(s.max_dist) * f32(s.max_dist)
    assert md2 == f32(0.140625)
    for name in S.SPECIAL:
        assert s.mask(name).sum() >= 32, name
    for name, ways in (("tie2", 2), ("tie4", 4)):
        for i in np.flatnonzero(s.mask(name)):
            d = _dist_sq(s.base, s.target[i])
            tied = np.flatnonzero(d == d.min())
            assert len(tied) == ways and ids[i] in tied and dsq[i] == d.min() and d.min() < md2, (name, i, tied)
    lim = s.mask("limit")
    for i in np.flatnonzero(lim):
        d = _dist_sq(s.base, s.target[i])
        assert d.min() == md2 and (d == d.min()).sum() == 1  # its only candidate, at exactly MaxDist
    assert np.all(dsq[lim].view(np.uint32) == md2.view(np.uint32))  # bit for bit, paired (a leaf) or not (a pivot)
    assert 0 < (ids[lim] >= 0).sum() < lim.sum()  # the reference accepts a leaf there and not a pivot: both occur
    assert np.all(ids[s.mask("beyond", "far")] == -1)
    assert np.all(ids[s.mask("ordinary")] >= 0) and np.all(dsq[s.mask("ordinary")] < f32(0.25) * md2)
    share = (ids >= 0).mean()
    assert 0.6 <= share <= 0.9, share
    # the larger MaxDist: the far cluster pairs, and so does everything finite
    big = S.oracle_ids(ot, s.target, s.max_dist_large)
    assert np.all(big[s.mask("far")] >= 0) and np.all(big[ok] >= 0)
    # ... although it is more than 9 cells from every base point, with a margin of 2 on the cell edge the documented
    # rule gives (the GPU test repeats this with the grid's own edge)
    h = s.grid_edge_estimate()
    far = s.target[s.mask("far")]
    nearest = np.sqrt(min(_dist_sq(s.base, p).min() for p in far))
    assert nearest > 2 * 9 * h and nearest < s.max_dist_large, (nearest, h)


def test_non_finite_targets_are_the_documented_exception(sc):
    """the reference pairs a NaN target (NaN DistSq) and leaves an infinite one alone until the
    re-projection makes a NaN of it; the device pairs neither, which is what oracle_ids states."""
    s, ot = sc
    nf = s.target[s.mask("nonfinite")]
    assert not S.finite_rows(nf).any()
    has_nan = np.isnan(nf).any(axis=1)
    ids, dsq = ot.nearest_batch(nf, s.max_dist)
    # (inf - inf along one axis is a NaN distance as well)
    assert np.all(np.isnan(dsq[has_nan])) and np.all(ids[has_nan] >= 0)
    one_inf = ~has_nan & (np.isinf(nf).sum(axis=1) == 1)
    assert one_inf.sum() >= 8 and np.all(ids[one_inf] == -1)
    moved = O.mat4_transform(s.shifted(1)[1], nf)
    assert not S.finite_rows(moved).any()
    assert np.all(S.oracle_ids(ot, s.target, s.max_dist)[s.mask("nonfinite")] == -1)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_shifted_poses_project_the_special_targets_exactly(sc, k):
    s, _ = sc
    target, pose = s.shifted(k)
    assert np.array_equal(pose, O.translate(*(-np.array(S.SHIFTS[k], f32))))
    back = O.mat4_transform(pose, target)
    sp = s.dyadic()
    assert sp.sum() == 48 + 48 + 64 + 64
    assert np.array_equal(back[sp].view(np.uint32), s.target[sp].view(np.uint32))
    assert k == 0 or not np.array_equal(target[sp], s.target[sp])


def test_cuts_keep_every_group(sc):
    s, _ = sc
    for nt in (7, 63, 64, 65, 255, 4609):
        _, g = s.cut(nt)
        assert len(g) == nt and set(g.tolist()) == set(range(len(S.GROUPS)))
    assert s.cut(1)[1].tolist() == [0] and s.cut(2)[1].tolist() == [0, 1]


def test_fsum_restatement_agrees_with_the_plane_oracle(sc):
    s, ot = sc
    ok = S.finite_rows(s.target)
    for md in (s.max_dist, s.max_dist_large):
        ref = S.reference_sums(O, ot, s.base, s.normals, s.target, md)
        assert ref[2] == (ref[3] >= 0).sum() > 3000 and np.all(ref[1][:28] > 0)
        S.assert_sums(O.plane_sums(ot, s.normals, s.target[ok], md), ref, "oracle, MaxDist %g" % md)
    # the bound notices one wrong partner among the 3 800: its terms differ by far more than N 2^-53 A
    ids = ref[3].copy()
    i = np.flatnonzero(ids >= 0)[1234]
    ids[i] = (ids[i] + 1) % len(s.base)
    wrong = S.fsum30(S.pair_terms(s.base, s.normals, s.target, ids))
    with pytest.raises(AssertionError):
        S.assert_sums(wrong[0], ref)
    # ... and one pair left out
    ids = ref[3].copy()
    ids[i] = -1
    with pytest.raises(AssertionError):
        S.assert_sums(S.fsum30(S.pair_terms(s.base, s.normals, s.target, ids))[0], ref)


def test_pair_terms_are_the_oracles_float32_terms():
    """one pair at a time the 30 sums ARE the terms: bit for bit the oracle's"""
    s = S.scene()
    ot = O.KDTree(s.base)
    idx = np.flatnonzero(s.mask("ordinary", "tie4", "limit"))[:200]
    ids = S.oracle_ids(ot, s.target, s.max_dist)
    for i in idx:
        if ids[i] < 0:
            continue
        terms = S.pair_terms(s.base, s.normals, s.target[i:i + 1], ids[i:i + 1])
        assert np.array_equal(terms[0].astype(np.float64), O.plane_sums(ot, s.normals, s.target[i:i + 1], s.max_dist))


@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_host_finish_and_update_equal_the_oracle_bitwise(damping):
    """the lockstep Fit of the GPU tests on the CPU: at every iteration the host's evaluate tail and Gauss-Newton update
    give the oracle's bits from the same 30 sums"""
    f = S.fit_scene()
    ot = O.KDTree(f["base"])
    th = np.full(6, -1.0, f32)
    pose, it, changed = O.translate(0, 0, 0), 0, 0
    prev = None
    for _ in range(6):
        pts = S.project(O, pose, it, f["target"])
        sums, _, n, ids = S.reference_sums(O, ot, f["base"], f["normals"], pts, f["max_dist"])
        if prev is not None:
            changed += int(((ids != prev) & (ids >= 0) & (prev >= 0)).sum())
        prev = ids
        fin = O.plane_finish(sums, 6)
        e = icp.FinishEvaluatePlane(sums, 6)
        assert e.Value == fin["value"] and e.NumPairs == n == fin["npairs"]
        assert np.array_equal(e.Gradient, fin["gradient"]) and np.array_equal(e.Hessian, fin["hessian"])
        assert np.array_equal(e.Hessian.reshape(6, 6), e.Hessian.reshape(6, 6).T)
        want, conv, it_next = O.gauss_newton_update(pose, fin["gradient"], fin["hessian"], it, th, damping, 20)
        u = icp.GaussNewtonUpdaterFactory(Threshold=th, MaxIteration=20, Damping=damping).New()
        u.i = it
        got, c = u.Update(pose, e)
        assert np.array_equal(got, want) and c == conv and u.i == it_next == it + 1
        pose, it = want, it_next
    assert changed > 0  # (the scene is for partners that change between iterations)


def test_the_flat_stop_and_the_late_failures_of_the_oracle_fit():
    """what the GPU tests expect of the device, stated by the oracle: FLAT_THRESHOLD stops the Fit at its third Evaluate;
    the singular scene fails at its second, for either reason"""
    f = S.fit_scene()
    ok = S.finite_rows(f["target"])
    o = O.plane_fit(O.KDTree(f["base"]), f["normals"], f["target"][ok], f["max_dist"], 6, S.FLAT_THRESHOLD, 0.0, 8)
    assert o["num_iteration"] == 3
    # (well between the gradients of the second and the third Evaluate: a last-bit difference decides nothing)
    assert np.abs(o["gradient"]).max() < 0.1 * S.FLAT_THRESHOLD[0]
    g = S.singular_scene()
    og = O.KDTree(g["base"])
    never = np.full(6, -1.0, f32)
    with pytest.raises(O.OracleError) as e:
        O.plane_fit(og, g["normals"], g["target"], g["max_dist"], 6, never, 0.0, 8)
    assert e.value.code == O.ORC_E_SINGULAR and e.value.num_iteration == 2
    with pytest.raises(O.OracleError) as e:
        O.plane_fit(og, g["normals"], g["target"], g["max_dist"], g["n_flat"] + 1, never, 0.0, 8)
    assert e.value.code == O.ORC_E_NOT_ENOUGH_PAIRS and e.value.num_iteration == 2


def test_bases_without_a_grid_hold_their_cases():
    for name, c in S.no_grid_scenes().items():
        ot = O.KDTree(c["base"])
        ids = S.oracle_ids(ot, c["target"], c["max_dist"])
        d = [np.sort(_dist_sq(c["base"], p))[:2] for p in c["target"][S.finite_rows(c["target"])]]
        ties = sum(1 for a in d if a[0] == a[1] and a[0] < f32(c["max_dist"]) ** 2)
        at_limit = sum(1 for a in d if a[0] == f32(c["max_dist"]) ** 2)
        assert ties >= 8 and at_limit >= 4, (name, ties, at_limit)
        assert 0.6 <= (ids >= 0).mean() <= 0.95 and (~S.finite_rows(c["target"])).sum() == 6, name
        assert len(c["base"]) < 64 or len(np.unique(c["base"], axis=0)) == 2, name
        ref = S.reference_sums(O, ot, c["base"], c["normals"], c["target"], c["max_dist"])
        S.assert_sums(O.plane_sums(ot, c["normals"], c["target"][S.finite_rows(c["target"])], c["max_dist"]), ref, name)
