"""The 30 sums of point-to-plane sessions against the oracle on every pairing route (tests/plane_icp_scenes.py): the grid
pass with its leftover walk, pairs kept on their partner's certificate, the plain tree walk, the patched tree's walk;
ragged sizes; device-resident inputs; the Gauss-Newton update on the device.

A session is driven in lockstep with the oracle: set_pose(pose, it) leaves match[], match_id[], the certificates and the
leaf hints of the iteration before in place, partials() evaluates at exactly the oracle's pose, read_sums() is compared
with the exactly rounded sums of the oracle's pairs (|d - s| <= N 2^-53 A_k, pair count and weight exact: the module
text of plane_icp_scenes).  grid_stats() before each partials() says which route the step takes, and every test named
for a route asserts it.  Normals are random per base point: one wrong, stale or missing partner id moves every sum by
many orders of magnitude more than the bound."""
import os
import sys

import numpy as np
import pytest

import oracle as O
from pcgol_amd import _lib as L
from pcgol_amd import icp, kdtree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_icp_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
TOL = 1e-5  # the transform tolerance BASELINE.json states for ICP
NEVER_FLAT = np.full(6, -1.0, f32)
IDENTITY = np.eye(4, dtype=f32).reshape(-1)
RAGGED = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 4609)


@pytest.fixture(scope="module")
def sc():
    s = S.scene()
    return s, O.KDTree(s.base), kdtree.New(s.base)


def _grid_edge(t):
    geom, dims = np.zeros(5, f32), np.zeros(3, np.int32)
    L.check(L.lib().pcgx_debug_grid_geometry(t._h, L.ptr(geom), L.ptr(dims)))
    return float(geom[3]), dims


def _has_grid(t):
    geom, dims = np.zeros(5, f32), np.zeros(3, np.int32)
    return L.lib().pcgx_debug_grid_geometry(t._h, L.ptr(geom), L.ptr(dims)) == L.PCGX_OK


def _session(tree, normals, target, max_dist, min_pairs=6, threshold=NEVER_FLAT, max_iteration=20, **kw):
    return icp.IcpSession(tree, target, max_dist, min_pairs, None, threshold, max_iteration, BaseNormals=normals, **kw)


def _evaluate(s, ot, base, normals, target, max_dist, pose, it, what):
    """one lockstep Evaluate -> (grid_stats before it, the reference, the device's sums), the sums asserted"""
    s.set_pose(pose, it)
    stats = s.grid_stats()
    s.partials()
    sums = s.read_sums()
    ref = S.reference_sums(O, ot, base, normals, S.project(O, pose, it, target), max_dist)
    S.assert_sums(sums, ref, "%s, iteration %d" % (what, it))
    return stats, ref, sums


# ------------------------------------------------------------------ the grid pass and its leftover walk

def test_the_scenes_base_gets_a_grid_and_the_far_cluster_is_far(sc):
    s, _, t = sc
    h, dims = _grid_edge(t)
    assert 0 < h <= s.grid_edge_estimate() * 1.0001 and np.all(dims >= 1)
    far = s.target[s.mask("far")].astype(np.float64)
    d = np.sqrt(((far[:, None, :] - s.base[None, ::1].astype(np.float64)) ** 2).sum(axis=2).min(axis=1))
    assert d.min() > 9 * h * np.sqrt(3.0) and d.max() < s.max_dist_large  # (beyond the 9 x 9 x 9 block whatever the direction)


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("large", [False, True], ids=["MaxDist", "MaxDistLarge"])
def test_grid_pass_with_leftover_walk(sc, k, large):
    """Iteration 0 on the targets as they are, then iterations 1 and 2 under the pose that takes shifted(k) back onto the
    scene: ties, limit targets and non-finite ones are exact there, with the hints and certificates of the iteration
    before live.  With MAX_DIST_LARGE the far cluster is walked and paired."""
    s, ot, t = sc
    target, pose = s.shifted(k)
    md = s.max_dist_large if large else s.max_dist
    walked = s.mask("tie2", "tie4", "nonfinite", "far" if large else "limit").sum()
    sess = _session(t, s.normals, target, md)
    for it in (0, 1, 2):
        stats, ref, _ = _evaluate(sess, ot, s.base, s.normals, target, md, IDENTITY if it == 0 else pose, it, "shifted(%d)" % k)
        assert stats[0] == len(target)
        if it > 0 or k == 0:  # the scene itself: every special target of these groups is the walk's
            assert stats[1] >= walked, (it, stats)
            ids = ref[3]
            assert np.all(ids[s.mask("tie2", "tie4")] >= 0) and np.all(ids[s.mask("far")] >= 0) == large
            assert large or 0 < (ids[s.mask("limit")] >= 0).sum() < s.mask("limit").sum()
        if it == 2:  # the same pose again: pairs are kept on their certificate
            assert stats[5] > 0, stats
    sess.close()


# ------------------------------------------------------------------ kept on certificate

def test_pairs_kept_on_their_certificate_through_a_real_fit(sc):
    """Six lockstep iterations of a Fit whose partners change: a kept pair's normal is normals[match_id[i]], written
    iterations ago by the grid pass or by the walk."""
    _, ot, t = sc
    f = S.fit_scene()
    sess = _session(t, f["normals"], f["target"], f["max_dist"])
    pose, it, prev, changed, kept, pairs = IDENTITY, 0, None, [0], [], []
    for _ in range(6):
        stats, ref, _ = _evaluate(sess, ot, f["base"], f["normals"], f["target"], f["max_dist"], pose, it, "fit")
        kept.append(stats[5])
        pairs.append(ref[2])
        ids = ref[3]
        if prev is not None:
            changed.append(int(((ids != prev) & (ids >= 0) & (prev >= 0)).sum()))
        prev = ids
        fin = O.plane_finish(ref[0], 6)
        pose, _, it = O.gauss_newton_update(pose, fin["gradient"], fin["hessian"], it, NEVER_FLAT, 0.0, 20)
    sess.close()
    assert kept[0] == 0 and kept[1] > 0 and kept[-1] > 0 and changed[1] > 100, (kept, changed)
    # more pairs are kept in iteration 2 than kept their partner in iteration 1: some kept pairs read an id that
    # iteration 1 wrote over iteration 0's (with an id that stayed behind, their normals would be another point's)
    assert kept[2] > pairs[1] - changed[1], (kept, pairs, changed)


# ------------------------------------------------------------------ the plain tree walk

@pytest.mark.parametrize("name", ["63 points", "all but one alike"])
def test_tree_walk_only(name):
    c = S.no_grid_scenes()[name]
    t, ot = kdtree.New(c["base"]), O.KDTree(c["base"])
    assert not _has_grid(t)
    sess = _session(t, c["normals"], c["target"], c["max_dist"])
    nudge = O.translate(2.0 ** -6, -(2.0 ** -7), 2.0 ** -6)
    for it, pose in ((0, IDENTITY), (1, IDENTITY), (2, nudge), (3, IDENTITY)):  # (iterations >= 1: last iteration's pair and leaf as hints)
        stats, ref, _ = _evaluate(sess, ot, c["base"], c["normals"], c["target"], c["max_dist"], pose, it, name)
        assert stats == (len(c["target"]), 0, 0, 0, 0, 0) and ref[2] > 0.6 * len(c["target"])
    sess.close()


def test_a_tree_made_with_min_dist_sq_is_refused_by_a_session_and_ignored_by_fit(sc):
    """include/pcgx.h, point-to-plane: min_dist_sq > 0 is PCGX_E_INVALID at session creation (IcpSession hands the tree
    handle's MinDistSq on), never an approximate search; PointToPlaneICP.Fit passes 0 and searches exactly, as
    orc_plane_sums does."""
    s, ot, t = sc
    tw = t.With(MinDistSq=1e-3)
    with pytest.raises(L.PcgxError) as e:
        _session(tw, s.normals, s.target, s.max_dist)
    assert e.value.code == L.PCGX_E_INVALID
    reg = icp.PointToPlaneICP(icp.PointToPlaneEvaluator(icp.NearestPointCorresponder(MaxDist=s.max_dist), s.normals, MinPairs=6),
                              icp.GaussNewtonUpdaterFactory(Threshold=NEVER_FLAT, MaxIteration=1))
    a, sa = reg.Fit(tw, s.target)
    b, sb = reg.Fit(t, s.target)
    assert np.array_equal(a, b) and np.array_equal(sa.Evaluated.Hessian, sb.Evaluated.Hessian)
    ref = S.reference_sums(O, ot, s.base, s.normals, s.target, s.max_dist)
    fin = O.plane_finish(ref[0], 6)
    assert sa.Evaluated.NumPairs == ref[2] and np.allclose(sa.Evaluated.Hessian, fin["hessian"], rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------ the patched tree

def _gone(s, ot):
    """about a tenth of the base ids, partners of tie and limit targets among them"""
    ids = S.oracle_ids(ot, s.target, s.max_dist)
    partners = np.concatenate([ids[s.mask(g)][:16] for g in ("tie2", "tie4", "limit")])
    gone = np.unique(np.concatenate([partners[partners >= 0], np.arange(3, len(s.base), 11)]))
    assert 0.08 * len(s.base) < len(gone) < 0.12 * len(s.base) and (partners >= 0).sum() >= 36
    return gone


def test_patched_base_deleted_before_the_session():
    s = S.scene()
    ot, t = O.KDTree(s.base), kdtree.New(s.base)
    gone = _gone(s, ot)
    t.DeletePoints(gone)
    for i in gone:
        ot.delete_point(int(i))
    poisoned = s.normals.copy()
    poisoned[gone] = np.nan  # a deleted id's normal must never contribute
    target, pose = s.shifted(1)
    sess = _session(t, poisoned, target, s.max_dist)
    for it in (0, 1, 2):
        stats, ref, sums = _evaluate(sess, ot, s.base, s.normals, target, s.max_dist, IDENTITY if it == 0 else pose, it, "patched")
        assert stats == (len(target), 0, 0, 0, 0, 0) and np.all(np.isfinite(sums))
        assert not np.isin(ref[3], gone).any()
    assert ref[2] > 0.6 * len(target)
    sess.close()


def test_patched_base_deleted_under_a_live_session():
    s = S.scene()
    ot, t = O.KDTree(s.base), kdtree.New(s.base)
    gone = _gone(s, ot)
    sess = _session(t, s.normals, s.target, s.max_dist)
    before = after = None
    for it in (0, 1, 2, 3):
        if it == 2:
            t.DeletePoints(gone)
            for i in gone:
                ot.delete_point(int(i))
        stats, ref, _ = _evaluate(sess, ot, s.base, s.normals, s.target, s.max_dist, IDENTITY, it, "deleted under a live session")
        if it == 1:
            before = ref[3]
            assert stats[1] > 0 and stats[5] > 0  # (the grid's routes, kept pairs among them, up to the deletion)
        if it == 2:
            after = ref[3]
        if it == 3:
            assert stats == (len(s.target), 0, 0, 0, 0, 0)  # (the session has noticed the deletion)
    assert np.isin(before, gone).sum() > 200 and not np.isin(after, gone).any()
    assert ((after != before) & (after >= 0)).sum() > 100  # (kept pairs whose partner is gone found another)
    sess.close()


# ------------------------------------------------------------------ ragged sizes

@pytest.mark.parametrize("nt", RAGGED)
def test_ragged_sizes(sc, nt):
    """64-target chunks, 256-target grid rows, 512-thread correspondence workgroups, and from 8 workgroups on a launch
    grid rounded down to a multiple of 8: 4 609 targets are 19 grid rows folded by 8 workgroups."""
    s, ot, t = sc
    target, group = s.cut(nt)
    codes = set(group.tolist())
    assert nt < 63 or {S.GROUPS.index("tie2"), S.GROUPS.index("tie4"), S.GROUPS.index("nonfinite")} <= codes
    sess = _session(t, s.normals, target, s.max_dist, min_pairs=6)
    for it in (0, 1):
        stats, ref, sums = _evaluate(sess, ot, s.base, s.normals, target, s.max_dist, IDENTITY, it, "nt = %d" % nt)
        assert stats[0] == nt and stats[1] >= np.isin(group, [S.GROUPS.index(g) for g in ("tie2", "tie4", "limit", "nonfinite")]).sum()
        assert it == 0 or nt < 255 or stats[5] > 0
        sess.update()
        if ref[2] < 6:
            with pytest.raises(icp.ErrNotEnoughPairs) as e:
                sess.result()
            assert e.value.stat.Evaluated.NumPairs == ref[2]
            assert np.array_equal(sess.read_sums(), sums)
        else:
            sess.result()
    assert (ref[2] < 6) == (nt <= 2)
    sess.close()


# ------------------------------------------------------------------ device-resident inputs

def test_device_resident_target_and_normals(sc):
    import torch
    s, ot, t = sc
    nt = 4609
    target, _ = s.cut(nt)
    host = _session(t, s.normals, target, s.max_dist)
    dt, dn = torch.from_numpy(target).to("cuda"), torch.from_numpy(s.normals).to("cuda")
    torch.cuda.synchronize()
    dev = _session(t, dn, dt.data_ptr(), s.max_dist, target_on_device=True, nt=nt)
    for it in (0, 1, 2):
        _, _, a = _evaluate(host, ot, s.base, s.normals, target, s.max_dist, IDENTITY, it, "host inputs")
        _, _, b = _evaluate(dev, ot, s.base, s.normals, target, s.max_dist, IDENTITY, it, "device inputs")
        assert np.array_equal(a, b)
    host.close()
    dev.close()


# ------------------------------------------------------------------ the update on the device

def _same_evaluated(st, fin):
    ev = st.Evaluated
    assert ev.Value == fin["value"] and ev.NumPairs == fin["npairs"]
    assert np.array_equal(ev.Gradient, fin["gradient"]) and np.array_equal(ev.Hessian, fin["hessian"])
    assert np.array_equal(ev.Hessian.reshape(6, 6), ev.Hessian.reshape(6, 6).T)


@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_update_on_the_device_is_the_oracles_on_the_devices_sums(sc, damping):
    """partials() -> update() -> result(): the pose, the evaluate tail and hessian() against the oracle applied to the
    device's own 30 sums -- identical input, so identical bits (tests/test_plane_icp_scenes.py holds the host's functions
    to the same)."""
    _, ot, t = sc
    f = S.fit_scene()
    sess = _session(t, f["normals"], f["target"], f["max_dist"], Damping=damping)
    pose, it = IDENTITY, 0
    for _ in range(5):
        _, _, sums = _evaluate(sess, ot, f["base"], f["normals"], f["target"], f["max_dist"], pose, it, "damping %g" % damping)
        sess.update()
        got, st, conv = sess.result()
        fin = O.plane_finish(sums, 6)
        want, want_conv, it = O.gauss_newton_update(pose, fin["gradient"], fin["hessian"], it, NEVER_FLAT, damping, 20)
        _same_evaluated(st, fin)
        assert np.array_equal(sess.hessian(), fin["hessian"])
        assert np.array_equal(got, want) and conv == want_conv and st.NumIteration == 1, (got - want)
        pose = want
    sess.close()


def _fit_by_steps(sess, n, fused):
    sess.reset()
    for _ in range(n):
        if fused:
            sess.step()
        else:
            sess.partials()
            sess.update()
    tr, st, conv = sess.result()
    return tr, st, conv, sess.read_sums()


def test_flat_gradient_stops_the_fit_at_its_third_evaluate(sc):
    _, ot, t = sc
    f = S.fit_scene()
    o = O.plane_fit(ot, f["normals"], f["target"][S.finite_rows(f["target"])], f["max_dist"], 6, S.FLAT_THRESHOLD, 0.0, 8)
    sess = _session(t, f["normals"], f["target"], f["max_dist"], threshold=S.FLAT_THRESHOLD, max_iteration=8)
    outs = [_fit_by_steps(sess, 8, fused) for fused in (True, False, True)]
    sess.close()
    for tr, st, conv, sums in outs:
        assert st.NumIteration == o["num_iteration"] == 3 and conv
        assert np.max(np.abs(tr - o["trans"])) <= TOL
        # (the fused step and partials + update, and a second Fit of the same session: the same bits)
        assert np.array_equal(tr, outs[0][0]) and np.array_equal(sums, outs[0][3])
        assert np.array_equal(st.Evaluated.Hessian, outs[0][1].Evaluated.Hessian) and st.Evaluated.Value == outs[0][1].Evaluated.Value
    # the stop is the flat test's: the pose is the one the second update left
    fin = O.plane_finish(outs[0][3], 6)
    assert np.all(np.abs(fin["gradient"]) <= S.FLAT_THRESHOLD)
    _same_evaluated(outs[0][1], fin)


@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_fused_step_equals_partials_then_update(sc, damping):
    _, _, t = sc
    f = S.fit_scene()
    sess = _session(t, f["normals"], f["target"], f["max_dist"], max_iteration=6, Damping=damping)
    a = _fit_by_steps(sess, 6, True)
    b = _fit_by_steps(sess, 6, False)
    sess.close()
    assert a[1].NumIteration == b[1].NumIteration == 6 and a[2] and b[2]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[1].Evaluated.Hessian, b[1].Evaluated.Hessian) and np.array_equal(a[1].Evaluated.Gradient, b[1].Evaluated.Gradient)
    assert not np.array_equal(a[0], IDENTITY)


@pytest.mark.parametrize("fused", [True, False], ids=["step", "partials+update"])
def test_a_system_that_turns_singular_or_short_of_pairs_after_the_first_update(fused):
    g = S.singular_scene()
    t, ot = kdtree.New(g["base"]), O.KDTree(g["base"])
    # the first Evaluate is sound, and is the oracle's
    sess = _session(t, g["normals"], g["target"], g["max_dist"], max_iteration=8)
    _, ref, sums = _evaluate(sess, ot, g["base"], g["normals"], g["target"], g["max_dist"], IDENTITY, 0, "singular scene")
    assert ref[2] == g["n_flat"] + g["n_side"]
    with pytest.raises(icp.ErrSingular) as e:
        _fit_by_steps(sess, 4, fused)
    assert "at iteration 2" in str(e.value)
    assert sess.read_sums()[29] == g["n_flat"]  # (the second Evaluate's: the side part has left MaxDist)
    sess.close()
    sess = _session(t, g["normals"], g["target"], g["max_dist"], min_pairs=g["n_flat"] + 1, max_iteration=8)
    with pytest.raises(icp.ErrNotEnoughPairs) as e:
        _fit_by_steps(sess, 4, fused)
    assert e.value.stat.NumIteration == 2 and e.value.stat.Evaluated.NumPairs == g["n_flat"]
    sess.close()
    with pytest.raises(icp.ErrSingular):
        icp.PointToPlaneICP(icp.PointToPlaneEvaluator(icp.NearestPointCorresponder(MaxDist=g["max_dist"]), g["normals"], MinPairs=6),
                            icp.GaussNewtonUpdaterFactory(Threshold=NEVER_FLAT, MaxIteration=8)).Fit(t, g["target"])


# ------------------------------------------------------------------ the whole Fit

def test_plane_fit_end_to_end_on_the_scene(sc):
    s, ot, t = sc
    o = O.plane_fit(ot, s.normals, s.target[S.finite_rows(s.target)], s.max_dist, 6, NEVER_FLAT, 0.0, 8)
    reg = icp.PointToPlaneICP(icp.PointToPlaneEvaluator(icp.NearestPointCorresponder(MaxDist=s.max_dist), s.normals, MinPairs=6),
                              icp.GaussNewtonUpdaterFactory(Threshold=NEVER_FLAT, MaxIteration=8))
    a, sa = reg.Fit(t, s.target)
    b, sb = reg.Fit(t, s.target)
    assert sa.NumIteration == sb.NumIteration == o["num_iteration"] == 8
    assert np.max(np.abs(a - o["trans"])) <= TOL
    assert np.array_equal(a, b) and np.array_equal(sa.Evaluated.Hessian, sb.Evaluated.Hessian) and sa.Evaluated.Value == sb.Evaluated.Value
    assert np.allclose(sa.Evaluated.Hessian, o["hessian"], rtol=1e-5, atol=1e-9) and not np.array_equal(a, IDENTITY)
