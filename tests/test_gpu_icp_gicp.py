"""GPU checks of the Generalized ICP extension (include/pcgx.h, "Generalized ICP").

NO REFERENCE PARITY EXISTS: pcgol has no GICP.  The HIP path is checked against the NumPy float64 restatement of the
contract (tests/gicp_oracle.py), whose pairs come from the parity-pinned corresponder, and against synthetic ground
truth.

The sums' bound, per sum k: c (kappa_max + 1) 2^-53 A_k + 48 2^-53 A_k with c = 9 the roundings on the longest chain
of csrc/gicp_terms.h (counted there), kappa_max the worst cond_2(S) of the evaluation, A_k the sum over the used pairs of
|J_k|^T |M| |r| (entrywise absolute values; likewise for H), and 48 the reduction depth of 2 log2(n) float64 additions
in a different order.  The pair count and sum w are exact.
Poses: within 1e-5 absolute of the oracle's (TOL, the tolerance BASELINE.json states for ICP)."""
import os
import sys

import numpy as np
import pytest

import oracle as O
from pcgol_amd import _lib as L
from pcgol_amd import icp, kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gicp_oracle as G  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TOL = 1e-5
C_CHAIN = 9
U = 2.0 ** -53
ALL = np.full(6, -1, f32)  # Threshold -1: every iteration runs
# The oracle's Fit on c4_plane(40_000), 8 iterations, PLANE covariances (k = 20, eps = 1e-3) from a brute-force k-NN,
# measured on the CPU beforehand: |T - inv(icp_pose())|_max
ORACLE_ERR_40K = 1.3e-7  # (1.287e-07 measured)


def _truth():
    return np.linalg.inv(synth.icp_pose().astype(f64).reshape(4, 4).T).T.reshape(-1)


def _covs(points, tree=None, mode="plane", k=20):
    t = tree if tree is not None else kdtree.New(points)
    return t.Covariances(k, Mode=mode)[0]


def _scene(n, seed=0):
    c = synth.c4_plane(n, base_seed=6 + seed, perm_seed=7 + seed)
    c["tree"] = kdtree.New(c["base"])
    c["bc"] = _covs(c["base"], c["tree"])
    c["tc"] = _covs(c["target"])
    return c


def _evaluator(c, min_pairs=6):
    return icp.GeneralizedICPEvaluator(icp.NearestPointCorresponder(MaxDist=c["max_dist"]), c["bc"], c["tc"], min_pairs)


def _assert_sums(sums, o, what=""):
    s, A = o["sums"], o["A"]
    assert sums[29] == s[29] == o["used"] and sums[28] == s[28]
    bound = (C_CHAIN * (o["kappa_max"] + 1) + 48) * U * A[:28]
    err = np.abs(sums[:28] - s[:28])
    share = np.max(err / np.maximum(bound, 1e-300))
    print("gicp sums %s: pairs %d, dropped %d, kappa_max %.1f, worst share of the bound %.3g (sum %d), bound / A = %.2e"
          % (what, o["used"], o["dropped"], o["kappa_max"], share, int(np.argmax(err / np.maximum(bound, 1e-300))),
             (C_CHAIN * (o["kappa_max"] + 1) + 48) * U))
    assert np.all(err <= bound)


def _session_sums(c, trans=None, bc=None, tc=None, tree=None):
    s = icp.IcpSession(tree if tree is not None else c["tree"], c["target"], c["max_dist"], 6, None, ALL, 8,
                       BaseCov=c["bc"] if bc is None else bc, TargetCov=c["tc"] if tc is None else tc)
    try:
        if trans is not None:
            s.set_pose(trans, 1)
        s.partials()
        return s.read_sums(), s.dropped()
    finally:
        s.close()


def test_gicp_sums_match_oracle():
    c = _scene(50_000)
    ot = O.KDTree(c["base"])
    assert np.all(c["bc"][:, [0, 3, 5]] > 0) and np.isfinite(c["tc"]).all()
    for what, trans in (("identity", None), ("posed", _truth().astype(f32))):
        sums, dropped = _session_sums(c, trans)
        o = G.sums(ot, c["bc"], c["target"], c["tc"], c["max_dist"], trans)
        assert dropped == o["dropped"] == 0 and sums[29] > 0.99 * len(c["target"])
        _assert_sums(sums, o, what)
    ev = _evaluator(c)
    assert ev.HasGradient() and ev.HasHessian()
    e = ev.Evaluate(c["tree"], c["target"])
    oe = G.finish(G.sums(ot, c["bc"], c["target"], c["tc"], c["max_dist"])["sums"], 6)
    assert np.allclose(e.Value, oe["value"], rtol=1e-6) and np.allclose(e.Gradient, oe["gradient"], rtol=1e-5, atol=1e-9)
    assert np.allclose(e.Hessian, oe["hessian"], rtol=1e-5, atol=1e-9)


def test_gicp_fit_matches_oracle_and_ground_truth():
    c = _scene(40_000)
    reg = icp.GeneralizedICP(_evaluator(c), icp.GaussNewtonUpdaterFactory(Threshold=ALL, MaxIteration=8))
    trans, stat = reg.Fit(c["tree"], c["target"])
    o = G.fit(O.KDTree(c["base"]), c["bc"], c["target"], c["tc"], c["max_dist"], 6, ALL, 0.0, 8)
    assert stat.NumIteration == o["num_iteration"] == 8
    d_oracle = np.max(np.abs(trans - o["trans"]))
    err, oerr = np.max(np.abs(trans.astype(f64) - _truth())), np.max(np.abs(o["trans"].astype(f64) - _truth()))
    print("gicp fit 40k: |gpu - oracle| %.3e, gpu error %.3e, oracle error %.3e (stated %.1e)" % (d_oracle, err, oerr, ORACLE_ERR_40K))
    assert d_oracle <= TOL
    assert err <= 2 * ORACLE_ERR_40K + 1e-5
    H = stat.Evaluated.Hessian.reshape(6, 6)
    assert np.array_equal(H, H.T) and np.all(np.diag(H) > 0)
    assert stat.Evaluated.NumPairs == o["evaluated"]["npairs"]


def test_gicp_two_different_samplings():
    """base and target are different samples of one surface: the case GICP is for.  The GPU pose against the oracle's;
    the three Fits' errors against ground truth are printed for DESIGN 3.9, not asserted."""
    n, w = 40_000, 6.0
    base, normals = synth.surface_cloud(n, w, 21)
    other, _ = synth.surface_cloud(n, w, 22)
    target = synth.transform_points(synth.icp_pose(), other)
    t = kdtree.New(base)
    bc, tc = _covs(base, t), _covs(target)
    corr = icp.NearestPointCorresponder(MaxDist=0.5)
    trans, stat = icp.GeneralizedICP(icp.GeneralizedICPEvaluator(corr, bc, tc, 6),
                                     icp.GaussNewtonUpdaterFactory(Threshold=ALL, MaxIteration=8)).Fit(t, target)
    o = G.fit(O.KDTree(base), bc, target, tc, 0.5, 6, ALL, 0.0, 8)
    assert stat.NumIteration == o["num_iteration"] == 8
    assert np.max(np.abs(trans - o["trans"])) <= TOL
    tp, _ = icp.PointToPlaneICP(icp.PointToPlaneEvaluator(corr, normals, 6),
                                icp.GaussNewtonUpdaterFactory(Threshold=ALL, MaxIteration=8)).Fit(t, target)
    t2, _ = icp.PointToPointICPGradient(icp.PointToPointEvaluator(corr, 6),
                                        icp.GradientDescentUpdaterFactory(np.full(6, 0.3, f32), ALL, 20)).Fit(t, target)
    truth = _truth()
    print("two samplings (n = %d, width %.0f): error against ground truth: GICP oracle %.3e, GICP gpu %.3e, "
          "point-to-plane (analytic normals, 8 it) %.3e, point-to-point (20 it) %.3e"
          % (n, w, np.max(np.abs(o["trans"].astype(f64) - truth)), np.max(np.abs(trans.astype(f64) - truth)),
             np.max(np.abs(tp.astype(f64) - truth)), np.max(np.abs(t2.astype(f64) - truth))))


def test_gicp_session_steps_equal_fit_and_reset():
    c = _scene(20_000, seed=1)
    s = icp.IcpSession(c["tree"], c["target"], c["max_dist"], 6, None, ALL, 5, BaseCov=c["bc"], TargetCov=c["tc"])
    assert s.n_sums == 30 and s.dropped() == 0
    outs = []
    for rep in range(2):
        s.reset()
        for _ in range(5):
            s.step()
        tr, st, conv = s.result()
        outs.append((tr.copy(), st.Evaluated.Hessian.copy()))
        assert conv and st.NumIteration == 5
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    s.reset()
    for _ in range(5):
        s.partials()
        s.update()
    tr2, _, _ = s.result()
    assert np.array_equal(tr2, outs[0][0])
    with pytest.raises(L.PcgxError):
        s.set_strict(1)
    s.close()
    reg = icp.GeneralizedICP(_evaluator(c), icp.GaussNewtonUpdaterFactory(Threshold=ALL, MaxIteration=5))
    fa, sa = reg.Fit(c["tree"], c["target"])
    fb, sb = reg.Fit(c["tree"], c["target"])
    assert np.array_equal(fa, fb) and np.array_equal(sa.Evaluated.Hessian, sb.Evaluated.Hessian)
    assert np.array_equal(fa, outs[0][0]) and np.array_equal(sa.Evaluated.Hessian, outs[0][1])


def test_gicp_dropped_pairs():
    # a lattice plane z = const with RAW covariances: C_zz == 0 exactly on both sides, S is singular, every pair goes
    g = np.arange(60, dtype=f32) * f32(0.125)
    base = np.stack([np.repeat(g, 60), np.tile(g, 60), np.full(3600, 0.5, f32)], axis=1).astype(f32)
    target = (base + np.array([0.03125, 0.015625, 0.0], f32)).astype(f32)
    t = kdtree.New(base)
    bc, tc = _covs(base, t, "raw", 9), _covs(target, None, "raw", 9)
    assert np.all(bc[:, [2, 4, 5]] == 0) and np.all(tc[:, [2, 4, 5]] == 0) and np.all(bc[:, 0] > 0)
    ev = icp.GeneralizedICPEvaluator(icp.NearestPointCorresponder(MaxDist=0.5), bc, tc, 6)
    sums, dropped = ev.Sums(t, target, with_dropped=True)
    o = G.sums(O.KDTree(base), bc, target, tc, 0.5)
    assert o["matched"] == len(target) and o["used"] == 0
    assert dropped == o["dropped"] == o["matched"] and np.all(sums == 0)
    with pytest.raises(icp.ErrNotEnoughPairs):
        icp.GeneralizedICP(ev, icp.GaussNewtonUpdaterFactory(Threshold=ALL, MaxIteration=3)).Fit(t, target)
    # mixed: PLANE covariances, NaN written into the covariances of every 10th target
    c = _scene(30_000, seed=3)
    tc = c["tc"].copy()
    tc[::10] = np.nan
    o = G.sums(O.KDTree(c["base"]), c["bc"], c["target"], tc, c["max_dist"])
    sums, dropped = _session_sums(c, tc=tc)
    assert o["dropped"] > 0.099 * len(tc) and dropped == o["dropped"] and o["used"] + o["dropped"] == o["matched"]
    _assert_sums(sums, o, "every 10th target's covariance NaN")
    # ... and the same through a pose (the NaN goes through R C_t R^T)
    pose = _truth().astype(f32)
    o = G.sums(O.KDTree(c["base"]), c["bc"], c["target"], tc, c["max_dist"], pose)
    sums, dropped = _session_sums(c, pose, tc=tc)
    assert dropped == o["dropped"] > 0
    _assert_sums(sums, o, "NaN covariances, posed")


def test_gicp_errors():
    c = _scene(2_000, seed=4)
    t, tg, md = c["tree"], c["target"], c["max_dist"]

    def invalid(**kw):
        with pytest.raises(L.PcgxError) as e:
            icp.IcpSession(kw.pop("tree", t), tg, md, 6, None, ALL, 3, **kw).close()
        assert e.value.code == L.PCGX_E_INVALID

    invalid(BaseCov=None, TargetCov=c["tc"])
    invalid(BaseCov=c["bc"], TargetCov=None)
    invalid(BaseCov=c["bc"], TargetCov=c["tc"], WeightFn=icp.WeightConstant(2.0))
    invalid(BaseCov=c["bc"], TargetCov=c["tc"], Damping=-1.0)
    invalid(BaseCov=c["bc"], TargetCov=c["tc"], Damping=float("nan"))
    tm = kdtree.New(c["base"])
    tm.MinDistSq = 1e-4
    invalid(tree=tm, BaseCov=c["bc"], TargetCov=c["tc"])
    s = icp.IcpSession(t, tg, md, 6)
    with pytest.raises(L.PcgxError) as e:
        s.dropped()
    assert e.value.code == L.PCGX_E_INVALID
    s.close()
    # 16 copies of one point away from the origin, identity covariances: every pair has the same J, sum H has rank 3.
    # Every entry of H is exact in float32 (2 / sum w is a power of two), so the Schur complement of the rotation block
    # is exactly 0 and no rounding lets a pivot slip through
    base = np.array([[1.25, 2, 3], [5, 5, 5], [-4, 0, 1], [0, 7, 0], [2, -6, 3], [9, 9, -9], [3, 3, 8], [-2, -2, -2]], f32)
    target = np.tile(np.array([1, 2, 3], f32), (16, 1))
    ident = np.array([1, 0, 0, 1, 0, 1], f32)
    bt = kdtree.New(base)
    reg = icp.GeneralizedICP(icp.GeneralizedICPEvaluator(icp.NearestPointCorresponder(MaxDist=1.0), np.tile(ident, (8, 1)),
                                                         np.tile(ident, (16, 1)), 6),
                             icp.GaussNewtonUpdaterFactory(Threshold=ALL, MaxIteration=3))
    with pytest.raises(icp.ErrSingular):
        reg.Fit(bt, target)
    with pytest.raises(icp.ErrNotEnoughPairs):
        icp.GeneralizedICP(icp.GeneralizedICPEvaluator(icp.NearestPointCorresponder(MaxDist=0.001), c["bc"], c["tc"][:3], 6)
                           ).Fit(t, c["base"][:3] + f32(50.0))


def test_gicp_fit_knn_equals_covariances_then_fit():
    c = _scene(30_000, seed=5)
    uf = icp.GaussNewtonUpdaterFactory(Threshold=ALL, MaxIteration=6)
    a, sa = icp.GeneralizedICP.FromKNN(c["max_dist"], K=20, Epsilon=1e-3, MinPairs=6, UpdaterFactory=uf).Fit(c["tree"], c["target"])
    b, sb = icp.GeneralizedICP(_evaluator(c), uf).Fit(c["tree"], c["target"])
    assert np.array_equal(a, b) and sa.NumIteration == sb.NumIteration == 6
    assert np.array_equal(sa.Evaluated.Hessian, sb.Evaluated.Hessian) and sa.Evaluated.Value == sb.Evaluated.Value
    # another k / range / epsilon, and the covariance call's errors unchanged
    kw = dict(K=12, Epsilon=1e-2, CovMaxRange=0.2, MinPairs=6, UpdaterFactory=uf)
    a, _ = icp.GeneralizedICP.FromKNN(c["max_dist"], **kw).Fit(c["tree"], c["target"])
    bc = c["tree"].Covariances(12, MaxRange=0.2, Epsilon=1e-2)[0]
    tc = kdtree.New(c["target"]).Covariances(12, MaxRange=0.2, Epsilon=1e-2)[0]
    b, _ = icp.GeneralizedICP(icp.GeneralizedICPEvaluator(icp.NearestPointCorresponder(c["max_dist"]), bc, tc, 6), uf).Fit(
        c["tree"], c["target"])
    assert np.array_equal(a, b)
    for bad in (dict(K=0), dict(K=65), dict(Epsilon=0.0), dict(CovMaxRange=-1.0)):
        with pytest.raises(L.PcgxError) as e:
            icp.GeneralizedICP.FromKNN(c["max_dist"], **bad).Fit(c["tree"], c["target"])
        assert e.value.code == L.PCGX_E_INVALID


def test_gicp_after_delete_point():
    c = _scene(30_000, seed=6)
    gone = np.arange(0, len(c["base"]), 3)
    t = kdtree.New(c["base"])
    bc = _covs(c["base"], t)  # indexed by original id, deleted ids included
    t.DeletePoints(gone)
    ot = O.KDTree(c["base"])
    for i in gone:
        ot.delete_point(int(i))
    for what, trans in (("after DeletePoint", None), ("after DeletePoint, posed", _truth().astype(f32))):
        sums, dropped = _session_sums(c, trans, bc=bc, tree=t)
        o = G.sums(ot, bc, c["target"], c["tc"], c["max_dist"], trans)
        assert dropped == o["dropped"] == 0 and o["used"] > 0.9 * len(c["target"])
        _assert_sums(sums, o, what)
    # a deletion made after the session exists: the next step walks the patched tree
    t2 = kdtree.New(c["base"])
    s = icp.IcpSession(t2, c["target"], c["max_dist"], 6, None, ALL, 8, BaseCov=bc, TargetCov=c["tc"])
    s.partials()
    t2.DeletePoints(gone)
    s.reset()
    s.partials()
    _assert_sums(s.read_sums(), G.sums(ot, bc, c["target"], c["tc"], c["max_dist"]), "deleted under a live session")
    s.close()


def test_gicp_sharded_rccl_single_rank():
    """The 30-double exchange path (partials -> all-reduce -> update) through a 1-rank RCCL group, and the library's own
    pcgx_icp_session_step_sharded through a one-rank communicator made to run its collective."""
    import torch
    import torch.distributed as dist
    from pcgol_amd.distributed import Comm, ShardedIcp
    c = _scene(30_000, seed=2)
    torch.cuda.set_device(0)
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        kw = dict(BaseCov=c["bc"], TargetCov=c["tc"])
        a = ShardedIcp(c["tree"], c["target"], c["max_dist"], 6, None, ALL, 6, force_exchange=True, **kw)
        assert a.exchange and a.sums.numel() == 30
        tr_a, st_a, _ = a.fit()
        b = ShardedIcp(c["tree"], c["target"], c["max_dist"], 6, None, ALL, 6, **kw)
        tr_b, st_b, _ = b.fit()
        assert np.array_equal(tr_a, tr_b) and st_a.NumIteration == st_b.NumIteration == 6
        assert np.array_equal(st_a.Evaluated.Hessian, st_b.Evaluated.Hessian)
        calls = []

        def same(buf):
            calls.append(len(buf))
            return buf

        old = os.environ.get("PCGX_COMM_FORCE_COLLECTIVE")
        os.environ["PCGX_COMM_FORCE_COLLECTIVE"] = "1"
        try:
            comm = Comm.callback(0, 1, same)
            d = ShardedIcp(c["tree"], c["target"], c["max_dist"], 6, None, ALL, 6, comm=comm, **kw)
            tr_d, st_d, _ = d.fit()
            d.close()
            comm.close()
        finally:
            if old is None:
                del os.environ["PCGX_COMM_FORCE_COLLECTIVE"]
            else:
                os.environ["PCGX_COMM_FORCE_COLLECTIVE"] = old
        assert calls and all(n == 31 for n in calls)  # (30 sums + the ranks' error flag)
        assert np.array_equal(tr_d, tr_b) and st_d.NumIteration == 6
        a.close()
        b.close()
    finally:
        if created:
            dist.destroy_process_group()


def test_gicp_c4_full_size():
    """synth.c4_plane(1_000_000), 20 iterations.  The NumPy oracle evaluates iteration 0's sums only (a Fit of 20
    evaluations at 1M pairs each is minutes of CPU); the ground-truth bound is therefore taken from the 40k oracle run
    (ORACLE_ERR_40K).  Two runs bit-identical."""
    c = _scene(1_000_000)
    ev = _evaluator(c)
    sums, dropped = ev.Sums(c["tree"], c["target"], with_dropped=True)
    o = G.sums(O.KDTree(c["base"]), c["bc"], c["target"], c["tc"], c["max_dist"])
    assert dropped == o["dropped"] == 0 and sums[29] > 0.99 * len(c["target"])
    _assert_sums(sums, o, "1M, iteration 0")
    reg = icp.GeneralizedICP(ev, icp.GaussNewtonUpdaterFactory(Threshold=ALL, MaxIteration=20))
    trans, stat = reg.Fit(c["tree"], c["target"])
    trans2, stat2 = reg.Fit(c["tree"], c["target"])
    assert stat.NumIteration == stat2.NumIteration == 20
    assert np.array_equal(trans, trans2) and np.array_equal(stat.Evaluated.Hessian, stat2.Evaluated.Hessian)
    err = np.max(np.abs(trans.astype(f64) - _truth()))
    print("gicp 1M: error against ground truth %.3e, value %.3e" % (err, float(stat.Evaluated.Value)))
    assert err <= 2 * ORACLE_ERR_40K + 1e-5
