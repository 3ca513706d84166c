"""pcgx_pose_from_correspondences[_dev] (pcgol_amd/alignment.py, csrc/pose.hip) against the NumPy oracle
(tests/pose_oracle.py).  Statuses, counts (from the library's own pose bits), the first best and the inlier lists are
compared for equality; poses within 2^-23 max(1, |.|) of the oracle's independent solve on well-conditioned triangles;
the refined pose within the same bound of the oracle's refit over the library's own pre-refinement inlier list."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import alignment, features, icp, kdtree, mat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_oracle as PO  # noqa: E402
from test_pose_oracle import TRI, line_scene, lower_refit_scene, scene_m_reference, words  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64, u32 = np.float32, np.float64, np.uint32


@pytest.fixture
def split(monkeypatch):
    def set_(v):
        if v is None:
            monkeypatch.delenv("PCGX_POSE_SPLIT", raising=False)
        else:
            monkeypatch.setenv("PCGX_POSE_SPLIT", str(v))
    return set_


def call(P, Q, src, dst, samples, max_dist_sq, es, refine, rc_only=False):
    """pcgx_pose_from_correspondences with every output"""
    P, Q = np.ascontiguousarray(P, f32), np.ascontiguousarray(Q, f32)
    src, dst = np.ascontiguousarray(src, np.int64), np.ascontiguousarray(dst, np.int64)
    samples = np.ascontiguousarray(samples, u32).reshape(-1, 3)
    n, m = len(samples), len(src)
    found, refined = C.c_int32(7), C.c_int32(7)
    best, best_count, n_in = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    pose = np.full(16, 7, f32)
    ids = np.full(m, 7, np.int64)
    status, counts, poses = np.full(n, 7, np.int32), np.full(n, 7, np.int64), np.full((n, 16), 7, f32)
    rc = L.lib().pcgx_pose_from_correspondences(
        L.ptr(P), len(P), L.ptr(Q), len(Q), L.ptr(src), L.ptr(dst), m, L.ptr(samples), n, float(f32(max_dist_sq)),
        float(f32(es)), int(refine), C.byref(found), C.byref(best), C.byref(best_count), L.ptr(pose), C.byref(refined),
        C.byref(n_in), L.ptr(ids), L.ptr(status), L.ptr(counts), L.ptr(poses))
    if rc_only:
        return rc
    L.check(rc)
    assert np.all(ids[n_in.value:] == -1) and np.all(ids[:n_in.value] >= 0)
    return dict(found=bool(found.value), best=best.value, best_count=best_count.value, refined=bool(refined.value),
                pose=pose, inliers=ids[:n_in.value].copy(), status=status, counts=counts, poses=poses)


def call_dev(P, Q, src, dst, samples, max_dist, es, refine, n_pairs=None, outputs=True):
    """pcgx_pose_from_correspondences_dev through alignment.EstimatePoseDev, everything device resident"""
    import torch
    dev = torch.device("cuda", 0)
    tP, tQ = (torch.from_numpy(np.ascontiguousarray(x, f32)).to(dev) for x in (P, Q))
    ts, td = (torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev) for x in (src, dst))
    tu = torch.from_numpy(np.ascontiguousarray(samples, u32).reshape(-1, 3).view(np.int32)).to(dev)
    n, m_cap = len(tu), len(ts)
    res = torch.full((alignment.RESULT_WORDS,), 7, dtype=torch.int32, device=dev)
    ids = torch.full((max(m_cap, 1),), 7, dtype=torch.int32, device=dev)
    st, cn = (torch.full((max(n, 1),), 7, dtype=torch.int32, device=dev) for _ in range(2))
    ps = torch.full((max(n, 1), 16), 7, dtype=torch.float32, device=dev)
    tn = torch.tensor([n_pairs], dtype=torch.int32, device=dev) if n_pairs is not None else None
    torch.cuda.synchronize()
    alignment.EstimatePoseDev(tP.data_ptr(), len(tP), tQ.data_ptr(), len(tQ), ts.data_ptr(), td.data_ptr(), m_cap,
                              tu.data_ptr(), n, res.data_ptr(), max_dist, EdgeSimilarity=es, Refine=refine,
                              d_n_pairs=tn.data_ptr() if tn is not None else 0,
                              d_inlier_ids=ids.data_ptr() if outputs else 0, d_status=st.data_ptr() if outputs else 0,
                              d_counts=cn.data_ptr() if outputs else 0, d_poses=ps.data_ptr() if outputs else 0,
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = alignment.ReadResult(res.cpu().numpy())
    if outputs:
        i = ids.cpu().numpy()[:m_cap]
        assert np.all(i[r["n_inliers"]:] == -1)
        r.update(inliers=i[:r["n_inliers"]].astype(np.int64), status=st.cpu().numpy()[:n],
                 counts=cn.cpu().numpy()[:n].astype(np.int64), poses=ps.cpu().numpy()[:n])
    return r


def check(got, P, Q, src, dst, samples, max_dist_sq, es, refine, what=""):
    """everything the contract fixes, against the oracle; -> the oracle's answer on the library's pose bits"""
    st, own, idx = PO.hypotheses(P, Q, src, dst, samples, es)
    assert np.array_equal(got["status"], st), what
    ok = st == PO.OK
    assert not got["poses"][~ok].any() and not got["counts"][~ok].any(), what
    assert np.all(got["poses"][ok][:, [3, 7, 11, 15]] == np.array([0, 0, 0, 1], f32)), what
    if len(src) >= 3:
        well = ok & PO.well_conditioned(P, Q, src, dst, idx)
        close, worst = PO.pose_close(got["poses"][well], own[well])
        assert close, (what, worst)
    want = PO.estimate(P, Q, src, dst, samples, max_dist_sq, es, refine, poses=got["poses"])
    assert np.array_equal(got["counts"], want["counts"]), what  # given the pose's bits: no tolerance
    assert (got["best"], got["best_count"], got["found"]) == (want["best"], want["best_count"], want["found"]), what
    if ok.any():  # the first maximum of the library's own counts
        assert got["best"] == int(np.nonzero(ok & (got["counts"] == got["counts"][ok].max()))[0][0]), what
    else:
        assert got["best"] == -1 and not got["found"] and not got["pose"].any() and len(got["inliers"]) == 0, what
        return want
    A, B, _ = PO.pair_points(P, Q, src, dst)
    if got["refined"]:
        assert refine and got["found"] and want["refit_pose"] is not None, what
        close, worst = PO.pose_close(got["pose"], want["refit_pose"])  # (the oracle's refit over the library's own list)
        assert close, (what, worst)
        assert PO.inlier_mask(got["pose"], A, B, max_dist_sq).sum() >= got["best_count"], what
    else:
        assert np.array_equal(got["pose"].view(u32), got["poses"][got["best"]].view(u32)), what
        assert not want["refined"], what
    assert np.array_equal(got["inliers"], np.nonzero(PO.inlier_mask(got["pose"], A, B, max_dist_sq))[0]), what
    return want


def same(a, b):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


# ------------------------------------------------------------------------------------------------ scene M

@pytest.mark.parametrize("s_", [None, 1, 2, 3, 7])
def test_scene_m_under_splits(split, s_):
    split(s_)
    s, r = scene_m_reference()
    args = (s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], 0.9, True)
    got = call(*args)
    want = check(got, *args, what="split %s" % s_)
    assert got["found"] and got["refined"] and got["best_count"] == r["best_count"] and got["best"] == r["best"]
    assert np.array_equal(got["inliers"], want["inliers"]) and len(got["inliers"]) >= got["best_count"]
    same(got, call(*args))  # two calls, the same bits


def test_scene_m_without_edge_test_and_without_refinement():
    s, _ = scene_m_reference()
    args = (s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], 0.0, False)
    got = call(*args)
    check(got, *args)
    assert got["found"] and not got["refined"] and (got["status"] == 0).sum() > 4000


def test_python_binding_draws_its_samples():
    s, r = scene_m_reference()
    pairs = np.stack([s["src"], s["dst"]], axis=1)
    found, pose, ids, info = alignment.EstimatePose(s["P"], s["Q"], pairs, 4096, s["max_dist"], seed=11,
                                                    per_hypothesis=True)
    assert np.array_equal(alignment.Samples(4096, 11), s["samples"])
    got = call(s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], 0.9, True)
    assert found and info["refined"] and info["best"] == got["best"] and info["best_count"] == got["best_count"]
    assert np.array_equal(pose.view(u32), got["pose"].view(u32)) and np.array_equal(ids, got["inliers"])
    assert np.array_equal(info["counts"], got["counts"]) and np.array_equal(info["status"], got["status"])
    f2, p2, i2, info2 = alignment.EstimatePose(s["P"], s["Q"], pairs, 0, s["max_dist"], samples=s["samples"])
    assert f2 and np.array_equal(p2, pose) and np.array_equal(i2, ids) and "status" not in info2
    assert np.max(np.abs(mat.Transform(pose, s["P"]) - s["Q"])) < s["max_dist"]


# ------------------------------------------------------------------------------------------------ shapes

def _sweep_scene(m, n_hyp):
    P, Q = PO.moved_clouds()
    src = (np.arange(m, dtype=np.int64) * 37) % 3000
    dst = src.copy()
    dst[3::4] = (dst[3::4] * 11 + 5) % 3000  # every fourth pair (never one of the first three) names a wrong partner
    samples = np.random.default_rng(1000 * m + n_hyp).integers(0, 2 ** 32, (n_hyp, 3)).astype(u32)
    return P, Q, src, dst, samples


@pytest.mark.parametrize("s_", [None, 1, 300])
def test_shape_sweep(split, s_):
    """partial waves, the second hypothesis of a lane missing, more chunks than pairs"""
    split(s_)
    tile = alignment.PoseTile()
    assert tile >= 64
    mds = float(f32(0.01) * f32(0.01))
    for n_hyp in (1, 63, 64, 65, tile - 1, tile, tile + 1):
        for m in (3, 4, 63, 64, 65, 257):
            args = _sweep_scene(m, n_hyp) + (mds, 0.5, True)
            got = call(*args)
            check(got, *args, what="n_hyp %d m %d split %s" % (n_hyp, m, s_))
            if m >= 63 and n_hyp >= 63:
                assert got["found"] and got["best_count"] >= m - (m // 4) - 1, (n_hyp, m)


# ------------------------------------------------------------------------------------------------ the rules, one by one

def test_every_hypothesis_rejected():
    s, _ = scene_m_reference()
    samples = s["samples"][:200].copy()
    samples[:, 1] = samples[:, 0]  # a repeated index in every one
    args = (s["P"], s["Q"], s["src"], s["dst"], samples, s["max_dist_sq"], 0.9, True)
    got = call(*args)
    check(got, *args)
    assert not got["found"] and got["best"] == -1 and got["best_count"] == 0 and not got["refined"]
    assert np.all(got["status"] == PO.BAD_SAMPLE) and not got["pose"].any() and len(got["inliers"]) == 0
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], f32)  # ... and every one degenerate
    ids = np.arange(4, dtype=np.int64)
    got = call(line, line, ids, ids, words([[0, 1, 2], [1, 2, 3]], 4), 1e-4, 0.9, True)
    assert got["status"].tolist() == [2, 2] and not got["found"] and got["best"] == -1


def test_tie_goes_to_the_smaller_h():
    s, r = scene_m_reference()
    samples = s["samples"][:300].copy()
    b = int(np.nonzero((r["status"][:300] == 0) & (r["counts"][:300] == r["counts"][:300].max()))[0][-1])
    assert r["counts"][b] == r["best_count"]
    samples[5] = samples[b]      # the same three samples at 5, at 130 (the other half of a lane's pair) and at b
    samples[130] = samples[b]
    args = (s["P"], s["Q"], s["src"], s["dst"], samples, s["max_dist_sq"], 0.9, False)
    got = call(*args)
    check(got, *args)
    assert got["counts"][5] == got["counts"][130] == got["counts"][b] == got["best_count"]
    assert got["best"] == min(5, int(np.nonzero(got["counts"] == got["best_count"])[0][0]))
    assert np.array_equal(got["poses"][5].view(u32), got["poses"][130].view(u32))


def test_strictly_less_than_max_dist_sq():
    P = np.concatenate([TRI, [[3, 3, 3]]]).astype(f32)
    Q = P.copy()
    Q[3] += np.array([0.25, 0.5, 0.125], f32)
    ids = np.arange(4, dtype=np.int64)
    samples = words([[0, 1, 2]], 4)
    got = call(P, Q, ids, ids, samples, 100.0, 0.9, False)
    assert got["best_count"] == 4
    D = PO.dist_sq(got["poses"][0], P[3:], Q[3:])[0]  # the pair's DistSq under the library's own pose
    assert 0.3 < D < 0.35
    for mds, n in ((D, 3), (np.nextafter(D, f32(1)), 4), (np.nextafter(D, f32(0)), 3)):
        args = (P, Q, ids, ids, samples, float(mds), 0.9, False)
        got = call(*args)
        check(got, *args)
        assert got["best_count"] == n and got["inliers"].tolist() == list(range(n))


def test_nan_and_inf_points():
    s, _ = scene_m_reference()
    P, Q = s["P"].copy(), s["Q"].copy()
    src, dst = s["src"], s["dst"]
    P[src[0], 0] = np.nan
    P[src[64], 1] = np.inf
    P[src[700], 2] = -np.inf
    Q[dst[1], 2] = np.nan
    Q[dst[1499], 0] = np.inf
    samples = s["samples"][:1024].copy()
    samples[3] = words([[0, 10, 20]], 1500)[0]      # hypotheses that draw them are degenerate
    samples[70] = words([[5, 1499, 20]], 1500)[0]
    args = (P, Q, src, dst, samples, s["max_dist_sq"], 0.0, True)
    got = call(*args)
    check(got, *args)
    assert got["status"][3] == got["status"][70] == PO.DEGENERATE and got["found"]
    assert not np.isin([0, 64, 700, 1, 1499], got["inliers"]).any()


def test_out_of_range_ids_on_the_device_path():
    s, _ = scene_m_reference()
    src, dst = s["src"].copy(), s["dst"].copy()
    src[[2, 100]] = [-1, 3000]
    dst[[64, 1499]] = [3000, -5]
    samples = s["samples"][:1024].copy()
    samples[9] = words([[2, 10, 20]], 1500)[0]
    samples[200] = words([[7, 10, 1499]], 1500)[0]
    got = call_dev(s["P"], s["Q"], src, dst, samples, s["max_dist"], 0.9, True)
    check(got, s["P"], s["Q"], src, dst, samples, s["max_dist_sq"], 0.9, True)
    assert got["status"][9] == got["status"][200] == PO.BAD_SAMPLE and got["found"] and got["m"] == 1500
    assert not np.isin([2, 100, 64, 1499], got["inliers"]).any()
    # the host path can read the list: the same call is refused there
    assert call(s["P"], s["Q"], src, dst, samples, s["max_dist_sq"], 0.9, True, rc_only=True) == L.PCGX_E_INVALID
    assert "out of range" in L.last_error()


def test_device_list_length_is_read_on_the_device():
    """d_n_pairs < m_cap: the pairs behind it do not exist -- the host path's answer on the shorter list"""
    s, _ = scene_m_reference()
    for m in (1000, 2, 0):
        got = call_dev(s["P"], s["Q"], s["src"], s["dst"], s["samples"][:512], s["max_dist"], 0.9, True, n_pairs=m)
        assert got["m"] == m
        if m:
            want = call(s["P"], s["Q"], s["src"][:m], s["dst"][:m], s["samples"][:512], s["max_dist_sq"], 0.9, True)
            for k in ("found", "best", "best_count", "refined", "pose", "inliers", "status", "counts", "poses"):
                assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).astype(np.asarray(got[k]).dtype).tobytes(), (m, k)
        else:
            assert not got["found"] and got["best"] == -1 and np.all(got["status"] == PO.BAD_SAMPLE)
    # n_pairs above the capacity is held to it; without the optional outputs the record is the same
    a = call_dev(s["P"], s["Q"], s["src"], s["dst"], s["samples"][:512], s["max_dist"], 0.9, True, n_pairs=5000)
    b = call_dev(s["P"], s["Q"], s["src"], s["dst"], s["samples"][:512], s["max_dist"], 0.9, True, outputs=False)
    assert a["m"] == b["m"] == 1500 and a["found"]
    for k in b:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_refinement_rules():
    # a collinear inlier set is not refitted
    s = line_scene()
    args = (s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], s["es"], True)
    got = call(*args)
    check(got, *args)
    assert got["found"] and got["best_count"] == 5 and not got["refined"] and got["inliers"].tolist() == [3, 4, 5, 6, 7]
    # a refit that keeps fewer pairs is dropped: the hypothesis's pose stays
    s = lower_refit_scene()
    args = (s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], s["es"], True)
    got = call(*args)
    want = check(got, *args)
    assert want["refit_pose"] is not None and not got["refined"] and got["best_count"] == 7 and len(got["inliers"]) == 7
    # Refine off: never refined; on: scene M's refit is kept (test_scene_m_under_splits)
    off = call(*(args[:-1] + (False,)))
    assert not off["refined"] and np.array_equal(off["pose"], got["pose"])


def test_bad_arguments_and_empty_inputs():
    s, _ = scene_m_reference()
    P, Q, src, dst, u = s["P"], s["Q"], s["src"][:50], s["dst"][:50], s["samples"][:10]
    lib = L.lib()
    E = L.PCGX_E_INVALID
    for mds in (0.0, -1.0, np.inf, np.nan):
        assert call(P, Q, src, dst, u, mds, 0.9, True, rc_only=True) == E
    for es in (-0.1, 1.5, np.nan):
        assert call(P, Q, src, dst, u, 1e-4, es, True, rc_only=True) == E
    assert call(P, Q, src, dst, u, 1e-4, 1.0, True, rc_only=True) == L.PCGX_OK
    out = [C.c_int32(), C.c_int64(), C.c_int64(), np.zeros(16, f32), C.c_int32(), C.c_int64()]

    def raw(P=P, ns=3000, Q=Q, nd=3000, src=src, dst=dst, m=50, u=u, n=10, found=True):
        return lib.pcgx_pose_from_correspondences(
            L.ptr(P), ns, L.ptr(Q), nd, L.ptr(src), L.ptr(dst), m, L.ptr(u), n, 1e-4, 0.9, 1,
            C.byref(out[0]) if found else None, C.byref(out[1]), C.byref(out[2]), L.ptr(out[3]), C.byref(out[4]),
            C.byref(out[5]), None, None, None, None)

    assert raw() == L.PCGX_OK and out[0].value == 1
    assert raw(P=None) == E and raw(Q=None) == E and raw(src=None) == E and raw(dst=None) == E and raw(u=None) == E
    assert raw(found=False) == E
    assert raw(ns=-1) == E and raw(nd=-1) == E and raw(m=-1) == E and raw(n=-1) == E
    assert raw(ns=2 ** 31) == E and raw(m=2 ** 31) == E and raw(n=2 ** 31) == E
    assert raw(ns=int(src.max())) == E  # an id out of range on the host path
    # nothing to do: PCGX_OK, found = 0
    for kw in (dict(n=0, u=None), dict(m=0, src=None, dst=None)):
        out[0].value, out[1].value = 7, 7
        assert raw(**kw) == L.PCGX_OK and out[0].value == 0 and out[1].value == -1 and not out[3].any()
    got = call(P, Q, src[:0], dst[:0], u, 1e-4, 0.9, True)
    assert not got["found"] and np.all(got["status"] == PO.BAD_SAMPLE) and not got["counts"].any()
    got = call(P, Q, src[:2], dst[:2], u, 1e-4, 0.9, True)  # m = 2 goes to the device: every sample is bad
    assert not got["found"] and got["best"] == -1 and np.all(got["status"] == PO.BAD_SAMPLE)
    # the device form
    import torch
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = z.data_ptr()
    with pytest.raises(L.PcgxError):
        alignment.EstimatePoseDev(p, 4, p, 4, p, p, 4, p, 4, 0, 0.1)          # NULL result
    with pytest.raises(L.PcgxError):
        alignment.EstimatePoseDev(p, 4, p, 4, p, p, 4, p, 4, p, float("inf"))  # max_dist_sq not finite
    with pytest.raises(L.PcgxError):
        alignment.EstimatePoseDev(p, 4, p, 4, 0, p, 4, p, 4, p, 0.1)           # NULL ids
    alignment.EstimatePoseDev(0, 0, 0, 0, 0, 0, 0, 0, 0, p, 0.1)              # nothing at all: a record that says so
    torch.cuda.synchronize()
    r = alignment.ReadResult(z.cpu().numpy()[:24])
    assert not r["found"] and r["best"] == -1 and r["m"] == 0


# ------------------------------------------------------------------------------------------------ the chain

def test_device_chain_to_a_starting_pose():
    """NormalsDev -> FPFHDev -> CorrespondencesDev -> EstimatePoseDev on one stream over the moved clouds, nothing read
    back in between; then the point-to-point Fit started from that pose converges where the same Fit from the identity
    does not."""
    import torch
    P, P2 = PO.moved_clouds()
    r, vp, vp2 = 0.1, (0.8, 0.8, 50.0), (-0.8 + 2.25, 0.8 - 0.5, 50.0 + 1.75)
    t, t2 = kdtree.New(P), kdtree.New(P2)
    n, n_hyp, max_dist = len(P), 2048, 0.01
    dev = torch.device("cuda", 0)
    samples = alignment.Samples(n_hyp, 3)

    def buf(shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=dev)

    dP, dP2 = torch.from_numpy(P).to(dev), torch.from_numpy(P2).to(dev)
    du = torch.from_numpy(samples.view(np.int32)).to(dev)
    dn, dn2, df, df2 = buf((n, 3)), buf((n, 3)), buf((n, 33)), buf((n, 33))
    src, dst, cnt = buf(n, torch.int32), buf(n, torch.int32), buf(1, torch.int32)
    res, ids = buf(alignment.RESULT_WORDS, torch.int32), buf(n, torch.int32)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    t.NormalsDev(r, dn.data_ptr(), Viewpoint=vp, stream=st)
    t.FPFHDev(r, dn.data_ptr(), df.data_ptr(), stream=st)
    t2.NormalsDev(r, dn2.data_ptr(), Viewpoint=vp2, stream=st)
    t2.FPFHDev(r, dn2.data_ptr(), df2.data_ptr(), stream=st)
    features.CorrespondencesDev(df.data_ptr(), n, df2.data_ptr(), n, src.data_ptr(), dst.data_ptr(), cnt.data_ptr(),
                                MaxRatio=1.0, Mutual=True, stream=st)
    alignment.EstimatePoseDev(dP.data_ptr(), n, dP2.data_ptr(), n, src.data_ptr(), dst.data_ptr(), n, du.data_ptr(), n_hyp,
                              res.data_ptr(), max_dist, d_n_pairs=cnt.data_ptr(), d_inlier_ids=ids.data_ptr(), stream=st)
    torch.cuda.synchronize()
    got = alignment.ReadResult(res.cpu().numpy())
    m = int(cnt.cpu().numpy()[0])
    assert got["found"] and got["m"] == m and 1000 < m < n
    pose = got["pose"]
    assert np.max(np.linalg.norm(mat.Transform(pose, P).astype(f64) - P2, axis=1)) < max_dist
    # the host entry point on the host copy of the same list: the same bits
    pairs = np.stack([src.cpu().numpy()[:m], dst.cpu().numpy()[:m]], axis=1).astype(np.int64)
    found, hpose, hids, info = alignment.EstimatePose(P, P2, pairs, n_hyp, max_dist, samples=samples)
    assert found and np.array_equal(hpose.view(u32), pose.view(u32))
    assert (info["best"], info["best_count"], info["refined"]) == (got["best"], got["best_count"], got["refined"])
    assert np.array_equal(hids, ids.cpu().numpy()[:got["n_inliers"]]) and np.all(ids.cpu().numpy()[got["n_inliers"]:] == -1)
    # a Fit from that pose: the target moved by it, then registered -- against the same Fit from the identity
    reg = icp.PointToPointICPGradient(icp.PointToPointEvaluator(icp.NearestPointCorresponder(MaxDist=0.2), MinPairs=100))

    def end_error(start):
        trans, _ = reg.Fit(t2, mat.Transform(start, P))
        whole = mat.Mul(trans, start)
        return whole, float(np.max(np.linalg.norm(mat.Transform(whole, P).astype(f64) - P2, axis=1)))

    with_pose, e1 = end_error(pose)
    try:
        from_identity, e0 = end_error(mat.Translate(0, 0, 0))
    except icp.ErrNotEnoughPairs as e:  # (too far apart to pair at all is one way of not getting there)
        from_identity, e0 = e.trans, float("inf")
    print("Fit from the estimated pose: max error %.3g, end pose %s\nFit from the identity: max error %.3g, end pose %s"
          % (e1, np.array2string(with_pose, precision=4), e0, np.array2string(from_identity, precision=4)))
    assert e1 < max_dist
