"""Surface normals on the GPU (pcgx_kdtree_normals / _dev, csrc/normals.hip) against the float64 oracle
(tests/normals_oracle.py): neighbour counts exact on every kind of handle, normals and curvature to 1e-6,
degenerate points exact, and the normals feeding a point-to-plane Fit end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle as O
from pcgol_amd import _lib as L
from pcgol_amd import icp, kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_oracle as NO  # noqa: E402

pytestmark = pytest.mark.gpu


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _range_counts(t, q, radius):
    q = L.f32c(q).reshape(-1, 3)
    c = np.zeros(len(q), np.int64)
    L.check(L.lib().pcgx_kdtree_range_count(t._h, L.ptr(q), len(q), float(radius), L.ptr(c)))
    return c


def _cube():
    return synth.uniform_cloud(200_000, 1.0, 11), 0.05


def _surface():
    return synth.surface_cloud(1_000_000, 30.0, 6)[0], 0.1


def _queries(base, seed):
    """random points off the cloud inside its box, and points outside the box (count 0)"""
    lo, hi = base.min(0), base.max(0)
    r = _rng(seed)
    inside = (lo + r.random((20_000, 3)) * (hi - lo)).astype(np.float32)
    outside = (hi + 1.0 + r.random((500, 3))).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([inside, outside]), dtype=np.float32)


def _handles(base, monkeypatch):
    """(name, tree) for the grid path, the forced walk and a handle with 10 % of its points deleted"""
    t = kdtree.New(base)
    yield "grid", t
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    yield "walk", t
    monkeypatch.delenv("PCGX_RANGE_WALK")
    td = kdtree.New(base)
    td.DeletePoints(_rng(5).choice(len(base), len(base) // 10, replace=False))
    yield "deleted", td


@pytest.mark.parametrize("cloud", [_cube, _surface])
def test_counts_equal_range_count(cloud, monkeypatch):
    base, r = cloud()
    q = _queries(base, 1)
    for name, t in _handles(base, monkeypatch):
        n_own, c_own, k_own = t.Normals(r)  # q == NULL: the tree's own points, id order
        assert np.array_equal(k_own, _range_counts(t, base, r)), name
        n_q, c_q, k_q = t.Normals(r, Queries=q)
        want = _range_counts(t, q, r)
        assert np.array_equal(k_q, want), name
        assert np.all(k_q[-500:] == 0) and np.all(n_q[-500:] == 0) and np.all(np.isnan(c_q[-500:])), name


def _check_against_oracle(got, ref, q, viewpoint, what):
    normals, curvature, counts = got
    assert np.array_equal(counts, ref["counts"]), what
    deg = ref["degenerate"]
    assert np.array_equal(normals[deg], np.zeros((int(deg.sum()), 3), np.float32)), what
    assert np.all(np.isnan(curvature[deg])), what
    assert not np.any(np.isnan(curvature[~deg])), what
    lam = ref["lam"]
    good = ~deg & (lam[:, 1] - lam[:, 0] >= 1e-6 * lam[:, 2])
    a = normals.astype(np.float64)
    b = ref["normals"].astype(np.float64)
    sin = np.linalg.norm(np.cross(a[good], b[good]), axis=1) / (np.linalg.norm(a[good], axis=1) * np.linalg.norm(b[good], axis=1))
    assert good.sum() > 0.9 * (~deg).sum(), what
    assert np.max(sin, initial=0.0) <= 1e-6, (what, float(np.max(sin)))
    to_v = np.asarray(viewpoint, np.float64)[None, :] - q.astype(np.float64)
    side = np.sum(b * to_v, axis=1)
    clear = good & (np.abs(side) > 1e-6 * np.linalg.norm(to_v, axis=1))
    assert np.array_equal(np.sign(np.sum(a[clear] * b[clear], axis=1)), np.ones(int(clear.sum()))), what
    assert np.max(np.abs(curvature[good].astype(np.float64) - ref["curvature"][good]), initial=0.0) <= 1e-6, what
    rest = ~deg & ~good  # near-repeated smallest eigenvalues: unit length and orientation only
    assert np.allclose(np.linalg.norm(a[rest], axis=1), 1.0, atol=1e-6), what
    assert np.all(np.sum(a[rest] * to_v[rest], axis=1) >= -1e-6 * np.linalg.norm(to_v[rest], axis=1)), what


@pytest.mark.parametrize("cloud", [_cube, _surface])
def test_normals_match_oracle(cloud, monkeypatch):
    base, r = cloud()
    vp = (0.3, -2.0, 5.0)
    sub = _rng(2).choice(len(base), 20_000, replace=False)
    q = np.concatenate([base[sub], _queries(base, 3)[:5000]])
    for name, t in _handles(base, monkeypatch):
        offs, ids = NO.range_lists(t, q, r)
        ref = NO.normals_from_lists(base, q, offs, ids, vp, 3)
        _check_against_oracle(t.Normals(r, Viewpoint=vp, Queries=q), ref, q, vp, name + " queries")
        own = t.Normals(r, Viewpoint=vp)
        _check_against_oracle(tuple(x[sub] for x in own), NO.normals_from_lists(base, base[sub], *NO.range_lists(t, base[sub], r), vp, 3),
                              base[sub], vp, name + " own points")
    # min_neighbors: points of the cube with fewer neighbours than asked for are degenerate, exactly
    t = kdtree.New(base)
    counts = t.Normals(r)[2]
    mn = int(np.median(counts))
    n_hi, c_hi, k_hi = t.Normals(r, Viewpoint=vp, MinNeighbors=mn)
    low = k_hi < mn
    assert np.array_equal(k_hi, counts) and low.any()
    assert np.all(n_hi[low] == 0) and np.all(np.isnan(c_hi[low])) and not np.any(np.isnan(c_hi[~low]))


def test_coincident_heap(monkeypatch):
    h = np.float32([0.5, 0.5, 0.5])
    u = synth.uniform_cloud(100_000, 1.0, 12)
    u = u[np.linalg.norm(u - h, axis=1) > 0.06][:95_000]
    base = np.ascontiguousarray(np.concatenate([u, np.tile(h, (5000, 1))]), dtype=np.float32)
    heap = np.arange(len(u), len(base))
    r = 0.05
    beside = np.float32([[0.505, 0.5, 0.5], [0.5, 0.497, 0.5]])  # the heap alone within r
    for grid_mode in (None, "2"):  # the crowded cell takes the tree walk; PCGX_GRID=2 keeps the grid (wave-wide rows)
        if grid_mode:
            monkeypatch.setenv("PCGX_GRID", grid_mode)
        t = kdtree.New(base)
        n, c, k = t.Normals(r)
        assert np.array_equal(k, _range_counts(t, base, r))
        assert np.all(k[heap] == 5000)
        assert np.all(n[heap] == 0) and np.all(np.isnan(c[heap]))
        assert not np.any(np.isnan(c[:len(u)][k[:len(u)] >= 3]))
        nb, cb, kb = t.Normals(r, Queries=beside)
        assert np.all(kb == 5000) and np.all(nb == 0) and np.all(np.isnan(cb))
        sub = _rng(4).choice(len(u), 5000, replace=False)
        ref = NO.normals_from_lists(base, base[sub], *NO.range_lists(t, base[sub], r))
        _check_against_oracle(tuple(x[sub] for x in (n, c, k)), ref, base[sub], (0, 0, 0), "heap cloud")
        monkeypatch.delenv("PCGX_GRID", raising=False)


def test_host_and_device_entry_points_and_launch_order():
    import torch
    base, r = _cube()
    t = kdtree.New(base)
    q = _queries(base, 6)
    vp = (1.0, 2.0, 3.0)
    n, c, k = t.Normals(r, Viewpoint=vp, Queries=q)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(q).to(dev)
    dn = torch.empty((len(q), 3), dtype=torch.float32, device=dev)
    dc = torch.empty(len(q), dtype=torch.float32, device=dev)
    dk = torch.empty(len(q), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    t.NormalsDev(r, dn.data_ptr(), dc.data_ptr(), dk.data_ptr(), d_q=dq.data_ptr(), nq=len(q), Viewpoint=vp, stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(dn.cpu().numpy().view(np.uint32), n.view(np.uint32))
    assert np.array_equal(dc.cpu().numpy().view(np.uint32), c.view(np.uint32))
    assert np.array_equal(dk.cpu().numpy(), k)
    # own points through the device entry point: the host's bits
    dn2 = torch.empty((len(base), 3), dtype=torch.float32, device=dev)
    t.NormalsDev(r, dn2.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(dn2.cpu().numpy().view(np.uint32), t.Normals(r)[0].view(np.uint32))
    # shuffled queries (another launch order): the same neighbour sets, the same normals up to summation order
    perm = _rng(7).permutation(len(q))
    n2, c2, k2 = t.Normals(r, Viewpoint=vp, Queries=q[perm])
    assert np.array_equal(k2, k[perm])
    ref = NO.normals_from_lists(base, q, *NO.range_lists(t, q, r), vp, 3)
    _check_against_oracle((n2, c2, k2), {key: v[perm] for key, v in ref.items()}, q[perm], vp, "shuffled")
    # the tree's own points given as queries (caller order, Morton-sorted) against q == NULL (the grid's cell order)
    n3, c3, k3 = t.Normals(r, Viewpoint=vp, Queries=base)
    n4, c4, k4 = t.Normals(r, Viewpoint=vp)
    assert np.array_equal(k3, k4)
    both = ~np.isnan(c4)
    assert np.array_equal(both, ~np.isnan(c3))
    assert np.max(np.abs(c3[both] - c4[both])) <= 1e-6


def _angle_deg(a, b):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    cosang = np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0)))


def test_end_to_end_plane_fit_with_estimated_normals():
    import torch
    c = synth.c4_plane(40_000)
    base, target = c["base"], c["target"]
    t = kdtree.New(base)
    dev = torch.device("cuda", 0)
    vp = (3.0, 3.0, 100.0)  # above the surface: the analytic normals' side
    dn = torch.empty((len(base), 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t.NormalsDev(0.1, dn.data_ptr(), Viewpoint=vp, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    est = dn.cpu().numpy()
    assert np.all(np.abs(np.linalg.norm(est, axis=1) - 1.0) < 1e-5)
    ang = _angle_deg(est, c["normals"])
    assert np.median(ang) < 0.3 and np.percentile(ang, 99) < 1.5, (np.median(ang), np.percentile(ang, 99), ang.max())
    reg = icp.PointToPlaneICP(
        icp.PointToPlaneEvaluator(icp.NearestPointCorresponder(MaxDist=c["max_dist"]), est, MinPairs=6),
        icp.GaussNewtonUpdaterFactory(Threshold=c["threshold"], MaxIteration=8))
    trans, stat = reg.Fit(t, target)
    o = O.plane_fit(O.KDTree(base), est, target, c["max_dist"], 6, c["threshold"], 0.0, 8)
    assert stat.NumIteration == o["num_iteration"] == 8
    assert np.max(np.abs(trans - o["trans"])) <= 1e-5
    inv = np.linalg.inv(synth.icp_pose().astype(np.float64).reshape(4, 4).T).T.reshape(-1)
    assert np.max(np.abs(trans.astype(np.float64) - inv)) <= 2e-4
    # the same on the device end to end: target and normals in HBM, no host copy of either
    dt = torch.from_numpy(target).to(dev)
    torch.cuda.synchronize()
    s = icp.IcpSession(t, dt.data_ptr(), c["max_dist"], 6, None, c["threshold"], 8, target_on_device=True,
                       nt=len(target), BaseNormals=dn)
    try:
        for _ in range(8):
            s.step()
        tr2, st2, _ = s.result()
    finally:
        s.close()
    assert st2.NumIteration == 8
    assert np.max(np.abs(tr2 - o["trans"])) <= 1e-5
    assert np.max(np.abs(tr2.astype(np.float64) - inv)) <= 2e-4


def test_bad_arguments():
    base, r = synth.uniform_cloud(5000, 1.0, 13), 0.05
    t = kdtree.New(base)
    lib = L.lib()
    q = base[:10].copy()
    out = np.empty((len(base), 3), np.float32)
    vp = np.zeros(3, np.float32)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.pcgx_kdtree_normals(t._h, L.ptr(q), 10, bad, L.ptr(vp), 3, L.ptr(out), None, None) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_normals_dev(t._h, None, len(base), bad, None, 3, C.c_void_p(16), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_normals(t._h, None, len(base) - 1, r, None, 3, L.ptr(out), None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_normals(t._h, L.ptr(q), 10, r, None, 3, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_normals_dev(t._h, None, len(base) + 1, r, None, 3, C.c_void_p(16), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_normals(None, L.ptr(q), 10, r, None, 3, L.ptr(out), None, None) == L.PCGX_E_INVALID
    # nothing to do is not an error; a single query runs on the device as well
    assert lib.pcgx_kdtree_normals(t._h, L.ptr(q), 0, r, None, 3, None, None, None) == L.PCGX_OK
    n1, c1, k1 = t.Normals(r, Queries=q[:1])
    nq, cq, kq = t.Normals(r, Queries=q)
    assert np.array_equal(n1[0], nq[0]) and k1[0] == kq[0]
