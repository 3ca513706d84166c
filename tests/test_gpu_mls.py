"""Moving-least-squares smoothing on the GPU (pcgx_kdtree_mls / _dev, csrc/mls.hip) against the float64 oracle
(tests/mls_oracle.py), over neighbour lists from RangeBatch on the same handle.

Tolerance (mls_oracle.check): every coordinate of a position within 2^-23 |oracle| (the one float32 rounding, doubled)
+ 1e-12 radius / p, p the oracle's pivot ratio (float64 summation order and eigenvector noise amplified by the solve's
conditioning; on the CPU two summation orders differ by 1.7e-15 radius at p >= 0.034 on the surface scene and by at
most 4.6e-10 radius on the heap scene, tests/test_mls_oracle.py); normals within sin 1e-6.  Both on the good queries
only: oracle kind 2, eigen-gap >= 1e-3, p >= 1e-6.  Counts are always exact; kinds are exact except where p lies in
(1e-12, 1e-8) or ||c0| - radius| <= 1e-6 radius (either of kind 1 and 2 passes); a kind 0 output is the query's bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mls_oracle as MO  # noqa: E402
import normals_oracle as NO  # noqa: E402
from test_mls_oracle import R, check_case_kinds, hand_cases  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32

_CACHE = {}


def _surface():
    """(noisy points, 500 queries inside the box + 50 outside)"""
    if "surface" not in _CACHE:
        noisy = MO.noisy_surface()[0]
        _CACHE["surface"] = (noisy, MO.surface_queries(noisy))
    return _CACHE["surface"]


def _tree(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _surface_tree():
    return _tree("surface tree", lambda: kdtree.New(_surface()[0]))


def _reference(t, points, queries, radius, **kw):
    """the oracle over RangeBatch's lists on the handle t"""
    return MO.mls_from_lists(points, queries, *NO.range_lists(t, queries, radius), radius, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("handle", ["grid", "walk", "deleted"])
def test_noisy_surface_against_oracle(handle, monkeypatch):
    noisy, q = _surface()
    if handle == "deleted":
        t = kdtree.New(noisy)
        t.DeletePoints(np.arange(0, len(noisy), 10))  # every tenth id
    else:
        t = _surface_tree()
        if handle == "walk":
            monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    vp = (1.0, 1.0, 50.0)
    ref = _reference(t, noisy, noisy, R, viewpoint=vp)
    own = t.MLS(R, Viewpoint=vp)
    good = MO.check(own, ref, R, handle + " own points")
    assert good.sum() >= 0.99 * (ref["kinds"] != 0).sum()
    ref_q = _reference(t, noisy, q, R, viewpoint=vp)
    got_q = t.MLS(R, Viewpoint=vp, Queries=q)
    good_q = MO.check(got_q, ref_q, R, handle + " queries")
    assert good_q[:500].sum() >= 0.95 * 500
    assert np.all(got_q[2][500:] == 0) and np.all(got_q[3][500:] == 0) and np.all(got_q[1][500:] == 0)
    assert np.array_equal(_bits(got_q[0][500:]), _bits(q[500:]))  # outside the box: the query's bits
    if handle == "deleted":
        assert ref["counts"].mean() < 0.92 * 47.5  # (the deleted ids are queries still, and nobody's neighbours)
    else:
        assert np.all(own[2] == 2) and abs(own[3].mean() - 47.5) < 0.1
        ratio, before, after = MO.rms_ratio(noisy, own[0])
        print("interior RMS distance to the surface %.6f -> %.6f: ratio %.2f" % (before, after, ratio))
        assert ratio >= 3.0  # the library's own output puts the points back onto the surface


def test_prefixes_orders_min_neighbors_and_sigma():
    noisy, _ = _surface()
    t = _surface_tree()
    offs, ids = NO.range_lists(t, noisy[:129], R)
    for nq in (0, 1, 63, 64, 65, 129):
        for order in (1, 2):
            for sigma in (R / 2, R):
                got = t.MLS(R, Sigma=sigma, Order=order, Queries=noisy[:nq])
                assert [a.shape for a in got] == [(nq, 3), (nq, 3), (nq,), (nq,)]
                ref = MO.mls_from_lists(noisy, noisy[:nq], offs[:nq + 1], ids[:offs[nq]], R, sigma, order)
                good = MO.check(got, ref, R, "nq %d order %d sigma %g" % (nq, order, sigma))
                assert np.all(ref["kinds"] == order) and (order == 1 or good.all())
                if order == 1:  # the plane's projection: no solve, so no conditioning to divide by
                    err = np.abs(got[0].astype(np.float64) - ref["points64"])
                    assert np.all(err <= 2.0 ** -23 * np.abs(ref["points64"]) + 1e-12 * R)
                    a, b = got[1].astype(np.float64), ref["normals64"]
                    assert np.all(np.linalg.norm(np.cross(a, b), axis=1) <= 1e-6) and np.all(np.sum(a * b, axis=1) > 0)
    counts = np.diff(offs)
    mn = int(np.median(counts))
    for order in (1, 2):
        got = t.MLS(R, Order=order, MinNeighbors=mn, Queries=noisy[:129])
        ref = MO.mls_from_lists(noisy, noisy[:129], offs, ids, R, order=order, min_neighbors=mn)
        MO.check(got, ref, R, "min neighbours %d order %d" % (mn, order))
        low = counts < mn
        assert low.any() and (~low).any() and np.all(got[2][low] == 0) and np.all(got[2][~low] == order)
        assert np.array_equal(_bits(got[0][low]), _bits(noisy[:129][low]))


@pytest.mark.parametrize("radius", [0.75, 1.0])
def test_fat_rows(radius, monkeypatch):
    from test_gpu_radius_edges import _heap_queries, _heap_scene
    pts, q = _heap_scene(), _heap_queries(5)
    t = _tree("heap tree", lambda: kdtree.New(pts))
    ref = _reference(t, pts, q, radius)
    fat = MO.good(ref) & (ref["counts"] >= 4096)
    print("good queries with a fat row: %d, fragile: %d" % (fat.sum(), MO.fragile(ref, radius).sum()))
    assert fat.sum() >= 50  # the scene does its job: the wave-shared rows are compared, not filtered away
    got = t.MLS(radius, Queries=q)
    MO.check(got, ref, radius, "heaps r=%g grid" % radius)
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    got_w = t.MLS(radius, Queries=q)
    MO.check(got_w, ref, radius, "heaps r=%g walk" % radius)


def test_hand_cases_and_non_finite_queries():
    for c in hand_cases():
        t = kdtree.New(c["points"])
        got = t.MLS(c["radius"], Sigma=c["sigma"], Order=c["order"], MinNeighbors=c["min_neighbors"], Queries=c["queries"])
        ref = _reference(t, c["points"], c["queries"], c["radius"], sigma=c["sigma"], order=c["order"],
                         min_neighbors=c["min_neighbors"])
        points, normals, kinds, counts = got
        assert np.array_equal(counts, ref["counts"]), c["name"]
        check_case_kinds(c, kinds)
        z = kinds == 0
        assert np.array_equal(_bits(points[z]), _bits(c["queries"][z])) and np.all(normals[z] == 0), c["name"]
        assert np.allclose(np.linalg.norm(normals[~z].astype(np.float64), axis=1), 1.0, atol=1e-6), c["name"]
        if not isinstance(c["kinds"], tuple):
            MO.check(got, ref, c["radius"], c["name"])
        if c["name"] == "coplanar lattice":
            assert np.all(np.abs(normals.astype(np.float64) - [0, 0, -1]) <= 1e-7)
            assert np.all(np.abs(points[:, 2] - f32(0.5)) <= 2.0 ** -23)
            assert np.max(np.abs(points[:, :2] - c["queries"][:, :2])) <= 2.0 ** -23
        if c["name"].startswith("collinear"):
            assert np.max(np.abs(points.astype(np.float64) - c["queries"])) <= 1e-6 * c["radius"]
        if c["name"] == "every weight underflows":
            assert np.all(np.abs(points[:, 2] - f32(0.5)) <= 2.0 ** -23)  # the plane's projection
    # a NaN query and a +Inf query have no neighbours on any path: kind 0, their own bits
    noisy, _ = _surface()
    t = _surface_tree()
    q = np.concatenate([noisy[:3], f32([[np.nan, 1.0, 0.2], [np.inf, 1.0, 0.2]]), noisy[3:6]])
    points, normals, kinds, counts = t.MLS(R, Queries=q)
    assert kinds.tolist() == [2, 2, 2, 0, 0, 2, 2, 2] and counts[3:5].tolist() == [0, 0]
    assert np.array_equal(_bits(points[3:5]), _bits(q[3:5])) and np.all(normals[3:5] == 0)


def test_same_bits_twice_host_and_device_and_nullable_outputs():
    import torch
    noisy, q = _surface()
    t = _surface_tree()
    vp = (1.0, 2.0, 30.0)
    for queries in (None, q):
        for order in (1, 2):
            a = t.MLS(R, Sigma=0.1, Order=order, Viewpoint=vp, Queries=queries)
            b = t.MLS(R, Sigma=0.1, Order=order, Viewpoint=vp, Queries=queries)
            for x, y in zip(a, b):
                assert np.array_equal(_bits(x), _bits(y))
    # the device form on torch tensors, on a stream of its own with one synchronise
    host = t.MLS(R, Sigma=0.1, Viewpoint=vp, Queries=q)
    dev = torch.device("cuda", 0)
    n = len(q)
    dq = torch.from_numpy(q).to(dev)
    dp = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dkind = torch.empty(n, dtype=torch.int32, device=dev)
    dk = torch.empty(n, dtype=torch.int32, device=dev)
    dp2 = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dp_own = torch.empty((len(noisy), 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        t.MLSDev(R, dp.data_ptr(), dn.data_ptr(), dkind.data_ptr(), dk.data_ptr(), d_q=dq.data_ptr(), nq=n, Sigma=0.1,
                 Viewpoint=vp, stream=st)
        t.MLSDev(R, dp2.data_ptr(), d_q=dq.data_ptr(), nq=n, Sigma=0.1, Viewpoint=vp, stream=st)  # every nullable output NULL
        t.MLSDev(R, dp_own.data_ptr(), Sigma=0.1, Viewpoint=vp, stream=st)  # the tree's own points
    stream.synchronize()
    for x, y in zip((dp, dn, dkind, dk), host):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y))
    assert np.array_equal(_bits(dp2.cpu().numpy()), _bits(host[0]))
    assert np.array_equal(_bits(dp_own.cpu().numpy()), _bits(t.MLS(R, Sigma=0.1, Viewpoint=vp)[0]))
    # the host form with every nullable output NULL, and a NULL viewpoint (the origin)
    lib = L.lib()
    only = np.empty((n, 3), f32)
    L.check(lib.pcgx_kdtree_mls(t._h, L.ptr(q), n, R, 0.1, 2, 3, L.ptr(np.asarray(vp, f32)), L.ptr(only), None, None, None))
    assert np.array_equal(_bits(only), _bits(host[0]))
    nrm = np.empty((n, 3), f32)
    L.check(lib.pcgx_kdtree_mls(t._h, L.ptr(q), n, R, 0.1, 2, 3, None, L.ptr(only), L.ptr(nrm), None, None))
    at_origin = t.MLS(R, Sigma=0.1, Queries=q)
    assert np.array_equal(_bits(only), _bits(at_origin[0])) and np.array_equal(_bits(nrm), _bits(at_origin[1]))


def test_bad_arguments():
    noisy, _ = _surface()
    t = _surface_tree()
    lib = L.lib()
    q = noisy[:10].copy()
    n = len(noisy)
    out = np.empty((n, 3), f32)
    some = C.c_void_p(16)  # (a device address that is never read: the arguments are refused first)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.pcgx_kdtree_mls(t._h, L.ptr(q), 10, bad, R, 2, 3, None, L.ptr(out), None, None, None) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_mls(t._h, L.ptr(q), 10, R, bad, 2, 3, None, L.ptr(out), None, None, None) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_mls_dev(t._h, None, n, bad, R, 2, 3, None, some, None, None, None, None) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_mls_dev(t._h, None, n, R, bad, 2, 3, None, some, None, None, None, None) == L.PCGX_E_INVALID
    for order in (0, 3, -1):
        assert lib.pcgx_kdtree_mls(t._h, L.ptr(q), 10, R, R, order, 3, None, L.ptr(out), None, None, None) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_mls_dev(t._h, None, n, R, R, order, 3, None, some, None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_mls(None, L.ptr(q), 10, R, R, 2, 3, None, L.ptr(out), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_mls_dev(None, some, 10, R, R, 2, 3, None, some, None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_mls(t._h, L.ptr(q), -1, R, R, 2, 3, None, L.ptr(out), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_mls_dev(t._h, some, -1, R, R, 2, 3, None, some, None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_mls(t._h, None, n - 1, R, R, 2, 3, None, L.ptr(out), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_mls_dev(t._h, None, n + 1, R, R, 2, 3, None, some, None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_mls(t._h, L.ptr(q), 10, R, R, 2, 3, None, None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_mls_dev(t._h, some, 10, R, R, 2, 3, None, None, None, None, None, None) == L.PCGX_E_INVALID
    assert "points" in L.last_error()
    # nothing to do is not an error, on either entry point
    assert lib.pcgx_kdtree_mls(t._h, L.ptr(q), 0, R, R, 2, 3, None, None, None, None, None) == L.PCGX_OK
    assert lib.pcgx_kdtree_mls_dev(t._h, some, 0, R, R, 2, 3, None, None, None, None, None, None) == L.PCGX_OK
    # a single query runs on the device as well
    one = t.MLS(R, Queries=q[:1])
    ten = t.MLS(R, Queries=q)
    assert np.array_equal(_bits(one[0][0]), _bits(ten[0][0])) and one[3][0] == ten[3][0]
