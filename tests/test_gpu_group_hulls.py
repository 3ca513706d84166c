"""Group footprints on the device (include/pcgx.h, "group footprints"; csrc/group_hull.hip) against the exact oracle
(tests/hull_oracle.py) on both entry points, every scene twice with the same bits.

hull_sizes and hull_ids are array_equal the oracle's: the hull of a set of float32 points is a property of the set.
Tolerances of area and rectangle (none invented here, include/pcgx.h derives them; tests/test_hull_terms_host.py
measures the host build against them on these same scenes: 1.04 and 2.08 x 2^-53 D^2): the area within 2 h 2^-53 D^2 of
the exact one, D the diagonal of the group's xy box; the rectangle by property: it holds every live member within
s = 16 x 2^-53 (|p| + |centre|), u is a unit vector parallel to a hull edge within 16 x 2^-53, and its area is at most the
exact minimum over the edges plus 32 x 2^-53 D^2.  Which of tied edges wins is not compared.

The scene "points (i, i^2) and (i, -i^2)" is run as written (tests/hull_scenes.py, parabolas) -- but of that family only
the four end points are vertices, whatever the range of i: the two parabolas open towards each other's far side -- and
moved apart until the polygon is convex (all_vertices), which is the scene with h_g = members that the long path of
the chain needs."""
import collections
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, segmentation

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_scenes as GS  # noqa: E402
import hull_oracle as HO  # noqa: E402
import hull_scenes as HS  # noqa: E402
from test_hull_terms_host import AREA_BOUND, RECT_BOUND  # noqa: E402

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
Got = collections.namedtuple("Got", "hull_sizes hull_ids area rect")

_CACHE = {}


def _want(key, pts, ids, sizes, **kw):
    """the oracle's answer, computed once per scene and left unchanged"""
    if key not in _CACHE:
        _CACHE[key] = HO.group_hulls(pts, ids, sizes, **kw)
        for a in _CACHE[key][0]:
            a.setflags(write=False)
    return _CACHE[key]


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def _host_once(t, ids, sizes, skip=()):
    g, m = len(sizes), len(ids)
    out = [np.full(g, -7, np.int64), np.full(m, -7, np.int64), np.full(g, -7.0), np.full((g, 6), -7.0)]
    ids, sizes = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(sizes, np.int64)
    rc = L.lib().pcgx_kdtree_group_hulls(t._h, L.ptr(ids) if m else None, m, L.ptr(sizes) if g else None, g,
                                         *[None if k in skip or not a.size else L.ptr(a) for k, a in enumerate(out)])
    return rc, Got(*out)


def _host(t, ids, sizes):
    """the host entry point's outputs; a second call gives the same bits"""
    rc, a = _host_once(t, ids, sizes)
    assert rc == L.PCGX_OK, L.last_error()
    rc, b = _host_once(t, ids, sizes)
    assert rc == L.PCGX_OK and _bits_equal(a, b)
    return a


def _dev_once(t, d_ids, cap_ids, d_sizes, cap_groups, d_n, skip=(), stream=None):
    import torch
    dev = torch.device("cuda", 0)
    out = [torch.full((cap_groups,), -7, dtype=torch.int32, device=dev), torch.full((max(cap_ids, 1),), -7, dtype=torch.int32, device=dev),
           torch.full((cap_groups,), -7, dtype=torch.float64, device=dev), torch.full((cap_groups, 6), -7, dtype=torch.float64, device=dev)]
    t.GroupHullsDev(d_ids.data_ptr() if d_ids is not None else 0, cap_ids, d_sizes.data_ptr(), cap_groups,
                    d_n.data_ptr() if d_n is not None else 0,
                    *[0 if k in skip else o.data_ptr() for k, o in enumerate(out)], stream=stream or 0)
    out[1] = out[1][:cap_ids]
    return out


def _dev(t, ids, sizes, n_groups=None, cap_ids=None, skip=()):
    """the device entry point over int32 tensors; a second call gives the same bits; the integers widened to int64"""
    import torch
    dev = torch.device("cuda", 0)
    ids32 = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(dev) if len(ids) else None
    siz32 = torch.from_numpy(np.ascontiguousarray(sizes, np.int32)).to(dev)
    d_n = None if n_groups is None else torch.tensor([n_groups], dtype=torch.int32, device=dev)
    cap_ids = len(ids) if cap_ids is None else cap_ids
    a = _dev_once(t, ids32, cap_ids, siz32, len(sizes), d_n, skip)
    b = _dev_once(t, ids32, cap_ids, siz32, len(sizes), d_n, skip)
    torch.cuda.synchronize()
    a, b = ([x.cpu().numpy() for x in o] for o in (a, b))
    assert _bits_equal(a, b)
    return Got(a[0].astype(np.int64), a[1].astype(np.int64), a[2], a[3])


def _check(got, want, info, what):
    """every property of the module docstring"""
    W = want
    assert np.array_equal(got.hull_sizes, W.hull_sizes), what
    assert np.array_equal(got.hull_ids, W.hull_ids), what
    worst_a = worst_r = 0.0
    for g, h in enumerate(W.hull_sizes):
        D, P, V = info["D"][g], info["members"][g][:, :2].astype(np.float64), info["hulls"][g]
        a, r = got.area[g], got.rect[g]
        if h == 0:
            assert a == 0 and not r.any(), (what, g)
            continue
        if h == 1:
            assert a == 0 and r.tolist() == [V[0, 0], V[0, 1], 1.0, 0.0, 0.0, 0.0], (what, g)
            continue
        assert abs(a - W.area[g]) <= AREA_BOUND(h, D), (what, g, a, W.area[g])
        worst_a = max(worst_a, abs(a - W.area[g]) / (U53 * D * D))
        c, u, hu, hn = r[:2], r[2:4], r[4], r[5]
        n = np.array([-u[1], u[0]])
        assert abs(u @ u - 1.0) <= 16 * U53 and hu >= 0 and hn >= 0, (what, g)
        s = 16 * U53 * (np.linalg.norm(P, axis=1) + np.linalg.norm(c))
        e = P - c
        assert np.all(np.abs(e @ u) <= hu + s) and np.all(np.abs(e @ n) <= hn + s), (what, g)
        E = np.roll(V, -1, axis=0) - V
        E = E[:1] if h == 2 else E
        cross = np.abs(E[:, 0] * u[1] - E[:, 1] * u[0]) / np.linalg.norm(E, axis=1)
        assert cross.min() <= 16 * U53, (what, g, cross.min())
        if h == 2:
            assert a == 0 and hn == 0 and (E[0] @ u) > 0, (what, g)
            assert abs(2 * hu - np.linalg.norm(E[0])) <= 16 * U53 * D, (what, g)
        else:
            assert 4 * hu * hn <= W.rect_area[g] + RECT_BOUND(D), (what, g, 4 * hu * hn, W.rect_area[g])
            worst_r = max(worst_r, (4 * hu * hn - W.rect_area[g]) / (U53 * D * D))
    print("%s: area error %.3g, rectangle excess %.3g (x 2^-53 D^2)" % (what, worst_a, worst_r))


def _both(key, scene, **kw):
    pts, ids, sizes = scene
    t = kdtree.New(pts)
    want, info = _want(key, pts, ids, sizes)
    host, dev = _host(t, ids, sizes), _dev(t, ids, sizes)
    _check(host, want, info, key + ", host")
    _check(dev, want, info, key + ", device")
    return t, want, info, host, dev


# ------------------------------------------------------------------------------------------------ 1. the ladder

@pytest.mark.parametrize("reverse", [False, True])
def test_group_size_ladder(reverse):
    T = kdtree.GroupStatsTile()
    assert T == HS.TILE and kdtree.GroupHullsChunk() == 16
    pts, ids, sizes = HS.ladder(reverse)
    for k in (0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5):
        assert k in sizes.tolist()
    t, want, info, host, dev = _both("ladder %s" % reverse, (pts, ids, sizes))
    assert (want.hull_sizes[sizes == 0] == 0).all() and want.hull_sizes[sizes == 3].tolist() == [3]
    hs = want.hull_sizes
    assert any(hs[i] == 0 and hs[:i].any() and hs[i + 1:].any() for i in range(len(hs)))  # empty hulls between others
    # the capacity beyond the groups, the count on the device: the rows behind it are zero
    more = np.concatenate([sizes, [0, 5, 0]])
    want2, info2 = _want("ladder+ %s" % reverse, pts, ids, more, n_groups=len(sizes))
    _check(_dev(t, ids, more, n_groups=len(sizes)), want2, info2, "device, G below cap_groups")


# ------------------------------------------------------------------------------------------------ 2. every place a vertex

def test_every_place_a_vertex():
    t, want, info, host, dev = _both("all vertices", HS.all_vertices())
    assert want.hull_sizes.tolist() == HS.all_vertices()[2].tolist() == [3 * HS.TILE + 5, 64, 65]  # h_g = members


def test_parabolas_as_written():
    t, want, info, host, dev = _both("parabolas", HS.parabolas())
    assert want.hull_sizes.tolist() == [4, 4, 4]


# ------------------------------------------------------------------------------------------------ 3. degenerate counts

def test_lattices_collinear_points_and_copies():
    t, want, info, host, dev = _both("lattices", HS.lattice_scene())
    assert want.hull_sizes.tolist() == [4, 4, 2, 1]
    pts, ids, sizes = HS.lattice_scene()
    twice = ids[1600:4800]
    for got in (host, dev):
        v = got.hull_ids[4:8]
        for i in v:  # the smaller of the two ids at the place
            same = twice[(pts[twice, :2] == pts[i, :2]).all(axis=1)]
            assert len(same) == 2 and i == same.min()
        assert got.hull_ids[10] == ids[5300:].min() and got.area[0] == 39.0 * 39.0


# ------------------------------------------------------------------------------------------------ 4. the exact branch

def test_near_collinear_groups_need_the_exact_branch():
    scene = HS.near_collinear()
    t, want, info, host, dev = _both("near collinear", scene)
    hs = want.hull_sizes.reshape(32, 32, 2)
    i, j = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    # far points on the left: b is a vertex when a lies left of the diagonal (j > i); on the right: when i > j
    assert np.array_equal(hs[:, :, 0] == 5, j > i) and np.array_equal(hs[:, :, 1] == 5, i > j)
    assert set(hs.ravel().tolist()) == {4, 5}


# ------------------------------------------------------------------------------------------------ 5. slots

def test_slots_repeated_deleted_and_non_finite_members():
    pts, ids, sizes = GS.slots()
    t, want, info, host, dev = _both("slots", (pts, ids, sizes))
    assert want.hull_sizes[2] == 1 and want.hull_sizes[3] == 0  # one id five times; the NaN and the infinite point alone
    assert host.hull_ids[want.hull_sizes[:2].sum()] == 60
    t.DeletePoints(np.concatenate([np.arange(0, 40, 3), [50, 60, 73], np.arange(100, 300, 7)]))
    _check(_host(t, ids, sizes), want, info, "host, after DeletePoints")  # deleted ids use the stored coordinates
    _check(_dev(t, ids, sizes), want, info, "device, after DeletePoints")


def test_slots_device_only_faults():
    pts, ids, sizes = GS.slots()
    n = len(pts)
    t = kdtree.New(pts)
    bad = ids.copy()
    bad[[3, 17, 44, 60, 61, 259]] = [-1, n, -1, n + 5, 2 ** 31 - 1, -1]  # -1 in the middle and at the end, ids >= Len()
    want, info = _want("slots bad ids", pts, bad, sizes)
    _check(_dev(t, bad, sizes), want, info, "dead ids")
    for ng in (len(sizes) + 3, -2, 0, 2):  # *d_n_groups above cap_groups, below 0, zero, inside
        w, i = _want(("slots G", ng), pts, ids, sizes, n_groups=ng)
        assert (w.hull_sizes > 0).sum() == (5 if ng > 2 else min(max(ng, 0), 2))
        _check(_dev(t, ids, sizes, n_groups=ng), w, i, "G = %d" % ng)
    for cap in (47, 45, 40, 0):  # a size sum beyond cap_ids: the list is clipped, the later groups are empty
        w, i = _want(("slots cap", cap), pts, ids, sizes, cap_ids=cap)
        _check(_dev(t, ids, sizes, cap_ids=cap), w, i, "cap_ids = %d" % cap)
        assert not w.hull_sizes[3:].any()
    big = sizes.copy()
    big[1] = 2 ** 31 - 1  # a size far beyond the list
    big[2] = -5           # a negative size owns nothing
    w, i = _want("slots big", pts, ids, big)
    assert w.hull_sizes[1] > 3 and not w.hull_sizes[2:].any()
    _check(_dev(t, ids, big), w, i, "a size beyond the list")


def test_host_form_rejects_and_writes_nothing():
    lib = L.lib()
    pts, ids, sizes = GS.slots()
    n = len(pts)
    t = kdtree.New(pts)
    E = L.PCGX_E_INVALID
    for k, v in ((3, -1), (259, -1), (17, n), (60, 2 ** 40)):
        bad = ids.copy()
        bad[k] = v
        rc, out = _host_once(t, bad, sizes)
        assert rc == E and all(np.all(a == -7) for a in out), (k, v)
        assert "pcgx_kdtree_group_hulls: id out of range" in L.last_error()
    big = sizes.copy()
    big[-1] += 1  # a size sum above n_ids
    rc, out = _host_once(t, ids, big)
    assert rc == E and all(np.all(a == -7) for a in out)
    assert "pcgx_kdtree_group_hulls: the sizes add up to more than n_ids" in L.last_error()
    neg = np.concatenate([sizes, [-4]])  # a negative size counts as 0
    rc, out = _host_once(t, ids, neg)
    assert rc == L.PCGX_OK and out.hull_sizes[-1] == 0 and out.hull_sizes[0] > 2
    i64 = np.zeros(4, np.int64)
    hs = np.full(4, -7, np.int64)

    def call(h=t._h, i=i64, ni=4, s=i64, ns=4):
        return lib.pcgx_kdtree_group_hulls(h, None if i is None else L.ptr(i), ni, None if s is None else L.ptr(s), ns,
                                           L.ptr(hs), None, None, None)

    assert call(ns=0) == L.PCGX_OK and np.all(hs == -7)  # no group: nothing to write
    assert call(ni=0, i=None) == L.PCGX_OK and not hs.any()  # no slot: every row zero
    assert call(h=None) == E and call(ni=-1) == E and call(ns=-1) == E
    assert call(i=None) == E and call(s=None) == E
    assert call(ni=2 ** 31) == E and call(ns=2 ** 31) == E
    d = lambda *a: lib.pcgx_kdtree_group_hulls_dev(*a, *([None] * 4), None)  # noqa: E731
    one = L.ptr(1 << 20)  # (never dereferenced: every call below is refused, or has nothing to do)
    assert d(None, one, 4, one, 4, None) == E
    assert d(t._h, one, -1, one, 4, None) == E and d(t._h, one, 4, one, -1, None) == E
    assert d(t._h, None, 4, one, 4, None) == E and d(t._h, one, 4, None, 4, None) == E
    assert d(t._h, one, 2 ** 31, one, 4, None) == E and d(t._h, one, 4, one, 2 ** 31, None) == E
    assert d(t._h, one, 4, one, 0, None) == L.PCGX_OK
    with pytest.raises(L.PcgxError):
        t.GroupHulls([0, n], [2])


# ------------------------------------------------------------------------------------------------ 6. the chain

def test_chain_clusters_to_footprints_on_one_stream():
    """ClustersDev -> GroupHullsDev on one stream over torch tensors, nothing read back in between: bit for bit the host
    form's over the host clusters call's ids and sizes; Extract() then Footprints(); the hull's box is the group's box;
    the hulls put back in come out unchanged."""
    import torch
    dev = torch.device("cuda", 0)
    pts = GS.chain_cloud()
    n = len(pts)
    t = kdtree.New(pts)
    lab, cnt, siz, ids, hs, hid = (torch.full((k,), -7, dtype=torch.int32, device=dev) for k in (n, 1, n, n, n, n))
    area, rect = torch.full((n,), -7.0, dtype=torch.float64, device=dev), torch.full((n, 6), -7.0, dtype=torch.float64, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        t.ClustersDev(GS.CHAIN_RADIUS, lab.data_ptr(), cnt.data_ptr(), siz.data_ptr(), ids.data_ptr(), stream=st.cuda_stream)
        t.GroupHullsDev(ids.data_ptr(), n, siz.data_ptr(), n, cnt.data_ptr(), hs.data_ptr(), hid.data_ptr(), area.data_ptr(),
                        rect.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    torch.cuda.synchronize()
    c = int(cnt.cpu()[0])
    got = Got(hs.cpu().numpy().astype(np.int64), hid.cpu().numpy().astype(np.int64), area.cpu().numpy(), rect.cpu().numpy())
    _, h_sizes, h_ids = t.Clusters(GS.CHAIN_RADIUS)
    assert c == len(h_sizes) == 3070 and h_sizes[0] == 1754
    host = _host(t, h_ids, h_sizes)
    assert np.array_equal(got.hull_sizes[:c], host.hull_sizes) and not got.hull_sizes[c:].any()
    assert np.array_equal(got.hull_ids[: len(h_ids)], host.hull_ids) and np.all(got.hull_ids[len(h_ids):] == -1)
    assert _bits_equal([got.area[:c], got.rect[:c]], [host.area, host.rect]) and not got.area[c:].any() and not got.rect[c:].any()
    want, info = _want("chain", *GS.chain())
    assert np.array_equal(GS.chain()[1], h_ids) and np.array_equal(GS.chain()[2], h_sizes)
    _check(host, want, info, "chain")
    ce = segmentation.ClusterExtraction(t, ClusterTolerance=GS.CHAIN_RADIUS)
    parts = ce.Extract()
    feet = ce.Footprints()
    assert len(parts) == c and _bits_equal(feet, host)
    total = int(host.hull_sizes.sum())
    box_all, box_hull = t.GroupStats(h_ids, h_sizes).aabb, t.GroupStats(host.hull_ids[:total], host.hull_sizes).aabb
    assert np.array_equal(box_hull[:, (0, 1, 3, 4)], box_all[:, (0, 1, 3, 4)])  # a hull reaches its group's x and y extremes
    again = t.GroupHulls(host.hull_ids[:total], host.hull_sizes)
    assert np.array_equal(again.hull_sizes, host.hull_sizes) and np.array_equal(again.hull_ids, host.hull_ids[:total])
    assert _bits_equal([again.area, again.rect], [host.area, host.rect])


# ------------------------------------------------------------------------------------------------ 7. null outputs

def test_each_output_left_out():
    pts, ids, sizes = GS.slots()
    t = kdtree.New(pts)
    full_h, full_d = _host(t, ids, sizes), _dev(t, ids, sizes)
    assert _bits_equal(full_h, full_d)
    for k in range(4):
        rc, h = _host_once(t, ids, sizes, skip=(k,))
        assert rc == L.PCGX_OK
        d = _dev(t, ids, sizes, skip=(k,))
        for j in range(4):
            if j == k:
                assert np.all(h[j] == -7) and np.all(d[j] == -7)  # not touched
            else:
                assert _bits_equal([h[j]], [full_h[j]]) and _bits_equal([d[j]], [full_d[j]]), (k, j)
    rc, h = _host_once(t, ids, sizes, skip=tuple(range(4)))
    assert rc == L.PCGX_OK
