"""Group geometry on the device (include/pcgx.h, "group geometry"; csrc/group_stats.hip) against the NumPy oracle
(tests/group_oracle.py) on both entry points, every scene twice with the same bits.

Tolerances (none invented here): count, aabb, padding rows and error codes exactly; cov and centroid within the
contract's bounds; frames by properties against TAU = 4 x the residual measured on the CPU over these same scenes
(tests/test_group_terms_host.py, TAU_MEASURED = 2.3e-15: the larger of the host-compiled group_terms.h's and
numpy.linalg.eigh's; the factor covers the difference of the device's arithmetic from the host build's); eigenvalues
against eigh's within the covariance bound plus TAU x trace (Weyl), axes against eigh's only where both neighbouring
eigenvalue gaps exceed 1e-3 x trace, within (covariance bound + TAU x trace) / gap (Davis-Kahan); the oriented box by
containment and tightness within s = 16 x 2^-53 (|p| + |centre|)."""
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, segmentation

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_oracle as GO  # noqa: E402
import group_scenes as GS  # noqa: E402
from test_group_terms_host import TAU_MEASURED  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
TAU = 4 * TAU_MEASURED  # measured 2.3e-15 on the CPU, x 4
U53 = 2.0 ** -53
GAP = 1e-3
SHAPES = ((), (6,), (3,), (6,), (3,), (3, 3), (6,))  # a row of count, aabb, centroid, cov, eig, axes, obb
DTYPES = (np.int64, f32, np.float64, np.float64, np.float64, np.float64, np.float64)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _want(key, pts, ids, sizes, **kw):
    """the oracle's answer, computed once per scene and left unchanged"""
    S, info = _cached(("want", key), lambda: GO.group_stats(pts, ids, sizes, **kw))
    for a in S:
        a.setflags(write=False)
    return S, info


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def _host_once(t, ids, sizes, skip=()):
    g = len(sizes)
    out = [np.full((g,) + s, -7, d) for s, d in zip(SHAPES, DTYPES)]
    ids, sizes = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(sizes, np.int64)
    rc = L.lib().pcgx_kdtree_group_stats(t._h, L.ptr(ids) if len(ids) else None, len(ids), L.ptr(sizes) if g else None, g,
                                         *[None if k in skip else L.ptr(a) for k, a in enumerate(out)])
    return rc, GO.Stats(*out)


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
    tds = (torch.int32, torch.float32) + (torch.float64,) * 5
    out = [torch.full((cap_groups,) + s, -7, dtype=d, device=dev) for s, d in zip(SHAPES, tds)]
    t.GroupStatsDev(d_ids.data_ptr() if d_ids is not None else 0, cap_ids, d_sizes.data_ptr(), cap_groups,
                    d_n.data_ptr() if d_n is not None else 0,
                    *[0 if k in skip else o.data_ptr() for k, o in enumerate(out)], stream=stream or 0)
    return out


def _dev(t, ids, sizes, n_groups=None, cap_ids=None, skip=()):
    """the device entry point over int32 tensors; a second call gives the same bits; count widened to int64"""
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
    a[0] = a[0].astype(np.int64)
    return GO.Stats(*a)


def _check(got, want, info, what, compare_axes=True):
    """every property of the module docstring; -> the share of groups of size >= 10 whose axes the gap rule left out"""
    assert np.array_equal(got.count, want.count), what
    assert np.array_equal(got.aabb, want.aabb), what
    empty = want.count == 0
    for a in got:
        assert not a[empty].any(), what  # rows of groups without a live member, and rows >= G: all zero
    live = ~empty
    assert np.all(np.abs(got.cov - want.cov) <= info["cov_bound"][:, None]), (what, np.abs(got.cov - want.cov).max())
    assert np.all(np.abs(got.centroid - want.centroid) <= info["centroid_bound"]), what
    if not live.any():
        return 0.0
    eig, axes = got.eig[live], got.axes[live]
    tr = got.cov[live][:, [0, 3, 5]].sum(axis=1)
    assert np.all(np.diff(eig, axis=1) <= 0), what
    flat = ~(tr > 0)  # every member at one place: eig 0, axes identity
    assert not eig[flat].any() and np.all(axes[flat] == np.eye(3)), what
    assert np.allclose(np.linalg.det(axes), 1.0, atol=8 * TAU), what
    orth, res = GO.frame_residuals(got.cov[live], eig, axes)
    assert orth.max() <= TAU and res.max() <= TAU, (what, orth.max(), res.max())
    for a in axes:  # the contract's signs, and the right hand
        assert np.array_equal(GO.sign(a[0]), a[0]) and np.array_equal(GO.sign(a[1]), a[1]), what
        assert np.all(np.abs(np.cross(a[0], a[1]) - a[2]) <= 2.0 ** -52), what
    weyl = info["cov_bound"][live] + TAU * tr
    assert np.all(np.abs(eig - want.eig[live]) <= weyl[:, None]), (what, np.abs(eig - want.eig[live]).max())
    gaps = np.stack([eig[:, 0] - eig[:, 1], np.minimum(eig[:, 0] - eig[:, 1], eig[:, 1] - eig[:, 2]), eig[:, 1] - eig[:, 2]], axis=1)
    clear = (tr > 0) & (np.minimum(eig[:, 0] - eig[:, 1], eig[:, 1] - eig[:, 2]) > GAP * np.where(tr > 0, tr, 1.0))
    if compare_axes and clear.any():
        sin = np.linalg.norm(np.cross(axes[clear], want.axes[live][clear]), axis=2)  # (m, 3): up to the sign
        assert np.all(sin <= weyl[clear, None] / gaps[clear]), (what, sin.max())
    # the oriented box: every member inside, every face touched
    for g in np.flatnonzero(live):
        P = info["members"][g].astype(np.float64)
        centre, h = got.obb[g, :3], got.obb[g, 3:]
        assert np.all(h >= 0), what
        e = (P - centre) @ got.axes[g].T
        s = (16 * U53 * (np.linalg.norm(P, axis=1) + np.linalg.norm(centre)))[:, None]
        assert np.all(np.abs(e) <= h + s), (what, g)
        assert np.all(((h - e) <= s).any(axis=0)) and np.all(((h + e) <= s).any(axis=0)), (what, g)
    big = want.count[live] >= 10
    return float(1.0 - clear[big].mean()) if big.any() else 0.0


# ------------------------------------------------------------------------------------------------ 1. run boundaries

@pytest.mark.parametrize("reverse", [False, True])
def test_run_boundaries(reverse):
    T = kdtree.GroupStatsTile()
    assert T == GS.TILE  # (the scenes of the CPU measurement are these)
    pts, ids, sizes = GS.boundaries(T, reverse)
    s = sizes.tolist()
    for k in (0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5):
        assert k in s
    off = np.cumsum(sizes)
    assert any(o % T == 0 and sizes[i] > 0 and i + 1 < len(sizes) and sizes[i + 1] > 0 for i, o in enumerate(off)) or reverse
    assert len(pts) <= 20_000
    t = kdtree.New(pts)
    want, info = _want(("boundaries", reverse), pts, ids, sizes)
    assert np.array_equal(want.count, sizes)
    _check(_host(t, ids, sizes), want, info, "host")
    _check(_dev(t, ids, sizes), want, info, "device")
    # the capacity beyond the groups, the count on the device: the rows behind it are zero
    more = np.concatenate([sizes, [0, 5, 0]])
    want2, info2 = _want(("boundaries+", reverse), pts, ids, more, n_groups=len(sizes))
    _check(_dev(t, ids, more, n_groups=len(sizes)), want2, info2, "device, G below cap_groups")


# ------------------------------------------------------------------------------------------------ 2. slots

def test_slots_repeated_deleted_and_non_finite_members():
    pts, ids, sizes = GS.slots()
    t = kdtree.New(pts)  # (a tree takes NaN and infinite points, as test_gpu_radius_edges.py's scenes do)
    want, info = _want("slots", pts, ids, sizes)
    assert want.count.tolist() == [38, 5, 5, 0, 6, 200]  # the NaN point 7 and the infinite point 11 are not counted
    assert not want.cov[2].any() and want.centroid[2].tolist() == pts[60].astype(np.float64).tolist()  # one id five times
    for name, got in (("host", _host(t, ids, sizes)), ("device", _dev(t, ids, sizes))):
        _check(got, want, info, name)
        assert got.count[2] == 5 and not got.eig[2].any() and np.array_equal(got.axes[2], np.eye(3))
        assert got.obb[2].tolist() == pts[60].astype(np.float64).tolist() + [0, 0, 0]
    # ids of deleted points use the stored coordinates
    t.DeletePoints(np.concatenate([np.arange(0, 40, 3), [50, 60, 73], np.arange(100, 300, 7)]))
    _check(_host(t, ids, sizes), want, info, "host, after DeletePoints")
    _check(_dev(t, ids, sizes), want, info, "device, after DeletePoints")


def test_slots_device_only_faults():
    pts, ids, sizes = GS.slots()
    n = len(pts)
    t = kdtree.New(pts)
    bad = ids.copy()
    bad[[3, 17, 44, 60, 61, 259]] = [-1, n, -1, n + 5, 2 ** 31 - 1, -1]  # -1 in the middle and at the end, ids >= Len()
    want, info = _want("slots bad ids", pts, bad, sizes)
    assert want.count.tolist() == [36, 4, 5, 0, 6, 197]
    _check(_dev(t, bad, sizes), want, info, "dead ids")
    for ng in (len(sizes) + 3, -2, 0, 2):  # *d_n_groups above cap_groups, below 0, zero, inside
        w, i = _want(("slots G", ng), pts, ids, sizes, n_groups=ng)
        assert (w.count > 0).sum() == (5 if ng > 2 else min(max(ng, 0), 2))
        _check(_dev(t, ids, sizes, n_groups=ng), w, i, "G = %d" % ng)
    # a size sum beyond cap_ids: the list is clipped, the later groups are empty
    for cap in (47, 45, 40, 0):
        w, i = _want(("slots cap", cap), pts, ids, sizes, cap_ids=cap)
        _check(_dev(t, ids, sizes, cap_ids=cap), w, i, "cap_ids = %d" % cap)
        assert not w.count[3:].any()
    big = sizes.copy()
    big[1] = 2 ** 31 - 1  # a size far beyond the list
    big[2] = -5           # a negative size owns nothing
    w, i = _want("slots big", pts, ids, big)
    assert w.count[0] == 38 and w.count[1] == len(ids) - 40 - 4 and not w.count[2:].any()
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
    big = sizes.copy()
    big[-1] += 1  # a size sum above n_ids
    rc, out = _host_once(t, ids, big)
    assert rc == E and all(np.all(a == -7) for a in out)
    neg = np.concatenate([sizes, [-4]])  # a negative size counts as 0
    rc, out = _host_once(t, ids, neg)
    assert rc == L.PCGX_OK and out.count.tolist() == [38, 5, 5, 0, 6, 200, 0]
    i64 = np.zeros(4, np.int64)
    cnt = np.full(4, -7, np.int64)
    nul = [None] * 6

    def call(h=t._h, i=i64, ni=4, s=i64, ns=4):
        return lib.pcgx_kdtree_group_stats(h, None if i is None else L.ptr(i), ni, None if s is None else L.ptr(s), ns,
                                           L.ptr(cnt), *nul)

    assert call(ns=0) == L.PCGX_OK and np.all(cnt == -7)  # no group: nothing to write
    assert call(ni=0, i=None) == L.PCGX_OK and not cnt.any()  # no slot: every row zero
    assert call(h=None) == E and call(ni=-1) == E and call(ns=-1) == E
    assert call(i=None) == E and call(s=None) == E
    assert call(ni=2 ** 31) == E and call(ns=2 ** 31) == E
    d = lambda *a: lib.pcgx_kdtree_group_stats_dev(*a, *([None] * 7), None)  # noqa: E731
    one = L.ptr(1 << 20)  # (never dereferenced: every call below is refused, or has nothing to do)
    assert d(None, one, 4, one, 4, None) == E
    assert d(t._h, one, -1, one, 4, None) == E and d(t._h, one, 4, one, -1, None) == E
    assert d(t._h, None, 4, one, 4, None) == E and d(t._h, one, 4, None, 4, None) == E
    assert d(t._h, one, 2 ** 31, one, 4, None) == E and d(t._h, one, 4, one, 2 ** 31, None) == E
    assert d(t._h, one, 4, one, 0, None) == L.PCGX_OK
    with pytest.raises(L.PcgxError):
        t.GroupStats([0, n], [2])


# ------------------------------------------------------------------------------------------------ 3. known frames

def test_known_frames():
    """Lattices of 9 x 5 x 3 and 33 x 17 x 5 points and a flat patch of 17 x 9, rotated and moved 100 units from the
    origin.  Half-extents within D theta + 2^-23 |p|max of the known ones, theta = (covariance bound + TAU trace) / gap.
    The axes against the rotation's columns: the lattice points were rounded to float32 after the rotation, each
    coordinate by up to 2^-24 |p|, a point by up to f = sqrt(3) 2^-24 |p|max; that moves the covariance by up to 2 D f
    (sum (d delta^T + delta d^T) / n with |d| <= D), so the axes by up to theta + 2 D f / gap (Davis-Kahan)."""
    pts, ids, sizes, half = GS.lattices()
    R = GS.rotation()
    t = kdtree.New(pts)
    want, info = _want("lattices", pts, ids, sizes)
    pmax = float(np.linalg.norm(pts.astype(np.float64), axis=1).max())
    f = np.sqrt(3) * 2.0 ** -24 * pmax
    assert np.linalg.norm(GS.SHIFT) == 100.0
    for name, got in (("host", _host(t, ids, sizes)), ("device", _dev(t, ids, sizes))):
        _check(got, want, info, name)
        tr = got.eig.sum(axis=1)
        for g in range(len(sizes)):
            D = info["D"][g]
            gaps = np.array([got.eig[g, 0] - got.eig[g, 1], min(got.eig[g, 0] - got.eig[g, 1], got.eig[g, 1] - got.eig[g, 2]),
                             got.eig[g, 1] - got.eig[g, 2]])
            assert np.all(gaps > GAP * tr[g])
            theta = (info["cov_bound"][g] + TAU * tr[g]) / gaps
            sin = [np.linalg.norm(np.cross(got.axes[g, k], R[:, k])) for k in range(3)]  # up to the contract's sign
            herr = np.abs(got.obb[g, 3:] - half[g])
            print(name, g, "axes", sin, "bound", theta + 2 * D * f / gaps, "half-extents", herr, "bound", D * theta.max() + 2.0 ** -23 * pmax)
            assert np.all(sin <= theta + 2 * D * f / gaps), (name, g)
            assert np.all(herr <= D * theta.max() + 2.0 ** -23 * pmax), (name, g)
        # the flat patch: eig[2] within the covariance bound of 0, axis 2 the patch's normal (the bound above)
        print(name, "flat patch eig[2]", got.eig[2, 2], "bound", info["cov_bound"][2])
        assert abs(got.eig[2, 2]) <= info["cov_bound"][2]
        assert half[2, 2] == 0.0


# ------------------------------------------------------------------------------------------------ 4. the chain

def test_chain_clusters_to_geometry_on_one_stream():
    """ClustersDev -> GroupStatsDev on one stream over torch tensors, nothing read back in between: every output equals,
    bit for bit, the host form's from the host clusters call's ids and sizes, and ClusterExtraction.Boxes() gives the
    same rows trimmed.  The gap rule leaves out none of the 277 clusters of 10 or more points (checked with the oracle
    on the CPU; asserted below at the issue's limit of a quarter)."""
    import torch
    dev = torch.device("cuda", 0)
    pts = GS.chain_cloud()
    n = len(pts)
    t = kdtree.New(pts)
    tds = (torch.int32, torch.float32) + (torch.float64,) * 5
    lab, cnt, siz, ids = (torch.full((k,), -7, dtype=torch.int32, device=dev) for k in (n, 1, n, n))
    out = [torch.full((n,) + s, -7, dtype=d, device=dev) for s, d in zip(SHAPES, tds)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        t.ClustersDev(GS.CHAIN_RADIUS, lab.data_ptr(), cnt.data_ptr(), siz.data_ptr(), ids.data_ptr(), stream=st.cuda_stream)
        t.GroupStatsDev(ids.data_ptr(), n, siz.data_ptr(), n, cnt.data_ptr(), *[o.data_ptr() for o in out], stream=st.cuda_stream)
    st.synchronize()
    torch.cuda.synchronize()
    c = int(cnt.cpu()[0])
    got = [o.cpu().numpy() for o in out]
    _, h_sizes, h_ids = t.Clusters(GS.CHAIN_RADIUS)
    assert c == len(h_sizes) == 3070 and h_sizes[0] == 1754
    host = _host(t, h_ids, h_sizes)
    assert np.array_equal(got[0][:c], host.count) and _bits_equal([g[:c] for g in got[1:]], list(host)[1:])
    assert not any(g[c:].any() for g in got)  # the rows behind the clusters are zero
    want, info = _want("chain", *GS.chain())
    assert np.array_equal(GS.chain()[1], h_ids) and np.array_equal(GS.chain()[2], h_sizes)
    share = _check(host, want, info, "chain")
    assert share <= 0.25, share
    ce = segmentation.ClusterExtraction(t, ClusterTolerance=GS.CHAIN_RADIUS)
    parts = ce.Extract()
    boxes = ce.Boxes()
    assert len(parts) == c and _bits_equal(boxes, host)


# ------------------------------------------------------------------------------------------------ 5. null outputs

def test_each_output_left_out():
    pts, ids, sizes = GS.slots()
    t = kdtree.New(pts)
    full_h, full_d = _host(t, ids, sizes), _dev(t, ids, sizes)
    assert _bits_equal(list(full_h)[1:], list(full_d)[1:]) and np.array_equal(full_h.count, full_d.count)
    for k in range(7):
        rc, h = _host_once(t, ids, sizes, skip=(k,))
        assert rc == L.PCGX_OK
        d = _dev(t, ids, sizes, skip=(k,))
        for j in range(7):
            if j == k:
                assert np.all(h[j] == -7) and np.all(d[j] == -7)  # not touched
            else:
                assert _bits_equal([h[j]], [full_h[j]]) and _bits_equal([d[j]], [full_d[j]]), (k, j)
    rc, h = _host_once(t, ids, sizes, skip=tuple(range(7)))
    assert rc == L.PCGX_OK
