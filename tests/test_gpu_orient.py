"""GPU: consistent normal orientation (csrc/orient.hip, csrc/orient_terms.h; include/pcgx.h, "consistent normal
orientation") against the NumPy oracle (tests/orient_oracle.py), everything by array_equal: the flips are the sign
parity along the minimum spanning forest of a graph with strictly ordered edges, a property of the point set, so the
flags, the normals' bits, the components and both counts are the oracle's on the grid, on the forced walk and after
DeletePoints, and after R rounds too.  Every call is made twice: the same bits on every call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import features, kdtree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orient_oracle as OO  # noqa: E402
from test_gpu_radius_edges import _grid_on  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
nan, inf = np.nan, np.inf
MODES = [(0, None), (1, (0.0, 0.0, 1.0)), (1, (0.3, -0.8, 0.2)), (2, (0.4, 0.5, 3.0))]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _raw(t, r, nrm, mode=0, ref=None, out=True, flipped=True, comp=True, in_place=False):
    """the host entry point's whole output -> (status, normals_out, flipped, component, n_components, n_open)"""
    n = t.Len()
    nrm = np.array(nrm, f32).reshape(-1, 3).copy()
    o = nrm if in_place else (np.full((n, 3), -7, f32) if out else None)
    fl = np.full(n, 77, np.uint8) if flipped else None
    co = np.full(n, -7, np.int64) if comp else None
    nc, no = C.c_int64(-7), C.c_int64(-7)
    ref = None if ref is None else np.array(ref, f32)
    rc = L.lib().pcgx_kdtree_orient_normals(t._h, float(r), L.ptr(nrm), mode, L.ptr(ref), L.ptr(o), L.ptr(fl), L.ptr(co),
                                            C.byref(nc), C.byref(no))
    return rc, o, fl, co, nc.value, no.value


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(np.asarray(x).view(u32) if np.asarray(x).dtype == f32 else x,
                                                           np.asarray(y).view(u32) if np.asarray(y).dtype == f32 else y)
               for x, y in zip(a, b))


def _check(t, pts, nrm, r, mode=0, ref=None, deleted=None, what="", want=None, lists=None):
    want = want or OO.orient(pts, nrm, r, mode, ref, deleted=deleted, lists=lists)
    got = _raw(t, r, nrm, mode, ref)
    assert got[0] == L.PCGX_OK, (what, L.last_error())
    assert _same(got, _raw(t, r, nrm, mode, ref)), what  # the same bits on every call
    _, o, fl, co, nc, no = got
    assert np.array_equal(fl, want["flipped"]), (what, np.nonzero(fl != want["flipped"])[0][:10])
    assert np.array_equal(o.view(u32), want["normals_out"].view(u32)), what
    assert np.array_equal(co, want["component"]), (what, np.nonzero(co != want["component"])[0][:10])
    assert (nc, no) == (want["n_components"], 0), (what, nc, no, want["n_components"])
    return want


def _dev(t, r, nrm, mode=0, ref=None, max_rounds=0, comp=True, stream=None, in_place=False, out=True, flipped=True):
    """OrientNormalsDev into pattern-filled buffers -> (normals_out, flipped, component, n_components, n_open)"""
    import torch
    dev = torch.device("cuda", 0)
    n = t.Len()
    dn = torch.from_numpy(np.array(nrm, f32).reshape(-1, 3).copy()).to(dev)
    do = dn if in_place else torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
    df = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    dc = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((2,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    kw = dict(Direction=ref) if mode == 1 else dict(Viewpoint=ref) if mode == 2 else {}
    t.OrientNormalsDev(r, dn.data_ptr(), do.data_ptr() if out else 0, df.data_ptr() if flipped else 0, cnt.data_ptr(),
                       cnt.data_ptr() + 4, d_component=dc.data_ptr() if comp else 0, MaxRounds=max_rounds,
                       stream=stream.cuda_stream if stream is not None else 0, **kw)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    return do.cpu().numpy(), df.cpu().numpy(), dc.cpu().numpy(), int(c[0]), int(c[1])


def _check_dev(t, want, r, nrm, mode=0, ref=None, what="", **kw):
    got = _dev(t, r, nrm, mode, ref, **kw)
    assert _same(got, _dev(t, r, nrm, mode, ref, **kw)), what
    o, fl, co, nc, no = got
    assert np.array_equal(fl, want["flipped"]), (what, np.nonzero(fl != want["flipped"])[0][:10])
    assert np.array_equal(o.view(u32), want["normals_out"].view(u32)), what
    assert np.array_equal(co.astype(np.int64), want["component"]), what
    assert (nc, no) == (want["n_components"], want["n_open"]), (what, nc, no, want["n_components"], want["n_open"])


# ------------------------------------------------------------------------------------------------ every source

def _sheet(n, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 1, (n, 2))
    z = 0.1 * np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1])
    return np.ascontiguousarray(np.concatenate([xy, z[:, None]], axis=1), f32), _unit(rng, n)


def test_tree_dependent_flips_on_every_source(monkeypatch):
    """3 000 points of a wavy sheet with fully random unit normals: which normals flip depends on which edges the forest
    took, so a wrong edge shows.  All modes on the grid, the forced walk and a handle with 10 % of its points deleted,
    among them id 0, a mode 1 anchor and one end of a first-round edge."""
    pts, nrm = _sheet(3000, 71)
    n, r = len(pts), 0.05
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 1
    first = OO.orient(pts, nrm, r, rounds=1)
    anchor = int(np.argmax(pts[:, 2]))
    gone = np.unique(np.concatenate([np.random.default_rng(72).choice(n, n // 10, replace=False),
                                     [0, anchor, int(first["forest"][0][0])]]))
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    flips = []
    for mode, ref in MODES:
        want = _check(t, pts, nrm, r, mode, ref, what=(mode, ref, "grid"))
        assert want["n_components"] < 20 and 0.3 < want["flipped"].mean() < 0.7
        monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        _check(t, pts, nrm, r, mode, ref, what=(mode, ref, "walk"), want=want)
        monkeypatch.delenv("PCGX_RANGE_WALK")
        wd = _check(td, pts, nrm, r, mode, ref, deleted=gone, what=(mode, ref, "deleted"))
        assert np.all(wd["component"][gone] == -1) and np.all(wd["flipped"][gone] == 0)
        assert not np.array_equal(wd["flipped"], np.where(np.isin(np.arange(n), gone), 0, want["flipped"]))
        flips.append(want["flipped"])
    if want["n_components"] == 1:
        assert all(np.all(f == flips[0]) or np.all(f == 1 - flips[0]) for f in flips)  # modes differ by a whole sign


# ------------------------------------------------------------------------------------------------ rounds

def test_a_chain_round_by_round():
    """4 096 points on a line, each with two neighbours, ids shuffled, random normals: many rounds and long parent
    chains.  The host form finishes; the device form after 1, 2 and 3 rounds is the oracle's F_R, open components
    included, and with max_rounds 0 it is final."""
    rng = np.random.default_rng(73)
    n = 4096
    pts = np.zeros((n, 3), f32)
    pts[:, 0] = rng.permutation(n).astype(f32) * f32(2.0 ** -6)
    nrm = _unit(rng, n)
    r = 1.5 * 2.0 ** -6
    t = kdtree.New(pts)
    full = _check(t, pts, nrm, r, 1, (1.0, 0.0, 0.0), what="host")
    assert full["n_components"] == 1 and full["rounds"] >= 5
    for R in (1, 2, 3):
        want = OO.orient(pts, nrm, r, 2, (5.0, 1.0, 0.0), rounds=R)
        assert want["n_open"] > 0 and want["n_components"] > 1
        _check_dev(t, want, r, nrm, 2, (5.0, 1.0, 0.0), what=R, max_rounds=R)
    _check_dev(t, OO.orient(pts, nrm, r, 2, (5.0, 1.0, 0.0)), r, nrm, 2, (5.0, 1.0, 0.0), what=0, max_rounds=0)
    _check_dev(t, full, r, nrm, 1, (1.0, 0.0, 0.0), what="more than enough", max_rounds=40)
    assert L.lib().pcgx_orient_full_rounds(n) == 12 and L.lib().pcgx_orient_full_rounds(n + 1) == 13
    assert L.lib().pcgx_orient_full_rounds(1) == 1 and L.lib().pcgx_orient_full_rounds(0) == 0


def test_exact_ties_go_by_id(monkeypatch):
    """a 40 x 40 lattice plane, identical normals with random signs: every |c| is 1, the id tie-break decides"""
    rng = np.random.default_rng(74)
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2)
    pts = np.zeros((1600, 3), f32)
    pts[:, :2] = g[rng.permutation(1600)] * 0.125
    nrm = np.zeros((1600, 3), f32)
    nrm[:, 2] = np.where(rng.integers(0, 2, 1600) == 1, -1, 1)
    t = kdtree.New(pts)
    for r in (0.13, 0.18):  # 4 and 8 neighbours
        for mode, ref in MODES[:2]:
            want = _check(t, pts, nrm, r, mode, ref, what=(r, mode))
            assert want["n_components"] == 1 and len(np.unique(want["normals_out"][:, 2])) == 1
        monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        _check(t, pts, nrm, r, 0, None, what=(r, "walk"))
        monkeypatch.delenv("PCGX_RANGE_WALK")
        for R in (1, 2):
            _check_dev(t, OO.orient(pts, nrm, r, rounds=R), r, nrm, what=(r, R), max_rounds=R)


def test_two_sheets():
    """two parallel lattice sheets: nearer than the radius they are one component, farther two, and each of the two gets
    its own anchor and its own vote"""
    rng = np.random.default_rng(75)
    g = np.stack(np.meshgrid(np.arange(25), np.arange(25), indexing="ij"), -1).reshape(-1, 2) * 0.1
    jitter = rng.uniform(-0.01, 0.01, (1250, 3))
    pts = np.concatenate([np.c_[g, np.zeros(625)], np.c_[g, np.full(625, 0.15)]]) + jitter
    pts = np.ascontiguousarray(pts[rng.permutation(1250)], f32)
    nrm = (np.array([[0, 0, 1]], f32) + rng.normal(0, 0.02, (1250, 3))).astype(f32)
    nrm *= np.where(rng.integers(0, 2, 1250) == 1, -1, 1)[:, None].astype(f32)
    t = kdtree.New(pts)
    for r, comps in ((0.22, 1), (0.125, 2)):
        for mode, ref in ((1, (0.0, 0.0, 1.0)), (2, (1.2, 1.2, 0.075)), (0, None)):
            want = _check(t, pts, nrm, r, mode, ref, what=(r, mode))
            assert want["n_components"] == comps
            up = want["normals_out"][:, 2] > 0
            if mode == 1:
                assert up.all()
            if mode == 2 and comps == 2:  # the viewpoint lies between the sheets: they look at each other
                assert np.array_equal(up, pts[:, 2] < 0.075)


def test_a_fat_row(monkeypatch):
    """5 000 coincident points with random normals inside a small cloud: a grid row of at least kRangeFatRow records is
    the wave's work, on the grid (PCGX_GRID=2); the walk gives the same"""
    rng = np.random.default_rng(76)
    cloud = rng.uniform(0, 4, (1200, 3)).astype(f32)
    pts = np.concatenate([cloud, np.tile(f32([2.0, 2.0, 2.0]), (5000, 1)), f32([[0, 0, 0], [4, 4, 4]])])
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))], f32)
    nrm = _unit(rng, len(pts))
    assert len(pts) % 64 != 0
    monkeypatch.setenv("PCGX_GRID", "2")
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 1
    want = _check(t, pts, nrm, 0.5, 2, (2.0, 2.0, 9.0), what="grid")
    assert np.bincount(want["component"][want["component"] >= 0]).max() > 5000
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    _check(t, pts, nrm, 0.5, 2, (2.0, 2.0, 9.0), what="walk", want=want)


# ------------------------------------------------------------------------------------------------ small and degenerate

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_small_len(n):
    rng = np.random.default_rng(80 + n)
    pts = rng.uniform(0, 1, (n, 3)).astype(f32)
    nrm = _unit(rng, n)
    t = kdtree.New(pts)
    for r in (0.3, 2.0):
        for mode, ref in MODES:
            want = _check(t, pts, nrm, r, mode, ref, what=(n, r, mode))
        _check_dev(t, want, r, nrm, *MODES[-1], what=(n, r, "dev"))
        _check_dev(t, OO.orient(pts, nrm, r, *MODES[-1], rounds=1), r, nrm, *MODES[-1], what=(n, r, "dev 1"), max_rounds=1)


def test_degenerate_input():
    """infinite and NaN points, zero, NaN and infinite normals; every point deleted; a NaN-only cloud"""
    rng = np.random.default_rng(90)
    n = 400
    pts = rng.uniform(0, 1, (n, 3)).astype(f32)
    nrm = _unit(rng, n)
    pts[3] = inf
    pts[17, 1] = inf
    pts[40, 2] = -inf
    pts[41, 0] = -inf
    nrm[5] = 0
    nrm[6] = (0.0, -0.0, 0.0)
    nrm[7, 1] = nan
    nrm[8, 0] = inf
    nrm[3] = (1, 0, 0)
    nrm[9] = (1e-30, 0, 0)  # tiny and huge normals are ordinary: they are taken as given
    nrm[10] = (3e38, 3e38, 3e38)
    t = kdtree.New(pts)
    for mode, ref in MODES:
        want = _check(t, pts, nrm, 0.2, mode, ref, what=("mixed", mode))
        assert np.all(want["component"][[3, 17, 40, 41, 5, 6, 7, 8]] == -1) and np.all(want["component"][[9, 10]] >= 0)
    # a NaN coordinate as well: the neighbourhoods are Range's on that handle, whose tree a NaN puts out of order, so
    # no brute force says what they are, and j in N(i) need not mean i in N(j) -- the handle's own Range lists do, and the
    # oracle's rule over them (a component is also offered what another takes into it) is the answer
    bad = pts.copy()
    bad[3] = nan
    bad[41, 0] = nan
    bad[60::9, 1] = nan
    tn = kdtree.New(bad)
    lists = tn.RangeBatch(bad, 0.2)[:2]
    out = np.nonzero(~np.isfinite(bad).all(axis=1))[0]
    for mode, ref in MODES:
        want = _check(tn, bad, nrm, 0.2, mode, ref, what=("nan", mode), lists=lists)
        assert np.all(want["component"][out] == -1) and (want["component"] >= 0).sum() > 100
    t.DeletePoints(np.arange(n))
    want = _check(t, pts, nrm, 0.2, 1, (0, 0, 1), deleted=np.arange(n), what="all deleted")
    assert want["n_components"] == 0 and np.all(want["component"] == -1)
    bad = np.full((70, 3), nan, f32)
    _check(kdtree.New(bad), bad, nrm[:70], 0.2, 2, (0, 0, 1), what="NaN cloud")
    zero = np.zeros((70, 3), f32)
    want = _check(kdtree.New(pts[100:170]), pts[100:170], zero, 0.5, 0, what="no normals")
    assert want["n_components"] == 0


def test_arguments():
    rng = np.random.default_rng(91)
    pts = rng.uniform(0, 1, (100, 3)).astype(f32)
    nrm = _unit(rng, 100)
    t = kdtree.New(pts)
    lib = L.lib()
    o, fl, co = np.zeros((100, 3), f32), np.zeros(100, np.uint8), np.zeros(100, np.int64)
    nc, no = C.c_int64(-7), C.c_int64(-7)
    u = np.array([0, 0, 1], f32)

    def call(tree=t._h, r=0.3, normals=nrm, mode=0, ref=None, out=o, flipped=fl, comp=co, pnc=C.byref(nc), pno=C.byref(no)):
        return lib.pcgx_kdtree_orient_normals(tree, float(r), L.ptr(normals), mode, L.ptr(ref), L.ptr(out), L.ptr(flipped),
                                              L.ptr(comp), pnc, pno)

    assert call() == L.PCGX_OK
    for kw in (dict(tree=None), dict(r=0.0), dict(r=-1.0), dict(r=nan), dict(r=inf), dict(normals=None),
               dict(out=None, flipped=None), dict(pnc=None), dict(pno=None), dict(mode=-1), dict(mode=3),
               dict(mode=1), dict(mode=2), dict(mode=1, ref=np.array([0, nan, 1], f32)),
               dict(mode=2, ref=np.array([inf, 0, 1], f32))):
        o[:], fl[:] = -7, 77
        assert call(**kw) == L.PCGX_E_INVALID, kw
        assert np.all(o == -7) and np.all(fl == 77), kw  # nothing written
    assert call(mode=0, ref=np.array([nan, nan, nan], f32)) == L.PCGX_OK  # mode 0 does not read it
    import torch
    d = torch.zeros(400, dtype=torch.float32, device="cuda")
    a = d.data_ptr()
    dev = lambda rounds: lib.pcgx_kdtree_orient_normals_dev(t._h, 0.3, L.ptr(a), 0, None, rounds, L.ptr(a), None, None,  # noqa: E731
                                                            L.ptr(a + 1200), L.ptr(a + 1204), None)
    assert dev(-1) == L.PCGX_E_INVALID and dev(0) == L.PCGX_OK
    torch.cuda.synchronize()
    # each optional output left out in turn: the others are what they were
    want = OO.orient(pts, nrm, 0.3, 1, u)
    for kw in (dict(out=False), dict(flipped=False), dict(comp=False)):
        rc, go, gf, gc, gnc, gno = _raw(t, 0.3, nrm, 1, u, **kw)
        assert rc == L.PCGX_OK and (gnc, gno) == (want["n_components"], 0), kw
        assert go is None or np.array_equal(go.view(u32), want["normals_out"].view(u32)), kw
        assert gf is None or np.array_equal(gf, want["flipped"]), kw
        assert gc is None or np.array_equal(gc, want["component"]), kw
        dv = _dev(t, 0.3, nrm, 1, u, **kw)
        assert dv[3:] == (want["n_components"], 0), kw
        if kw.get("out", True):
            assert np.array_equal(dv[0].view(u32), want["normals_out"].view(u32)), kw
        else:
            assert np.all(dv[0] == -7), kw
        assert np.array_equal(dv[1], want["flipped"] if kw.get("flipped", True) else np.full(100, 77, np.uint8)), kw
        assert np.array_equal(dv[2], want["component"] if kw.get("comp", True) else np.full(100, -7)), kw
    # (Len() == 0 cannot be reached from here: pcgx_kdtree_build refuses an empty cloud)


def test_in_place_and_on_a_stream():
    import torch
    pts, nrm = _sheet(2000, 92)
    t = kdtree.New(pts)
    r, mode, ref = 0.07, 1, (0.0, 0.0, 1.0)
    want = OO.orient(pts, nrm, r, mode, ref)
    rc, o, fl, co, nc, no = _raw(t, r, nrm, mode, ref, in_place=True)
    assert rc == L.PCGX_OK and np.array_equal(o.view(u32), want["normals_out"].view(u32)) and np.array_equal(fl, want["flipped"])
    _check_dev(t, want, r, nrm, mode, ref, what="in place", in_place=True)
    s = torch.cuda.Stream()
    _check_dev(t, want, r, nrm, mode, ref, what="stream", stream=s)
    _check_dev(t, OO.orient(pts, nrm, r, mode, ref, rounds=2), r, nrm, mode, ref, what="stream 2", stream=s, max_rounds=2)
    # the wrappers
    got = t.OrientNormals(r, nrm, Direction=ref, Component=True)
    assert np.array_equal(got[0].view(u32), want["normals_out"].view(u32)) and np.array_equal(got[1], want["flipped"])
    assert got[2] == want["n_components"] and np.array_equal(got[3], want["component"])
    est = features.NormalOrientation(r, features.WithDirection(ref))
    assert np.array_equal(est.Compute(t, nrm).view(u32), want["normals_out"].view(u32))
    want_v = OO.orient(pts, nrm, r, 2, (0.5, 0.5, 4.0))
    est = features.NormalOrientation(r, features.WithViewpoint((0.5, 0.5, 4.0)))
    assert np.array_equal(est.Compute(t, nrm).view(u32), want_v["normals_out"].view(u32))
    assert est.n_components == want_v["n_components"] and np.array_equal(est.flipped, want_v["flipped"])
    assert np.array_equal(features.NormalOrientation(r).Compute(t, nrm).view(u32), OO.orient(pts, nrm, r)["normals_out"].view(u32))


# ------------------------------------------------------------------------------------------------ what it is for

def test_clusters_stop_cutting_a_smooth_face():
    """the sign-randomised sphere: oriented clusters cut it into many pieces; after OrientNormals it is one"""
    rng = np.random.default_rng(7)
    outward = _unit(rng, 2000)
    pts = outward.copy()
    nrm = outward * np.where(rng.integers(0, 2, 2000) == 1, f32(-1), f32(1))[:, None]
    t = kdtree.New(pts)
    before = t.Clusters(0.15, Normals=nrm, MinCos=0.5, Oriented=True)[1]
    assert len(before) > 10
    want = _check(t, pts, nrm, 0.15, 1, (0.0, 0.0, 1.0), what="sphere")
    fixed = t.OrientNormals(0.15, nrm, Direction=(0, 0, 1))[0]
    assert np.array_equal(fixed, outward) and np.array_equal(fixed, want["normals_out"])
    after = t.Clusters(0.15, Normals=fixed, MinCos=0.5, Oriented=True)[1]
    assert after.tolist() == [2000]
