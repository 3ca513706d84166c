"""k-NN covariances on the GPU (pcgx_kdtree_covariances / _dev, csrc/knearest.hip in covariance mode) against the
float64 oracle (tests/cov_oracle.py on tests/knn_oracle.py's neighbour lists): counts equal pcgx_kdtree_knearest's on
the grid, the forced walk (PCGX_RANGE_WALK=1) and a patched handle; RAW to its float32 rounding plus 1e-9 of the
trace, which pins the neighbour set; PLANE entries to 1e-6 and normals to 1e-6 rad where the smallest eigenvalue is
apart (lambda1 - lambda0 >= 1e-6 lambda2, the normals tests' rule); degenerate lists and a coincident heap exact;
host and device entries, q == NULL and q = the tree's points bit for bit."""
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_oracle as CO  # noqa: E402
import knn_oracle as KO  # noqa: E402

pytestmark = pytest.mark.gpu

VP = (0.3, -2.0, 5.0)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _sources(pts, monkeypatch, deleted):
    """(name, tree, excluded ids): the grid, the forced walk, a handle after DeletePoints"""
    t = kdtree.New(pts)
    yield "grid", t, None
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    yield "walk", t, None
    monkeypatch.delenv("PCGX_RANGE_WALK")
    td = kdtree.New(pts)
    td.DeletePoints(deleted)
    yield "deleted", td, deleted


def _check(t, pts, q, k, r, ex, what, eps=1e-3):
    qq = pts if q is None else q
    oi, _, oc = KO.knearest(pts, qq, k, r, exclude=ex)
    raw, rn, rc = t.Covariances(k, r, Mode="raw", Queries=q, Viewpoint=VP)
    pl, pn, pc = t.Covariances(k, r, Mode="plane", Epsilon=eps, Queries=q, Viewpoint=VP)
    assert np.array_equal(t.KNearestBatch(q, k, r)[2], oc), what
    assert np.array_equal(rc, oc) and np.array_equal(pc, oc), what
    assert np.array_equal(rn.view(np.uint32), pn.view(np.uint32)), what  # the normal does not depend on the mode
    ref = CO.covariances(pts, qq, oi, oc, CO.RAW, viewpoint=VP)
    err = np.abs(raw.astype(np.float64) - ref["cov6"])
    bound = 2.0 ** -24 * np.abs(ref["cov6"]) + 1e-9 * ref["trace"][:, None]
    bad = np.nonzero((err > bound).any(1))[0]
    assert len(bad) == 0, (what, k, r, len(bad), bad[:3], raw[bad[:1]], ref["cov6"][bad[:1]])
    ref = CO.covariances(pts, qq, oi, oc, CO.PLANE, eps, viewpoint=VP)
    deg = ref["degenerate"]
    eye6 = np.tile(np.float32([1, 0, 0, 1, 0, 1]), (int(deg.sum()), 1))
    assert np.array_equal(pl[deg], eye6) and np.array_equal(raw[deg], np.zeros_like(eye6)), what
    assert np.array_equal(pn[deg], np.zeros((int(deg.sum()), 3), np.float32)), what
    lam = ref["lam"]
    good = ~deg & (lam[:, 1] - lam[:, 0] >= 1e-6 * lam[:, 2])
    assert good.sum() >= 0.9 * (~deg).sum(), what
    assert np.max(np.abs(pl[good].astype(np.float64) - ref["cov6"][good]), initial=0.0) <= 1e-6, what
    a, b = pn[good].astype(np.float64), ref["normals"][good]
    sin = np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    assert np.max(sin, initial=0.0) <= 1e-6, (what, float(np.max(sin, initial=0.0)))
    to_v = np.asarray(VP, np.float64)[None, :] - qq[good].astype(np.float64)
    clear = np.abs(np.sum(b * to_v, axis=1)) > 1e-6 * np.linalg.norm(to_v, axis=1)
    assert np.all(np.sum(a[clear] * b[clear], axis=1) > 0), what
    return deg


def test_uniform_cloud_every_source(monkeypatch):
    pts = synth.uniform_cloud(20_000, 1.0, 61)
    r = _rng(62)
    q = np.ascontiguousarray(np.concatenate([r.random((3000, 3)), pts[:200], 3.0 + r.random((20, 3))]),
                             dtype=np.float32)
    deleted = r.choice(len(pts), 2000, replace=False)
    for name, t, ex in _sources(pts, monkeypatch, deleted):
        for k, rr in ((20, np.inf), (8, 0.05), (64, np.inf), (2, np.inf)):
            deg = _check(t, pts, q, k, rr, ex, name)
            assert deg[-20:].all() == (rr != np.inf or k < 3), name  # queries far outside: no neighbour within 0.05


def test_surface_own_points(monkeypatch):
    pts = synth.surface_cloud(30_000, 5.0, 63)[0]
    deleted = _rng(64).choice(len(pts), 3000, replace=False)
    for name, t, ex in _sources(pts, monkeypatch, deleted):
        deg = _check(t, pts, None, 20, np.inf, ex, name)
        assert not deg.any(), name
        _check(t, pts, None, 10, 0.08, ex, name, eps=0.25)


def test_coincident_heap_and_degenerate_lists(monkeypatch):
    """a heap of coincident points (a fat grid row): every list inside it is degenerate, exactly I / 0"""
    h = np.float32([0.5, 0.5, 0.5])
    u = synth.uniform_cloud(20_000, 1.0, 65)
    pts = np.ascontiguousarray(np.concatenate([u, np.tile(h, (5000, 1))])[_rng(66).permutation(25_000)],
                               dtype=np.float32)
    q = np.ascontiguousarray(np.concatenate([np.tile(h, (70, 1)), u[:300]]), dtype=np.float32)
    monkeypatch.setenv("PCGX_GRID", "2")
    for name, t, ex in _sources(pts, monkeypatch, np.arange(0, 25_000, 97)):
        for k in (16, 64):
            deg = _check(t, pts, q, k, np.inf, ex, "heap " + name)
            assert deg[:70].all(), name
        deg = _check(t, pts, q, 2, np.inf, ex, "k=2 " + name)
        assert deg.all(), name


def test_own_points_host_and_device_entries(monkeypatch):
    import torch
    pts = synth.surface_cloud(40_000, 6.0, 67)[0]
    deleted = _rng(68).choice(len(pts), 4000, replace=False)
    dev = torch.device("cuda", 0)
    for name, t, ex in _sources(pts, monkeypatch, deleted):
        for mode in ("plane", "raw"):
            a = t.Covariances(20, Mode=mode, Viewpoint=VP)
            b = t.Covariances(20, Mode=mode, Queries=np.stack([t.Vec3At(i) for i in range(len(pts))]), Viewpoint=VP)
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (name, mode)
            for own in (True, False):
                dq = torch.from_numpy(pts).to(dev)
                dc = torch.empty((len(pts), 6), dtype=torch.float32, device=dev)
                dn = torch.empty((len(pts), 3), dtype=torch.float32, device=dev)
                dk = torch.empty(len(pts), dtype=torch.int32, device=dev)
                t.CovariancesDev(20, dc.data_ptr(), dn.data_ptr(), dk.data_ptr(), d_q=0 if own else dq.data_ptr(),
                                 nq=None if own else len(pts), Mode=mode, Viewpoint=VP)
                torch.cuda.synchronize()
                for x, y in zip(a, (dc, dn, dk)):
                    assert np.array_equal(x.view(np.uint32), y.cpu().numpy().view(np.uint32)), (name, mode, own)
            # without normals and counts the covariances are the same bits
            c6 = np.empty((len(pts), 6), np.float32)
            L.check(L.lib().pcgx_kdtree_covariances(t._h, None, len(pts), 20, np.inf, L.PCGX_COV_PLANE if mode == "plane"
                                                    else L.PCGX_COV_RAW, 1e-3, L.ptr(np.float32(VP)), L.ptr(c6), None,
                                                    None))
            assert np.array_equal(c6.view(np.uint32), a[0].view(np.uint32)), (name, mode)


def test_invalid_arguments():
    pts = synth.uniform_cloud(100, 1.0, 69)
    t = kdtree.New(pts)
    cov = np.empty((100, 6), np.float32)
    lib = L.lib()

    def call(q=pts, nq=100, k=8, r=1.0, mode=L.PCGX_COV_PLANE, eps=1e-3, out=cov):
        return lib.pcgx_kdtree_covariances(t._h, None if q is None else L.ptr(q), nq, k, r, mode, eps, None,
                                           None if out is None else L.ptr(out), None, None)
    for kw in (dict(k=0), dict(k=65), dict(eps=0.0), dict(eps=-1e-3), dict(eps=1.5), dict(eps=float("nan")),
               dict(mode=2), dict(mode=-1), dict(r=float("nan")), dict(r=-1.0), dict(q=None, nq=99), dict(out=None)):
        assert call(**kw) == L.PCGX_E_INVALID, kw
    assert call(eps=1.0) == 0 and call(k=64, r=np.inf) == 0 and call(q=None) == 0
    assert call(nq=0, out=None) == 0
