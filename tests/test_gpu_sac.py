"""Sample consensus plane detection on the GPU (pcgol_amd.sac, csrc/sac.hip) against the float32 oracle
(tests/sac_oracle.py) over the same pre-drawn ids: the ok flags, the coefficient bits and the scores of every
hypothesis, the choice of Compute, and Inliers.  The reference's own tables: tests/golden/ref_sac.json."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import pc, sac, segmentation

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sac_oracle as S  # noqa: E402

pytestmark = pytest.mark.gpu


class RecordingSampler:
    """a seeded sampler that remembers what it drew (the oracle replays the same ids)"""

    def __init__(self, n, seed):
        self.s = sac.NewRandomSampler(n, seed)
        self.drawn = []

    def Sample(self):
        v = self.s.Sample()
        self.drawn.append(v)
        return v


def _grid(res, size, origin, pts):
    g = segmentation.StorageVoxelGrid(res, size, origin)
    g.AddAll(np.asarray(pts, np.float32))
    return g


def _both(res, size, origin, pts, ra=None):
    pts = np.asarray(pts, np.float32)
    g = _grid(res, size, origin, pts)
    gm = sac.NewVoxelGridSurfaceModel(g, pts if ra is None else ra)
    om = S.SurfaceModel(S.Grid(res, size, origin, pts), pts)
    return g, gm, om


def _expected(om, ids):
    n = len(ids) // 3
    found, best, best_e, per = S.compute(om, ids, n)
    ok = np.array([p[1] for p in per], bool)
    coeff = np.stack([p[0].as_array() if p[1] else np.zeros(15, np.float32) for p in per]) if n else np.zeros((0, 15), np.float32)
    score = np.array([p[2] for p in per], np.int64)
    return found, best, best_e, ok, coeff, score, per


def _check_parity(gm, om, ids):
    ids = np.asarray(ids, np.int64)
    found, best, best_e, ok, coeff, score, per = _expected(om, ids)
    gf, gb, gs, gbest, gok, gcs, gscore = gm.compute(ids)
    gcoeff = np.stack([c.Array() if c is not None else np.zeros(15, np.float32) for c in gcs])
    assert np.array_equal(gok, ok), np.nonzero(gok != ok)[0][:10]
    bad = np.nonzero((gcoeff.view(np.uint32) != coeff.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (bad[:10], gcoeff[bad[:1]], coeff[bad[:1]])
    bad = np.nonzero(gscore != score)[0]
    assert len(bad) == 0, (bad[:10], gscore[bad[:10]], score[bad[:10]])
    assert (gf, gb, gs) == (found, best, best_e)
    if found:
        assert np.array_equal(gbest.Array().view(np.uint32), coeff[best].view(np.uint32))
    return per


# ------------------------------------------------------------------ 1. the reference's tables
def test_golden_sac(golden):
    t = golden("ref_sac.json")["sac"]
    pts = np.array(t["points"], np.float32)
    g, gm, om = _both(t["resolution"], t["size"], t["origin"], pts)
    for seed in range(6):
        smp = RecordingSampler(len(pts), seed)
        s = sac.New(smp, gm)
        assert s.Compute(t["n"])
        found, best, best_e, per = S.compute(om, smp.drawn, t["n"])
        assert found
        c = s.Coefficients()
        assert np.array_equal(c.Array().view(np.uint32), per[best][0].as_array().view(np.uint32)), seed
        assert c.Evaluate() == best_e
        assert np.array_equal(c.Inliers(t["inlier_d"]), per[best][0].Inliers(t["inlier_d"]))
    # a pinned seed: both return the reference's expected inliers
    smp = RecordingSampler(len(pts), 0)
    s = sac.New(smp, gm)
    assert s.Compute(t["n"])
    assert s.Coefficients().Inliers(t["inlier_d"]).tolist() == t["expected_inliers"]
    found, best, _, per = S.compute(om, smp.drawn, t["n"])
    assert per[best][0].Inliers(t["inlier_d"]).tolist() == t["expected_inliers"]


def test_golden_surface(golden):
    s = golden("ref_sac.json")["surface"]
    for c in s["cases"]:
        pts = np.array(s["clouds"][c["cloud"]], np.float32)
        g, gm, om = _both(s["resolution"], s["size"], c["origin"], pts)
        co, ok = gm.Fit(s["fit_ids"])
        assert ok, c["name"]
        assert sorted(co.Inliers(s["inlier_d"]).tolist()) == s["expected_inliers"], c["name"]
        for i, want in s["is_in"]:
            assert co.IsIn(pts[i], s["inlier_d"]) == want, (c["name"], i)
        for name, ids in s["failing_fits"].items():
            assert gm.Fit(ids) == (None, False), (c["name"], name)
        oc, _ = om.Fit(s["fit_ids"])
        assert np.array_equal(co.Array().view(np.uint32), oc.as_array().view(np.uint32)), c["name"]
        assert co.Evaluate() == oc.Evaluate()


# ------------------------------------------------------------------ 2. per-hypothesis parity
def _scene(rng, origin, ext):
    """a floor, two walls, clutter and points outside the grid, plus the points the degenerate triples use"""
    o = np.asarray(origin, np.float32)
    e = np.asarray(ext, np.float32)
    floor = np.c_[rng.random(1500) * e[0], rng.random(1500) * e[1], 0.1 + rng.normal(0, 0.005, 1500)]
    wall_x = np.c_[0.2 + rng.normal(0, 0.005, 800), rng.random(800) * e[1], rng.random(800) * e[2]]
    wall_y = np.c_[rng.random(800) * e[0], e[1] - 0.3 + rng.normal(0, 0.005, 800), rng.random(800) * e[2]]
    clutter = rng.random((600, 3)) * e
    outside = rng.random((200, 3)) * e * 1.6 - 0.3 * e
    base = np.concatenate([floor, wall_x, wall_y, clutter, outside]) + o
    # special points: a line, an exactly axis-parallel plane (z = const, x = const), the box's corners and edges
    line = o + np.array([[0.3, 0.3, 0.3], [0.6, 0.6, 0.6], [0.9, 0.9, 0.9], [0.45, 0.45, 0.45]])
    zc = o + np.array([[0.1, 0.1, 0.5], [0.7, 0.2, 0.5], [0.3, 0.9, 0.5]])
    xc = o + np.array([[0.4, 0.1, 0.1], [0.4, 0.8, 0.2], [0.4, 0.3, 0.9]])
    corners = o + np.array([[0, 0, 0], [e[0], 0, 0], [0, e[1], 0], [0, 0, e[2]], [e[0], e[1], 0], [e[0], 0, e[2]],
                            [0, e[1], e[2]], [e[0], e[1], e[2]], [e[0] / 2, 0, 0], [0, e[1] / 2, 0], [0, 0, e[2] / 2]])
    pts = np.concatenate([base, line, zc, xc, corners]).astype(np.float32)
    k = len(base)
    special = {"line": list(range(k, k + 4)), "zc": list(range(k + 4, k + 7)), "xc": list(range(k + 7, k + 10)),
               "corners": list(range(k + 10, k + 21))}
    return pts, special


def _hypotheses(rng, n_pts, special, count):
    ids = rng.integers(0, n_pts, size=(count, 3))
    k = 0
    for h in range(0, count, 7):  # every seventh hypothesis a degenerate or boundary one
        kind = k % 5
        k += 1
        if kind == 0:
            ids[h] = [ids[h, 0], ids[h, 0], ids[h, 2]]                    # repeated id
        elif kind == 1:
            ids[h] = rng.choice(special["line"], 3, replace=False)         # collinear
        elif kind == 2:
            ids[h] = special["zc"] if k % 2 else special["xc"]             # parallel to an axis
        elif kind == 3:
            ids[h] = rng.choice(special["corners"], 3, replace=False)      # through the box's corners / edges
        else:
            ids[h] = [rng.choice(special["corners"]), ids[h, 1], ids[h, 2]]
    return ids.reshape(-1)


@pytest.mark.parametrize("res", [0.05, 0.1, 0.2])
def test_per_hypothesis_parity(res):
    rng = np.random.default_rng(int(res * 1000))
    origin = (-0.35, 0.15, -0.2)
    ext = (2.0, 1.6, 1.2)
    size = [int(np.ceil(e / res)) for e in ext]
    pts, special = _scene(rng, origin, ext)
    ids = _hypotheses(rng, len(pts), special, 700)
    # the plain (n,3) array
    g, gm, om = _both(res, size, origin, pts)
    per = _check_parity(gm, om, ids)
    oks = [p[1] for p in per]
    assert 0 < sum(oks) < len(oks)
    assert any(p[1] and (p[0].norm[0] == 0 or p[0].norm[1] == 0) for p in per), "no axis-parallel plane was fitted"
    # the same cloud as 16-byte records with xyz at offset 4 (a field in front of it)
    rec = np.zeros((len(pts), 4), np.float32)
    rec[:, 0] = rng.random(len(pts))
    rec[:, 1:] = pts
    cloud = pc.PointCloud(pc.PointCloudHeader(["intensity", "x", "y", "z"], [4, 4, 4, 4], [1, 1, 1, 1],
                                              Width=len(pts)), len(pts), rec)
    gm16 = sac.NewVoxelGridSurfaceModel(g, cloud)
    _check_parity(gm16, om, ids)


# ------------------------------------------------------------------ 3. the rules of Compute
def test_first_max_wins_and_zero_is_never_chosen(golden):
    t = golden("ref_sac.json")["sac"]
    pts = np.array(t["points"], np.float32)
    g, gm, om = _both(t["resolution"], t["size"], t["origin"], pts)
    best = [1, 5, 7]
    ids = np.array([[0, 1, 2], [3, 10, 11], best, [4, 8, 12], best, [1, 5, 7], [0, 0, 1]], np.int64).reshape(-1)
    found, b, e, _, ok, _, score = gm.compute(ids)
    assert found and b == 2 and e == score.max() and score[4] == score[2] == score[5]
    _check_parity(gm, om, ids)
    # only degenerate hypotheses: nothing scores, Compute is false
    found, b, e, c, ok, _, score = gm.compute(np.array([0, 1, 2, 1, 1, 8], np.int64))
    assert (found, b, e, c) == (False, -1, 0, None) and not ok.any() and not score.any()


def test_empty_grid_keeps_previous_coefficients(golden):
    t = golden("ref_sac.json")["sac"]
    pts = np.array(t["points"], np.float32)
    g, gm, om = _both(t["resolution"], t["size"], t["origin"], pts)
    s = sac.New(sac.NewRandomSampler(len(pts), 3), gm)
    assert s.Compute(t["n"])
    prev = s.Coefficients()
    empty = segmentation.StorageVoxelGrid(t["resolution"], t["size"], t["origin"])  # no point added
    em = sac.NewVoxelGridSurfaceModel(empty, pts)
    ids = np.random.default_rng(1).integers(0, len(pts), size=90)
    found, b, e, _, ok, _, score = em.compute(ids)
    assert ok.any() and not score.any() and not found and b == -1
    s.Model = em
    assert not s.Compute(t["n"])
    assert s.Coefficients() is prev
    assert not s.Compute(0)
    assert s.Coefficients() is prev
    s.Model = gm
    assert not s.Compute(0)


# ------------------------------------------------------------------ 4. scale
def test_scale_global_bits():
    rng = np.random.default_rng(11)
    res = 0.04
    size = (256, 256, 128)                     # 8.4M voxels
    origin = np.array([-5.0, -4.0, -0.5], np.float32)
    e = np.array(size) * res
    floor = np.c_[rng.random(400000) * e[0], rng.random(400000) * e[1], 0.3 + rng.normal(0, 0.004, 400000)]
    wall = np.c_[rng.random(250000) * e[0], 2.5 + rng.normal(0, 0.004, 250000), rng.random(250000) * e[2]]
    ramp_xy = rng.random((150000, 2)) * e[:2]
    ramp = np.c_[ramp_xy, 0.4 * ramp_xy[:, 0] + rng.normal(0, 0.004, 150000)]
    clutter = rng.random((750000, 3)) * e
    pts = (np.concatenate([floor, wall, ramp, clutter]) + origin).astype(np.float32)
    g, gm, om = _both(res, size, origin, pts)
    _, _, n_occ = g._counts()
    assert len(pts) >= 1_000_000 and g.Len() >= 8_000_000
    assert n_occ > 20480 * 32, n_occ           # more occupied voxels than the LDS bitmap holds
    k = [0, 400000, 650000, 800000, len(pts)]
    ids = []
    for h in range(512):                       # triples within one structure, and mixed ones
        part = h % 5
        if part < 3:
            ids.append(rng.integers(k[part], k[part + 1], size=3))
        else:
            ids.append(rng.integers(0, len(pts), size=3))
    ids = np.concatenate(ids).astype(np.int64)
    per = _check_parity(gm, om, ids)
    sizes = [len(p[0].sequences()[0]) * len(p[0].sequences()[1]) for p in per if p[1]]
    assert max(sizes) >= 100_000, max(sizes)
    found, best, _, c, _, _, _ = gm.compute(ids, per_hypothesis=False)
    assert found
    assert np.array_equal(c.Inliers(0.05), per[best][0].Inliers(0.05))


# ------------------------------------------------------------------ 5. the model owns its copies
def test_cloud_ownership():
    import torch
    rng = np.random.default_rng(5)
    pts, special = _scene(rng, (0.0, 0.0, 0.0), (1.5, 1.5, 1.0))
    res, size, origin = 0.1, (15, 15, 10), (0.0, 0.0, 0.0)
    ids = _hypotheses(rng, len(pts), special, 300)
    host = pts.copy()
    g = _grid(res, size, origin, pts)
    hm = sac.NewVoxelGridSurfaceModel(g, host)
    dev = torch.zeros((len(pts), 5), dtype=torch.float32, device="cuda")
    dev[:, :3] = torch.from_numpy(pts).cuda()
    dm = sac.NewVoxelGridSurfaceModel(g, dev)
    want = hm.compute(ids)
    host[:] = 7.0                               # the caller's buffers change after creation
    dev.fill_(-3.0)
    torch.cuda.synchronize()
    g.AddAll(np.zeros((0, 3), np.float32))      # ... and so does the grid
    for m in (hm, dm):
        got = m.compute(ids)
        assert got[:3] == want[:3]
        assert np.array_equal(got[4], want[4]) and np.array_equal(got[6], want[6])
        assert all((a is None and b is None) or np.array_equal(a.Array(), b.Array()) for a, b in zip(got[5], want[5]))
        assert np.array_equal(got[3].Inliers(0.05), want[3].Inliers(0.05))


# ------------------------------------------------------------------ 6. errors
def _raw_compute(m, ids, n):
    found, best, bs = C.c_int32(-7), C.c_int64(-7), C.c_int64(-7)
    bc = L.SacPlane()
    C.memset(C.byref(bc), 0x5A, C.sizeof(bc))
    ok = np.full(4, -7, np.int32)
    score = np.full(4, -7, np.int64)
    coeff = (L.SacPlane * 4)()
    C.memset(coeff, 0x5A, C.sizeof(coeff))
    rc = L.lib().pcgx_sac_plane_compute(m, L.ptr(ids) if ids is not None else None, n, C.byref(found), C.byref(best),
                                        C.byref(bs), C.byref(bc), L.ptr(ok), C.cast(coeff, C.c_void_p), L.ptr(score))
    untouched = (found.value, best.value, bs.value) == (-7, -7, -7) and (ok == -7).all() and (score == -7).all() and \
        set(bytes(coeff)) == {0x5A} and set(bytes(bc)) == {0x5A}
    return rc, untouched


def test_errors(golden):
    t = golden("ref_sac.json")["sac"]
    pts = np.array(t["points"], np.float32)
    g, gm, om = _both(t["resolution"], t["size"], t["origin"], pts)
    for bad in ([1, 5, 13], [1, -1, 7]):
        rc, untouched = _raw_compute(gm._h, np.array([1, 5, 7] + bad, np.int64), 2)
        assert rc == L.PCGX_E_OUT_OF_RANGE and untouched, bad
    rc, untouched = _raw_compute(gm._h, np.array([1, 5, 7], np.int64), -1)
    assert rc == L.PCGX_E_INVALID and untouched
    rc, untouched = _raw_compute(None, np.array([1, 5, 7], np.int64), 1)
    assert rc == L.PCGX_E_INVALID and untouched
    rc, untouched = _raw_compute(gm._h, None, 1)
    assert rc == L.PCGX_E_INVALID and untouched
    with pytest.raises(L.PcgxError) as ei:
        gm.compute(np.array([0, 1, 99], np.int64))
    assert ei.value.code == L.PCGX_E_OUT_OF_RANGE
    h = C.c_void_p()
    assert L.lib().pcgx_sac_plane_model_create(None, L.ptr(pts), len(pts), 12, 0, 0, C.byref(h)) == L.PCGX_E_INVALID
    assert L.lib().pcgx_sac_plane_model_create(g._h, L.ptr(pts), len(pts), 8, 0, 0, C.byref(h)) == L.PCGX_E_BAD_FIELD
    c, ok = gm.Fit([1, 5, 7])
    assert ok
    for d in (0.0, -0.1):                       # -d < dd < d holds for no dd (surface.go:230)
        assert len(c.Inliers(d)) == 0
        assert not c.IsIn(pts[0], d)


def test_lattice_too_large():
    """a cut more than 8192 lattice steps long is PCGX_E_TOO_LARGE, not a shorter lattice"""
    pts = np.array([[0.2, 0.2, 1.0], [5000.0, 0.3, 1.0], [0.3, 1.2, 1.0], [3.0, 1.0, 0.5]], np.float32)
    g, gm, om = _both(1.0, (10000, 2, 2), (0, 0, 0), pts)
    c, ok = om.Fit([0, 1, 2])
    assert ok and max(len(s) for s in c.sequences(cap=8192)) > 8192
    rc, untouched = _raw_compute(gm._h, np.array([0, 1, 2], np.int64), 1)
    assert rc == L.PCGX_E_TOO_LARGE and untouched
    # a small hypothesis of the same grid is fine
    c2, ok2 = om.Fit([0, 2, 3])
    if ok2 and max(len(s) for s in c2.sequences(cap=8192)) <= 8192:
        _check_parity(gm, om, np.array([0, 2, 3], np.int64))
