"""Ground segmentation on the GPU (KDTree.Ground / GroundDev, csrc/ground.hip) against the NumPy restatement of its
contract (tests/ground_oracle.py).  Rule of every case: every integer output is array_equal to the oracle, surface and hag
are equal to the oracle's by uint32 view, the padding is checked, a second call gives the first call's bits, and the
device form over tensors filled with rubbish equals the host form."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_oracle as GO  # noqa: E402
import ground_scenes as GS  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def K():
    from pcgol_amd import kdtree
    return kdtree


@pytest.fixture(scope="module")
def hill(K):
    P, is_terrain = GS.hill()
    return P, is_terrain, K.KDTree(P)


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def ground_dev(t, cell, half, height, origin, dims, want=("window", "surface", "hag")):
    """The device form over torch tensors filled with rubbish -> dict of arrays, ids with their padding."""
    import torch
    dev = torch.device("cuda", 0)
    n, cells = t.Len(), int(dims[0]) * int(dims[1])
    i32 = torch.int32
    d_lab, d_ids, d_win = (torch.full((max(n, 1),), -7, dtype=i32, device=dev) for _ in range(3))
    d_sz, d_n = torch.full((2,), -7, dtype=i32, device=dev), torch.full((1,), -7, dtype=i32, device=dev)
    d_sf = torch.full((cells,), 7.0, dtype=torch.float32, device=dev)
    d_hag = torch.full((max(n, 1),), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t.GroundDev(cell, half, height, origin, dims, d_lab.data_ptr(), d_sz.data_ptr(), d_ids.data_ptr(), d_n.data_ptr(),
                d_window=d_win.data_ptr() if "window" in want else 0, d_surface=d_sf.data_ptr() if "surface" in want else 0,
                d_hag=d_hag.data_ptr() if "hag" in want else 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = dict(labels=d_lab, sizes=d_sz, ids=d_ids, n_groups=d_n, window=d_win, surface=d_sf, hag=d_hag)
    return {k: v.cpu().numpy() for k, v in r.items()}


def check(K, P, origin, dims, cell, half, height, t=None, deleted=None):
    """Both forms against the oracle -> (host result, oracle result)."""
    t = t if t is not None else K.KDTree(P)
    n = len(P)
    want = GO.ground(P, origin, dims, cell, half, height, deleted=deleted)
    got = t.Ground(cell, half, height, Origin=origin, Dims=dims)
    k = int(want["sizes"].sum())
    assert got.n_groups == 2 and np.array_equal(got.sizes, want["sizes"]), (got.sizes, want["sizes"])
    assert np.array_equal(got.labels, want["labels"]) and got.labels.dtype == np.int64 and len(got.labels) == n
    assert np.array_equal(got.ids, want["ids"][:k]) and np.array_equal(got.window, want["window"])
    assert got.surface.shape == (dims[1], dims[0]) and np.array_equal(bits(got.surface), bits(want["surface"]))
    assert np.array_equal(bits(got.hag), bits(want["hag"]))
    again = t.Ground(cell, half, height, Origin=origin, Dims=dims)
    for f in ("labels", "sizes", "ids", "window"):
        assert np.array_equal(getattr(got, f), getattr(again, f)), f
    assert np.array_equal(bits(got.surface), bits(again.surface)) and np.array_equal(bits(got.hag), bits(again.hag))
    dev = ground_dev(t, cell, half, height, origin, dims)
    assert dev["n_groups"][0] == 2 and np.array_equal(dev["sizes"], want["sizes"])
    assert np.array_equal(dev["labels"][:n], want["labels"]) and np.array_equal(dev["window"][:n], want["window"])
    assert np.array_equal(dev["ids"][:n], want["ids"]) and np.all(want["ids"][k:] == -1)  # ... with the padding
    assert np.array_equal(bits(dev["surface"]), bits(want["surface"]).reshape(-1))
    assert np.array_equal(bits(dev["hag"][:n]), bits(want["hag"]))
    return got, want


def cloud(rng, n, nx, ny, cell=1.0, spread=4.0, margin=0.0):
    """n random points over an nx x ny grid of `cell` from the origin (margin: that far beyond it on every side)"""
    lo = np.array([-margin, -margin, -spread])
    ext = np.array([nx * cell + 2 * margin, ny * cell + 2 * margin, 2 * spread])
    return (rng.random((n, 3)) * ext + lo).astype(f32)


def test_hill(K, hill):
    P, is_terrain, t = hill
    got, want = check(K, P, GS.HILL_ORIGIN, GS.HILL_DIMS, GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT, t=t)
    g = got.labels == 0
    assert g[is_terrain].mean() >= 0.99 and g[~is_terrain].mean() <= 0.05  # (the oracle's own test says why)
    assert len(np.unique(got.window[got.window >= 0])) >= 2
    # the grid left out: the box of the live points, in float32
    o, d = t.GroundGrid(GS.HILL_CELL)
    assert np.array_equal(o, P[:, :2].min(axis=0))
    assert np.array_equal(d, (np.floor((P[:, :2].max(axis=0) - o) / f32(GS.HILL_CELL)) + 1).astype(np.int32))
    auto = t.Ground(GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT)
    w = GO.ground(P, o, d, GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT)
    assert np.array_equal(auto.labels, w["labels"]) and np.array_equal(bits(auto.surface), bits(w["surface"]))
    assert np.all(auto.labels >= 0) and np.array_equal(auto.origin, o) and np.array_equal(auto.dims, d)


def test_no_window(K, hill):
    P, _, t = hill
    got, _ = check(K, P, GS.HILL_ORIGIN, GS.HILL_DIMS, GS.HILL_CELL, [], [], t=t)
    assert got.sizes[1] == 0 and np.all(got.window == -1) and np.isinf(got.surface).any()  # S_0, its empty cells +inf


def test_optional_outputs_null(K, hill):
    P, _, t = hill
    full = ground_dev(t, GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT, GS.HILL_ORIGIN, GS.HILL_DIMS)
    none = ground_dev(t, GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT, GS.HILL_ORIGIN, GS.HILL_DIMS, want=())
    for f in ("labels", "sizes", "ids", "n_groups"):
        assert np.array_equal(full[f], none[f]), f
    assert np.all(none["window"] == -7) and np.all(none["surface"] == 7.0) and np.all(none["hag"] == 7.0)  # untouched
    for one in ("window", "surface", "hag"):
        r = ground_dev(t, GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT, GS.HILL_ORIGIN, GS.HILL_DIMS, want=(one,))
        assert np.array_equal(bits(r[one]) if one != "window" else r[one], bits(full[one]) if one != "window" else full[one])
        assert np.array_equal(r["ids"], full["ids"])


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 37), (37, 1), (2, 2)])
def test_thin_grids(K, nx, ny):
    rng = np.random.default_rng(nx * 100 + ny)
    P = cloud(rng, 300, nx, ny, margin=0.5)
    check(K, P, (0, 0), (nx, ny), 1.0, [1, 3, 50], [0.5, 1.0, 2.0])


def test_sizes_across_the_tile(K):
    tile = K.GroundTile()
    assert tile == 1024
    rng = np.random.default_rng(8)
    for m in (tile - 1, tile, tile + 1):
        for nx, ny in ((m, 3), (3, m)):
            P = cloud(rng, 2500, nx, ny)  # most cells empty: holes of every width
            P[:40, :2] = [[nx - 0.5, ny - 0.5]] * 20 + [[0.25, 0.25]] * 20  # the last cell and the first
            check(K, P, (0, 0), (nx, ny), 1.0, [1, 6, 40], [0.5, 1.0, 3.0])
    m = 2 * tile + 1  # a lane holds three cells of a row
    check(K, cloud(rng, 3000, m, 2), (0, 0), (m, 2), 1.0, [2, 700], [0.5, 3.0])


def test_one_long_row(K):
    rng = np.random.default_rng(9)
    P = cloud(rng, 6000, 8192, 1)
    P[0, :2] = [8191.5, 0.5]
    check(K, P, (0, 0), (8192, 1), 1.0, [3, 300, 8192], [0.5, 2.0, 4.0])
    check(K, P[:, [1, 0, 2]].copy(), (0, 0), (1, 8192), 1.0, [5, 5000], [0.5, 4.0])


def test_half_at_least_both_dims(K):
    rng = np.random.default_rng(10)
    P = cloud(rng, 500, 12, 9)
    got, _ = check(K, P, (0, 0), (12, 9), 1.0, [12], [0.5])
    assert np.all(bits(got.surface) == bits(P[:, 2].min()))  # the opening of the whole grid: its minimum
    check(K, P, (0, 0), (12, 9), 1.0, [9, 11, 12, 13, 8192], [0.5] * 5)


def test_half_across_the_loop_threshold(K):
    h = K.GroundLoopMax()
    assert h >= 2
    rng = np.random.default_rng(12)
    P = cloud(rng, 5000, 3 * h, 2 * h + 5)  # wider and higher than the windows at the threshold
    for half in ([h - 1], [h], [h + 1], [h - 1, h, h + 1, 2 * h + 1]):
        check(K, P, (0, 0), (3 * h, 2 * h + 5), 1.0, half, [0.3 * (k + 1) for k in range(len(half))])
    P = cloud(rng, 1500, 70, 45)
    for hh in (1, 2, 3, 5, 8, 16, 17, 33):  # the plain loop, windows inside the grid and beyond it
        check(K, P, (0, 0), (70, 45), 1.0, [hh], [0.4])
    P = cloud(rng, 1500, 600, 7)
    for hh in (h + 1, h + 2, 95, 96, 127, 128, 129, 200, 255, 256, 257, 511, 512):  # the doubling: d = 0, 1, ..., 2^p - 1
        if hh > h:
            check(K, P, (0, 0), (600, 7), 1.0, [hh], [0.4])


def test_hole_between_the_windows(K):
    rng = np.random.default_rng(13)
    P = cloud(rng, 12000, 40, 40, spread=1.0)
    hole = (P[:, 0] >= 15) & (P[:, 0] < 24) & (P[:, 1] >= 15) & (P[:, 1] < 24)  # 9 x 9 cells
    P = P[~hole]
    got, want = check(K, P, (0, 0), (40, 40), 1.0, [2, 8], [0.5, 1.5])
    s0 = GO.surfaces(P, (0, 0), (40, 40), 1.0, [2])[1]
    # wider than the first window: its middle cell sees no point in either half, and stays empty
    assert (s0[0] == GO.EMPTY)[15:24, 15:24].all() and np.array_equal(np.argwhere(s0[1] == GO.EMPTY), [[19, 19]])
    assert not np.isinf(got.surface).any()  # narrower than the last


def test_all_cells_empty_but_one(K):
    rng = np.random.default_rng(14)
    P = cloud(rng, 400, 1, 1)
    P[:, :2] += [17, 11]
    P[::9, 0] += 40  # and some points outside the grid
    got, _ = check(K, P, (0, 0), (30, 20), 1.0, [1, 4], [0.5, 1.0])
    # each half of each window reaches its half-width further: 1 + 2 (1 + 1 + 4 + 4) = 21 cells, 19 where the grid ends
    assert np.isinf(got.surface).sum() == 30 * 20 - 21 * 19


def test_signed_zeros_and_equal_z(K):
    P = np.array([[0.5, 0.5, 0.0], [0.6, 0.5, -0.0], [0.7, 0.5, 0.0], [1.5, 0.5, 0.0]], f32)
    got, _ = check(K, P, (0, 0), (2, 1), 1.0, [1], [1.0])
    assert bits(got.surface)[0, 0] == 0x80000000 and bits(got.surface)[0, 1] == 0x80000000 and got.sizes[0] == 4
    rng = np.random.default_rng(15)
    P = cloud(rng, 3000, 25, 25)
    P[:, 2] = f32(1.25)
    got, _ = check(K, P, (0, 0), (25, 25), 1.0, [1, 3, 9], [1e-6, 1e-6, 1e-6])
    assert got.sizes[1] == 0 and np.all(got.hag == 0)


def test_non_finite_and_outside_points(K):
    rng = np.random.default_rng(16)
    P = cloud(rng, 4000, 20, 14, margin=3.0)  # outside on all four sides
    P[5], P[6], P[7], P[8] = [np.nan, 3, 0], [3, np.inf, 0], [3, 3, -np.inf], [3, 3, np.nan]
    P[9], P[10], P[11], P[12] = [20.0, 3, 0], [3, 14.0, 0], [-1e-30, 3, 0], [0.0, 0.0, -9.0]  # the far edges; the near corner
    got, want = check(K, P, (0, 0), (20, 14), 1.0, [1, 5], [0.5, 1.5])
    assert list(got.labels[5:12]) == [-1] * 7 and got.labels[12] == 0
    assert (got.labels == -1).sum() > 1000 and np.all(bits(got.hag)[got.labels == -1] == 0x7FC00000)
    for side in (P[:, 0] < 0, P[:, 0] >= 20, P[:, 1] < 0, P[:, 1] >= 14):
        assert side.sum() > 100 and np.all(got.labels[side & np.isfinite(P).all(axis=1)] == -1)
    check(K, P, (-1.5, 2.25), (9, 7), 2.5, [1, 2], [0.5, 1.5])  # a grid inside the cloud, cells that are not unit


def test_deleted_points(K):
    rng = np.random.default_rng(17)
    P = cloud(rng, 5000, 30, 30)
    t = K.KDTree(P)
    args = ((0, 0), (30, 30), 1.0, [1, 4], [0.4, 1.2])
    before, _ = check(K, P, *args, t=t)
    lowest = np.flatnonzero(before.hag == 0)[::2]  # every other cell's lowest point: the surface itself changes
    gone = np.concatenate([lowest, np.arange(100, 400)])
    t.DeletePoints(gone)
    deleted = np.zeros(len(P), bool)
    deleted[gone] = True
    after, _ = check(K, P, *args, t=t, deleted=deleted)
    assert np.all(after.labels[gone] == -1) and not np.array_equal(bits(after.surface), bits(before.surface))
    t.DeletePoint(int(np.flatnonzero(after.labels == 0)[0]))
    deleted[np.flatnonzero(after.labels == 0)[0]] = True
    check(K, P, *args, t=t, deleted=deleted)


def test_atomic_contention_in_one_cell(K):
    rng = np.random.default_rng(18)
    P = np.concatenate([rng.random((50000, 2)) * 0.99 + 1, rng.standard_normal((50000, 1)) * 5], axis=1).astype(f32)
    got, _ = check(K, P, (0, 0), (3, 3), 1.0, [1], [2.0])
    assert bits(got.surface)[1, 1] == bits(P[:, 2].min()) and got.sizes.sum() == 50000 and got.sizes[1] > 10000


def test_invalid_arguments_write_nothing(K, hill):
    import ctypes as C
    from pcgol_amd import _lib as L
    P, _, t = hill
    nan, inf = float("nan"), float("inf")
    ok = dict(CellSize=0.5, Half=[1, 2], Height=[0.2, 0.4], Origin=(0, 0), Dims=(96, 64))
    bad = [dict(CellSize=0.0), dict(CellSize=-1.0), dict(CellSize=nan), dict(CellSize=inf), dict(Origin=(nan, 0)),
           dict(Origin=(0, -inf)), dict(Dims=(0, 64)), dict(Dims=(96, 8193)), dict(Dims=(-3, 64)), dict(Half=[0, 2]),
           dict(Half=[1, 8193]), dict(Half=[1, -2]), dict(Height=[0.2, 0.0]), dict(Height=[nan, 0.4]), dict(Height=[0.2, inf]),
           dict(Height=[-0.2, 0.4]), dict(Half=[1] * 65, Height=[0.5] * 65), dict(Half=[1, 2, 3])]
    for kw in bad:
        a = dict(ok)
        a.update(kw)
        with pytest.raises((L.PcgxError, ValueError)):
            t.Ground(a.pop("CellSize"), a.pop("Half"), a.pop("Height"), **a)
    assert t.Ground(0.5, [8192], [0.5], Origin=(0, 0), Dims=(8, 8)).n_groups == 2  # the bounds themselves are inside
    # ... and nothing is written: the raw calls with rubbish in every output
    n = len(P)
    out = [np.full(k, 77, d) for k, d in ((n, np.int64), (2, np.int64), (n, np.int64), (n, np.int32), (96 * 64, f32), (n, f32))]
    cnt = C.c_int64(77)
    lib = L.lib()
    origin, dims = np.zeros(2, f32), np.array([96, 64], np.int32)
    half, height = np.array([1, 2], np.int32), np.array([0.2, 0.4], f32)

    def raw(tree=t._h, o=origin, d=dims, cell=0.5, k=2, hf=half, ht=height, skip=None, cnt_ptr=True):
        p = [None if i == skip else L.ptr(a) for i, a in enumerate(out)]
        q = lambda a: L.ptr(a) if a is not None else None  # noqa: E731
        return lib.pcgx_kdtree_ground(tree, q(o), q(d), cell, k, q(hf), q(ht), p[0], p[1], p[2],
                                      C.byref(cnt) if cnt_ptr else None, p[3], p[4], p[5])
    calls = [dict(tree=None), dict(o=None), dict(d=None), dict(cell=nan), dict(cell=0.0), dict(k=-1), dict(k=65), dict(hf=None),
             dict(ht=None), dict(o=np.array([inf, 0], f32)), dict(d=np.array([96, 0], np.int32)),
             dict(d=np.array([8193, 64], np.int32)), dict(hf=np.array([1, 0], np.int32)), dict(hf=np.array([8193, 1], np.int32)),
             dict(ht=np.array([0.2, nan], f32)), dict(ht=np.array([0.0, 0.4], f32)), dict(skip=0), dict(skip=1), dict(skip=2),
             dict(cnt_ptr=False)]
    for kw in calls:
        assert raw(**kw) == L.PCGX_E_INVALID, kw
        assert cnt.value == 77 and all(np.all(a == 77) for a in out), kw
    for skip in (3, 4, 5):  # the optional ones may be NULL
        for a in out:
            a[...] = 77
        assert raw(skip=skip) == L.PCGX_OK and np.all(out[skip] == 77) and cnt.value == 2 and out[1].sum() == (out[0] >= 0).sum()
    assert np.all(out[2][out[1].sum():] == -1)  # the host form's padding
    # the device form: the same checks before anything is enqueued
    import torch
    d = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    for kw in (dict(CellSize=nan), dict(Dims=(96, 0)), dict(Half=[0, 1]), dict(Height=[0.2, -1.0])):
        a = dict(ok)
        a.update(kw)
        with pytest.raises(L.PcgxError):
            t.GroundDev(a["CellSize"], a["Half"], a["Height"], a["Origin"], a["Dims"], d.data_ptr(), d.data_ptr(), d.data_ptr(),
                        d.data_ptr())
    for miss in range(4):
        p = [0 if i == miss else d.data_ptr() for i in range(4)]
        with pytest.raises(L.PcgxError):
            t.GroundDev(0.5, [1], [0.5], (0, 0), (96, 64), *p)
    torch.cuda.synchronize()
    assert bool((d == -7).all())


def test_the_chain_on_one_stream(K, hill):
    """GroundDev -> GroupStatsDev -> GroupHullsDev on d_ids / d_sizes / d_n_groups as they are, one stream, no
    synchronise in between; then GroundSegmentation's Extract, Boxes and Footprints: equal to the host forms."""
    import torch
    from pcgol_amd import segmentation
    P, is_terrain, t = hill
    n = len(P)
    dev = torch.device("cuda", 0)
    i32, f64 = torch.int32, torch.float64
    host = t.Ground(GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT, Origin=GS.HILL_ORIGIN, Dims=GS.HILL_DIMS)
    d_lab, d_ids, h_ids = (torch.full((n,), -7, dtype=i32, device=dev) for _ in range(3))
    d_sz, d_n = torch.full((2,), -7, dtype=i32, device=dev), torch.full((1,), -7, dtype=i32, device=dev)
    g_cnt, h_sz = torch.zeros(2, dtype=i32, device=dev), torch.zeros(2, dtype=i32, device=dev)
    g_cen, g_axes, g_obb = (torch.zeros((2, k), dtype=f64, device=dev) for k in (3, 9, 6))
    h_area, h_rect = torch.zeros(2, dtype=f64, device=dev), torch.zeros((2, 6), dtype=f64, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t.GroundDev(GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT, GS.HILL_ORIGIN, GS.HILL_DIMS, d_lab.data_ptr(), d_sz.data_ptr(),
                    d_ids.data_ptr(), d_n.data_ptr(), stream=s.cuda_stream)
        t.GroupStatsDev(d_ids.data_ptr(), n, d_sz.data_ptr(), 2, d_n_groups=d_n.data_ptr(), d_count=g_cnt.data_ptr(),
                        d_centroid=g_cen.data_ptr(), d_axes=g_axes.data_ptr(), d_obb=g_obb.data_ptr(), stream=s.cuda_stream)
        t.GroupHullsDev(d_ids.data_ptr(), n, d_sz.data_ptr(), 2, d_n_groups=d_n.data_ptr(), d_hull_sizes=h_sz.data_ptr(),
                        d_hull_ids=h_ids.data_ptr(), d_area=h_area.data_ptr(), d_rect=h_rect.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert int(d_n[0]) == 2 and np.array_equal(d_sz.cpu().numpy(), host.sizes)
    assert np.array_equal(d_lab.cpu().numpy(), host.labels) and np.array_equal(d_ids.cpu().numpy()[:len(host.ids)], host.ids)
    geo, feet = t.GroupStats(host.ids, host.sizes), t.GroupHulls(host.ids, host.sizes)
    assert np.array_equal(g_cnt.cpu().numpy(), geo.count) and np.array_equal(g_cen.cpu().numpy(), geo.centroid)
    assert np.array_equal(g_axes.cpu().numpy().reshape(2, 3, 3), geo.axes) and np.array_equal(g_obb.cpu().numpy(), geo.obb)
    assert np.array_equal(h_sz.cpu().numpy(), feet.hull_sizes) and np.array_equal(h_area.cpu().numpy(), feet.area)
    assert np.array_equal(h_rect.cpu().numpy(), feet.rect)
    assert 0.97 * 48 * 32 < feet.area[0] <= 48 * 32  # the ground's footprint is the whole field
    gs = segmentation.GroundSegmentation(t, CellSize=GS.HILL_CELL, MaxWindowSize=16.5, Slope=0.3, InitialDistance=0.15,
                                         MaxDistance=2.5, Origin=GS.HILL_ORIGIN, Dims=GS.HILL_DIMS)
    ground, other = gs.Extract()
    assert np.array_equal(np.concatenate([ground, other]), host.ids) and len(ground) == host.sizes[0]
    assert np.array_equal(bits(gs.surface), bits(host.surface)) and np.array_equal(bits(gs.hag), bits(host.hag))
    assert np.array_equal(gs.window, host.window)
    assert np.array_equal(gs.Boxes().obb, geo.obb) and np.array_equal(gs.Footprints().rect, feet.rect)
    tall = (gs.hag > 0.3) & (gs.hag < 5.0)  # "keep what stands 0.3 to 5 m above the ground": the things on the hill
    assert tall[~is_terrain].mean() > 0.9 and gs.hag[is_terrain].max() < 2.5  # (the terrain is ground: below the last height)
