"""Statistical outlier removal on the GPU (pcgx_sor_filter / _dev, csrc/sor.hip; pcgol_amd.outlier) against the
float64 oracle (tests/sor_oracle.py): mean distances to 1e-14, mu / sigma / T to 1e-12, the kept set exact but for
points within 1e-12 T of the threshold, records byte for byte in input order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import outlier, synth
from pcgol_amd.pc import PointCloud, PointCloudHeader

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sor_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _check(f, pp, xyz, mean_k, std_mul, negative=False):
    if not isinstance(pp, PointCloud):
        pp = PointCloud.from_xyz(pp)
    out = f.Filter(pp)
    ref = SO.sor(xyz, mean_k, std_mul, negative)
    md = f.MeanDist
    fin = ~np.isnan(ref["mean_dist"])
    assert np.array_equal(np.isnan(md), ~fin)
    assert np.allclose(md[fin], ref["mean_dist"][fin], rtol=1e-14, atol=0)
    mu, sigma, T = f.Stats
    assert mu == pytest.approx(ref["mu"], rel=1e-12) and sigma == pytest.approx(ref["sigma"], rel=1e-12)
    assert T == pytest.approx(ref["T"], rel=1e-12)
    keep = ref["keep"].copy()
    near = fin & (np.abs(ref["mean_dist"] - ref["T"]) <= 1e-12 * abs(ref["T"]))
    got = (md > T) if negative else (md <= T)
    assert not np.any((got != keep) & ~near)
    got &= fin
    stride = pp.Stride()
    recs = pp.Data[: pp.Points * stride].reshape(pp.Points, stride)
    assert out.Points == got.sum() and out.PointCloudHeader.Width == out.Points and out.PointCloudHeader.Height == 1
    assert np.array_equal(out.Data.reshape(-1, stride), recs[got])
    return out, got, ref


def _plane(n, outliers, seed):
    r = _rng(seed)
    p = np.zeros((n, 3), np.float32)
    p[:, :2] = r.random((n, 2)) * 10.0
    p[:, 2] = r.normal(0.0, 0.01, n)
    far = (r.random((outliers, 3)) * 10.0).astype(np.float32)
    far[:, 2] = 3.0 + r.random(outliers) * 5.0
    pts = np.concatenate([p, far])
    perm = r.permutation(len(pts))
    return np.ascontiguousarray(pts[perm], dtype=np.float32), perm >= n


def test_noisy_plane_with_planted_outliers():
    pts, planted = _plane(12_000, 60, 61)
    f = outlier.New(16, 2.0)
    out, kept, ref = _check(f, pts, pts, 16, 2.0)
    assert not kept[planted].any()
    assert kept[~planted].mean() >= 0.99
    # the complement among finite points
    fn = outlier.New(16, 2.0, outlier.WithNegative(True))
    outn, keptn, _ = _check(fn, pts, pts, 16, 2.0, negative=True)
    assert np.array_equal(keptn, ~kept)
    assert fn.Stats == f.Stats


def _records(xyz, seed, layout):
    r = _rng(seed)
    n = len(xyz)
    if layout == "label16":
        dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("label", "<u4")])
        h = PointCloudHeader(["x", "y", "z", "label"], [4, 4, 4, 4], [1, 1, 1, 1], ["F", "F", "F", "U"], Width=n)
    else:  # 15-byte records, xyz at byte 1: nothing aligned
        dt = np.dtype([("a", "u1"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "<u2")])
        h = PointCloudHeader(["a", "x", "y", "z", "b"], [1, 4, 4, 4, 2], [1] * 5, ["U", "F", "F", "F", "U"], Width=n)
    rec = np.zeros(n, dt)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    for name in dt.names:
        if name not in ("x", "y", "z"):
            rec[name] = r.integers(0, np.iinfo(dt[name]).max, n)
    assert dt.itemsize == (16 if layout == "label16" else 15)
    return PointCloud(h, n, rec.view(np.uint8))


def test_records_carried_byte_for_byte_with_nan_points():
    pts, planted = _plane(6000, 30, 62)
    pts[::97] = np.nan
    pts[5::101, 1] = np.inf
    for layout in ("label16", "unaligned15"):
        pp = _records(pts, 63, layout)
        for neg in (False, True):
            f = outlier.New(8, 0.5, outlier.WithNegative(neg))
            out, kept, ref = _check(f, pp, pts, 8, 0.5, negative=neg)
            assert not kept[::97].any() and not kept[5::101].any()


def test_lattice_with_duplicates():
    r = _rng(64)
    g = np.stack(np.meshgrid(*[np.arange(14)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 0.5
    pts = np.repeat(g, r.integers(1, 4, len(g)), axis=0)
    pts = np.concatenate([pts, np.float32([[20, 20, 20], [-9, 3, 3]])])
    pts = np.ascontiguousarray(pts[r.permutation(len(pts))], dtype=np.float32)
    for k in (1, 4, 26, 64):
        _check(outlier.New(k, 2.0), pts, pts, k, 2.0)


def test_deterministic_and_device_agrees():
    import torch
    pts, _ = _plane(40_000, 200, 65)  # above the device tree build's threshold
    pp = _records(pts, 66, "label16")
    f = outlier.New(16, 1.0)
    a = f.Filter(pp)
    md_a, st_a = f.MeanDist.copy(), f.Stats
    b = f.Filter(pp)
    assert np.array_equal(a.Data, b.Data) and f.Stats == st_a
    assert np.array_equal(md_a.view(np.uint64), f.MeanDist.view(np.uint64))
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(pp.Data.copy()).to(dev)
    d_out = torch.zeros(len(pp.Data), dtype=torch.uint8, device=dev)
    d_md = torch.empty(pp.Points, dtype=torch.float64, device=dev)
    m = f.FilterDev(d_in.data_ptr(), pp.Points, 16, 0, d_out.data_ptr(), d_md.data_ptr())
    assert m == a.Points and f.Stats == st_a
    assert np.array_equal(d_out[: m * 16].cpu().numpy(), a.Data)
    assert np.array_equal(d_md.cpu().numpy().view(np.uint64), md_a.view(np.uint64))


def test_errors():
    lib = L.lib()
    pts = synth.uniform_cloud(100, 1.0, 67)
    out = np.empty(100 * 12, np.uint8)
    m = C.c_int64()

    def call(data, n, stride, off, k):
        return lib.pcgx_sor_filter(L.ptr(data), n, stride, off, k, 1.0, 0, L.ptr(out), C.byref(m), None, None)
    assert call(pts, 100, 12, 0, 0) == L.PCGX_E_INVALID
    assert call(pts, 100, 12, 0, 65) == L.PCGX_E_INVALID
    assert call(pts, 100, 8, 0, 4) == L.PCGX_E_BAD_FIELD
    assert call(pts, 100, 12, 4, 4) == L.PCGX_E_BAD_FIELD
    assert call(pts, 8, 12, 0, 8) == L.PCGX_E_NO_POINT   # m == mean_k
    assert call(pts, 0, 12, 0, 8) == L.PCGX_E_NO_POINT
    few = pts.copy()
    few[3:] = np.nan
    assert call(few, 100, 12, 0, 3) == L.PCGX_E_NO_POINT  # three finite points
    assert call(few, 100, 12, 0, 2) == 0 and m.value <= 3
    with pytest.raises(L.ErrNoPoint):
        outlier.New(64, 1.0).Filter(pts[:64])
    assert outlier.New(64, 1.0).Filter(pts[:65]).Points > 0
