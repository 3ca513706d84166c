"""GPU: radius outlier removal (csrc/sor.hip over csrc/dbscan.hip's flag pass; include/pcgx.h, pcgx_ror_filter) against
tests/dbscan_oracle.py: the kept records byte for byte in input order, both modes, the device form, the definition by
DBSCAN's core points, and the errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, outlier, synth
from pcgol_amd.pc import PointCloud, PointCloudHeader

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbscan_oracle as DO  # noqa: E402
from dbscan_scenes import cached, uniform  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
R = 0.032


def _scene():
    """the uniform cloud as 16-byte records {tag, x, y, z} (xyz at byte 4) with 50 NaN rows -> (cloud, xyz)"""
    def make():
        xyz = uniform().copy()
        rng = np.random.default_rng(81)
        bad = rng.choice(len(xyz), 50, replace=False)
        xyz[bad[:30]] = np.nan
        xyz[bad[30:40], 1] = np.inf
        xyz[bad[40:], 2] = np.nan
        dt = np.dtype([("tag", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
        rec = np.zeros(len(xyz), dt)
        rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        rec["tag"] = rng.integers(0, 1 << 32, len(xyz), dtype=np.uint64)
        return np.ascontiguousarray(rec.view(np.uint8)), xyz
    data, xyz = cached("ror-scene", make)
    n = len(xyz)
    h = PointCloudHeader(["tag", "x", "y", "z"], [4, 4, 4, 4], [1, 1, 1, 1], ["U", "F", "F", "F"], Width=n)
    pp = PointCloud(h, n, data)
    assert pp.Stride() == 16 and pp.xyz_offset() == 4
    return pp, xyz


def _keep(xyz, min_neighbors, negative):
    return cached(("ror-keep", min_neighbors, negative), lambda: DO.ror_keep(xyz, R, min_neighbors, negative))


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("min_neighbors", [1, 4])
def test_kept_records_byte_for_byte(min_neighbors, negative):
    import torch
    pp, xyz = _scene()
    n = pp.Points
    finite = np.all(np.isfinite(xyz), axis=1)
    assert int((~finite).sum()) == 50
    keep = _keep(xyz, min_neighbors, negative)
    recs = pp.Data.reshape(n, 16)
    f = outlier.RadiusOutlierRemoval(R, min_neighbors, outlier.WithNegative(negative))
    out = f.Filter(pp)
    assert out.Points == int(keep.sum()) and out.PointCloudHeader.Width == out.Points and out.PointCloudHeader.Height == 1
    assert np.array_equal(out.Data.reshape(-1, 16), recs[keep])
    again = f.Filter(pp)
    assert np.array_equal(again.Data, out.Data)  # the same bits on every call
    if min_neighbors == 1:  # every finite point has itself in reach
        assert np.array_equal(keep, np.zeros(n, bool) if negative else finite)
    else:
        assert 0 < keep.sum() < finite.sum() and not keep[~finite].any()
    # the device form
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(pp.Data.copy()).to(dev)
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    m = f.FilterDev(d_in.data_ptr(), n, 16, 4, d_out.data_ptr())
    assert m == out.Points and np.array_equal(d_out[: m * 16].cpu().numpy(), out.Data)
    # by definition: kind == 2 of DBSCAN on a tree over F with min_pts = min_neighbors
    if not negative:
        kind = kdtree.New(np.ascontiguousarray(xyz[finite])).DBSCAN(R, min_neighbors)[3]
        assert np.array_equal(keep[finite], kind == 2)


def test_plain_xyz_and_the_forced_walk(monkeypatch):
    xyz = synth.uniform_cloud(3000, 1.0, 82)
    want = xyz[DO.ror_keep(xyz, 0.06, 5)]
    assert 0 < len(want) < len(xyz)
    assert np.array_equal(outlier.RadiusOutlierRemoval(0.06, 5).Filter(xyz).Data.view(f32).reshape(-1, 3), want)
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    assert np.array_equal(outlier.RadiusOutlierRemoval(0.06, 5).Filter(xyz).Data.view(f32).reshape(-1, 3), want)


def test_errors():
    lib = L.lib()
    pts = synth.uniform_cloud(100, 1.0, 67)
    out = np.full(100 * 12, 7, np.uint8)
    m = C.c_int64(-7)

    def call(data, n, stride, off, r, k, neg=0):
        return lib.pcgx_ror_filter(L.ptr(data), n, stride, off, r, k, neg, L.ptr(out), C.byref(m))
    for r in (0.0, -1.0, np.inf, np.nan):
        assert call(pts, 100, 12, 0, r, 2) == L.PCGX_E_INVALID
    assert call(pts, 100, 12, 0, 0.1, 0) == L.PCGX_E_INVALID and call(pts, 100, 12, 0, 0.1, -3) == L.PCGX_E_INVALID
    assert call(pts, 100, 8, 0, 0.1, 2) == L.PCGX_E_BAD_FIELD and call(pts, 100, 12, 4, 0.1, 2) == L.PCGX_E_BAD_FIELD
    assert call(pts, 0, 12, 0, 0.1, 2) == L.PCGX_E_NO_POINT
    none = np.full((100, 3), np.nan, f32)
    assert call(none, 100, 12, 0, 0.1, 2) == L.PCGX_E_NO_POINT  # F is empty
    assert m.value == -7 and np.all(out == 7)  # nothing was written
    assert lib.pcgx_ror_filter_dev(None, 100, 12, 0, 0.1, 2, 0, None, C.byref(m), None) == L.PCGX_E_INVALID
    few = pts.copy()
    few[3:] = np.nan
    assert call(few, 100, 12, 0, 10.0, 3) == L.PCGX_OK and m.value == 3
    assert call(few, 100, 12, 0, 10.0, 4) == L.PCGX_OK and m.value == 0
    assert call(few, 100, 12, 0, 10.0, 4, 1) == L.PCGX_OK and m.value == 3
    with pytest.raises(L.ErrNoPoint):
        outlier.RadiusOutlierRemoval(0.1, 2).Filter(none)
