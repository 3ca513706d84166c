"""Statistical outlier removal (extension: no reference counterpart; PCL's StatisticalOutlierRemoval) behind the
filter.Filter shape (pc/filter/filter.go:7-9), in the option style of pc/filter/voxelgrid:
New(meanK, stddevMul, WithNegative(True)).Filter(pp).

A point's mean distance d_i is the mean of the distances to its meanK nearest other finite points (float64); points
with d_i <= mu + stddevMul * sigma are kept (WithNegative(True): the others), in input order, records byte for byte.
Non-finite points are dropped in both modes.  The contract is include/pcgx.h's pcgx_sor_filter.

RadiusOutlierRemoval(radius, minNeighbors, WithNegative(True)) beside it keeps the finite points with at least
minNeighbors finite points within radius, themselves included (include/pcgx.h's pcgx_ror_filter)."""
import ctypes as C

import numpy as np

from . import _lib as L
from .pc import PointCloud


def WithNegative(negative):
    def opt(o):
        o.Negative = bool(negative)
    return opt


class StatisticalOutlierRemoval:
    def __init__(self, meanK, stddevMul, *opts):
        self.MeanK = int(meanK)
        self.StddevMul = float(stddevMul)
        self.Negative = False
        self.MeanDist = None  # after Filter: float64 [n] by input index, NaN for non-finite points
        self.Stats = None     # after Filter / FilterDev: (mu, sigma, threshold)
        for o in opts:
            o(self)

    def Filter(self, pp):
        """Returns a new PointCloud (header cloned, Width = M, Height = 1)."""
        if not isinstance(pp, PointCloud):
            pp = PointCloud.from_xyz(pp)
        stride, off = pp.Stride(), pp.xyz_offset()
        n = pp.Points
        out = np.empty(max(n, 1) * stride, np.uint8)
        md = np.empty(max(n, 1), np.float64)
        stats = np.empty(3, np.float64)
        m = C.c_int64()
        L.check(L.lib().pcgx_sor_filter(L.ptr(pp.Data), n, stride, off, self.MeanK, self.StddevMul, int(self.Negative),
                                        L.ptr(out), C.byref(m), L.ptr(md), L.ptr(stats)))
        self.MeanDist = md[:n]
        self.Stats = tuple(float(v) for v in stats)
        h = pp.PointCloudHeader.Clone()
        h.Width, h.Height = m.value, 1
        return PointCloud(h, m.value, out[: m.value * stride].copy())

    def FilterDev(self, d_data, n, stride, off, d_out, d_mean_dist=0, stream=0):
        """Device-resident variant (raw device addresses; d_out >= n * stride bytes, d_mean_dist float64 [n] or 0).
        Returns M; self.Stats holds (mu, sigma, threshold).  Returns when the work on `stream` is done."""
        stats = np.empty(3, np.float64)
        m = C.c_int64()
        L.check(L.lib().pcgx_sor_filter_dev(L.ptr(int(d_data)), int(n), int(stride), int(off), self.MeanK,
                                            self.StddevMul, int(self.Negative), L.ptr(int(d_out)), C.byref(m),
                                            L.ptr(int(d_mean_dist)) if d_mean_dist else None, L.ptr(stats),
                                            L.ptr(stream) if stream else None))
        self.Stats = tuple(float(v) for v in stats)
        return m.value


def New(meanK, stddevMul, *opts):
    return StatisticalOutlierRemoval(meanK, stddevMul, *opts)


class RadiusOutlierRemoval:
    """Radius outlier removal (extension: no reference counterpart; PCL's RadiusOutlierRemoval): a finite point is kept
    when at least minNeighbors finite points lie within radius of it (DistSq < radius^2, itself included), in input
    order, records byte for byte; WithNegative(True) keeps the other finite points.  The contract is include/pcgx.h's
    pcgx_ror_filter."""

    def __init__(self, radius, minNeighbors, *opts):
        self.Radius = float(radius)
        self.MinNeighbors = int(minNeighbors)
        self.Negative = False
        for o in opts:
            o(self)

    def Filter(self, pp):
        """Returns a new PointCloud (header cloned, Width = M, Height = 1)."""
        if not isinstance(pp, PointCloud):
            pp = PointCloud.from_xyz(pp)
        stride, off = pp.Stride(), pp.xyz_offset()
        n = pp.Points
        out = np.empty(max(n, 1) * stride, np.uint8)
        m = C.c_int64()
        L.check(L.lib().pcgx_ror_filter(L.ptr(pp.Data), n, stride, off, self.Radius, self.MinNeighbors,
                                        int(self.Negative), L.ptr(out), C.byref(m)))
        h = pp.PointCloudHeader.Clone()
        h.Width, h.Height = m.value, 1
        return PointCloud(h, m.value, out[: m.value * stride].copy())

    def FilterDev(self, d_data, n, stride, off, d_out, stream=0):
        """Device-resident variant (raw device addresses; d_out >= n * stride bytes).  Returns M when the work on
        `stream` is done."""
        m = C.c_int64()
        L.check(L.lib().pcgx_ror_filter_dev(L.ptr(int(d_data)), int(n), int(stride), int(off), self.Radius,
                                            self.MinNeighbors, int(self.Negative), L.ptr(int(d_out)), C.byref(m),
                                            L.ptr(stream) if stream else None))
        return m.value
