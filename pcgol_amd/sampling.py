"""Samplers that keep ORIGINAL records: MinDistance (a radius) and FarthestPoint (a target count, below).

Minimum-distance subsampling (extension: no reference counterpart; CloudCompare's "subsample by space", Poisson-disk
sampling) behind the filter.Filter shape (pc/filter/filter.go:7-9), in the option style of pc/filter/voxelgrid:
MinDistance(radius, WithSeed(7)).Filter(pp).

The kept records are ORIGINAL records, byte for byte and in input order: a maximal set of the finite points no two of
which are within radius of each other (DistSq < radius^2, strict), the one greedy selection by hash(seed, index among
the finite points) keeps.  Non-finite points are dropped.  The contract is include/pcgx.h's pcgx_thin_filter; KDTree.Thin
is the same selection over a tree, with a score as priority and the owner of every dropped point."""
import ctypes as C

import numpy as np

from . import _lib as L
from .pc import PointCloud


def WithSeed(seed):
    def opt(o):
        o.Seed = int(seed) & 0xffffffff
    return opt


class MinDistance:
    def __init__(self, radius, *opts):
        self.Radius = float(radius)
        self.Seed = 0
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
        L.check(L.lib().pcgx_thin_filter(L.ptr(pp.Data), n, stride, off, self.Radius, self.Seed, L.ptr(out), C.byref(m)))
        h = pp.PointCloudHeader.Clone()
        h.Width, h.Height = m.value, 1
        return PointCloud(h, m.value, out[: m.value * stride].copy())

    def FilterDev(self, d_data, n, stride, off, d_out, stream=0):
        """Device-resident variant (raw device addresses; d_out >= n * stride bytes).  Returns M when the work on
        `stream` is done."""
        m = C.c_int64()
        L.check(L.lib().pcgx_thin_filter_dev(L.ptr(int(d_data)), int(n), int(stride), int(off), self.Radius, self.Seed,
                                             L.ptr(int(d_out)), C.byref(m), L.ptr(stream) if stream else None))
        return m.value


def New(radius, *opts):
    return MinDistance(radius, *opts)


def WithStart(index):
    """The first pick: an index among the finite records (-1: the first finite record)."""
    def opt(o):
        o.Start = int(index)
    return opt


class FarthestPoint:
    """Farthest-point sampling to a target count (extension: no reference counterpart; PointNet++'s sampling layer,
    Open3D's farthest_point_down_sample): FarthestPoint(4096, WithStart(0)).Filter(pp).  The output records are ORIGINAL
    records, byte for byte, IN PICK ORDER -- each the finite point farthest (float32 DistSq to the nearest pick so far,
    ties to the earlier record) from those before it -- so the first K records of the output are the output for count K.
    Non-finite points are dropped.  The contract is include/pcgx.h's pcgx_fps_filter; KDTree.FarthestPoints is the same
    selection over a tree, with the distances and the owner of every point."""

    def __init__(self, count, *opts):
        self.Count = int(count)
        self.Start = -1
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
        L.check(L.lib().pcgx_fps_filter(L.ptr(pp.Data), n, stride, off, self.Count, self.Start, L.ptr(out), C.byref(m)))
        h = pp.PointCloudHeader.Clone()
        h.Width, h.Height = m.value, 1
        return PointCloud(h, m.value, out[: m.value * stride].copy())

    def FilterDev(self, d_data, n, stride, off, d_out, stream=0):
        """Device-resident variant (raw device addresses; d_out >= n * stride bytes).  Returns M when the work on
        `stream` is done."""
        m = C.c_int64()
        L.check(L.lib().pcgx_fps_filter_dev(L.ptr(int(d_data)), int(n), int(stride), int(off), self.Count, self.Start,
                                            L.ptr(int(d_out)), C.byref(m), L.ptr(stream) if stream else None))
        return m.value
