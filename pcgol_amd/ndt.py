"""Normal Distributions Transform registration on the GPU (include/pcgx.h "Normal Distributions Transform").

NOT in the reference.  The base cloud (fixed) becomes an NDTMap: one Gaussian per voxel of a StorageVoxelGrid.  NDT.Fit
moves a target cloud onto the map by Gauss-Newton on Magnusson's score; no nearest-neighbour search is involved."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import icp as _icp
from .pc import PointCloud


def _cloud_args(cloud):
    """-> (keep-alive, data pointer, n, stride, xyz offset, on_device)"""
    if isinstance(cloud, PointCloud):
        return cloud.Data, L.ptr(cloud.Data), cloud.Points, cloud.Stride(), cloud.xyz_offset(), 0
    if getattr(cloud, "is_cuda", False):
        if str(cloud.dtype) != "torch.float32" or cloud.dim() != 2 or cloud.shape[1] < 3 or cloud.stride(1) != 1:
            raise ValueError("a device cloud is a (n, >= 3) float32 tensor with unit column stride")
        return cloud, C.c_void_p(cloud.data_ptr()), cloud.shape[0], cloud.stride(0) * 4, 0, 1
    keep = L.f32c(cloud).reshape(-1, 3)
    return keep, L.ptr(keep), len(keep), 12, 0, 0


def _pose(trans):
    return None if trans is None else L.f32c(trans).reshape(16)


class NDTMap:
    """One Gaussian per occupied voxel of vg (segmentation.StorageVoxelGrid) over `cloud`, the cloud vg.AddAll was given:
    a PointCloud, an (n, 3) float32 array or a CUDA (ROCm) torch tensor.  The map copies what it needs: vg and cloud may
    change afterwards.  A voxel with fewer than max(MinPoints, 3) points, or whose points coincide, is invalid; the
    eigenvalues of a valid voxel's covariance are raised to MinEigenRatio times the largest."""

    def __init__(self, vg, cloud, MinPoints=6, MinEigenRatio=0.01):
        self._h = None
        keep, data, n, s, o, on_device = _cloud_args(cloud)
        h = C.c_void_p()
        L.check(L.lib().pcgx_ndt_map_create(vg._h, data if n else None, n, s, o, on_device, int(MinPoints),
                                            float(np.float32(MinEigenRatio)), C.byref(h)))
        self._h = h
        self.Resolution = np.float32(vg.resolution)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                L.lib().pcgx_ndt_map_free(self._h)
                self._h = None
        except Exception:
            pass

    def Counts(self):
        """-> (occupied voxels, valid voxels)"""
        a, b = C.c_int64(), C.c_int64()
        L.check(L.lib().pcgx_ndt_map_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def Cells(self):
        """The occupied voxels in ascending address: dict(addr int64 [m], count, valid int32 [m], mean float32 [m, 3],
        cov6, icov6 float32 [m, 6] in the order xx, xy, xz, yy, yz, zz; zero for invalid voxels)."""
        m = self.Counts()[0]
        out = dict(addr=np.zeros(m, np.int64), count=np.zeros(m, np.int32), valid=np.zeros(m, np.int32),
                   mean=np.zeros((m, 3), np.float32), cov6=np.zeros((m, 6), np.float32),
                   icov6=np.zeros((m, 6), np.float32))
        L.check(L.lib().pcgx_ndt_map_cells(self._h, *[L.ptr(out[k]) if m else None
                                                      for k in ("addr", "count", "valid", "mean", "cov6", "icov6")]))
        return out

    def Evaluate(self, target, trans=None, Neighbors=7, OutlierRatio=0.55):
        """The 30 float64 sums {sum e, sum g [6], sum H upper triangle [21], sum omega, pairs} of the target at pose
        trans (None: the identity)."""
        t = L.f32c(target).reshape(-1, 3)
        tr = _pose(trans)
        sums = np.zeros(30, np.float64)
        L.check(L.lib().pcgx_ndt_evaluate(self._h, L.ptr(t) if len(t) else None, len(t), L.ptr(tr), int(Neighbors),
                                          float(np.float32(OutlierRatio)), L.ptr(sums)))
        return sums

    def EvaluateDev(self, target, sums, trans=None, Neighbors=7, OutlierRatio=0.55, stream=0):
        """Device resident: target a contiguous (n, 3) float32 CUDA tensor, sums a float64 CUDA tensor of 30; enqueued on
        `stream` (a raw stream handle; 0: the library's), returns without waiting."""
        if str(target.dtype) != "torch.float32" or not target.is_contiguous() or target.dim() != 2 or target.shape[1] != 3:
            raise ValueError("target: a contiguous (n, 3) float32 device tensor")
        if str(sums.dtype) != "torch.float64" or sums.numel() < 30 or not sums.is_contiguous():
            raise ValueError("sums: a contiguous float64 device tensor of 30")
        tr = _pose(trans)
        nt = target.shape[0]
        L.check(L.lib().pcgx_ndt_evaluate_dev(self._h, C.c_void_p(target.data_ptr()) if nt else None, nt, L.ptr(tr),
                                              int(Neighbors), float(np.float32(OutlierRatio)),
                                              C.c_void_p(sums.data_ptr()), C.c_void_p(stream) if stream else None))


class NDT:
    """The Fit: evaluate, the plane Fit's evaluate tail (MinPairs on the (point, voxel) pair count, 0 -> 6), the
    Gauss-Newton update (Threshold: the flat test, None -> 0.01; Damping; MaxIteration, 0 -> 20), repeated on the device
    with one read-back.  Neighbors: 1, 7 or 27 candidate voxels per point."""

    def __init__(self, map, Neighbors=7, OutlierRatio=0.55, MinPairs=0, Threshold=None, MaxIteration=0, Damping=0.0):
        self.Map = map
        self.Neighbors = int(Neighbors)
        self.OutlierRatio = float(OutlierRatio)
        self.MinPairs = int(MinPairs)
        self.Threshold = np.zeros(6, np.float32) if Threshold is None else np.asarray(Threshold, np.float32)
        self.MaxIteration = int(MaxIteration)
        self.Damping = float(Damping)

    def Fit(self, target, init=None):
        """-> (trans float32 [16], Stat with Evaluated.Hessian).  target: (n, 3) float32 array or CUDA tensor; init: the
        starting pose (None: the identity).  When no point sees a valid voxel with a weight above zero the gradient is 0
        and `init` comes back as converged: Map.Evaluate(...)[28] (sum omega) tells."""
        if getattr(target, "is_cuda", False):
            if str(target.dtype) != "torch.float32" or target.dim() != 2 or target.shape[1] != 3 or not target.is_contiguous():
                raise ValueError("a device target is a contiguous (n, 3) float32 tensor")
            keep, n, on_device = target, target.shape[0], 1
            data = C.c_void_p(target.data_ptr())
        else:
            keep = L.f32c(target).reshape(-1, 3)
            n, on_device, data = len(keep), 0, L.ptr(keep)
        p = _icp._params(0.0, 0.0, self.MinPairs, np.zeros(6, np.float32), self.Threshold, self.MaxIteration)
        ini = _pose(init)
        trans = np.zeros(16, np.float32)
        st = L.IcpStat()
        h = np.zeros(36, np.float32)
        rc = L.lib().pcgx_ndt_fit(self.Map._h, data if n else None, n, on_device, C.byref(p), self.Damping,
                                  self.Neighbors, float(np.float32(self.OutlierRatio)), L.ptr(ini), L.ptr(trans),
                                  C.byref(st), L.ptr(h))
        if rc == L.PCGX_E_NOT_ENOUGH_PAIRS:
            e = _icp.ErrNotEnoughPairs(rc, L.last_error())
            e.trans, e.stat = trans, _icp.Stat(st)
            raise e
        L.check(rc)
        stat = _icp.Stat(st)
        stat.Evaluated.Hessian = h
        return trans, stat
