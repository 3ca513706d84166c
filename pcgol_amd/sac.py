"""Mirror of pc/sac (sac.go, randomsample.go, surface.go) on the GPU (include/pcgx.h "sample consensus plane
detection").

SAC.Compute(n) draws the 3n ids of its n hypotheses from the caller's sampler first, in the reference's order
(sac.go:40-43), then fits and evaluates all of them in one device call: neither Fit nor Evaluate draws random
numbers, so the result is the reference loop's for the same draws.  The sampler stays on the host."""
import ctypes as C

import numpy as np

from . import _lib as L
from .pc import PointCloud


class _Sampler:
    def __init__(self, n, seed):
        self.n = int(n)
        self._rng = np.random.default_rng(seed)

    def Sample(self):
        return int(self._rng.integers(self.n))


def NewRandomSampler(n, seed=None):
    """randomsample.go:7-12: a uniform id in [0, n).  Go's unseeded math/rand is not reproducible outside Go; this one
    draws from numpy's default generator (seeded with `seed`).  Any object with Sample() -> int serves SAC."""
    return _Sampler(n, seed)


class Coefficients:
    """voxelGridSurfaceModelCoefficients (surface.go:191-240)."""

    def __init__(self, model, plane, score):
        self._model = model      # (keeps the device copy alive)
        self._c = plane          # _lib.SacPlane
        self._score = int(score)

    def Evaluate(self):
        """surface.go:202-220: the sum of the bucket lengths of the distinct voxels the plane's lattice hits (computed
        on the device by the call that fitted these coefficients)."""
        return self._score

    def Inliers(self, d):
        """surface.go:222-235: ids (ascending) of the model's points with |norm . (p - vgMin) - d_plane| < d."""
        cnt = C.c_int64()
        f = L.lib().pcgx_sac_plane_inliers
        L.check(f(self._model._h, C.byref(self._c), float(np.float32(d)), None, 0, C.byref(cnt)))
        out = np.empty(max(cnt.value, 1), np.int64)
        L.check(f(self._model._h, C.byref(self._c), float(np.float32(d)), L.ptr(out), len(out), C.byref(cnt)))
        return out[: cnt.value]

    def IsIn(self, p, d):  # surface.go:237-240
        p = L.f32c(p).reshape(3)
        r = C.c_int32()
        L.check(L.lib().pcgx_sac_plane_is_in(self._model._h, C.byref(self._c), L.ptr(p), float(np.float32(d)), C.byref(r)))
        return bool(r.value)

    def Array(self):
        """the coefficients as 15 float32: origin, v1, v2, l1, l2, norm, d (pcgx_sac_plane)"""
        return np.frombuffer(bytes(self._c), np.float32).copy()


class VoxelGridSurfaceModel:
    """voxelGridSurfaceModel (surface.go:9-30).  vg: segmentation.StorageVoxelGrid; ra: PointCloud, (n,3) float32
    array, or a CUDA (ROCm) torch tensor of shape (n, >= 3) float32 (xyz in its first three columns).  The model
    copies both at creation: later changes to vg or ra do not reach it."""

    def __init__(self, vg, ra):
        self._h = None
        on_device = 0
        keep = None
        if isinstance(ra, PointCloud):
            keep, n, s, o = ra.Data, ra.Points, ra.Stride(), ra.xyz_offset()
            data = L.ptr(keep)
        elif getattr(ra, "is_cuda", False):
            if str(ra.dtype) != "torch.float32" or ra.dim() != 2 or ra.shape[1] < 3 or ra.stride(1) != 1:
                raise ValueError("a device cloud is a (n, >= 3) float32 tensor with unit column stride")
            n, s, o, on_device = ra.shape[0], ra.stride(0) * 4, 0, 1
            data = C.c_void_p(ra.data_ptr()) if n else None
        else:
            keep = L.f32c(ra).reshape(-1, 3)
            n, s, o = len(keep), 12, 0
            data = L.ptr(keep)
        h = C.c_void_p()
        L.check(L.lib().pcgx_sac_plane_model_create(vg._h, data if n else None, n, s, o, on_device, C.byref(h)))
        self._h = h
        self._n = n

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                L.lib().pcgx_sac_plane_model_free(self._h)
                self._h = None
        except Exception:
            pass

    def NumRange(self):  # surface.go:32-34
        return 3, 3

    def Len(self):
        return self._n

    def compute(self, ids, per_hypothesis=True):
        """Fit + Evaluate of len(ids)/3 hypotheses in one device call.
        -> (found, best index or -1, best score, best Coefficients or None, ok[n], Coefficients-or-None per
        hypothesis, score[n]); the per-hypothesis lists are None unless per_hypothesis."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if len(ids) % 3:
            raise ValueError("ids: three per hypothesis")
        n = len(ids) // 3
        found, best, best_score, bc = C.c_int32(), C.c_int64(), C.c_int64(), L.SacPlane()
        ok = np.zeros(max(n, 1), np.int32) if per_hypothesis else None
        coeff = (L.SacPlane * max(n, 1))() if per_hypothesis else None
        score = np.zeros(max(n, 1), np.int64) if per_hypothesis else None
        L.check(L.lib().pcgx_sac_plane_compute(self._h, L.ptr(ids) if n else None, n, C.byref(found), C.byref(best),
                                               C.byref(best_score), C.byref(bc), L.ptr(ok) if per_hypothesis else None,
                                               C.cast(coeff, C.c_void_p) if per_hypothesis else None,
                                               L.ptr(score) if per_hypothesis else None))
        best_c = Coefficients(self, bc, best_score.value) if found.value else None
        if not per_hypothesis:
            return bool(found.value), best.value, best_score.value, best_c, None, None, None
        cs = [Coefficients(self, coeff[h], score[h]) if ok[h] else None for h in range(n)]
        return bool(found.value), best.value, best_score.value, best_c, ok[:n].astype(bool), cs, score[:n]

    def Fit(self, ids):
        """surface.go:36-181 -> (Coefficients, True) or (None, False)."""
        if len(ids) != 3:
            return None, False
        _, _, _, _, ok, cs, _ = self.compute(ids)
        return cs[0], bool(ok[0])


def NewVoxelGridSurfaceModel(vg, ra):
    return VoxelGridSurfaceModel(vg, ra)


class SAC:
    """sac.go:23-63."""

    def __init__(self, sampler, model):
        self.Sampler = sampler
        self.Model = model
        self._best = None

    def Compute(self, n):
        """sac.go:33-59: True when a hypothesis scored above 0; the first one of the largest score becomes
        Coefficients().  False keeps the previous Coefficients()."""
        num, _ = self.Model.NumRange()
        ids = [self.Sampler.Sample() for _ in range(int(n) * num)]  # i-th hypothesis: draws 3i, 3i+1, 3i+2
        found, _, _, best, _, _, _ = self.Model.compute(np.array(ids, np.int64), per_hypothesis=False)
        if not found:
            return False
        self._best = best
        return True

    def Coefficients(self):
        return self._best


def New(sampler, model):
    return SAC(sampler, model)
