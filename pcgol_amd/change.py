"""Change detection between two registered epochs: M3C2 (Lague, Brodu and Leroux 2013; extension: no reference
counterpart), in the option style of pc/filter/voxelgrid:

    distance, lod, significant, n1, n2 = change.M3C2(0.1, 0.5, WithRegistrationError(0.01)).Compute(tree1, tree2, cores, normals)

For each core point with a normal, the points of each epoch inside a cylinder of `radius` along the normal,
`half_length` each way, are averaged along the normal (KDTree.CylinderStats); `distance` is the signed difference of
the two means, epoch 2 minus epoch 1, in metric units along the normal; `lod` is the level of detection at 95 % from
the two spreads and counts plus the registration error, and `significant` is |distance| > lod.  A core with fewer than
MinCount points in either cylinder, or an unusable normal, gets NaN, NaN, False.  The arithmetic is the library's
(include/pcgx.h, "cylinder statistics" and "M3C2"); normals come from KDTree.Normals / MLS / OrientNormals, cores from
MinDistance or FarthestPoint.  Left out: median / IQR statistics, multi-scale normals, precision maps, a radius per
core."""
import numpy as np

from . import _lib as L


def WithRegistrationError(e):
    def opt(o):
        o.RegistrationError = float(e)
    return opt


def WithMinCount(k):
    def opt(o):
        o.MinCount = int(k)
    return opt


def finish(axes, counts1, sums1, counts2, sums2, registration_error=0.0, min_count=4):
    """pcgx_m3c2_finish on host arrays -> (distance float64 (m,), lod float64 (m,), significant bool (m,))."""
    d = L.f32c(axes).reshape(-1, 3)
    m = len(d)
    n1, n2 = (np.ascontiguousarray(c, np.int32).reshape(-1) for c in (counts1, counts2))
    s1, s2 = (np.ascontiguousarray(s, np.float64).reshape(-1) for s in (sums1, sums2))
    if not (len(n1) == len(n2) == m and len(s1) == len(s2) == 2 * m):
        raise ValueError("one count and two sums per axis and epoch are required")
    distance, lod, sig = np.empty(m, np.float64), np.empty(m, np.float64), np.zeros(m, np.uint8)
    L.check(L.lib().pcgx_m3c2_finish(L.ptr(d), L.ptr(n1), L.ptr(s1), L.ptr(n2), L.ptr(s2), m, float(registration_error),
                                     int(min_count), L.ptr(distance), L.ptr(lod), L.ptr(sig)))
    return distance, lod, sig.astype(bool)


class M3C2:
    def __init__(self, radius, half_length, *opts):
        self.Radius = float(radius)
        self.HalfLength = float(half_length)
        self.RegistrationError = 0.0
        self.MinCount = 4  # (CloudCompare's default: below it a spread says little)
        for o in opts:
            o(self)

    def Compute(self, tree1, tree2, cores, normals):
        """-> (distance float64 (m,), lod float64 (m,), significant bool (m,), n1 int32 (m,), n2 int32 (m,))."""
        n1, s1 = tree1.CylinderStats(cores, normals, self.Radius, self.HalfLength)
        n2, s2 = tree2.CylinderStats(cores, normals, self.Radius, self.HalfLength)
        distance, lod, sig = finish(normals, n1, s1, n2, s2, self.RegistrationError, self.MinCount)
        return distance, lod, sig, n1, n2

    def ComputeDev(self, tree1, tree2, d_cores, d_normals, m, d_distance, d_lod, d_significant, d_counts1, d_sums1,
                   d_counts2, d_sums2, stream=0):
        """Device-resident Compute: raw device addresses (e.g. torch .data_ptr()); d_cores, d_normals float32 [3 m],
        d_distance, d_lod float64 [m], d_significant uint8 [m], and the caller's room for the statistics: d_counts1,
        d_counts2 int32 [m], d_sums1, d_sums2 float64 [2 m].  Two statistics calls and the finish are enqueued on
        `stream`; returns without waiting, reads nothing back."""
        tree1.CylinderStatsDev(d_cores, d_normals, m, self.Radius, self.HalfLength, d_counts1, d_sums1, stream)
        tree2.CylinderStatsDev(d_cores, d_normals, m, self.Radius, self.HalfLength, d_counts2, d_sums2, stream)
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_m3c2_finish_dev(
            opt(d_normals), opt(d_counts1), opt(d_sums1), opt(d_counts2), opt(d_sums2), int(m),
            self.RegistrationError, self.MinCount, opt(d_distance), opt(d_lod), opt(d_significant),
            L.ptr(stream) if stream else None))


def New(radius, half_length, *opts):
    return M3C2(radius, half_length, *opts)
