"""Matching of FPFH descriptors (extension: no reference counterpart; include/pcgx.h, "FPFH matching"): for every row
of one descriptor array the nearest and second nearest row of another, brute force on the GPU, and the correspondence
list feature-based coarse alignment starts from.  Descriptors are (n, 33) float32, what KDTree.FPFH returns first.
Below them, boundary points in PCL's wording (BoundaryEstimation over KDTree.Boundary; include/pcgx.h, "boundary
points")."""
import numpy as np

from . import _lib as L

LEN = 33


def MatchTile():
    """Queries per workgroup of the match kernel (the boundary the tests put rows across)."""
    return int(L.lib().pcgx_fpfh_match_tile())


def _rows(a, what):
    a = L.f32c(a)
    if a.ndim != 2 or a.shape[1] != LEN:
        raise ValueError("%s: an (n, 33) array of descriptors is required" % what)
    return a


def Match(A, B):
    """-> (ids (na,) int64, distSq (na,) float32, secondDistSq (na,) float32): for every row of A the usable row of B
    at the smallest float32 squared distance (ties: the smaller id) and the runner-up's distance; -1, inf, inf where
    there is none or the row of A is unusable (not finite, or all zero)."""
    a, b = _rows(A, "A"), _rows(B, "B")
    na = len(a)
    ids = np.empty(na, np.int64)
    d1 = np.empty(na, np.float32)
    d2 = np.empty(na, np.float32)
    L.check(L.lib().pcgx_fpfh_match(L.ptr(a), na, L.ptr(b), len(b), L.ptr(ids), L.ptr(d1), L.ptr(d2)))
    return ids, d1, d2


def Correspondences(A, B, MaxRatio=1.0, Mutual=True):
    """-> (m, 2) int64 pairs (row of A, row of B) in ascending row of A: the matches of A in B that pass Lowe's ratio
    test distSq <= float32(MaxRatio)^2 * secondDistSq and, with Mutual, whose row of B matches back to the same row
    of A."""
    a, b = _rows(A, "A"), _rows(B, "B")
    na = len(a)
    r = np.float32(MaxRatio)
    src = np.empty(na, np.int64)
    dst = np.empty(na, np.int64)
    n = np.zeros(1, np.int64)
    L.check(L.lib().pcgx_fpfh_correspondences(L.ptr(a), na, L.ptr(b), len(b), float(r * r), 1 if Mutual else 0,
                                              L.ptr(src), L.ptr(dst), L.ptr(n)))
    m = int(n[0])
    return np.stack([src[:m], dst[:m]], axis=1)


def MatchDev(d_a, na, d_b, nb, d_ids, d_dist_sq, d_second_dist_sq=0, stream=0):
    """Device-resident Match: raw device addresses (e.g. torch .data_ptr()); d_a float32 [33 na], d_b float32 [33 nb],
    d_ids int32 [na], d_dist_sq and d_second_dist_sq float32 [na].  Enqueued on `stream`, returns without waiting."""
    L.check(L.lib().pcgx_fpfh_match_dev(
        L.ptr(int(d_a)) if d_a else None, int(na), L.ptr(int(d_b)) if d_b else None, int(nb), L.ptr(int(d_ids)),
        L.ptr(int(d_dist_sq)), L.ptr(int(d_second_dist_sq)) if d_second_dist_sq else None,
        L.ptr(stream) if stream else None))


def CorrespondencesDev(d_a, na, d_b, nb, d_src_ids, d_dst_ids, d_n_pairs, MaxRatio=1.0, Mutual=True, stream=0):
    """Device-resident Correspondences: d_src_ids and d_dst_ids int32 [na] (-1 behind the pairs), d_n_pairs int32 [1].
    Enqueued on `stream`, returns without waiting."""
    r = np.float32(MaxRatio)
    L.check(L.lib().pcgx_fpfh_correspondences_dev(
        L.ptr(int(d_a)) if d_a else None, int(na), L.ptr(int(d_b)) if d_b else None, int(nb), float(r * r),
        1 if Mutual else 0, L.ptr(int(d_src_ids)), L.ptr(int(d_dst_ids)), L.ptr(int(d_n_pairs)),
        L.ptr(stream) if stream else None))


# ------------------------------------------------------------------------------------------------ boundary points
# (extension: no reference counterpart; include/pcgx.h, "boundary points")

BOUNDARY_SECTORS = 64


def boundary_min_gap(angle):
    """The MinGap (sectors of 2 pi / 64 = 5.625 degrees) of an angle in radians: ceil(angle / (2 pi / 64)), clamped to
    1..64.  The gap of a point is a count of empty sectors, not an angle: a true angular opening g between neighbouring
    directions gives g / w - 2 < gap < g / w with w one sector.  So a point flagged at MinGap has an opening wider than
    MinGap w, and every opening of at least (MinGap + 2) w is flagged; in between it depends on where the sector borders
    fall.  boundary_min_gap(pi / 2) = 16: nothing below 90 degrees is flagged and everything from 101.25 degrees is."""
    sectors = int(np.ceil(float(angle) / (2.0 * np.pi / BOUNDARY_SECTORS)))
    return min(max(sectors, 1), BOUNDARY_SECTORS)


class BoundaryEstimation:
    """KDTree.Boundary in PCL's wording (pcl::BoundaryEstimation): the points of `tree` whose neighbours within the
    search radius leave an angular gap wider than the threshold in the tangent plane of the input normals."""

    def __init__(self, tree):
        self._tree = tree
        self._radius = None
        self._normals = None
        self._min_gap = boundary_min_gap(np.pi / 2.0)  # PCL's default angle threshold
        self._min_neighbors = 1

    def SetRadiusSearch(self, radius):
        self._radius = float(radius)

    def SetInputNormals(self, normals):
        self._normals = L.f32c(normals).reshape(-1, 3)

    def SetAngleThreshold(self, angle):
        """radians; applied in whole sectors (boundary_min_gap)"""
        self._min_gap = boundary_min_gap(angle)

    def SetMinNeighbors(self, min_neighbors):
        self._min_neighbors = int(min_neighbors)

    def Compute(self):
        """-> (ids int64 ascending, gaps int32 (n,), masks uint64 (n,), counts int32 (n,)), as KDTree.Boundary"""
        if self._radius is None or self._normals is None:
            raise ValueError("SetRadiusSearch and SetInputNormals come first")
        return self._tree.Boundary(self._radius, self._normals, self._min_gap, self._min_neighbors)

    def Loops(self, group_radius, MinSize=1):
        """The connected outlines among the boundary points: the outer rim and every hole as one group each ->
        (labels int64 (n,), sizes int64 (C,), ids int64 (sum(sizes),)) in the tree's ids, the largest group first:
        labels is -1 off the boundary and for a group below MinSize, ids holds group 0's members ascending, then group
        1's, ...  A host-level convenience, not a kernel: it reads the boundary ids and their number back, builds a
        second KDTree over those points and takes its Clusters(group_radius).  The points of a loop are not ordered
        along the outline."""
        from . import kdtree
        ids = self.Compute()[0]
        n = self._tree.Len()
        labels = np.full(n, -1, np.int64)
        if len(ids) == 0:
            return labels, np.zeros(0, np.int64), np.zeros(0, np.int64)
        pts = np.empty((len(ids), 3), np.float32)
        L.check(L.lib().pcgx_kdtree_points(self._tree._h, L.ptr(ids), len(ids), L.ptr(pts)))
        sub_labels, sizes, sub_ids = kdtree.New(pts).Clusters(float(group_radius), MinSize=MinSize)
        kept = sub_labels >= 0
        labels[ids[kept]] = sub_labels[kept]
        return labels, sizes, ids[sub_ids]  # (ids ascends, so a group's members stay ascending)


# ------------------------------------------------------------------------------------------ consistent orientation
# (extension: no reference counterpart; include/pcgx.h, "consistent normal orientation")

def WithDirection(u):
    """NormalOrientation option: every component's topmost point along u looks along u (Hoppe's rule)"""
    return ("direction", tuple(float(v) for v in np.asarray(u, np.float32).reshape(3)))


def WithViewpoint(v):
    """NormalOrientation option: the majority of every component's normals looks towards v"""
    return ("viewpoint", tuple(float(w) for w in np.asarray(v, np.float32).reshape(3)))


class NormalOrientation:
    """KDTree.OrientNormals as an estimator beside BoundaryEstimation: neighbouring normals get the same side, the sign
    carried along the minimum spanning forest of the radius graph (Hoppe et al. 1992; Open3D's
    orient_normals_consistent_tangent_plane).  Without an option the smallest id of a component keeps its sign."""

    def __init__(self, radius, *options):
        self._radius = float(radius)
        self._direction = self._viewpoint = None
        for kind, value in options:
            if kind == "direction":
                self._direction = value
            elif kind == "viewpoint":
                self._viewpoint = value
            else:
                raise ValueError("unknown option %r" % (kind,))
        if self._direction is not None and self._viewpoint is not None:
            raise ValueError("WithDirection or WithViewpoint, not both")
        self.flipped = self.component = self.n_components = None

    def Compute(self, tree, normals):
        """-> the oriented normals float32 (n,3); .flipped uint8 (n,), .component int64 (n,) and .n_components keep the
        rest of what KDTree.OrientNormals returned"""
        out, self.flipped, self.n_components, self.component = tree.OrientNormals(
            self._radius, normals, Direction=self._direction, Viewpoint=self._viewpoint, Component=True)
        return out
