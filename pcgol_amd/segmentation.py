"""Mirrors of pc/storage/voxelgrid (bucket grid), pc/segmentation/voxelgrid (flood fill) and
pc/segmentation/regiongrowing on the GPU (include/pcgx.h "bucket voxel grid + segmentation").

The reference fills a VoxelGrid with Add(p, index) calls one by one; the batch seam here is the
whole cloud: StorageVoxelGrid(resolution, size, origin).AddAll(cloud) == Add(point i, i) for all i.
Result order of the Segment calls: see include/pcgx.h (set-equal to the reference's BFS order)."""
import ctypes as C

import numpy as np

from . import _lib as L
from .pc import PointCloud


class StorageVoxelGrid:
    """pc/storage/voxelgrid.VoxelGrid (voxelgrid.go:7-122)."""

    def __init__(self, resolution, size, origin):
        self.resolution = float(resolution)
        self.size = np.ascontiguousarray(size, dtype=np.int64)
        self.origin = L.f32c(origin)
        self._h = None
        self._n = 0
        self.AddAll(np.zeros((0, 3), np.float32))

    def Resolution(self):
        return np.float32(self.resolution)

    def MinMax(self):  # voxelgrid.go:25-31
        ext = self.size.astype(np.float32) * np.float32(self.resolution)
        return self.origin.copy(), self.origin + ext

    def AddAll(self, cloud):
        """Reset() + Add(point i, i) for every point (PointCloud or (n,3) float32)."""
        if isinstance(cloud, PointCloud):
            data, n, s, o = cloud.Data, cloud.Points, cloud.Stride(), cloud.xyz_offset()
        else:
            data = L.f32c(cloud).reshape(-1, 3)
            n, s, o = len(data), 12, 0
        self._free()
        h = C.c_void_p()
        L.check(L.lib().pcgx_bucket_grid_build(L.ptr(data) if n else None, n, s, o, self.resolution, L.ptr(self.size),
                                               L.ptr(self.origin), C.byref(h)))
        self._h, self._n = h, n
        return self.AddedMask()

    def _free(self):
        if getattr(self, "_h", None):
            L.lib().pcgx_bucket_grid_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    def _counts(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib().pcgx_bucket_grid_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def Len(self):  # voxelgrid.go:110-112
        return self._counts()[0]

    def PointAddrs(self):
        out = np.empty(self._n, np.int64)
        L.check(L.lib().pcgx_bucket_grid_point_addrs(self._h, L.ptr(out) if self._n else None))
        return out

    def AddedMask(self):
        """What Add returned for every point (voxelgrid.go:37-45)."""
        return self.PointAddrs() >= 0

    def Addr(self, p):  # voxelgrid.go:64-79
        p = L.f32c(p)
        a, ok = C.c_int64(), C.c_int32()
        L.check(L.lib().pcgx_bucket_grid_addr(self._h, L.ptr(p), C.byref(a), C.byref(ok)))
        return a.value, bool(ok.value)

    def GetByAddr(self, a):
        cnt = C.c_int64()
        L.check(L.lib().pcgx_bucket_grid_get_by_addr(self._h, int(a), None, 0, C.byref(cnt)))
        out = np.empty(max(cnt.value, 1), np.int64)
        L.check(L.lib().pcgx_bucket_grid_get_by_addr(self._h, int(a), L.ptr(out), len(out), C.byref(cnt)))
        return out[: cnt.value]

    def Get(self, p):
        """ids of p's voxel; None (nil) when p is outside the grid (voxelgrid.go:52-58)."""
        a, ok = self.Addr(p)
        return self.GetByAddr(a) if ok else None

    def Indice(self):  # voxelgrid.go:114-120
        out = np.empty(max(self._counts()[1], 1), np.int64)
        L.check(L.lib().pcgx_bucket_grid_indice(self._h, L.ptr(out)))
        return out[: self._counts()[1]]


class SegmentationVoxelGrid(StorageVoxelGrid):
    """pc/segmentation/voxelgrid.VoxelGrid (embeds the storage grid, voxelgrid.go:27-37)."""

    def Storage(self):
        return self

    def Components(self):
        """Segment() for every seed at once: per point the smallest voxel address of its
        26-connected set of occupied voxels (-1 outside the grid)."""
        out = np.empty(self._n, np.int64)
        L.check(L.lib().pcgx_bucket_grid_components(self._h, L.ptr(out) if self._n else None))
        return out

    def Segment(self, p, order="bfs"):
        """segmentation/voxelgrid/voxelgrid.go:39-73.  order="bfs": ids exactly as the reference
        appends them (its FIFO flood fill, run over the device-built buckets); order="address":
        the same set from the device's component labels, ascending voxel address (fast path)."""
        fn = L.lib().pcgx_bucket_grid_segment_bfs if order == "bfs" else L.lib().pcgx_bucket_grid_segment
        p = L.f32c(p)
        cnt = C.c_int64()
        L.check(fn(self._h, L.ptr(p), None, 0, C.byref(cnt)))
        out = np.empty(max(cnt.value, 1), np.int64)
        L.check(fn(self._h, L.ptr(p), L.ptr(out), len(out), C.byref(cnt)))
        return out[: cnt.value]


class RegionGrowing:
    """pc/segmentation/regiongrowing.RegionGrowing (regiongrowing.go:13-56): New(search, propertyIter).
    search: a pcgol_amd KDTree; propertyIter: uint32 value per point (Uint32At)."""

    def __init__(self, search, propertyIter):
        self.search = search
        self.labels = np.ascontiguousarray(propertyIter, dtype=np.uint32)
        if len(self.labels) != search.Len():
            raise ValueError("propertyIter must hold one value per point of search")
        self._comp = {}

    New = classmethod(lambda cls, search, propertyIter: cls(search, propertyIter))

    def Components(self, maxRange):
        """Segment() for every seed at once (cached per maxRange): per point the smallest id of its
        region."""
        key = float(np.float32(maxRange))
        if key not in self._comp:
            out = np.empty(len(self.labels), np.int64)
            L.check(L.lib().pcgx_region_growing_components(self.search._h, L.ptr(self.labels), key, L.ptr(out)))
            self._comp[key] = out
        return self._comp[key]

    def Segment(self, p, maxRange, order="bfs"):
        """regiongrowing.go:23-56.  order="bfs": ids exactly as the reference appends them (its FIFO
        search, one device Range batch per BFS level); order="id": the same set from the device's
        region labels (Components), ascending id (fast path for many seeds)."""
        p = L.f32c(p)
        out = np.empty(max(len(self.labels), 1), np.int64)
        cnt = C.c_int64()
        if order == "bfs":
            L.check(L.lib().pcgx_region_growing_segment_bfs(self.search._h, L.ptr(self.labels), L.ptr(p),
                                                            float(np.float32(maxRange)), L.ptr(out), len(out),
                                                            C.byref(cnt)))
            return out[: cnt.value].copy()
        comp = self.Components(maxRange)
        L.check(L.lib().pcgx_region_growing_segment(self.search._h, L.ptr(self.labels), L.ptr(comp), L.ptr(p),
                                                    float(np.float32(maxRange)), L.ptr(out), len(out), C.byref(cnt)))
        return out[: cnt.value].copy()


class _Grouped:
    """What ClusterExtraction and DBSCAN share: Extract() splits one grouped id list, Boxes() and Footprints() pass it on.
    A subclass says in _run() which call makes the list -> (labels, sizes, ids)."""
    search = labels = sizes = ids = None

    New = classmethod(lambda cls, search, *a, **k: cls(search, *a, **k))

    def SetMinClusterSize(self, n):
        self.min_size = int(n)

    def SetMaxClusterSize(self, n):
        """0: no upper limit"""
        self.max_size = int(n)

    def Extract(self):
        """-> [ids of cluster 0, ids of cluster 1, ...]; .labels and .sizes hold the call's other two results"""
        self.labels, self.sizes, self.ids = self._run()
        return np.split(self.ids, np.cumsum(self.sizes)[:-1]) if len(self.sizes) else []

    def Boxes(self):
        """After Extract(): the geometry of the extracted clusters, one row each -> KDTree.GroupStats' tuple (count,
        aabb, centroid, cov, eig, axes, obb): a centre, a box to track, a plane to test."""
        if self.sizes is None:
            raise RuntimeError("Boxes() needs Extract() first")
        return self.search.GroupStats(self.ids, self.sizes)

    def Footprints(self):
        """After Extract(): what the extracted clusters stand on, one row each -> KDTree.GroupHulls' tuple (hull_sizes,
        hull_ids, area, rect): the exact convex hull of a cluster's (x, y) and the smallest upright rectangle with a side
        along one of its edges."""
        if self.sizes is None:
            raise RuntimeError("Footprints() needs Extract() first")
        return self.search.GroupHulls(self.ids, self.sizes)


class ClusterExtraction(_Grouped):
    """Cluster extraction in PCL's vocabulary (EuclideanClusterExtraction; with normals, its smooth variant), over
    KDTree.Clusters (extension: no reference parity; include/pcgx.h, "clusters").  search: a pcgol_amd KDTree.

        ce = ClusterExtraction(tree, ClusterTolerance=0.05, MinClusterSize=100)
        for ids in ce.Extract(): ...

    The clusters come largest first, equal sizes by smallest id, each as ascending int64 ids."""

    def __init__(self, search, ClusterTolerance=0.0, MinClusterSize=1, MaxClusterSize=0):
        self.search = search
        self.tolerance = float(ClusterTolerance)
        self.min_size, self.max_size = int(MinClusterSize), int(MaxClusterSize)
        self.normals = self.curvature = None
        self.min_cos, self.oriented, self.max_curvature = 0.0, False, 0.0
        self.labels = self.sizes = self.ids = None

    def SetClusterTolerance(self, tolerance):
        self.tolerance = float(tolerance)

    def SetInputNormals(self, Normals, MinCos=0.0, Oriented=False):
        """an edge also needs |n_i . n_j| >= MinCos (n_i . n_j when Oriented); None: Euclidean clustering again"""
        self.normals, self.min_cos, self.oriented = Normals, float(MinCos), bool(Oriented)

    def SetSmoothnessThreshold(self, angle):
        """PCL's form of MinCos: the largest angle (radians) between the normals of two joined points"""
        self.min_cos = float(np.cos(angle))

    def SetInputCurvature(self, Curvature, MaxCurvature=0.0):
        """a point whose curvature is above MaxCurvature (or NaN) belongs to no cluster; None: no such test"""
        self.curvature, self.max_curvature = Curvature, float(MaxCurvature)

    def _run(self):
        return self.search.Clusters(
            self.tolerance, Normals=self.normals, MinCos=self.min_cos, Oriented=self.oriented, Curvature=self.curvature,
            MaxCurvature=self.max_curvature, MinSize=self.min_size, MaxSize=self.max_size)


class DBSCAN(_Grouped):
    """Density clustering in Open3D's and scikit-learn's vocabulary, over KDTree.DBSCAN (extension: no reference parity;
    include/pcgx.h, "density clusters").  search: a pcgol_amd KDTree.

        db = DBSCAN(tree, Eps=0.05, MinPoints=10)
        for ids in db.Extract(): ...

    A point with at least MinPoints points within Eps (itself included) is core; a cluster is a component of core points
    plus the border points beside it, each with its nearest core neighbour.  The clusters come largest first, equal sizes
    by smallest id, each as ascending int64 ids; .kind says per point 0 noise, 1 border, 2 core."""

    def __init__(self, search, Eps=0.0, MinPoints=1, MinClusterSize=1, MaxClusterSize=0):
        self.search = search
        self.eps, self.min_points = float(Eps), int(MinPoints)
        self.min_size, self.max_size = int(MinClusterSize), int(MaxClusterSize)
        self.labels = self.sizes = self.ids = self.kind = None

    def SetEps(self, eps):
        self.eps = float(eps)

    def SetMinPoints(self, n):
        self.min_points = int(n)

    def _run(self):
        labels, sizes, ids, self.kind = self.search.DBSCAN(self.eps, self.min_points, MinSize=self.min_size,
                                                           MaxSize=self.max_size)
        return labels, sizes, ids


class PlaneSegmentation(_Grouped):
    """Plane segmentation in PCL's vocabulary (SACSegmentation with SACMODEL_PLANE / PERPENDICULAR_PLANE / NORMAL_PLANE,
    run in a loop with ExtractIndices), over KDTree.Planes (extension: no reference parity; include/pcgx.h, "planes").
    search: a pcgol_amd KDTree.

        ps = PlaneSegmentation(tree, DistanceThreshold=0.02, MaxPlanes=4, MinInliers=500)
        ps.SetAxis((0, 0, 1)); ps.SetEpsAngle(np.radians(10))      # the floor first: only planes within 10 degrees of it
        for ids in ps.Extract(): ...                               # ps.planes[k] = (nx, ny, nz, d) of plane k

    The planes come in the order they were found (the one with most inliers among what is left), each as ascending int64
    ids; Boxes() and Footprints() give their geometry.  .result holds everything KDTree.Planes returned."""

    def __init__(self, search, DistanceThreshold=0.0, MaxPlanes=1, MinInliers=3, MaxIterations=256, Refine=True, Seed=0):
        self.search = search
        self.max_dist, self.max_planes, self.min_inliers = float(DistanceThreshold), int(MaxPlanes), int(MinInliers)
        self.n_hyp, self.refine, self.seed = int(MaxIterations), bool(Refine), Seed
        self.axis, self.min_axis_cos = None, 0.0
        self.normals, self.min_normal_cos = None, 0.0
        self.labels = self.sizes = self.ids = self.planes = self.result = None

    def SetDistanceThreshold(self, d):
        self.max_dist = float(d)

    def SetMaxIterations(self, n):
        """hypotheses a round draws (all of them are scored: there is no early stop)"""
        self.n_hyp = int(n)

    def SetMaxPlanes(self, n):
        self.max_planes = int(n)

    def SetMinInliers(self, n):
        self.min_inliers = int(n)

    def SetAxis(self, axis):
        """only planes whose normal lies within the angle of SetEpsAngle of this axis (PCL's perpendicular plane: the
        plane is perpendicular to the axis); None: any plane"""
        self.axis = None if axis is None else np.asarray(axis, np.float32).reshape(3)

    def SetEpsAngle(self, angle):
        """the largest angle (radians) between a plane's normal and the axis, either way round"""
        self.min_axis_cos = float(np.cos(angle))

    def SetInputNormals(self, Normals, MinCos=0.0):
        """an inlier's normal also needs |n . m| >= MinCos with the plane's, and a point with a zero or non-finite
        normal takes no part; None: distances alone"""
        self.normals, self.min_normal_cos = Normals, float(MinCos)

    def _run(self):
        r = self.result = self.search.Planes(
            self.max_dist, NHyp=self.n_hyp, MaxPlanes=self.max_planes, MinInliers=self.min_inliers, Axis=self.axis,
            MinAxisCos=self.min_axis_cos, Normals=self.normals, MinNormalCos=self.min_normal_cos, Refine=self.refine,
            Seed=self.seed)
        self.planes = r.planes[:r.n_planes]
        return r.labels, r.sizes[:r.n_planes], r.ids


class ShapeSegmentation(_Grouped):
    """Cylinder and sphere segmentation in PCL's vocabulary (SACSegmentationFromNormals with SACMODEL_CYLINDER /
    SACMODEL_SPHERE, run in a loop with ExtractIndices), over KDTree.Shapes (extension: no reference parity;
    include/pcgx.h, "shapes").  search: a pcgol_amd KDTree; Normals: one per point, e.g. what KDTree.Normals returns.

        ss = ShapeSegmentation(tree, normals, Model="cylinder", DistanceThreshold=0.02, MaxShapes=4, MinInliers=500)
        ss.SetRadiusLimits(0.03, 0.3); ss.SetSampleRadius(0.3)
        ss.SetAxis((0, 0, 1)); ss.SetEpsAngle(np.radians(15))     # upright poles only
        for ids in ss.Extract(): ...                              # ss.shapes[k] = (qx, qy, qz, r, ax, ay, az, 0)

    The shapes come in the order they were found, each as ascending int64 ids; Boxes() and Footprints() give their
    geometry.  .result holds everything KDTree.Shapes returned."""

    MODELS = {"sphere": 0, "cylinder": 1}

    def __init__(self, search, Normals, Model="cylinder", DistanceThreshold=0.0, MaxShapes=1, MinInliers=2,
                 MaxIterations=256, SampleRadius=0.0, RadiusLimits=(0.0, float("inf")), NormalMinCos=0.0, Refine=True,
                 Seed=0):
        self.search, self.normals = search, Normals
        self.kind = self.MODELS[Model] if isinstance(Model, str) else int(Model)
        self.max_dist, self.max_shapes, self.min_inliers = float(DistanceThreshold), int(MaxShapes), int(MinInliers)
        self.n_hyp, self.refine, self.seed = int(MaxIterations), bool(Refine), Seed
        self.sample_radius = float(SampleRadius)
        self.r_min, self.r_max = float(RadiusLimits[0]), float(RadiusLimits[1])
        self.axis, self.min_axis_cos, self.min_normal_cos = None, 0.0, float(NormalMinCos)
        self.labels = self.sizes = self.ids = self.shapes = self.result = None

    def SetDistanceThreshold(self, d):
        self.max_dist = float(d)

    def SetMaxIterations(self, n):
        """hypotheses a round draws (all of them are scored: there is no early stop)"""
        self.n_hyp = int(n)

    def SetMaxShapes(self, n):
        self.max_shapes = int(n)

    def SetMinInliers(self, n):
        self.min_inliers = int(n)

    def SetSampleRadius(self, r):
        """the second point of a hypothesis comes out of this radius about the first; 0: out of everything left"""
        self.sample_radius = float(r)

    def SetRadiusLimits(self, r_min, r_max):
        self.r_min, self.r_max = float(r_min), float(r_max)

    def SetAxis(self, axis):
        """only cylinders whose axis lies within the angle of SetEpsAngle of this one; None: any"""
        self.axis = None if axis is None else np.asarray(axis, np.float32).reshape(3)

    def SetEpsAngle(self, angle):
        self.min_axis_cos = float(np.cos(angle))

    def SetInputNormals(self, Normals, MinCos=None):
        """an inlier's normal also needs |cos| >= MinCos with the shape's at that point (0: distances alone)"""
        self.normals = Normals
        if MinCos is not None:
            self.min_normal_cos = float(MinCos)

    def _run(self):
        r = self.result = self.search.Shapes(
            self.kind, self.max_dist, self.normals, NHyp=self.n_hyp, MaxShapes=self.max_shapes,
            MinInliers=self.min_inliers, SampleRadius=self.sample_radius, RMin=self.r_min, RMax=self.r_max, Axis=self.axis,
            MinAxisCos=self.min_axis_cos, MinNormalCos=self.min_normal_cos, Refine=self.refine, Seed=self.seed)
        self.shapes = r.shapes[:r.n_shapes]
        return r.labels, r.sizes[:r.n_shapes], r.ids


def pmf_windows(CellSize, MaxWindowSize, Slope=1.0, InitialDistance=0.5, MaxDistance=3.0, Base=2, Exponential=True):
    """The window schedule of the progressive morphological filter (Zhang et al. 2003, PCL's parameters) ->
    (half int32 (k,), height float32 (k,)), what KDTree.Ground takes.  Widths in cells: w_i = 2 Base^i + 1
    (Exponential) or 2 (i + 1) Base + 1, for every i = 0, 1, ... with w_i CellSize <= MaxWindowSize; half_i =
    (w_i - 1) / 2; height_0 = InitialDistance, height_i = min(Slope (w_i - w_{i-1}) CellSize + InitialDistance,
    MaxDistance), computed in float64 and rounded once to float32.  A pure function: nothing here touches the GPU."""
    cell, max_w, base = float(CellSize), float(MaxWindowSize), int(Base)
    if not cell > 0.0 or base < 1 or (Exponential and base < 2):
        raise ValueError("CellSize must be > 0 and Base at least 1 (2 for an exponential schedule)")
    half, height, prev = [], [], None
    i = 0
    while True:
        w = 2 * base ** i + 1 if Exponential else 2 * (i + 1) * base + 1
        if not w * cell <= max_w:
            break
        half.append((w - 1) // 2)
        height.append(float(InitialDistance) if prev is None else
                      min(float(Slope) * (w - prev) * cell + float(InitialDistance), float(MaxDistance)))
        prev = w
        i += 1
    return np.asarray(half, np.int32), np.asarray(height, np.float64).astype(np.float32)


class GroundSegmentation(_Grouped):
    """Ground segmentation in PCL's vocabulary (ApproximateProgressiveMorphologicalFilter), over KDTree.Ground
    (extension: no reference parity; include/pcgx.h, "ground").  search: a pcgol_amd KDTree; the up axis is z.

        gs = GroundSegmentation(tree, CellSize=0.5, MaxWindowSize=16.5, Slope=0.3, InitialDistance=0.15, MaxDistance=2.5)
        ground, other = gs.Extract()                               # gs.hag: every point's height above the terrain
        keep = np.flatnonzero((gs.hag > 0.3) & (gs.hag < 2.5))     # "between 0.3 and 2.5 m above ground"

    Extract() returns [ground ids, other ids], each ascending int64; .surface is the terrain model (ny, nx), +inf where
    a cell holds no point, .hag the height above it per point (NaN where a point takes no part), .window the first
    window a point failed (-1: ground).  Boxes() and Footprints() give the geometry of the two groups.  .result holds
    everything KDTree.Ground returned.  Origin and Dims: the grid; left out, the box of the live points."""

    def __init__(self, search, CellSize=1.0, MaxWindowSize=33.0, Slope=1.0, InitialDistance=0.5, MaxDistance=3.0, Base=2,
                 Exponential=True, Origin=None, Dims=None):
        self.search = search
        self.cell, self.max_window = float(CellSize), float(MaxWindowSize)
        self.slope, self.initial, self.max_dist = float(Slope), float(InitialDistance), float(MaxDistance)
        self.base, self.exponential = int(Base), bool(Exponential)
        self.origin, self.dims = Origin, Dims
        self.labels = self.sizes = self.ids = self.surface = self.hag = self.window = self.result = None

    def SetCellSize(self, c):
        self.cell = float(c)

    def SetMaxWindowSize(self, w):
        self.max_window = float(w)

    def SetSlope(self, s):
        self.slope = float(s)

    def SetInitialDistance(self, d):
        self.initial = float(d)

    def SetMaxDistance(self, d):
        self.max_dist = float(d)

    def SetBase(self, b):
        self.base = int(b)

    def SetExponential(self, e):
        self.exponential = bool(e)

    def SetGrid(self, Origin, Dims):
        """the grid's corner (x, y) and its size (nx, ny) in cells; None, None: the box of the live points"""
        self.origin, self.dims = Origin, Dims

    def _run(self):
        half, height = pmf_windows(self.cell, self.max_window, self.slope, self.initial, self.max_dist, self.base,
                                   self.exponential)
        r = self.result = self.search.Ground(self.cell, half, height, Origin=self.origin, Dims=self.dims)
        self.surface, self.hag, self.window = r.surface, r.hag, r.window
        return r.labels, r.sizes, r.ids
