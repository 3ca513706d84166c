"""pc/storage/kdtree mirror: KDTree on the GPU behind the storage.Search shape
(pc/storage/search.go:13-17): Vec3At / Len / Nearest, plus batched NearestBatch, and extensions with no
reference counterpart: surface normals (Normals), moving-least-squares smoothing (MLS), FPFH descriptors
(FPFH, FPFHAt), keypoints (LocalMaxima, ISSKeypoints), cluster extraction (Clusters), density clusters (DBSCAN), plane segmentation (Planes), cylinder and sphere segmentation (Shapes), ground segmentation (Ground), boundary points (Boundary), ray queries (RayCast, RayPierce), cylinder statistics (CylinderStats), per-group
geometry (GroupStats), k nearest neighbours (KNearest) and their covariances (Covariances)."""
import collections
import ctypes as C

import numpy as np

from . import _lib as L
from .pc import PointCloud


class Neighbor:  # pc/storage/search.go:8-11
    __slots__ = ("ID", "DistSq")

    def __init__(self, ID, DistSq):
        self.ID = int(ID)
        self.DistSq = np.float32(DistSq)

    def __repr__(self):
        return "Neighbor{ID:%d, DistSq:%r}" % (self.ID, float(self.DistSq))


GroupGeometry = collections.namedtuple("GroupGeometry", "count aabb centroid cov eig axes obb")  # KDTree.GroupStats
GroupFootprints = collections.namedtuple("GroupFootprints", "hull_sizes hull_ids area rect")  # KDTree.GroupHulls


PlaneSegments = collections.namedtuple("PlaneSegments",  # KDTree.Planes
                                       "n_planes planes sizes refined best labels ids status counts hyp_planes")


ShapeSegments = collections.namedtuple("ShapeSegments",  # KDTree.Shapes
                                       "n_shapes shapes sizes refined best labels ids status counts hyp_shapes")
SHAPE_SPHERE, SHAPE_CYLINDER = 0, 1


GroundSegments = collections.namedtuple("GroundSegments",  # KDTree.Ground
                                        "labels sizes ids n_groups window surface hag origin dims")


def GroundTile():
    """Cells of a grid row one pass of Ground's morphology workgroup handles (the boundary the tests put nx, ny across)."""
    return int(L.lib().pcgx_ground_tile())


def GroundLoopMax():
    """The largest half-width Ground's morphology kernel takes with its plain loop (above it: doubling in LDS)."""
    return int(L.lib().pcgx_ground_loop_max())


def ShapesTile():
    """Hypotheses per workgroup of Shapes' count kernel (the boundary the tests put NHyp across)."""
    return int(L.lib().pcgx_shapes_tile())


def PlanesTile():
    """Hypotheses per workgroup of Planes' count kernel (the boundary the tests put NHyp across)."""
    return int(L.lib().pcgx_planes_tile())


def GroupHullsChunk():
    """Survivors a lane of GroupHulls' reduce rounds takes at a time (the boundary the tests put hulls across)."""
    return int(L.lib().pcgx_group_hulls_chunk())


def GroupStatsTile():
    """Slots per tile of GroupStats' slot -> group map (the gathers cut a group's runs every 64 slots and take four
    tiles to a workgroup): the boundaries the tests put groups across."""
    return int(L.lib().pcgx_group_stats_tile())


class KDTree:
    """kdtree.New(ra, opts...) (kdtree.go:33-56).  `ra`: PointCloud or (n,3) float32 array.
    MinDistSq > 0 makes Nearest the reference's approximate search (kdtree.go:20-22)."""

    def __init__(self, ra, MinDistSq=0.0, _share=None):
        self.MinDistSq = float(MinDistSq)
        if _share is not None:
            self._h, self._owner = _share._h, _share
            return
        if isinstance(ra, PointCloud):
            data, n, s, o = ra.Data, ra.Points, ra.Stride(), ra.xyz_offset()
        else:
            data = L.f32c(ra).reshape(-1, 3)
            n, s, o = len(data), 12, 0
        h = C.c_void_p()
        L.check(L.lib().pcgx_kdtree_build(L.ptr(data), n, s, o, C.byref(h)))
        self._h, self._owner = h, None

    New = classmethod(lambda cls, ra, **opts: cls(ra, **opts))

    def With(self, MinDistSq):  # kdtree.go:59-65: shallow copy with options
        return KDTree(None, MinDistSq=MinDistSq, _share=self if self._owner is None else self._owner)

    def __del__(self):
        if getattr(self, "_owner", 1) is None and getattr(self, "_h", None):
            try:
                L.lib().pcgx_kdtree_free(self._h)
            except Exception:
                pass
            self._h = None

    # -- pc.Vec3RandomAccessor
    def Len(self):
        n = C.c_int64()
        L.check(L.lib().pcgx_kdtree_len(self._h, C.byref(n)))
        return n.value

    def Vec3At(self, i):
        ids = np.array([i], np.int64)
        out = np.empty(3, np.float32)
        L.check(L.lib().pcgx_kdtree_points(self._h, L.ptr(ids), 1, L.ptr(out)))
        return out

    def RawIndexAt(self, i):
        return i

    def MaxDepth(self):
        d = C.c_int32()
        L.check(L.lib().pcgx_kdtree_max_depth(self._h, C.byref(d)))
        return d.value

    def Tree(self):
        """The tree as the reference holds it, nested [id, dim, child0, child1] (None = nil); after
        DeletePoint the patched tree (kdtree.go:264-320)."""
        n = C.c_int64()
        L.check(L.lib().pcgx_kdtree_dump(self._h, None, 0, C.byref(n)))
        d = np.empty((max(n.value, 1), 4), np.int64)
        L.check(L.lib().pcgx_kdtree_dump(self._h, L.ptr(d), n.value, C.byref(n)))

        def rec(k):
            return None if k < 0 else [int(d[k][0]), int(d[k][1]), rec(int(d[k][2])), rec(int(d[k][3]))]
        return rec(0) if n.value else None

    def InOrder(self):
        out = np.empty(self.LiveCount(), np.int64)
        L.check(L.lib().pcgx_kdtree_inorder(self._h, L.ptr(out)))
        return out

    # -- KDTree.DeletePoint (kdtree.go:322-332)
    def DeletePoint(self, pID):
        """Removes point pID from the tree (the accessor, Len() and Vec3At() keep it).  An id
        outside [0, Len()) raises IndexError with the reference's message (kdtree.go:323-325)."""
        self.DeletePoints([pID])

    def DeletePoints(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        rc = L.lib().pcgx_kdtree_delete_points(self._h, L.ptr(ids), len(ids))
        if rc == L.PCGX_E_OUT_OF_RANGE:
            raise IndexError(L.last_error())
        L.check(rc)

    def LiveCount(self):
        n = C.c_int64()
        L.check(L.lib().pcgx_kdtree_live_count(self._h, C.byref(n)))
        return n.value

    # -- storage.Search
    def Nearest(self, p, maxRange):
        ids, dsq = self.NearestBatch(np.asarray(p, np.float32).reshape(1, 3), maxRange)
        return Neighbor(ids[0], dsq[0])

    def NearestBatch(self, q, maxRange):
        """k.Nearest(q[i], maxRange) for every row of q -> (ids int64[n], distSq float32[n])."""
        q = L.f32c(q).reshape(-1, 3)
        ids = np.empty(len(q), np.int64)
        dsq = np.empty(len(q), np.float32)
        L.check(L.lib().pcgx_kdtree_nearest_batch(self._h, L.ptr(q), len(q), maxRange, self.MinDistSq,
                                                  L.ptr(ids), L.ptr(dsq)))
        return ids, dsq

    def Range(self, p, maxRange):
        """KDTree.Range (kdtree.go:148-161): [Neighbor] with DistSq < maxRange^2 sorted by DistSq."""
        offs, ids, dsq = self.RangeBatch(np.asarray(p, np.float32).reshape(1, 3), maxRange)
        return [Neighbor(i, d) for i, d in zip(ids, dsq)]

    def RangeBatch(self, q, maxRange):
        """Range for every row of q -> (offsets int64[n+1], ids int64[total], distSq float32[total]);
        query i owns [offsets[i], offsets[i+1])."""
        q = L.f32c(q).reshape(-1, 3)
        n = len(q)
        counts = np.zeros(n, np.int64)
        L.check(L.lib().pcgx_kdtree_range_count(self._h, L.ptr(q), n, maxRange, L.ptr(counts)))
        offs = np.zeros(n + 1, np.int64)
        np.cumsum(counts, out=offs[1:])
        total = int(offs[-1])
        ids = np.empty(total, np.int64)
        dsq = np.empty(total, np.float32)
        L.check(L.lib().pcgx_kdtree_range_fill(self._h, L.ptr(q), n, maxRange, L.ptr(offs), L.ptr(ids), L.ptr(dsq)))
        return offs, ids, dsq

    # -- extension (no reference parity): surface normals for the point-to-plane evaluator
    def Normals(self, radius, Viewpoint=(0.0, 0.0, 0.0), MinNeighbors=3, Queries=None):
        """Unit normal of the radius neighbourhood (DistSq < radius^2, Range's set) of every query ->
        (normals (n,3) float32, curvature (n,) float32, counts (n,) int32).  Queries None: the tree's own
        points, in id order (the BaseNormals of PointToPlaneEvaluator).  Fewer than max(MinNeighbors, 3)
        neighbours, or all of them at one place: normal 0, curvature NaN (include/pcgx.h).  The same where the
        float64 trace of the covariance rounds to <= 0, which takes neighbours whose spread is below ~1e-8 of
        their distance from the query."""
        q = None if Queries is None else L.f32c(Queries).reshape(-1, 3)
        n = self.Len() if q is None else len(q)
        vp = L.f32c(Viewpoint).reshape(3)
        normals = np.empty((n, 3), np.float32)
        curvature = np.empty(n, np.float32)
        counts = np.empty(n, np.int32)
        L.check(L.lib().pcgx_kdtree_normals(self._h, L.ptr(q), n, float(radius), L.ptr(vp), int(MinNeighbors),
                                            L.ptr(normals), L.ptr(curvature), L.ptr(counts)))
        return normals, curvature, counts

    def NormalsDev(self, radius, d_normals, d_curvature=0, d_counts=0, d_q=0, nq=None, Viewpoint=(0.0, 0.0, 0.0),
                   MinNeighbors=3, stream=0):
        """Device-resident Normals: raw device addresses (e.g. torch .data_ptr()); d_q 0 takes the tree's own
        points (nq = Len()).  Enqueued on `stream`, returns without waiting."""
        if nq is None:
            if d_q:
                raise ValueError("nq is required with d_q")
            nq = self.Len()
        vp = L.f32c(Viewpoint).reshape(3)
        L.check(L.lib().pcgx_kdtree_normals_dev(
            self._h, L.ptr(int(d_q)) if d_q else None, int(nq), float(radius), L.ptr(vp), int(MinNeighbors),
            L.ptr(int(d_normals)), L.ptr(int(d_curvature)) if d_curvature else None,
            L.ptr(int(d_counts)) if d_counts else None, L.ptr(stream) if stream else None))

    # -- extension (no reference parity): moving-least-squares smoothing, which puts noisy points back onto the surface
    def MLS(self, radius, Sigma=None, Order=2, MinNeighbors=3, Viewpoint=(0.0, 0.0, 0.0), Queries=None):
        """Every query projected onto the polynomial (Order 2: a quadratic height field over the neighbourhood's
        plane; Order 1: the plane) fitted to its radius neighbourhood (DistSq < radius^2, Range's set) with Gauss
        weights of width Sigma (None: the radius) -> (points (n,3) float32, normals (n,3) float32, kinds (n,) int32,
        counts (n,) int32).  Queries None: the tree's own points, in id order.  kinds: 0 the query came back
        unchanged (fewer than max(MinNeighbors, 3) neighbours, or all of them at one place; normal 0), 1 projected
        onto the plane, 2 onto the polynomial (include/pcgx.h, pcgx_kdtree_mls)."""
        q = None if Queries is None else L.f32c(Queries).reshape(-1, 3)
        n = self.Len() if q is None else len(q)
        vp = L.f32c(Viewpoint).reshape(3)
        points = np.empty((n, 3), np.float32)
        normals = np.empty((n, 3), np.float32)
        kinds = np.empty(n, np.int32)
        counts = np.empty(n, np.int32)
        L.check(L.lib().pcgx_kdtree_mls(self._h, L.ptr(q), n, float(radius), float(radius if Sigma is None else Sigma),
                                        int(Order), int(MinNeighbors), L.ptr(vp), L.ptr(points), L.ptr(normals),
                                        L.ptr(kinds), L.ptr(counts)))
        return points, normals, kinds, counts

    def MLSDev(self, radius, d_points, d_normals=0, d_kinds=0, d_counts=0, d_q=0, nq=None, Sigma=None, Order=2,
               MinNeighbors=3, Viewpoint=(0.0, 0.0, 0.0), stream=0):
        """Device-resident MLS: raw device addresses (e.g. torch .data_ptr()); d_q 0 takes the tree's own points
        (nq = Len()).  Enqueued on `stream`, returns without waiting."""
        if nq is None:
            if d_q:
                raise ValueError("nq is required with d_q")
            nq = self.Len()
        vp = L.f32c(Viewpoint).reshape(3)

        def opt(a):
            return L.ptr(int(a)) if a else None
        L.check(L.lib().pcgx_kdtree_mls_dev(
            self._h, opt(d_q), int(nq), float(radius), float(radius if Sigma is None else Sigma), int(Order),
            int(MinNeighbors), L.ptr(vp), opt(d_points), opt(d_normals), opt(d_kinds), opt(d_counts),
            L.ptr(stream) if stream else None))

    # -- extension (no reference parity): FPFH descriptors, the input of feature-based coarse alignment
    def FPFH(self, radius, Normals):
        """Fast Point Feature Histogram of every point of the tree over its radius neighbourhood (DistSq < radius^2,
        Range's set) -> (fpfh (n,33) float32, counts (n,3,11) int32, pairs (n,) int32), in id order.  Normals: (n,3)
        float32 unit normals in id order, e.g. Normals(radius)[0]; a zero or non-finite normal takes its point out of
        every pair.  counts: the valid pairs of a point per feature and bin (the SPFH before scaling), pairs: how
        many there are; fpfh = 100 counts / pairs + the 1 / DistSq weighted mean of the neighbours' SPFH, scaled to 100
        per feature (include/pcgx.h, pcgx_kdtree_fpfh)."""
        n = self.Len()
        nrm = L.f32c(Normals).reshape(-1, 3)
        if len(nrm) != n:
            raise ValueError("one normal per point of the tree is required")
        fpfh = np.empty((n, 33), np.float32)
        counts = np.empty((n, 3, 11), np.int32)
        pairs = np.empty(n, np.int32)
        L.check(L.lib().pcgx_kdtree_fpfh(self._h, L.ptr(nrm), float(radius), L.ptr(fpfh), L.ptr(counts), L.ptr(pairs)))
        return fpfh, counts, pairs

    def FPFHDev(self, radius, d_normals, d_fpfh, d_counts=0, d_pairs=0, stream=0):
        """Device-resident FPFH: raw device addresses (e.g. torch .data_ptr()); d_normals float32 [3 Len()] (what
        NormalsDev writes for the tree's own points), d_fpfh float32 [33 Len()], d_counts int32 [33 Len()], d_pairs
        int32 [Len()].  Enqueued on `stream`, returns without waiting."""
        L.check(L.lib().pcgx_kdtree_fpfh_dev(
            self._h, L.ptr(int(d_normals)), float(radius), L.ptr(int(d_fpfh)),
            L.ptr(int(d_counts)) if d_counts else None, L.ptr(int(d_pairs)) if d_pairs else None,
            L.ptr(stream) if stream else None))

    def FPFHAt(self, radius, Normals, Ids):
        """FPFH's rows at the listed point ids only -> (fpfh (k,33) float32, xyz (k,3) float32, counts (k,3,11) int32,
        pairs (k,) int32, n_spfh int).  Ids: int64, any order, repeats allowed; an id outside [0, Len()) raises.  Row s
        is FPFH(radius, Normals)'s row Ids[s], bit for bit, and xyz[s] is that point; n_spfh: how many points' SPFH
        records had to be computed -- the listed points and their neighbours, not the cloud (include/pcgx.h,
        pcgx_kdtree_fpfh_at)."""
        n = self.Len()
        nrm = L.f32c(Normals).reshape(-1, 3)
        if len(nrm) != n:
            raise ValueError("one normal per point of the tree is required")
        ids = np.ascontiguousarray(Ids, dtype=np.int64).reshape(-1)
        k = len(ids)
        fpfh = np.empty((k, 33), np.float32)
        xyz = np.empty((k, 3), np.float32)
        counts = np.empty((k, 3, 11), np.int32)
        pairs = np.empty(k, np.int32)
        n_spfh = C.c_int64()
        L.check(L.lib().pcgx_kdtree_fpfh_at(self._h, L.ptr(nrm), float(radius), L.ptr(ids), k, L.ptr(fpfh), L.ptr(xyz),
                                            L.ptr(counts), L.ptr(pairs), C.byref(n_spfh)))
        return fpfh, xyz, counts, pairs, n_spfh.value

    def FPFHAtDev(self, radius, d_normals, d_ids, cap, d_fpfh, d_xyz, d_n_ids=0, d_counts=0, d_pairs=0, d_n_spfh=0,
                  stream=0):
        """Device-resident FPFHAt with a fixed capacity: raw device addresses (e.g. torch .data_ptr()); d_ids int32
        [cap] and d_n_ids one int32 (0: all cap slots), e.g. what ISSKeypointsDev writes; d_fpfh float32 [33 cap],
        d_xyz float32 [3 cap], d_counts int32 [33 cap], d_pairs int32 [cap], d_n_spfh one int32.  Slots from
        clamp(*d_n_ids, 0, cap) on, and slots whose id is outside [0, Len()) (the -1 padding), get zero rows: the
        matcher's "no descriptor".  Enqueued on `stream`, returns without waiting; nothing is read back."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_fpfh_at_dev(
            self._h, L.ptr(int(d_normals)), float(radius), opt(d_ids), int(cap), opt(d_n_ids), opt(d_fpfh), opt(d_xyz),
            opt(d_counts), opt(d_pairs), opt(d_n_spfh), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): keypoints, what a large cloud is described and matched at
    def LocalMaxima(self, radius, Score):
        """The points whose score is the largest of their radius neighbourhood (DistSq < radius^2, Range's set) -> ids
        int64, ascending.  Score: (n,) float32 in id order.  Only a score > 0 qualifies (NaN never, +inf does); ties go
        to the smaller id; a deleted id or a point with a NaN coordinate is never a maximum (include/pcgx.h,
        pcgx_kdtree_local_maxima)."""
        n = self.Len()
        score = L.f32c(Score).reshape(-1)
        if len(score) != n:
            raise ValueError("one score per point of the tree is required")
        ids = np.empty(n, np.int64)
        cnt = C.c_int64()
        L.check(L.lib().pcgx_kdtree_local_maxima(self._h, float(radius), L.ptr(score), L.ptr(ids), C.byref(cnt)))
        return ids[:cnt.value]

    def LocalMaximaDev(self, radius, d_score, d_ids, d_n_ids, stream=0):
        """Device-resident LocalMaxima: raw device addresses (e.g. torch .data_ptr()); d_score float32 [Len()], d_ids
        int32 [Len()] (the maxima ascending, then -1), d_n_ids one int32.  Enqueued on `stream`, returns without
        waiting."""
        L.check(L.lib().pcgx_kdtree_local_maxima_dev(
            self._h, float(radius), L.ptr(int(d_score)), L.ptr(int(d_ids)), L.ptr(int(d_n_ids)),
            L.ptr(stream) if stream else None))

    def ISSKeypoints(self, SalientRadius, NonMaxRadius, Gamma21=0.975, Gamma32=0.975, MinNeighbors=5):
        """ISS keypoints (Zhong 2009, Open3D's form) -> (ids int64 ascending, eigenvalues (n,3) float32 ascending,
        saliency (n,) float32).  eigenvalues: of Normals' covariance at SalientRadius, (0, 0, 0) where Normals answers
        "degenerate"; saliency: l0 where l0 > 0, l1 < Gamma21 l2 and l0 < Gamma32 l1, else 0; ids: LocalMaxima of the
        saliency at NonMaxRadius (include/pcgx.h, pcgx_kdtree_iss_keypoints)."""
        n = self.Len()
        eig = np.empty((n, 3), np.float32)
        sal = np.empty(n, np.float32)
        ids = np.empty(n, np.int64)
        cnt = C.c_int64()
        L.check(L.lib().pcgx_kdtree_iss_keypoints(self._h, float(SalientRadius), float(NonMaxRadius), float(Gamma21),
                                                  float(Gamma32), int(MinNeighbors), L.ptr(eig), L.ptr(sal), L.ptr(ids),
                                                  C.byref(cnt)))
        return ids[:cnt.value], eig, sal

    def ISSKeypointsDev(self, SalientRadius, NonMaxRadius, d_ids, d_n_ids, d_eigenvalues=0, d_saliency=0, Gamma21=0.975,
                        Gamma32=0.975, MinNeighbors=5, stream=0):
        """Device-resident ISSKeypoints: raw device addresses (e.g. torch .data_ptr()); d_ids int32 [Len()] (the
        keypoints ascending, then -1), d_n_ids one int32, d_eigenvalues float32 [3 Len()], d_saliency float32 [Len()].
        Enqueued on `stream`, returns without waiting."""
        L.check(L.lib().pcgx_kdtree_iss_keypoints_dev(
            self._h, float(SalientRadius), float(NonMaxRadius), float(Gamma21), float(Gamma32), int(MinNeighbors),
            L.ptr(int(d_eigenvalues)) if d_eigenvalues else None, L.ptr(int(d_saliency)) if d_saliency else None,
            L.ptr(int(d_ids)), L.ptr(int(d_n_ids)), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): minimum-distance subsampling, a maximal set of points at least radius apart
    def Thin(self, radius, Seed=0, Score=None, Owner=False):
        """A maximal subset of the tree's own points no two of which are within radius (DistSq < radius^2, Range's
        set, strict) -> ids int64 ascending, or (ids, owner int64 (n,)) with Owner=True.  The set is what greedy
        selection in priority order keeps: by hash(Seed, id) when Score is None, else the larger Score first, ties to
        the smaller id (a NaN score, a deleted id or a non-finite point takes no part: owner -1).  owner: a kept point
        itself, a dropped point its kept neighbour of the smallest (DistSq, id) (include/pcgx.h, pcgx_kdtree_thin)."""
        n = self.Len()
        score = None
        if Score is not None:
            score = L.f32c(Score).reshape(-1)
            if len(score) != n:
                raise ValueError("one score per point of the tree is required")
        ids = np.empty(n, np.int64)
        owner = np.empty(n, np.int64) if Owner else None
        cnt = C.c_int64()
        L.check(L.lib().pcgx_kdtree_thin(self._h, float(radius), int(Seed) & 0xffffffff, L.ptr(score), L.ptr(ids),
                                         C.byref(cnt), L.ptr(owner)))
        return (ids[:cnt.value], owner) if Owner else ids[:cnt.value]

    def ThinDev(self, radius, d_ids, d_n_ids, d_n_left, d_owner=0, d_score=0, Seed=0, MaxRounds=0, stream=0):
        """Device-resident Thin: raw device addresses (e.g. torch .data_ptr()); d_ids int32 [Len()] (the kept ids
        ascending, then -1), d_n_ids and d_n_left one int32 each, d_owner int32 [Len()], d_score float32 [Len()].
        MaxRounds rounds are enqueued (0: the library's default); *d_n_left > 0 afterwards means the kept set is not
        maximal yet and d_owner is all -2.  Enqueued on `stream`, returns without waiting."""
        L.check(L.lib().pcgx_kdtree_thin_dev(
            self._h, float(radius), int(Seed) & 0xffffffff, L.ptr(int(d_score)) if d_score else None, int(MaxRounds),
            L.ptr(int(d_ids)) if d_ids else None, L.ptr(int(d_n_ids)) if d_n_ids else None,
            L.ptr(int(d_owner)) if d_owner else None, L.ptr(int(d_n_left)) if d_n_left else None,
            L.ptr(stream) if stream else None))

    # -- extension (no reference parity): farthest-point sampling, a target count of well-spread points in pick order
    def FarthestPoints(self, count, Start=-1, Owner=False):
        """count of the tree's own points, each the one farthest (float32 DistSq to the nearest pick so far, ties to the
        smallest id) from those picked before it -> (ids int64 in pick order, dist_sq float32, cover_sq float32), or
        with Owner=True (..., owner int64 (n,)).  The first pick is Start, or the smallest eligible id (-1); deleted
        and non-finite points are never picked.  ids and dist_sq have min(count, eligible points) entries and are a
        prefix of what any larger count gives; dist_sq[0] is +inf; cover_sq is the d the next pick would have had
        (every eligible point lies within it of a pick), -1 when no point is left.  owner: the nearest pick's id, the
        earlier pick among equal distances, -1 for a point that is not eligible (include/pcgx.h, pcgx_kdtree_fps)."""
        n, count = self.Len(), int(count)
        ids = np.empty(max(count, 0), np.int64)
        dist = np.empty(max(count, 0), np.float32)
        cover = np.empty(1, np.float32)
        owner = np.empty(n, np.int64) if Owner else None
        cnt = C.c_int64()
        L.check(L.lib().pcgx_kdtree_fps(self._h, count, int(Start), L.ptr(ids), C.byref(cnt), L.ptr(dist), L.ptr(cover),
                                        L.ptr(owner)))
        out = (ids[:cnt.value], dist[:cnt.value], cover[0])
        return out + (owner,) if Owner else out

    def FarthestPointsDev(self, count, d_ids, d_n_ids, d_dist_sq=0, d_cover_sq=0, d_owner=0, Start=-1, stream=0):
        """Device-resident FarthestPoints: raw device addresses (e.g. torch .data_ptr()); d_ids int32 [count] (the picks
        in order, then -1), d_n_ids one int32, d_dist_sq float32 [count] (then -1), d_cover_sq one float32, d_owner
        int32 [Len()].  Enqueued on `stream`, returns without waiting, reads nothing back."""
        L.check(L.lib().pcgx_kdtree_fps_dev(
            self._h, int(count), int(Start), L.ptr(int(d_ids)) if d_ids else None,
            L.ptr(int(d_n_ids)) if d_n_ids else None, L.ptr(int(d_dist_sq)) if d_dist_sq else None,
            L.ptr(int(d_cover_sq)) if d_cover_sq else None, L.ptr(int(d_owner)) if d_owner else None,
            L.ptr(stream) if stream else None))

    # -- extension (no reference parity): boundary points, where a scanned surface ends
    def Boundary(self, radius, Normals, MinGap=16, MinNeighbors=1):
        """The points whose radius neighbours (DistSq < radius^2, Range's set) leave an angular gap of at least MinGap
        sectors of 5.625 degrees in the tangent plane of Normals (n,3) float32 in id order -> (ids int64 ascending, gaps
        int32 (n,), masks uint64 (n,), counts int32 (n,)).  masks: bit s set where a neighbour's direction falls in
        sector s; gaps: the longest cyclic run of zero bits, 64 for an empty mask, -1 where the point is not evaluated
        (deleted, a NaN coordinate, a non-finite or zero normal, fewer than max(MinNeighbors, 1) neighbours).  A true
        opening of g sectors gives g - 2 < gap < g (include/pcgx.h, pcgx_kdtree_boundary)."""
        n = self.Len()
        nrm = L.f32c(Normals).reshape(-1, 3)
        if len(nrm) != n:
            raise ValueError("one normal per point of the tree is required")
        ids = np.empty(n, np.int64)
        gaps = np.empty(n, np.int32)
        masks = np.empty(n, np.uint64)
        counts = np.empty(n, np.int32)
        cnt = C.c_int64()
        L.check(L.lib().pcgx_kdtree_boundary(self._h, float(radius), L.ptr(nrm), int(MinGap), int(MinNeighbors), L.ptr(ids),
                                             C.byref(cnt), L.ptr(gaps), L.ptr(masks), L.ptr(counts)))
        return ids[:cnt.value], gaps, masks, counts

    def BoundaryDev(self, radius, d_normals, d_ids, d_n_ids, d_gaps=0, d_masks=0, d_counts=0, MinGap=16, MinNeighbors=1,
                    stream=0):
        """Device-resident Boundary: raw device addresses (e.g. torch .data_ptr()); d_normals float32 [3 Len()] (what
        NormalsDev wrote on the same stream), d_ids int32 [Len()] (the boundary points ascending, then -1), d_n_ids one
        int32, d_gaps int32 [Len()], d_masks uint64 [Len()], d_counts int32 [Len()] (each optional).  Enqueued on
        `stream`, returns without waiting."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_boundary_dev(
            self._h, float(radius), L.ptr(int(d_normals)), int(MinGap), int(MinNeighbors), L.ptr(int(d_ids)),
            L.ptr(int(d_n_ids)), opt(d_gaps), opt(d_masks), opt(d_counts), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): consistent normal orientation along the radius graph's minimum spanning forest
    def OrientNormals(self, radius, Normals, Direction=None, Viewpoint=None, Component=False):
        """Normals (n,3) float32 in id order with their signs made consistent between neighbours (DistSq < radius^2,
        Range's set): the sign is propagated along the minimum spanning forest of the radius graph, edges ordered by
        |n_i . n_j| descending, then the smaller ids -> (normals float32 (n,3), flipped uint8 (n,), n_components), or
        with Component=True (..., component int64 (n,)): the smallest id of each point's component, -1 for a point
        that takes no part (deleted, non-finite, a zero or non-finite normal; its normal comes back as given).  A
        component's overall sign: its smallest id keeps its own (default); Direction=u: its topmost point along u looks
        along u (Hoppe's rule); Viewpoint=v: the majority of its normals looks towards v (include/pcgx.h,
        pcgx_kdtree_orient_normals)."""
        n = self.Len()
        nrm = L.f32c(Normals).reshape(-1, 3)
        if len(nrm) != n:
            raise ValueError("one normal per point of the tree is required")
        if Direction is not None and Viewpoint is not None:
            raise ValueError("Direction or Viewpoint, not both")
        mode = 1 if Direction is not None else 2 if Viewpoint is not None else 0
        ref = L.f32c(Direction if mode == 1 else Viewpoint).reshape(3) if mode else None
        out = np.empty((n, 3), np.float32)
        flipped = np.empty(n, np.uint8)
        comp = np.empty(n, np.int64) if Component else None
        nc, no = C.c_int64(), C.c_int64()
        L.check(L.lib().pcgx_kdtree_orient_normals(self._h, float(radius), L.ptr(nrm), mode, L.ptr(ref), L.ptr(out),
                                                   L.ptr(flipped), L.ptr(comp), C.byref(nc), C.byref(no)))
        res = (out, flipped, nc.value)
        return res + (comp,) if Component else res

    def OrientNormalsDev(self, radius, d_normals, d_normals_out, d_flipped, d_n_components, d_n_open, d_component=0,
                         Direction=None, Viewpoint=None, MaxRounds=0, stream=0):
        """Device-resident OrientNormals: raw device addresses (e.g. torch .data_ptr()); d_normals float32 [3 Len()]
        (what NormalsDev wrote on the same stream), d_normals_out float32 [3 Len()] (may be d_normals; or 0),
        d_flipped uint8 [Len()] (or 0, not both), d_component int32 [Len()] (optional), d_n_components and d_n_open one
        int32 each.  MaxRounds rounds are enqueued (0: enough to finish for certain); *d_n_open > 0 afterwards means the
        forest is that of MaxRounds rounds, not yet spanning.  Direction / Viewpoint are host values.  Enqueued on
        `stream`, returns without waiting, reads nothing back."""
        if Direction is not None and Viewpoint is not None:
            raise ValueError("Direction or Viewpoint, not both")
        mode = 1 if Direction is not None else 2 if Viewpoint is not None else 0
        ref = L.f32c(Direction if mode == 1 else Viewpoint).reshape(3) if mode else None
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_orient_normals_dev(
            self._h, float(radius), opt(d_normals), mode, L.ptr(ref), int(MaxRounds), opt(d_normals_out), opt(d_flipped),
            opt(d_component), opt(d_n_components), opt(d_n_open), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): ray queries, the points inside a thin tube around each ray
    @staticmethod
    def _rays(origins, directions, s_min, s_max):
        o = L.f32c(origins).reshape(-1, 3)
        d = L.f32c(directions).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("one direction per origin is required")
        lo = None if s_min is None else np.ascontiguousarray(np.broadcast_to(np.asarray(s_min, np.float32), (len(o),)))
        hi = None if s_max is None else np.ascontiguousarray(np.broadcast_to(np.asarray(s_max, np.float32), (len(o),)))
        return o, d, lo, hi

    def RayCast(self, origins, directions, radius, s_min=None, s_max=None):
        """The first point along each ray o + s d, s in [s_min, s_max] (None: 0 and +inf; scalars or (nr,) arrays), among
        the tree's points within `radius` of the ray's line -> (ids int64 (nr,), -1 for a miss, along float64 (nr,),
        off_sq float64 (nr,)).  d is not normalised; along = (p - o) . d and off_sq = |(p - o) x d|^2 in float64, 0 for a
        miss, so s = along / |d|^2 and the metric offset is sqrt(off_sq / |d|^2); a tie in along goes to the smallest id
        (include/pcgx.h, pcgx_kdtree_raycast)."""
        o, d, lo, hi = self._rays(origins, directions, s_min, s_max)
        nr = len(o)
        ids = np.empty(nr, np.int64)
        along = np.empty(nr, np.float64)
        off = np.empty(nr, np.float64)
        L.check(L.lib().pcgx_kdtree_raycast(self._h, L.ptr(o), L.ptr(d), L.ptr(lo), L.ptr(hi), nr, float(radius),
                                            L.ptr(ids), L.ptr(along), L.ptr(off)))
        return ids, along, off

    def RayCastDev(self, d_origins, d_directions, nr, radius, d_ids, d_along=0, d_off_sq=0, d_s_min=0, d_s_max=0,
                   stream=0):
        """Device-resident RayCast: raw device addresses (e.g. torch .data_ptr()); d_origins, d_directions float32
        [3 nr], d_s_min, d_s_max float32 [nr] (0: 0 and +inf), d_ids int32 [nr], d_along, d_off_sq float64 [nr] (each
        optional).  Enqueued on `stream`, returns without waiting."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_raycast_dev(
            self._h, opt(d_origins), opt(d_directions), opt(d_s_min), opt(d_s_max), int(nr), float(radius), opt(d_ids),
            opt(d_along), opt(d_off_sq), L.ptr(stream) if stream else None))

    def RayPierce(self, origins, directions, radius, s_min=None, s_max=None):
        """How often each point was pierced: counts int32 (Len(),) in id order, one added for every (ray, point) pair
        where the point lies within `radius` of the ray's line and s_min <= s <= s_max (RayCast's member test; a deleted
        point counts 0; include/pcgx.h, pcgx_kdtree_ray_pierce)."""
        o, d, lo, hi = self._rays(origins, directions, s_min, s_max)
        counts = np.zeros(self.Len(), np.int32)
        L.check(L.lib().pcgx_kdtree_ray_pierce(self._h, L.ptr(o), L.ptr(d), L.ptr(lo), L.ptr(hi), len(o), float(radius),
                                               L.ptr(counts)))
        return counts

    def RayPierceDev(self, d_origins, d_directions, nr, radius, d_counts, d_s_min=0, d_s_max=0, stream=0):
        """Device-resident RayPierce, ADDING into d_counts int32 [Len()]: zero it before the first scan, and successive
        scans accumulate on one stream with nothing read back.  Enqueued on `stream`, returns without waiting."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_ray_pierce_dev(
            self._h, opt(d_origins), opt(d_directions), opt(d_s_min), opt(d_s_max), int(nr), float(radius),
            opt(d_counts), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): cylinder statistics, what M3C2 (pcgol_amd/change.py) is made of
    def CylinderStats(self, cores, axes, radius, half_length):
        """Per cylinder (core o, axis d not normalised, `radius`, `half_length` each way along the axis) over the tree's
        live points -> (counts int32 (m,), sums float64 (m, 2)): the number of members and S1 = sum of a, S2 = sum of
        a a, a = (p - o) . d in float64.  Unnormalised: the metric mean is S1 / n / |d|, the metric variance the sample
        variance of a over |d|^2.  counts are exact; sums carry the bound of a summation order
        (include/pcgx.h, pcgx_kdtree_cylinder_stats)."""
        o = L.f32c(cores).reshape(-1, 3)
        d = L.f32c(axes).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("one axis per core is required")
        counts = np.zeros(len(o), np.int32)
        sums = np.zeros((len(o), 2), np.float64)
        L.check(L.lib().pcgx_kdtree_cylinder_stats(self._h, L.ptr(o), L.ptr(d), len(o), float(radius), float(half_length),
                                                   L.ptr(counts), L.ptr(sums)))
        return counts, sums

    def CylinderStatsDev(self, d_cores, d_axes, m, radius, half_length, d_counts, d_sums, stream=0):
        """Device-resident CylinderStats: raw device addresses (e.g. torch .data_ptr()); d_cores, d_axes float32 [3 m],
        d_counts int32 [m], d_sums float64 [2 m].  Enqueued on `stream`, returns without waiting, reads nothing back."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_cylinder_stats_dev(
            self._h, opt(d_cores), opt(d_axes), int(m), float(radius), float(half_length), opt(d_counts), opt(d_sums),
            L.ptr(stream) if stream else None))

    # -- extension (no reference parity): clusters, the connected components of the radius graph
    def Clusters(self, radius, Normals=None, MinCos=0.0, Oriented=False, Curvature=None, MaxCurvature=0.0, MinSize=1,
                 MaxSize=0):
        """The connected components of the radius graph (DistSq < radius^2, Range's set) over the tree's own points,
        kept when MinSize <= size (<= MaxSize unless 0), largest first, equal sizes by smallest id -> (labels int64
        (n,), sizes int64 (C,), ids int64 (sum(sizes),)).  Normals (n,3): an edge also needs (|n_i . n_j| or, Oriented,
        n_i . n_j) >= MinCos, and a non-finite or zero normal makes its point unusable; Curvature (n,): a point above
        MaxCurvature (or NaN) is unusable.  labels: the cluster's number, -1 for an unusable point or one of a
        component outside the size range; ids: cluster 0's members ascending, then cluster 1's, ... (include/pcgx.h,
        pcgx_kdtree_clusters)."""
        n = self.Len()
        nrm = cur = None
        if Normals is not None:
            nrm = L.f32c(Normals).reshape(-1, 3)
            if len(nrm) != n:
                raise ValueError("one normal per point of the tree is required")
        if Curvature is not None:
            cur = L.f32c(Curvature).reshape(-1)
            if len(cur) != n:
                raise ValueError("one curvature per point of the tree is required")
        labels = np.empty(n, np.int64)
        sizes = np.empty(n, np.int64)
        ids = np.empty(n, np.int64)
        cnt = C.c_int64()
        L.check(L.lib().pcgx_kdtree_clusters(
            self._h, float(radius), L.ptr(nrm) if nrm is not None else None, float(MinCos), int(bool(Oriented)),
            L.ptr(cur) if cur is not None else None, float(MaxCurvature), int(MinSize), int(MaxSize),
            L.ptr(labels) if n else None, C.byref(cnt), L.ptr(sizes) if n else None, L.ptr(ids) if n else None))
        sizes = sizes[:cnt.value]
        return labels, sizes, ids[:int(sizes.sum())]

    def ClustersDev(self, radius, d_labels, d_n_clusters, d_sizes=0, d_ids=0, d_normals=0, MinCos=0.0, Oriented=False,
                    d_curvature=0, MaxCurvature=0.0, MinSize=1, MaxSize=0, stream=0):
        """Device-resident Clusters: raw device addresses (e.g. torch .data_ptr()); d_labels int32 [Len()],
        d_n_clusters one int32, d_sizes int32 [Len()] (the sizes, then 0), d_ids int32 [Len()] (the members cluster by
        cluster, then -1), d_normals float32 [3 Len()] and d_curvature float32 [Len()] (what NormalsDev writes for the
        tree's own points).  Enqueued on `stream`, returns without waiting; nothing is read back."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_clusters_dev(
            self._h, float(radius), opt(d_normals), float(MinCos), int(bool(Oriented)), opt(d_curvature),
            float(MaxCurvature), int(MinSize), int(MaxSize), opt(d_labels), opt(d_n_clusters), opt(d_sizes), opt(d_ids),
            L.ptr(stream) if stream else None))

    # -- extension (no reference parity): density clusters, DBSCAN over the same neighbourhoods
    def DBSCAN(self, radius, MinPts, MinSize=1, MaxSize=0):
        """DBSCAN over the tree's own points: a point is core when its neighbourhood (DistSq < radius^2, Range's set,
        itself included) holds at least MinPts points; the clusters are the components of the core points plus the
        border points, each with its nearest core neighbour (smallest DistSq, then smallest id); kept when MinSize <=
        size (<= MaxSize unless 0), largest first, equal sizes by smallest id -> (labels int64 (n,), sizes int64 (C,),
        ids int64 (sum(sizes),), kind uint8 (n,): 0 noise, 1 border, 2 core).  MinPts = 1 is Clusters(radius)
        (include/pcgx.h, pcgx_kdtree_dbscan)."""
        n = self.Len()
        labels = np.empty(n, np.int64)
        sizes = np.empty(n, np.int64)
        ids = np.empty(n, np.int64)
        kind = np.empty(n, np.uint8)
        cnt = C.c_int64()
        L.check(L.lib().pcgx_kdtree_dbscan(
            self._h, float(radius), int(MinPts), int(MinSize), int(MaxSize), L.ptr(labels) if n else None, C.byref(cnt),
            L.ptr(sizes) if n else None, L.ptr(ids) if n else None, L.ptr(kind) if n else None))
        sizes = sizes[:cnt.value]
        return labels, sizes, ids[:int(sizes.sum())], kind

    def DBSCANDev(self, radius, MinPts, d_labels, d_n_clusters, d_sizes=0, d_ids=0, d_kind=0, MinSize=1, MaxSize=0,
                  stream=0):
        """Device-resident DBSCAN: raw device addresses (e.g. torch .data_ptr()); d_labels int32 [Len()], d_n_clusters
        one int32, d_sizes int32 [Len()] (the sizes, then 0), d_ids int32 [Len()] (the members cluster by cluster, then
        -1), d_kind uint8 [Len()].  Enqueued on `stream`, returns without waiting; nothing is read back."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_dbscan_dev(
            self._h, float(radius), int(MinPts), int(MinSize), int(MaxSize), opt(d_labels), opt(d_n_clusters),
            opt(d_sizes), opt(d_ids), opt(d_kind), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): group geometry, the moments, boxes and planes of a grouped id list
    def GroupStats(self, ids, sizes):
        """Per group of a grouped id list over the tree's own points (ids: group 0's members, then group 1's, ...;
        sizes: per group -- what Clusters returns) -> GroupGeometry(count int64 (G,), aabb float32 (G, 6) lo xyz hi
        xyz, centroid float64 (G, 3), cov float64 (G, 6) xx xy xz yy yz zz, eig float64 (G, 3) descending, axes float64
        (G, 3, 3) unit eigenvectors as rows (axis 2: the fitted plane's normal), obb float64 (G, 6) centre xyz and
        half-extents along the axes).  A group without a live member is all zero (include/pcgx.h,
        pcgx_kdtree_group_stats)."""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        sizes = np.ascontiguousarray(sizes, np.int64).reshape(-1)
        g = len(sizes)
        out = GroupGeometry(np.zeros(g, np.int64), np.zeros((g, 6), np.float32), np.zeros((g, 3)), np.zeros((g, 6)),
                            np.zeros((g, 3)), np.zeros((g, 3, 3)), np.zeros((g, 6)))
        L.check(L.lib().pcgx_kdtree_group_stats(self._h, L.ptr(ids) if len(ids) else None, len(ids),
                                                L.ptr(sizes) if g else None, g, *[L.ptr(a) if g else None for a in out]))
        return out

    def GroupStatsDev(self, d_ids, cap_ids, d_sizes, cap_groups, d_n_groups=0, d_count=0, d_aabb=0, d_centroid=0, d_cov=0,
                      d_eig=0, d_axes=0, d_obb=0, stream=0):
        """Device-resident GroupStats: raw device addresses (e.g. torch .data_ptr()); d_ids int32 [cap_ids], d_sizes
        int32 [cap_groups], d_n_groups one int32 (0: cap_groups groups) -- ClustersDev's d_ids, d_sizes and d_n_clusters
        as they are, with cap_ids = cap_groups = Len(); the outputs (0: not wanted) hold cap_groups rows: d_count int32,
        d_aabb float32 [6], d_centroid [3], d_cov [6], d_eig [3], d_axes [9], d_obb [6] float64.  Enqueued on `stream`,
        returns without waiting; nothing is read back."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_group_stats_dev(
            self._h, opt(d_ids), int(cap_ids), opt(d_sizes), int(cap_groups), opt(d_n_groups), opt(d_count), opt(d_aabb),
            opt(d_centroid), opt(d_cov), opt(d_eig), opt(d_axes), opt(d_obb), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): group footprints, the exact 2-D hulls and upright boxes of a grouped id list
    def GroupHulls(self, ids, sizes):
        """Per group of a grouped id list (as GroupStats takes it) -> GroupFootprints(hull_sizes int64 (G,), hull_ids
        int64 (len(ids),), area float64 (G,), rect float64 (G, 6)): the vertices of the exact convex hull of the group's
        (x, y), again a grouped id list (counter-clockwise from the lexicographically least place, a place by its
        smallest id, -1 behind the last hull), the polygon's area, and the minimum-area rectangle with a side along a
        hull edge as centre x, y, the unit direction u of that edge and the half-extents along u and (-u_y, u_x)
        (include/pcgx.h, pcgx_kdtree_group_hulls)."""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        sizes = np.ascontiguousarray(sizes, np.int64).reshape(-1)
        g = len(sizes)
        out = GroupFootprints(np.zeros(g, np.int64), np.full(len(ids), -1, np.int64), np.zeros(g), np.zeros((g, 6)))
        L.check(L.lib().pcgx_kdtree_group_hulls(self._h, L.ptr(ids) if len(ids) else None, len(ids),
                                                L.ptr(sizes) if g else None, g,
                                                *[L.ptr(a) if g and a.size else None for a in out]))
        return out

    def GroupHullsDev(self, d_ids, cap_ids, d_sizes, cap_groups, d_n_groups=0, d_hull_sizes=0, d_hull_ids=0, d_area=0,
                      d_rect=0, stream=0):
        """Device-resident GroupHulls: raw device addresses as GroupStatsDev takes them; the outputs (0: not wanted):
        d_hull_sizes int32 [cap_groups], d_hull_ids int32 [cap_ids], d_area float64 [cap_groups], d_rect float64
        [6 cap_groups].  Enqueued on `stream`, returns without waiting; nothing is read back."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_group_hulls_dev(
            self._h, opt(d_ids), int(cap_ids), opt(d_sizes), int(cap_groups), opt(d_n_groups), opt(d_hull_sizes),
            opt(d_hull_ids), opt(d_area), opt(d_rect), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): plane segmentation, consensus planes peeled one by one
    def Planes(self, MaxDist, NHyp=256, MaxPlanes=1, MinInliers=3, Axis=None, MinAxisCos=0.0, Normals=None,
               MinNormalCos=0.0, Refine=True, Samples=None, Seed=0):
        """The plane most of the tree's live points lie within MaxDist of, by sample consensus over NHyp three-point
        hypotheses; its inliers are taken out and the next plane is looked for, up to MaxPlanes times, until a round's
        best has fewer than max(MinInliers, 3) inliers -> PlaneSegments(n_planes, planes float32 (MaxPlanes, 4) as
        (nx, ny, nz, d), sizes int64, refined int32, best int64, labels int64 (n,), ids int64 (sum(sizes),), status
        int32 (MaxPlanes, NHyp), counts int64, hyp_planes float32 (MaxPlanes, NHyp, 4)).  Axis: only planes whose
        normal has |cos| >= MinAxisCos with it; Normals (n, 3): an inlier's normal has |cos| >= MinNormalCos with the
        plane's, and a point with a zero or non-finite normal takes no part; Refine: the best is refitted once to its
        inliers by GroupStats' least-squares plane and kept where that loses no inlier.  Samples: uint32 (MaxPlanes,
        NHyp, 3) random words, drawn from np.random.default_rng(Seed) when None (include/pcgx.h, pcgx_kdtree_planes)."""
        n, nh, mp = self.Len(), int(NHyp), int(MaxPlanes)
        if Samples is None:
            Samples = np.random.default_rng(Seed).integers(0, 2 ** 32, (max(mp, 0), max(nh, 0), 3),
                                                           dtype=np.uint64).astype(np.uint32)
        smp = np.ascontiguousarray(Samples, np.uint32).reshape(-1)
        if nh > 0 and mp > 0 and len(smp) != 3 * nh * mp:
            raise ValueError("three sample words per hypothesis and round are required")
        nrm = axis = None
        if Normals is not None:
            nrm = L.f32c(Normals).reshape(-1, 3)
            if len(nrm) != n:
                raise ValueError("one normal per point of the tree is required")
        if Axis is not None:
            axis = L.f32c(Axis).reshape(3)
        rows = max(nh, 0) * max(mp, 0)
        out = PlaneSegments(0, np.zeros((max(mp, 0), 4), np.float32), np.zeros(max(mp, 0), np.int64),
                            np.zeros(max(mp, 0), np.int32), np.full(max(mp, 0), -1, np.int64), np.full(n, -1, np.int64),
                            np.full(n, -1, np.int64), np.full(rows, -1, np.int32), np.zeros(rows, np.int64),
                            np.zeros((rows, 4), np.float32))
        cnt = C.c_int64()
        opt = lambda a: L.ptr(a) if a is not None and a.size else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_planes(
            self._h, opt(smp), nh, mp, float(MaxDist), int(MinInliers), opt(axis), float(MinAxisCos),
            L.ptr(nrm) if nrm is not None else None, float(MinNormalCos), int(bool(Refine)), C.byref(cnt),
            opt(out.planes), opt(out.sizes), opt(out.refined), opt(out.best), opt(out.labels), opt(out.ids),
            opt(out.status), opt(out.counts), opt(out.hyp_planes)))
        k = int(out.sizes[:cnt.value].sum())
        return out._replace(n_planes=int(cnt.value), ids=out.ids[:k], status=out.status.reshape(mp, nh),
                            counts=out.counts.reshape(mp, nh), hyp_planes=out.hyp_planes.reshape(mp, nh, 4))

    def PlanesDev(self, MaxDist, d_samples, NHyp, d_n_planes, d_planes, d_sizes, d_refined, d_best, d_labels, d_ids=0,
                  d_status=0, d_counts=0, d_hyp_planes=0, MaxPlanes=1, MinInliers=3, Axis=None, MinAxisCos=0.0,
                  d_normals=0, MinNormalCos=0.0, Refine=True, stream=0):
        """Device-resident Planes: raw device addresses (e.g. torch .data_ptr()); d_samples uint32 [3 NHyp MaxPlanes],
        d_n_planes one int32, d_planes float32 [4 MaxPlanes], d_sizes / d_refined / d_best int32 [MaxPlanes], d_labels
        int32 [Len()], d_ids int32 [Len()] (the inliers plane by plane, then -1), d_status / d_counts int32 [MaxPlanes
        NHyp], d_hyp_planes float32 [4 MaxPlanes NHyp], d_normals float32 [3 Len()] (what NormalsDev writes); Axis stays
        a host value.  Enqueued on `stream`, returns without waiting; nothing is read back: every round is enqueued at
        once and reads from device words what the rounds before it left.  d_ids, d_sizes and d_n_planes are a grouped
        list for GroupStatsDev and GroupHullsDev (cap_ids = Len(), cap_groups = MaxPlanes).

        What is NOT on a plane, clustered without a rebuild, all on one stream and with nothing read back:

            t.PlanesDev(0.02, smp.data_ptr(), 256, n_planes.data_ptr(), planes.data_ptr(), sizes.data_ptr(),
                        refined.data_ptr(), best.data_ptr(), labels.data_ptr(), d_ids=ids.data_ptr(), MaxPlanes=4,
                        MinInliers=500, stream=s)
            with torch.cuda.stream(stream):              # the torch stream that wraps s
                on_plane = (labels >= 0).float()         # 1.0 on a plane, 0.0 off it
            t.ClustersDev(0.1, c_labels.data_ptr(), c_n.data_ptr(), d_curvature=on_plane.data_ptr(), MaxCurvature=0.5,
                          stream=s)                      # a point "above MaxCurvature" is unusable: the planes' points
        """
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        axis = L.f32c(Axis).reshape(3) if Axis is not None else None
        L.check(L.lib().pcgx_kdtree_planes_dev(
            self._h, opt(d_samples), int(NHyp), int(MaxPlanes), float(MaxDist), int(MinInliers),
            L.ptr(axis) if axis is not None else None, float(MinAxisCos), opt(d_normals), float(MinNormalCos),
            int(bool(Refine)), opt(d_n_planes), opt(d_planes), opt(d_sizes), opt(d_refined), opt(d_best), opt(d_labels),
            opt(d_ids), opt(d_status), opt(d_counts), opt(d_hyp_planes), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): cylinder and sphere segmentation from oriented pairs
    def Shapes(self, Kind, MaxDist, Normals, NHyp=256, MaxShapes=1, MinInliers=2, SampleRadius=0.0, RMin=0.0,
               RMax=float("inf"), Axis=None, MinAxisCos=0.0, MinNormalCos=0.0, Refine=True, Samples=None, Seed=0):
        """The sphere (Kind 0) or cylinder (Kind 1) most of the tree's live points lie within MaxDist of, by sample
        consensus over NHyp hypotheses made from two oriented points -- a seed and a partner out of its SampleRadius
        neighbourhood (0: out of everything that is left); its inliers are taken out and the next shape is looked for,
        up to MaxShapes times, until a round's best has fewer than max(MinInliers, 2) inliers -> ShapeSegments(n_shapes,
        shapes float32 (MaxShapes, 8) as (cx, cy, cz, r, 0, 0, 0, 0) or (qx, qy, qz, r, ax, ay, az, 0), sizes int64,
        refined int32, best int64, labels int64 (n,), ids int64 (sum(sizes),), status int32 (MaxShapes, NHyp), counts
        int64, hyp_shapes float32 (MaxShapes, NHyp, 8)).  Normals (n, 3) are mandatory; RMin <= r <= RMax; Axis: only
        cylinders whose axis has |cos| >= MinAxisCos with it; an inlier's normal has |cos| >= MinNormalCos with the
        shape's; Refine: the best's centre and radius are refitted once to its inliers and kept where that loses no
        inlier.  Samples: uint32 (MaxShapes, NHyp, 2) random words, drawn from np.random.default_rng(Seed) when None
        (include/pcgx.h, pcgx_kdtree_shapes)."""
        n, nh, mp = self.Len(), int(NHyp), int(MaxShapes)
        if Samples is None:
            Samples = np.random.default_rng(Seed).integers(0, 2 ** 32, (max(mp, 0), max(nh, 0), 2),
                                                           dtype=np.uint64).astype(np.uint32)
        smp = np.ascontiguousarray(Samples, np.uint32).reshape(-1)
        if nh > 0 and mp > 0 and len(smp) != 2 * nh * mp:
            raise ValueError("two sample words per hypothesis and round are required")
        nrm = axis = None
        if Normals is not None:
            nrm = L.f32c(Normals).reshape(-1, 3)
            if len(nrm) != n:
                raise ValueError("one normal per point of the tree is required")
        if Axis is not None:
            axis = L.f32c(Axis).reshape(3)
        rows = max(nh, 0) * max(mp, 0)
        out = ShapeSegments(0, np.zeros((max(mp, 0), 8), np.float32), np.zeros(max(mp, 0), np.int64),
                            np.zeros(max(mp, 0), np.int32), np.full(max(mp, 0), -1, np.int64), np.full(n, -1, np.int64),
                            np.full(n, -1, np.int64), np.full(rows, -1, np.int32), np.zeros(rows, np.int64),
                            np.zeros((rows, 8), np.float32))
        cnt = C.c_int64()
        opt = lambda a: L.ptr(a) if a is not None and a.size else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_shapes(
            self._h, int(Kind), opt(smp), nh, mp, float(MaxDist), int(MinInliers), float(SampleRadius), float(RMin),
            float(RMax), opt(axis), float(MinAxisCos), L.ptr(nrm) if nrm is not None else None, float(MinNormalCos),
            int(bool(Refine)), C.byref(cnt), opt(out.shapes), opt(out.sizes), opt(out.refined), opt(out.best),
            opt(out.labels), opt(out.ids), opt(out.status), opt(out.counts), opt(out.hyp_shapes)))
        k = int(out.sizes[:cnt.value].sum())
        return out._replace(n_shapes=int(cnt.value), ids=out.ids[:k], status=out.status.reshape(mp, nh),
                            counts=out.counts.reshape(mp, nh), hyp_shapes=out.hyp_shapes.reshape(mp, nh, 8))

    def ShapesDev(self, Kind, MaxDist, d_normals, d_samples, NHyp, d_n_shapes, d_shapes, d_sizes, d_refined, d_best,
                  d_labels, d_ids=0, d_status=0, d_counts=0, d_hyp_shapes=0, MaxShapes=1, MinInliers=2, SampleRadius=0.0,
                  RMin=0.0, RMax=float("inf"), Axis=None, MinAxisCos=0.0, MinNormalCos=0.0, Refine=True, stream=0):
        """Device-resident Shapes: raw device addresses (e.g. torch .data_ptr()); d_normals float32 [3 Len()] (what
        NormalsDev writes), d_samples uint32 [2 NHyp MaxShapes], d_n_shapes one int32, d_shapes float32 [8 MaxShapes],
        d_sizes / d_refined / d_best int32 [MaxShapes], d_labels int32 [Len()], d_ids int32 [Len()] (the inliers shape
        by shape, then -1), d_status / d_counts int32 [MaxShapes NHyp], d_hyp_shapes float32 [8 MaxShapes NHyp]; Axis
        stays a host value.  Enqueued on `stream`, returns without waiting; nothing is read back.  d_ids, d_sizes and
        d_n_shapes are a grouped list for GroupStatsDev and GroupHullsDev (cap_ids = Len(), cap_groups = MaxShapes)."""
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        axis = L.f32c(Axis).reshape(3) if Axis is not None else None
        L.check(L.lib().pcgx_kdtree_shapes_dev(
            self._h, int(Kind), opt(d_samples), int(NHyp), int(MaxShapes), float(MaxDist), int(MinInliers),
            float(SampleRadius), float(RMin), float(RMax), L.ptr(axis) if axis is not None else None, float(MinAxisCos),
            opt(d_normals), float(MinNormalCos), int(bool(Refine)), opt(d_n_shapes), opt(d_shapes), opt(d_sizes),
            opt(d_refined), opt(d_best), opt(d_labels), opt(d_ids), opt(d_status), opt(d_counts), opt(d_hyp_shapes),
            L.ptr(stream) if stream else None))

    # -- extension (no reference parity): ground segmentation, a progressive morphological filter on a grid
    def GroundGrid(self, CellSize):
        """The grid Ground takes when none is given: origin = (min x, min y) of the live points (not deleted, finite),
        dims = floor((max - origin) / CellSize) + 1, in float32 -> (origin float32 (2,), dims int32 (2,))."""
        ids = self.InOrder()
        pts = np.empty((len(ids), 3), np.float32)
        if len(ids):
            L.check(L.lib().pcgx_kdtree_points(self._h, L.ptr(ids), len(ids), L.ptr(pts)))
        pts = pts[np.isfinite(pts).all(axis=1)]
        if not len(pts):
            return np.zeros(2, np.float32), np.ones(2, np.int32)
        lo, hi = pts[:, :2].min(axis=0), pts[:, :2].max(axis=0)
        with np.errstate(over="ignore"):
            dims = np.floor((hi - lo) / np.float32(CellSize)) + np.float32(1)
        return lo, np.clip(dims, 1, 2.0 ** 30).astype(np.int32)

    def Ground(self, CellSize, Half, Height, Origin=None, Dims=None):
        """Ground segmentation by a progressive morphological filter: the minimum z surface of the live points over a
        grid of CellSize cells (Origin (x, y), Dims (nx, ny); left out: GroundGrid's) is opened with squares of
        half-widths Half[k] cells one after the other, and a point is ground iff z - surface_k < Height[k] after every
        window k (segmentation.pmf_windows makes such a schedule) -> GroundSegments(labels int64 (n,) 0 ground, 1 not,
        -1 no part; sizes int64 (2,); ids int64 (sum(sizes),) the ground ascending, then the rest; n_groups 2; window
        int32 (n,) the first window failed or -1; surface float32 (ny, nx) the terrain model, +inf at an empty cell;
        hag float32 (n,) the height above it; origin, dims as used) (include/pcgx.h, pcgx_kdtree_ground)."""
        n = self.Len()
        half = np.ascontiguousarray(Half, np.int32).reshape(-1)
        height = np.ascontiguousarray(Height, np.float32).reshape(-1)
        if len(half) != len(height):
            raise ValueError("one height per window is required")
        if Origin is None or Dims is None:
            o, d = self.GroundGrid(CellSize)
            Origin = o if Origin is None else Origin
            Dims = d if Dims is None else Dims
        origin = np.ascontiguousarray(Origin, np.float32).reshape(2)
        dims = np.ascontiguousarray(Dims, np.int32).reshape(2)
        cells = int(dims[0]) * int(dims[1]) if 0 < dims[0] <= 8192 and 0 < dims[1] <= 8192 else 0
        out = GroundSegments(np.full(n, -1, np.int64), np.zeros(2, np.int64), np.full(n, -1, np.int64), 0,
                             np.full(n, -1, np.int32), np.full(cells, np.inf, np.float32), np.full(n, np.nan, np.float32),
                             origin, dims)
        cnt = C.c_int64()
        opt = lambda a: L.ptr(a) if a.size else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_ground(
            self._h, L.ptr(origin), L.ptr(dims), float(CellSize), len(half), opt(half), opt(height), opt(out.labels),
            L.ptr(out.sizes), opt(out.ids), C.byref(cnt), opt(out.window), opt(out.surface), opt(out.hag)))
        return out._replace(ids=out.ids[:int(out.sizes.sum())], n_groups=int(cnt.value),
                            surface=out.surface.reshape(int(dims[1]), int(dims[0])))

    def GroundDev(self, CellSize, Half, Height, Origin, Dims, d_labels, d_sizes, d_ids, d_n_groups, d_window=0,
                  d_surface=0, d_hag=0, stream=0):
        """Device-resident Ground: raw device addresses (e.g. torch .data_ptr()); Half, Height, Origin and Dims stay
        host values (the caller gives the grid, so nothing is read back); d_labels and d_ids int32 [Len()], d_sizes
        int32 [2], d_n_groups one int32 (always 2), d_window int32 [Len()], d_surface float32 [nx ny], d_hag float32
        [Len()] (0: not wanted).  Enqueued on `stream`, returns without waiting: every window is enqueued at once.
        d_ids, d_sizes and d_n_groups are a grouped list for GroupStatsDev and GroupHullsDev (cap_ids = Len(),
        cap_groups = 2)."""
        half = np.ascontiguousarray(Half, np.int32).reshape(-1)
        height = np.ascontiguousarray(Height, np.float32).reshape(-1)
        if len(half) != len(height):
            raise ValueError("one height per window is required")
        origin = np.ascontiguousarray(Origin, np.float32).reshape(2)
        dims = np.ascontiguousarray(Dims, np.int32).reshape(2)
        opt = lambda a: L.ptr(int(a)) if a else None  # noqa: E731
        L.check(L.lib().pcgx_kdtree_ground_dev(
            self._h, L.ptr(origin), L.ptr(dims), float(CellSize), len(half), L.ptr(half) if len(half) else None,
            L.ptr(height) if len(height) else None, opt(d_labels), opt(d_sizes), opt(d_ids), opt(d_n_groups),
            opt(d_window), opt(d_surface), opt(d_hag), L.ptr(stream) if stream else None))

    # -- extension (no reference parity): k nearest neighbours
    def KNearest(self, p, k, maxRange):
        """The k points with the smallest (DistSq, ID) among those with DistSq < maxRange^2, ascending ->
        [Neighbor] of length <= k (include/pcgx.h, pcgx_kdtree_knearest: ties go by ID)."""
        ids, dsq, counts = self.KNearestBatch(np.asarray(p, np.float32).reshape(1, 3), k, maxRange)
        return [Neighbor(i, d) for i, d in zip(ids[0, :counts[0]], dsq[0, :counts[0]])]

    def KNearestBatch(self, q, k, maxRange):
        """KNearest for every row of q (None: the tree's own points, in id order) -> (ids int64 (n, k),
        distSq float32 (n, k), counts int32 (n,)); slots past counts[i] are {-1, maxRange^2}."""
        q = None if q is None else L.f32c(q).reshape(-1, 3)
        n = self.Len() if q is None else len(q)
        ids = np.empty((n, k), np.int64)
        dsq = np.empty((n, k), np.float32)
        counts = np.empty(n, np.int32)
        L.check(L.lib().pcgx_kdtree_knearest(self._h, L.ptr(q), n, int(k), float(maxRange), L.ptr(ids), L.ptr(dsq),
                                             L.ptr(counts)))
        return ids, dsq, counts

    def KNearestDev(self, k, maxRange, d_ids, d_dsq, d_counts=0, d_q=0, nq=None, stream=0):
        """Device-resident KNearestBatch: raw device addresses (e.g. torch .data_ptr()); ids int32 [nq * k]; d_q 0
        takes the tree's own points (nq = Len()).  Enqueued on `stream`, returns without waiting."""
        if nq is None:
            if d_q:
                raise ValueError("nq is required with d_q")
            nq = self.Len()
        L.check(L.lib().pcgx_kdtree_knearest_dev(
            self._h, L.ptr(int(d_q)) if d_q else None, int(nq), int(k), float(maxRange), L.ptr(int(d_ids)),
            L.ptr(int(d_dsq)), L.ptr(int(d_counts)) if d_counts else None, L.ptr(stream) if stream else None))

    # -- extension (no reference parity): covariances of k-NN neighbourhoods (Generalized ICP's input)
    def Covariances(self, k, MaxRange=np.inf, Mode="plane", Epsilon=1e-3, Queries=None, Viewpoint=None):
        """Covariance of the k nearest neighbours (KNearestBatch's lists) of every query -> (cov (n,6) float32 as xx,
        xy, xz, yy, yz, zz; normals (n,3) float32; counts (n,) int32).  Mode "plane": I - (1 - Epsilon) u u^T, u the
        unit normal (Segal's GICP regularisation); "raw": the covariance as it is.  Fewer than 3 neighbours, or all
        at one place: I ("plane") / 0 ("raw"), normal 0.  Where the float64 trace of the covariance rounds to <= 0
        (neighbours whose spread is below ~1e-8 of their distance from the query): I ("plane") and normal 0 as well,
        "raw" the covariance as computed.  Queries None: the tree's own points, in id order;
        Viewpoint None: the origin (include/pcgx.h, pcgx_kdtree_covariances).  The normals always come back, so
        "raw" runs the eigen-solve too; CovariancesDev without d_normals skips it."""
        q = None if Queries is None else L.f32c(Queries).reshape(-1, 3)
        n = self.Len() if q is None else len(q)
        vp = None if Viewpoint is None else L.f32c(Viewpoint).reshape(3)
        cov = np.empty((n, 6), np.float32)
        normals = np.empty((n, 3), np.float32)
        counts = np.empty(n, np.int32)
        L.check(L.lib().pcgx_kdtree_covariances(self._h, L.ptr(q), n, int(k), float(MaxRange), _cov_mode(Mode),
                                                float(Epsilon), L.ptr(vp), L.ptr(cov), L.ptr(normals), L.ptr(counts)))
        return cov, normals, counts

    def CovariancesDev(self, k, d_cov6, d_normals=0, d_counts=0, d_q=0, nq=None, MaxRange=np.inf, Mode="plane",
                       Epsilon=1e-3, Viewpoint=None, stream=0):
        """Device-resident Covariances: raw device addresses (e.g. torch .data_ptr()); d_q 0 takes the tree's own
        points (nq = Len()).  Enqueued on `stream`, returns without waiting."""
        if nq is None:
            if d_q:
                raise ValueError("nq is required with d_q")
            nq = self.Len()
        vp = None if Viewpoint is None else L.f32c(Viewpoint).reshape(3)
        L.check(L.lib().pcgx_kdtree_covariances_dev(
            self._h, L.ptr(int(d_q)) if d_q else None, int(nq), int(k), float(MaxRange), _cov_mode(Mode),
            float(Epsilon), L.ptr(vp), L.ptr(int(d_cov6)), L.ptr(int(d_normals)) if d_normals else None,
            L.ptr(int(d_counts)) if d_counts else None, L.ptr(stream) if stream else None))

    def NearestBatchDev(self, d_q, nq, maxRange, d_ids, d_dsq, presort=True, stream=0):
        """Device-resident variant: raw device addresses (e.g. torch .data_ptr())."""
        L.check(L.lib().pcgx_kdtree_nearest_batch_dev(
            self._h, L.ptr(d_q), nq, maxRange, self.MinDistSq, L.PCGX_KNN_PRESORT if presort else 0,
            L.ptr(d_ids), L.ptr(d_dsq), L.ptr(stream) if stream else None))


def _cov_mode(mode):
    """"plane" / "raw" (or the PCGX_COV_* value) -> pcgx_kdtree_covariances' mode"""
    if isinstance(mode, str):
        if mode not in ("plane", "raw"):
            raise ValueError("Mode must be 'plane' or 'raw', not %r" % mode)
        return L.PCGX_COV_PLANE if mode == "plane" else L.PCGX_COV_RAW
    return int(mode)


New = KDTree.New
