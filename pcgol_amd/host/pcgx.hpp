// pcgx.hpp -- header-only C++ mirror of the reference's Go interfaces on the
// hot path, over the C ABI (include/pcgx.h).  The reference is compiled code
// (Go) whose toolchain is absent from the build image, so the host side above
// the C ABI is mirrored in C++ (and in Python, pcgol_amd/*.py, for the tests):
// same names, argument meaning and error behaviour.
//
//   pcgx::KDTree            <- pc/storage/kdtree.KDTree      (storage.Search)
//   pcgx::VoxelGrid         <- pc/filter/voxelgrid.New(...)  (filter.Filter)
//   pcgx::PointToPointICP   <- icp.PointToPointICPGradient{Evaluator, UpdaterFactory}
//   pcgx::BucketVoxelGrid   <- pc/storage/voxelgrid.VoxelGrid + pc/segmentation/voxelgrid (Segment)
//   pcgx::RegionGrowing     <- pc/segmentation/regiongrowing.RegionGrowing
//   pcgx::sac::SAC          <- pc/sac.SAC over NewVoxelGridSurfaceModel (the plane model of a BucketVoxelGrid)
//   pcgx::PointToPlaneICP   <- (extension, no counterpart in the reference) the same Fit shape with
//                              the point-to-plane evaluator / Gauss-Newton updater, HasHessian() == true
//   pcgx::GeneralizedICP    <- (extension, no counterpart in the reference) Generalized ICP over the k-NN
//                              covariances of both clouds (KDTree::Covariances), the same Fit shape
//   pcgx::StatisticalOutlierRemoval <- (extension, no counterpart) a filter.Filter on k-nearest distances
//   pcgx::Comm              <- (no counterpart: the reference is one process) the exchange of the
//                              several-GPU paths: PointToPointICP::FitSharded, VoxelGrid::FilterSharded
#pragma once
#include <array>
#include <functional>
#include <initializer_list>
#include <limits>
#include <memory>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pcgx.h"

namespace pcgx {

struct Error : std::runtime_error {
  pcgx_status code;
  Error(pcgx_status c, const std::string &m) : std::runtime_error(m), code(c) {}
};
struct ErrNoPoint : Error { using Error::Error; };          // pc/minmax.go:11
struct ErrNotEnoughPairs : Error { using Error::Error; };   // icp/evaluator.go:16
struct ErrSingular : Error { using Error::Error; };         // point-to-plane extension

inline void check(pcgx_status rc) {
  if (rc == PCGX_OK) return;
  char buf[512];
  pcgx_last_error(buf, sizeof buf);
  if (rc == PCGX_E_NO_POINT) throw ErrNoPoint(rc, buf);
  if (rc == PCGX_E_NOT_ENOUGH_PAIRS) throw ErrNotEnoughPairs(rc, buf);
  if (rc == PCGX_E_SINGULAR) throw ErrSingular(rc, buf);
  throw Error(rc, buf);
}

using Vec3 = std::array<float, 3>;   // mat.Vec3
using Mat4 = std::array<float, 16>;  // mat.Mat4, column-major

struct Neighbor {  // pc/storage/search.go:8-11
  int64_t ID;
  float DistSq;
};

// pc.PointCloud's layout contract (pc/pointcloud.go:64-78): AoS records.
struct CloudView {
  const void *data;
  int64_t points;
  int32_t stride, xyz_offset;
};

// The exchange between the ranks of a several-GPU run (one process per GPU, include/pcgx.h
// "sharded"): RCCL inside the library from an id that rank 0 makes and the host passes on, or a host
// function that sums `count` float64 in place over the ranks.
class Comm {
 public:
  static pcgx_comm_id UniqueId() { pcgx_comm_id id; check(pcgx_comm_unique_id(&id)); return id; }
  Comm(int rank, int world, const pcgx_comm_id &id) { check(pcgx_comm_init(rank, world, &id, &h_)); }
  Comm(int rank, int world, pcgx_allreduce_fn fn, void *user) { check(pcgx_comm_init_callback(rank, world, fn, user, &h_)); }
  ~Comm() { pcgx_comm_free(h_); }
  Comm(const Comm &) = delete;
  Comm &operator=(const Comm &) = delete;
  int Rank() const { int32_t r, w; check(pcgx_comm_rank(h_, &r, &w)); return r; }
  int World() const { int32_t r, w; check(pcgx_comm_rank(h_, &r, &w)); return w; }
  pcgx_comm *handle() const { return h_; }

 private:
  pcgx_comm *h_ = nullptr;
};

// the struct layouts this header was compiled against must be the library's (call once after loading it)
inline void CheckAbi() {
  if (pcgx_abi_version() != PCGX_ABI_VERSION)
    throw Error(PCGX_E_INVALID, "libpcgx.so speaks another ABI version than the pcgx.h this program was built against");
}

class KDTree;
// kdtree.KDTreeOption (kdtree.go:31): New(ra, opts...) / (*KDTree).With(opts...) apply them to the tree value.
using KDTreeOption = std::function<void(KDTree &)>;

class KDTree {  // pc/storage/kdtree/kdtree.go:14-23
 public:
  float MinDistSq = 0.0f;
  explicit KDTree(const CloudView &c, std::initializer_list<KDTreeOption> opts = {}) {
    pcgx_kdtree *h = nullptr;
    check(pcgx_kdtree_build(c.data, c.points, c.stride, c.xyz_offset, &h));
    h_ = std::shared_ptr<pcgx_kdtree>(h, [](pcgx_kdtree *p) { pcgx_kdtree_free(p); });
    for (const auto &o : opts) o(*this);
  }
  explicit KDTree(const std::vector<Vec3> &pts, std::initializer_list<KDTreeOption> opts = {})
      : KDTree(CloudView{pts.data(), (int64_t)pts.size(), 12, 0}, opts) {}
  // With (kdtree.go:58-65): a shallow copy with the options applied; the copies share the device tree.
  KDTree With(std::initializer_list<KDTreeOption> opts) const {
    KDTree k2(*this);
    for (const auto &o : opts) o(k2);
    return k2;
  }
  static KDTreeOption WithMinDistSq(float d) { return [d](KDTree &k) { k.MinDistSq = d; }; }
  int64_t Len() const { int64_t n; check(pcgx_kdtree_len(h_.get(), &n)); return n; }
  Vec3 Vec3At(int64_t i) const { Vec3 v; check(pcgx_kdtree_points(h_.get(), &i, 1, v.data())); return v; }
  Neighbor Nearest(const Vec3 &p, float maxRange) const { return NearestBatch({p}, maxRange)[0]; }
  std::vector<Neighbor> NearestBatch(const std::vector<Vec3> &q, float maxRange) const {
    std::vector<int64_t> ids(q.size());
    std::vector<float> d(q.size());
    check(pcgx_kdtree_nearest_batch(h_.get(), q.empty() ? nullptr : q[0].data(), (int64_t)q.size(), maxRange, MinDistSq,
                                    ids.data(), d.data()));
    std::vector<Neighbor> out(q.size());
    for (size_t i = 0; i < q.size(); i++) out[i] = Neighbor{ids[i], d[i]};
    return out;
  }
  // KDTree.Range (kdtree.go:148-197): neighbours with DistSq < maxRange^2, sorted by DistSq.
  std::vector<Neighbor> Range(const Vec3 &p, float maxRange) const {
    int64_t cnt = 0;
    check(pcgx_kdtree_range_count(h_.get(), p.data(), 1, maxRange, &cnt));
    const int64_t offs[2] = {0, cnt};
    std::vector<int64_t> ids((size_t)cnt);
    std::vector<float> d((size_t)cnt);
    check(pcgx_kdtree_range_fill(h_.get(), p.data(), 1, maxRange, offs, ids.data(), d.data()));
    std::vector<Neighbor> out((size_t)cnt);
    for (int64_t i = 0; i < cnt; i++) out[(size_t)i] = Neighbor{ids[(size_t)i], d[(size_t)i]};
    return out;
  }
  // KDTree.DeletePoint (kdtree.go:322-332); std::out_of_range for an id outside [0, Len()).
  void DeletePoint(int64_t pID) {
    pcgx_status rc = pcgx_kdtree_delete_points(h_.get(), &pID, 1);
    if (rc == PCGX_E_OUT_OF_RANGE) {
      char buf[256];
      pcgx_last_error(buf, sizeof buf);
      throw std::out_of_range(buf);
    }
    check(rc);
  }
  int32_t MaxDepth() const { int32_t d; check(pcgx_kdtree_max_depth(h_.get(), &d)); return d; }
  // Surface normals from radius neighbourhoods (extension: no reference parity; include/pcgx.h,
  // pcgx_kdtree_normals).  An empty `queries` takes the tree's own points: the result is in id order, the
  // baseNormals PointToPlaneICP::Fit takes.  Degenerate points: normal {0, 0, 0}, curvature NaN.
  struct NormalsResult {
    std::vector<Vec3> normals;
    std::vector<float> curvature;
    std::vector<int32_t> counts;
  };
  NormalsResult Normals(float radius, const Vec3 &viewpoint = Vec3{0.0f, 0.0f, 0.0f}, int32_t minNeighbors = 3,
                        const std::vector<Vec3> &queries = {}) const {
    const bool own = queries.empty();
    const int64_t n = own ? Len() : (int64_t)queries.size();
    NormalsResult r;
    r.normals.resize((size_t)n);
    r.curvature.resize((size_t)n);
    r.counts.resize((size_t)n);
    check(pcgx_kdtree_normals(h_.get(), own ? nullptr : queries[0].data(), n, radius, viewpoint.data(), minNeighbors,
                              n ? r.normals[0].data() : nullptr, r.curvature.data(), r.counts.data()));
    return r;
  }
  // Moving-least-squares smoothing over radius neighbourhoods (extension: no reference parity; include/pcgx.h,
  // pcgx_kdtree_mls): every query projected onto the plane (order 1) or the quadratic height field (order 2) fitted to
  // its neighbourhood with Gauss weights of width sigma (<= 0: the radius).  An empty `queries` takes the tree's own
  // points, in id order.  kinds: PCGX_MLS_UNCHANGED (the query came back as it was, normal {0, 0, 0}), _PLANE, _POLY.
  struct MLSResult {
    std::vector<Vec3> points;
    std::vector<Vec3> normals;
    std::vector<int32_t> kinds;
    std::vector<int32_t> counts;
  };
  MLSResult MLS(float radius, float sigma = 0.0f, int32_t order = 2, int32_t minNeighbors = 3,
                const Vec3 &viewpoint = Vec3{0.0f, 0.0f, 0.0f}, const std::vector<Vec3> &queries = {}) const {
    const bool own = queries.empty();
    const int64_t n = own ? Len() : (int64_t)queries.size();
    MLSResult r;
    r.points.resize((size_t)n);
    r.normals.resize((size_t)n);
    r.kinds.resize((size_t)n);
    r.counts.resize((size_t)n);
    check(pcgx_kdtree_mls(h_.get(), own ? nullptr : queries[0].data(), n, radius, sigma > 0.0f ? sigma : radius, order,
                          minNeighbors, viewpoint.data(), n ? r.points[0].data() : nullptr,
                          n ? r.normals[0].data() : nullptr, r.kinds.data(), r.counts.data()));
    return r;
  }
  // FPFH descriptors of the tree's own points over radius neighbourhoods (extension: no reference parity;
  // include/pcgx.h, pcgx_kdtree_fpfh).  `normals`: one per point in id order, e.g. Normals(radius).normals.  counts:
  // the valid pairs per feature and bin (3 x 11, feature major), pairs: how many there are.  All in id order.
  struct FPFHResult {
    std::vector<std::array<float, 33>> fpfh;
    std::vector<std::array<int32_t, 33>> counts;
    std::vector<int32_t> pairs;
  };
  FPFHResult FPFH(float radius, const std::vector<Vec3> &normals) const {
    const int64_t n = Len();
    if ((int64_t)normals.size() != n) throw Error(PCGX_E_INVALID, "one normal per point of the tree is required");
    FPFHResult r;
    r.fpfh.resize((size_t)n);
    r.counts.resize((size_t)n);
    r.pairs.resize((size_t)n);
    check(pcgx_kdtree_fpfh(h_.get(), n ? normals[0].data() : nullptr, radius, n ? r.fpfh[0].data() : nullptr,
                           n ? r.counts[0].data() : nullptr, r.pairs.data()));
    return r;
  }
  // FPFH's rows at the listed point ids only (extension: no reference parity; include/pcgx.h, pcgx_kdtree_fpfh_at):
  // row s is FPFH(radius, normals)'s row ids[s] bit for bit, xyz[s] that point.  Ids in any order, repeats allowed; an
  // id outside [0, Len()) throws.  nSpfh: the points whose SPFH record had to be computed -- the listed points and
  // their neighbours, not the cloud.
  struct FPFHAtResult {
    std::vector<std::array<float, 33>> fpfh;
    std::vector<Vec3> xyz;
    std::vector<std::array<int32_t, 33>> counts;
    std::vector<int32_t> pairs;
    int64_t nSpfh = 0;
  };
  FPFHAtResult FPFHAt(float radius, const std::vector<Vec3> &normals, const std::vector<int64_t> &ids) const {
    const int64_t n = Len(), k = (int64_t)ids.size();
    if ((int64_t)normals.size() != n) throw Error(PCGX_E_INVALID, "one normal per point of the tree is required");
    FPFHAtResult r;
    r.fpfh.resize((size_t)k);
    r.xyz.resize((size_t)k);
    r.counts.resize((size_t)k);
    r.pairs.resize((size_t)k);
    check(pcgx_kdtree_fpfh_at(h_.get(), n ? normals[0].data() : nullptr, radius, ids.data(), k,
                              k ? r.fpfh[0].data() : nullptr, k ? r.xyz[0].data() : nullptr,
                              k ? r.counts[0].data() : nullptr, r.pairs.data(), &r.nSpfh));
    return r;
  }
  // The points whose score is the largest of their radius neighbourhood, ascending ids (extension: no reference
  // parity; include/pcgx.h, pcgx_kdtree_local_maxima).  `score`: one per point in id order; only a score > 0
  // qualifies, ties go to the smaller id.
  std::vector<int64_t> LocalMaxima(float radius, const std::vector<float> &score) const {
    const int64_t n = Len();
    if ((int64_t)score.size() != n) throw Error(PCGX_E_INVALID, "one score per point of the tree is required");
    std::vector<int64_t> ids((size_t)n);
    int64_t m = 0;
    check(pcgx_kdtree_local_maxima(h_.get(), radius, score.data(), ids.data(), &m));
    ids.resize((size_t)m);
    return ids;
  }
  // Minimum-distance subsampling (extension: no reference parity; include/pcgx.h, pcgx_kdtree_thin): a maximal subset of
  // the tree's own points no two of which are within radius, the one greedy selection keeps -- by hash(seed, id) where
  // `score` is empty, else the larger score first, ties to the smaller id.  ids: ascending; owner (id order, filled
  // where withOwner): a kept point itself, a dropped point its kept neighbour of the smallest (DistSq, id), -1 for a
  // point that takes no part.
  struct ThinResult {
    std::vector<int64_t> ids, owner;
  };
  ThinResult Thin(float radius, uint32_t seed = 0, const std::vector<float> &score = {}, bool withOwner = false) const {
    const int64_t n = Len();
    if (!score.empty() && (int64_t)score.size() != n) throw Error(PCGX_E_INVALID, "one score per point of the tree is required");
    ThinResult r;
    r.ids.resize((size_t)n);
    if (withOwner) r.owner.resize((size_t)n);
    int64_t m = 0;
    check(pcgx_kdtree_thin(h_.get(), radius, seed, score.empty() ? nullptr : score.data(), r.ids.data(), &m,
                           withOwner ? r.owner.data() : nullptr));
    r.ids.resize((size_t)m);
    return r;
  }
  // Farthest-point sampling (extension: no reference parity; include/pcgx.h, pcgx_kdtree_fps): `count` of the tree's own
  // points in pick order, each the one farthest (float32 DistSq to the nearest pick so far, ties to the smallest id)
  // from those before it; start: the first pick, -1 for the smallest eligible id.  ids and distSq have min(count,
  // eligible points) entries and are a prefix of what a larger count gives; distSq[0] is +inf; coverSq: the d the next
  // pick would have had, -1 when no point is left; owner (id order, filled where withOwner): the nearest pick's id, the
  // earlier pick among equal distances, -1 for a deleted or non-finite point.
  struct FarthestResult {
    std::vector<int64_t> ids, owner;
    std::vector<float> distSq;
    float coverSq = -1.0f;
  };
  FarthestResult FarthestPoints(int64_t count, int64_t start = -1, bool withOwner = false) const {
    if (count < 0) throw Error(PCGX_E_INVALID, "count must be >= 0");
    FarthestResult r;
    r.ids.resize((size_t)count);
    r.distSq.resize((size_t)count);
    if (withOwner) r.owner.resize((size_t)Len());
    int64_t m = 0;
    check(pcgx_kdtree_fps(h_.get(), count, start, r.ids.data(), &m, r.distSq.data(), &r.coverSq,
                          withOwner ? r.owner.data() : nullptr));
    r.ids.resize((size_t)m);
    r.distSq.resize((size_t)m);
    return r;
  }
  // ISS keypoints (extension: no reference parity; include/pcgx.h, pcgx_kdtree_iss_keypoints).  eigenvalues: of
  // Normals' covariance at salientRadius, ascending, {0, 0, 0} where Normals answers "degenerate"; saliency: the
  // smallest eigenvalue of a salient point, else 0; ids: LocalMaxima(nonMaxRadius, saliency).  All in id order.
  struct ISSResult {
    std::vector<int64_t> ids;
    std::vector<Vec3> eigenvalues;
    std::vector<float> saliency;
  };
  ISSResult ISSKeypoints(float salientRadius, float nonMaxRadius, float gamma21 = 0.975f, float gamma32 = 0.975f,
                         int32_t minNeighbors = 5) const {
    const int64_t n = Len();
    ISSResult r;
    r.ids.resize((size_t)n);
    r.eigenvalues.resize((size_t)n);
    r.saliency.resize((size_t)n);
    int64_t m = 0;
    check(pcgx_kdtree_iss_keypoints(h_.get(), salientRadius, nonMaxRadius, gamma21, gamma32, minNeighbors,
                                    n ? r.eigenvalues[0].data() : nullptr, r.saliency.data(), r.ids.data(), &m));
    r.ids.resize((size_t)m);
    return r;
  }
  // Boundary points (extension: no reference parity; include/pcgx.h, pcgx_kdtree_boundary): the points whose radius
  // neighbours leave an angular gap of at least minGap sectors of 5.625 degrees in the tangent plane of `normals` (one
  // per point in id order).  ids ascending; gaps: the longest cyclic run of empty sectors, 64 for an empty mask, -1 where
  // the point is not evaluated; masks: bit s set where a neighbour falls in sector s; counts: the neighbourhood's size.
  struct BoundaryResult {
    std::vector<int64_t> ids;
    std::vector<int32_t> gaps, counts;
    std::vector<uint64_t> masks;
  };
  BoundaryResult Boundary(float radius, const std::vector<Vec3> &normals, int32_t minGap = 16,
                          int32_t minNeighbors = 1) const {
    const int64_t n = Len();
    if ((int64_t)normals.size() != n) throw Error(PCGX_E_INVALID, "one normal per point of the tree is required");
    BoundaryResult r;
    r.ids.resize((size_t)n);
    r.gaps.resize((size_t)n);
    r.masks.resize((size_t)n);
    r.counts.resize((size_t)n);
    int64_t m = 0;
    check(pcgx_kdtree_boundary(h_.get(), radius, n ? normals[0].data() : nullptr, minGap, minNeighbors, r.ids.data(), &m,
                               r.gaps.data(), r.masks.data(), r.counts.data()));
    r.ids.resize((size_t)m);
    return r;
  }
  // Consistent normal orientation (extension: no reference parity; include/pcgx.h, pcgx_kdtree_orient_normals):
  // neighbouring normals (one per point in id order) get the same side, the sign carried along the minimum spanning
  // forest of the radius graph.  A component's overall sign: its smallest id keeps its own (OrientKeep); its topmost
  // point along ref looks along ref (OrientDirection); the majority of its normals looks towards ref (OrientViewpoint).
  // normals: the given bits, the signs inverted where flipped; component: the smallest id of the point's component, -1
  // for a point that takes no part.
  enum OrientMode : int32_t { OrientKeep = 0, OrientDirection = 1, OrientViewpoint = 2 };
  struct OrientResult {
    std::vector<Vec3> normals;
    std::vector<uint8_t> flipped;
    std::vector<int64_t> component;
    int64_t components = 0;
  };
  OrientResult OrientNormals(float radius, const std::vector<Vec3> &normals, OrientMode mode = OrientKeep,
                             const Vec3 &ref = Vec3{{0.0f, 0.0f, 0.0f}}) const {
    const int64_t n = Len();
    if ((int64_t)normals.size() != n) throw Error(PCGX_E_INVALID, "one normal per point of the tree is required");
    OrientResult r;
    r.normals.resize((size_t)n);
    r.flipped.resize((size_t)n);
    r.component.resize((size_t)n);
    int64_t open = 0;
    check(pcgx_kdtree_orient_normals(h_.get(), radius, n ? normals[0].data() : nullptr, (int32_t)mode, ref.data(),
                                     n ? r.normals[0].data() : nullptr, r.flipped.data(), r.component.data(),
                                     &r.components, &open));
    return r;
  }
  // Ray queries (extension: no reference parity; include/pcgx.h, pcgx_kdtree_raycast / _ray_pierce): ray j is
  // origins[j] + s directions[j], s in [sMin[j], sMax[j]] (an empty vector: 0 and +inf); directions are not normalised.
  // RayCast: per ray the first of the tree's points within `radius` of the ray's line -- ids (-1: none), along =
  // (p - o) . d and offSq = |(p - o) x d|^2 in float64 (0 for a miss), a tie in along going to the smallest id.
  // RayPierce: per point in id order, how many rays it lies in the tube of.
  struct RayHits {
    std::vector<int64_t> ids;
    std::vector<double> along, offSq;
  };
  RayHits RayCast(const std::vector<Vec3> &origins, const std::vector<Vec3> &directions, float radius,
                  const std::vector<float> &sMin = {}, const std::vector<float> &sMax = {}) const {
    const size_t nr = RayCount(origins, directions, sMin, sMax);
    RayHits r;
    r.ids.resize(nr);
    r.along.resize(nr);
    r.offSq.resize(nr);
    check(pcgx_kdtree_raycast(h_.get(), nr ? origins[0].data() : nullptr, nr ? directions[0].data() : nullptr,
                              sMin.empty() ? nullptr : sMin.data(), sMax.empty() ? nullptr : sMax.data(), (int64_t)nr, radius,
                              r.ids.data(), r.along.data(), r.offSq.data()));
    return r;
  }
  std::vector<int32_t> RayPierce(const std::vector<Vec3> &origins, const std::vector<Vec3> &directions, float radius,
                                 const std::vector<float> &sMin = {}, const std::vector<float> &sMax = {}) const {
    const size_t nr = RayCount(origins, directions, sMin, sMax);
    std::vector<int32_t> counts((size_t)Len(), 0);
    check(pcgx_kdtree_ray_pierce(h_.get(), nr ? origins[0].data() : nullptr, nr ? directions[0].data() : nullptr,
                                 sMin.empty() ? nullptr : sMin.data(), sMax.empty() ? nullptr : sMax.data(), (int64_t)nr,
                                 radius, counts.data()));
    return counts;
  }
  // Cylinder statistics (extension: no reference parity; include/pcgx.h, pcgx_kdtree_cylinder_stats): cylinder j has
  // the core cores[j], the axis axes[j] (not normalised), `radius` and `halfLength` each way along the axis.  counts:
  // the tree's live points in it; sums: S1 = sum of a and S2 = sum of a a at [2 j] and [2 j + 1], a = (p - core) . axis
  // in float64, unnormalised.  M3C2Finish (below the class) turns the statistics of two epochs into distances.
  struct CylinderStatsResult {
    std::vector<int32_t> counts;
    std::vector<double> sums;
  };
  CylinderStatsResult CylinderStats(const std::vector<Vec3> &cores, const std::vector<Vec3> &axes, float radius,
                                    float halfLength) const {
    const size_t m = cores.size();
    if (axes.size() != m) throw Error(PCGX_E_INVALID, "one axis per core is required");
    CylinderStatsResult r;
    r.counts.resize(m);
    r.sums.resize(2 * m);
    check(pcgx_kdtree_cylinder_stats(h_.get(), m ? cores[0].data() : nullptr, m ? axes[0].data() : nullptr, (int64_t)m,
                                     radius, halfLength, r.counts.data(), r.sums.data()));
    return r;
  }
  // Cluster extraction (extension: no reference parity; include/pcgx.h, pcgx_kdtree_clusters): the connected
  // components of the radius graph over the tree's own points, kept when max(minSize, 1) <= size (<= maxSize unless 0),
  // largest first, equal sizes by smallest id.  normals (empty: none): an edge also needs |n_i . n_j| >= minCos
  // (n_i . n_j when oriented); curvature (empty: none): a point above maxCurvature, or NaN, belongs to no cluster.
  // labels: per point its cluster's number or -1; sizes: per cluster; ids: cluster 0's members ascending, then cluster
  // 1's, ...; Members(c) cuts cluster c out of ids.
  struct ClustersResult {
    std::vector<int64_t> labels, sizes, ids;
    std::vector<int64_t> Members(size_t c) const {
      size_t at = 0;
      for (size_t k = 0; k < c; k++) at += (size_t)sizes[k];
      return std::vector<int64_t>(ids.begin() + (std::ptrdiff_t)at, ids.begin() + (std::ptrdiff_t)(at + (size_t)sizes[c]));
    }
  };
  ClustersResult Clusters(float radius, const std::vector<Vec3> &normals = {}, float minCos = 0.0f, bool oriented = false,
                          const std::vector<float> &curvature = {}, float maxCurvature = 0.0f, int64_t minSize = 1,
                          int64_t maxSize = 0) const {
    const int64_t n = Len();
    if (!normals.empty() && (int64_t)normals.size() != n)
      throw Error(PCGX_E_INVALID, "one normal per point of the tree is required");
    if (!curvature.empty() && (int64_t)curvature.size() != n)
      throw Error(PCGX_E_INVALID, "one curvature per point of the tree is required");
    ClustersResult r;
    r.labels.resize((size_t)n);
    r.sizes.resize((size_t)n);
    r.ids.resize((size_t)n);
    int64_t c = 0;
    check(pcgx_kdtree_clusters(h_.get(), radius, normals.empty() ? nullptr : normals[0].data(), minCos, oriented ? 1 : 0,
                               curvature.empty() ? nullptr : curvature.data(), maxCurvature, minSize, maxSize,
                               r.labels.data(), &c, r.sizes.data(), r.ids.data()));
    r.sizes.resize((size_t)c);
    size_t total = 0;
    for (int64_t s : r.sizes) total += (size_t)s;
    r.ids.resize(total);
    return r;
  }
  // Density clusters (extension: no reference parity; include/pcgx.h, pcgx_kdtree_dbscan): DBSCAN over the tree's own
  // points.  A point with at least minPts points within radius (DistSq < radius^2, itself included) is core; a cluster
  // is a component of core points plus its border points, each with its nearest core neighbour (smallest DistSq, then
  // smallest id).  labels, sizes and ids as Clusters (a DBSCANResult is a ClustersResult: GroupStats and GroupHulls
  // take it); kind: per point 0 noise, 1 border, 2 core, whatever the size range.
  struct DBSCANResult : ClustersResult {
    std::vector<uint8_t> kind;
  };
  DBSCANResult DBSCAN(float radius, int32_t minPts, int64_t minSize = 1, int64_t maxSize = 0) const {
    const int64_t n = Len();
    DBSCANResult r;
    r.labels.resize((size_t)n);
    r.sizes.resize((size_t)n);
    r.ids.resize((size_t)n);
    r.kind.resize((size_t)n);
    int64_t c = 0;
    check(pcgx_kdtree_dbscan(h_.get(), radius, minPts, minSize, maxSize, r.labels.data(), &c, r.sizes.data(), r.ids.data(),
                             r.kind.data()));
    r.sizes.resize((size_t)c);
    size_t total = 0;
    for (int64_t s : r.sizes) total += (size_t)s;
    r.ids.resize(total);
    return r;
  }
  // Plane segmentation (extension: no reference parity; include/pcgx.h, pcgx_kdtree_planes): the plane most live points
  // lie within maxDist of, by sample consensus over the caller's random words (samples: 3 per hypothesis and round,
  // nHyp * maxPlanes hypotheses), its inliers taken out, then the next, until a round's best has fewer than
  // max(minInliers, 3).  axis (nullptr: none): only planes whose normal has |cos| >= minAxisCos with it; normals (empty:
  // none): an inlier's normal has |cos| >= minNormalCos with the plane's.  labels, sizes and ids as Clusters (a
  // PlanesResult is a ClustersResult: GroupStats and GroupHulls take it), one group a plane in the order found; planes:
  // (nx, ny, nz, d) per plane; refined, best: per plane; status, counts, hypPlanes: per round and hypothesis.
  struct PlanesResult : ClustersResult {
    std::vector<float> planes, hypPlanes;
    std::vector<int32_t> refined, status;
    std::vector<int64_t> best, counts;
  };
  PlanesResult Planes(float maxDist, const std::vector<uint32_t> &samples, int64_t nHyp, int32_t maxPlanes = 1,
                      int64_t minInliers = 3, const float *axis = nullptr, float minAxisCos = 0.0f,
                      const std::vector<Vec3> &normals = {}, float minNormalCos = 0.0f, bool refine = true) const {
    const int64_t n = Len();
    if (!normals.empty() && (int64_t)normals.size() != n)
      throw Error(PCGX_E_INVALID, "one normal per point of the tree is required");
    if (nHyp > 0 && maxPlanes > 0 && (int64_t)samples.size() != 3 * nHyp * maxPlanes)
      throw Error(PCGX_E_INVALID, "three sample words per hypothesis and round are required");
    const size_t mp = maxPlanes > 0 ? (size_t)maxPlanes : 0, rows = nHyp > 0 ? mp * (size_t)nHyp : 0;
    PlanesResult r;
    r.labels.resize((size_t)n);
    r.ids.resize((size_t)n);
    r.sizes.resize(mp);
    r.planes.resize(4 * mp);
    r.refined.resize(mp);
    r.best.resize(mp);
    r.status.resize(rows);
    r.counts.resize(rows);
    r.hypPlanes.resize(4 * rows);
    int64_t c = 0;
    check(pcgx_kdtree_planes(h_.get(), samples.empty() ? nullptr : samples.data(), nHyp, maxPlanes, maxDist, minInliers, axis,
                             minAxisCos, normals.empty() ? nullptr : normals[0].data(), minNormalCos, refine ? 1 : 0, &c,
                             r.planes.data(), r.sizes.data(), r.refined.data(), r.best.data(), r.labels.data(), r.ids.data(),
                             r.status.data(), r.counts.data(), r.hypPlanes.data()));
    r.sizes.resize((size_t)c);
    r.planes.resize(4 * (size_t)c);
    r.refined.resize((size_t)c);
    r.best.resize((size_t)c);
    size_t total = 0;
    for (int64_t s : r.sizes) total += (size_t)s;
    r.ids.resize(total);
    return r;
  }
  // Cylinder and sphere segmentation (extension: no reference parity; include/pcgx.h, pcgx_kdtree_shapes): the sphere
  // (kind PCGX_SHAPE_SPHERE) or cylinder (PCGX_SHAPE_CYLINDER) most live points lie within maxDist of, by sample
  // consensus over hypotheses made from two oriented points -- a seed and a partner out of its sampleRadius
  // neighbourhood (0: out of everything left) -- drawn by the caller's random words (samples: 2 per hypothesis and round);
  // its inliers taken out, then the next, until a round's best has fewer than max(minInliers, 2).  normals: one per
  // point; rMin <= r <= rMax; axis (nullptr: none): only cylinders whose axis has |cos| >= minAxisCos with it; an
  // inlier's normal has |cos| >= minNormalCos with the shape's.  A ShapesResult is a ClustersResult (GroupStats and
  // GroupHulls take it), one group a shape in the order found; shapes: 8 floats per shape, (cx, cy, cz, r, 0, 0, 0, 0) or
  // (qx, qy, qz, r, ax, ay, az, 0); refined, best: per shape; status, counts, hypShapes: per round and hypothesis.
  struct ShapesResult : ClustersResult {
    std::vector<float> shapes, hypShapes;
    std::vector<int32_t> refined, status;
    std::vector<int64_t> best, counts;
  };
  ShapesResult Shapes(int32_t kind, float maxDist, const std::vector<Vec3> &normals, const std::vector<uint32_t> &samples,
                      int64_t nHyp, int32_t maxShapes = 1, int64_t minInliers = 2, float sampleRadius = 0.0f,
                      float rMin = 0.0f, float rMax = __builtin_inff(), const float *axis = nullptr, float minAxisCos = 0.0f,
                      float minNormalCos = 0.0f, bool refine = true) const {
    const int64_t n = Len();
    if ((int64_t)normals.size() != n) throw Error(PCGX_E_INVALID, "one normal per point of the tree is required");
    if (nHyp > 0 && maxShapes > 0 && (int64_t)samples.size() != 2 * nHyp * maxShapes)
      throw Error(PCGX_E_INVALID, "two sample words per hypothesis and round are required");
    const size_t mp = maxShapes > 0 ? (size_t)maxShapes : 0, rows = nHyp > 0 ? mp * (size_t)nHyp : 0;
    ShapesResult r;
    r.labels.resize((size_t)n);
    r.ids.resize((size_t)n);
    r.sizes.resize(mp);
    r.shapes.resize(8 * mp);
    r.refined.resize(mp);
    r.best.resize(mp);
    r.status.resize(rows);
    r.counts.resize(rows);
    r.hypShapes.resize(8 * rows);
    int64_t c = 0;
    check(pcgx_kdtree_shapes(h_.get(), kind, samples.empty() ? nullptr : samples.data(), nHyp, maxShapes, maxDist, minInliers,
                             sampleRadius, rMin, rMax, axis, minAxisCos, normals.empty() ? nullptr : normals[0].data(),
                             minNormalCos, refine ? 1 : 0, &c, r.shapes.data(), r.sizes.data(), r.refined.data(),
                             r.best.data(), r.labels.data(), r.ids.data(), r.status.data(), r.counts.data(),
                             r.hypShapes.data()));
    r.sizes.resize((size_t)c);
    r.shapes.resize(8 * (size_t)c);
    r.refined.resize((size_t)c);
    r.best.resize((size_t)c);
    size_t total = 0;
    for (int64_t s : r.sizes) total += (size_t)s;
    r.ids.resize(total);
    return r;
  }
  // Ground segmentation (extension: no reference parity; include/pcgx.h, pcgx_kdtree_ground): a progressive
  // morphological filter.  The minimum z surface of the live points over the grid (origin (x, y), dims (nx, ny), cells
  // of `cell`) is opened with squares of half[k] cells one after the other; a point is ground iff z - surface_k <
  // height[k] after every window k.  A GroundResult is a ClustersResult (GroupStats and GroupHulls take it) of two
  // groups, the ground and the rest: labels 0 / 1 / -1 (no part), ids the ground ascending, then the rest.  window: the
  // first window a point failed, -1 for ground; surface: the terrain model, ny rows of nx, +inf at an empty cell; hag:
  // the height above it, NaN where a point takes no part.
  struct GroundResult : ClustersResult {
    std::vector<int32_t> window;
    std::vector<float> surface, hag;
  };
  GroundResult Ground(const float (&origin)[2], const int32_t (&dims)[2], float cell, const std::vector<int32_t> &half,
                      const std::vector<float> &height) const {
    const int64_t n = Len();
    if (half.size() != height.size()) throw Error(PCGX_E_INVALID, "one height per window is required");
    const bool grid = dims[0] >= 1 && dims[0] <= 8192 && dims[1] >= 1 && dims[1] <= 8192;
    GroundResult r;
    r.labels.resize((size_t)n);
    r.ids.resize((size_t)n);
    r.sizes.resize(2);
    r.window.resize((size_t)n);
    r.hag.resize((size_t)n);
    r.surface.resize(grid ? (size_t)dims[0] * (size_t)dims[1] : 0);
    int64_t g = 0;
    check(pcgx_kdtree_ground(h_.get(), origin, dims, cell, (int32_t)half.size(), half.empty() ? nullptr : half.data(),
                             height.empty() ? nullptr : height.data(), r.labels.data(), r.sizes.data(), r.ids.data(), &g,
                             r.window.data(), r.surface.empty() ? nullptr : r.surface.data(), r.hag.data()));
    r.sizes.resize((size_t)g);
    size_t total = 0;
    for (int64_t s : r.sizes) total += (size_t)s;
    r.ids.resize(total);
    return r;
  }
  // Group geometry (extension: no reference parity; include/pcgx.h, pcgx_kdtree_group_stats): per group of a grouped id
  // list over the tree's own points -- ids: group 0's members, then group 1's, ...; sizes: per group; what Clusters
  // returns -- the count of live members, the axis-aligned box (lo xyz, hi xyz), centroid and covariance (xx, xy, xz,
  // yy, yz, zz), the covariance's eigenvalues (descending) and unit axes (three rows of three; axis 2 is the fitted
  // plane's normal) and the oriented box in that frame (centre xyz, then the half-extents).  Row g of every array is
  // group g's; a group without a live member is all zero.
  struct GroupStatsResult {
    std::vector<int64_t> count;
    std::vector<float> aabb;                           // 6 per group
    std::vector<double> centroid, cov, eig, axes, obb; // 3, 6, 3, 9, 6 per group
  };
  GroupStatsResult GroupStats(const std::vector<int64_t> &ids, const std::vector<int64_t> &sizes) const {
    const size_t g = sizes.size();
    GroupStatsResult r;
    r.count.resize(g);
    r.aabb.resize(6 * g);
    r.centroid.resize(3 * g);
    r.cov.resize(6 * g);
    r.eig.resize(3 * g);
    r.axes.resize(9 * g);
    r.obb.resize(6 * g);
    check(pcgx_kdtree_group_stats(h_.get(), ids.data(), (int64_t)ids.size(), sizes.data(), (int64_t)g, r.count.data(),
                                  r.aabb.data(), r.centroid.data(), r.cov.data(), r.eig.data(), r.axes.data(),
                                  r.obb.data()));
    return r;
  }
  GroupStatsResult GroupStats(const ClustersResult &c) const { return GroupStats(c.ids, c.sizes); }
  // Per group of a grouped id list, what the group stands on: the exact convex hull of its (x, y), again a grouped id
  // list (counter-clockwise from the lexicographically least place, -1 behind the last hull), the polygon's area and the
  // minimum-area rectangle with a side along a hull edge (extension: no reference parity; include/pcgx.h,
  // pcgx_kdtree_group_hulls).
  struct GroupHullsResult {
    std::vector<int64_t> hull_sizes, hull_ids;  // per group; per slot of ids
    std::vector<double> area, rect;             // 1, 6 per group: centre x y, u x y, half-extents along u and (-u_y, u_x)
  };
  GroupHullsResult GroupHulls(const std::vector<int64_t> &ids, const std::vector<int64_t> &sizes) const {
    const size_t g = sizes.size();
    GroupHullsResult r;
    r.hull_sizes.resize(g);
    r.hull_ids.assign(ids.size(), -1);
    r.area.resize(g);
    r.rect.resize(6 * g);
    check(pcgx_kdtree_group_hulls(h_.get(), ids.data(), (int64_t)ids.size(), sizes.data(), (int64_t)g, r.hull_sizes.data(),
                                  r.hull_ids.data(), r.area.data(), r.rect.data()));
    return r;
  }
  GroupHullsResult GroupHulls(const ClustersResult &c) const { return GroupHulls(c.ids, c.sizes); }
  // The k points with the smallest (DistSq, ID) among those with DistSq < maxRange^2, ascending (extension: no
  // reference parity; include/pcgx.h, pcgx_kdtree_knearest: ties go by ID).
  std::vector<Neighbor> KNearest(const Vec3 &p, int32_t k, float maxRange) const {
    return KNearestBatch({p}, k, maxRange)[0];
  }
  // ... for every query; an empty `queries` takes the tree's own points (result in id order).
  std::vector<std::vector<Neighbor>> KNearestBatch(const std::vector<Vec3> &queries, int32_t k, float maxRange) const {
    const bool own = queries.empty();
    const int64_t n = own ? Len() : (int64_t)queries.size();
    std::vector<int64_t> ids((size_t)(n * (k > 0 ? k : 0)));
    std::vector<float> d(ids.size());
    std::vector<int32_t> counts((size_t)n);
    check(pcgx_kdtree_knearest(h_.get(), own ? nullptr : queries[0].data(), n, k, maxRange, ids.data(), d.data(),
                               counts.data()));
    std::vector<std::vector<Neighbor>> out((size_t)n);
    for (int64_t i = 0; i < n; i++)
      for (int32_t s = 0; s < counts[(size_t)i]; s++)
        out[(size_t)i].push_back(Neighbor{ids[(size_t)(i * k + s)], d[(size_t)(i * k + s)]});
    return out;
  }
  // The covariance of every query's k nearest neighbours (KNearestBatch's lists; extension: no reference parity;
  // include/pcgx.h, pcgx_kdtree_covariances).  mode PCGX_COV_PLANE (Generalized ICP's input): I - (1 - epsilon) u u^T
  // with u the unit normal; PCGX_COV_RAW: the covariance as it is.  Fewer than 3 neighbours, or all at one place: I
  // (PLANE) / 0 (RAW), normal {0, 0, 0}.  An empty `queries` takes the tree's own points: the result is in id order.
  struct CovariancesResult {
    std::vector<std::array<float, 6>> cov;  // xx, xy, xz, yy, yz, zz
    std::vector<Vec3> normals;              // u turned towards the viewpoint
    std::vector<int32_t> counts;
  };
  CovariancesResult Covariances(int32_t k, float maxRange = std::numeric_limits<float>::infinity(),
                                int32_t mode = PCGX_COV_PLANE, float epsilon = 1e-3f,
                                const std::vector<Vec3> &queries = {}, const Vec3 &viewpoint = Vec3{0.0f, 0.0f, 0.0f}) const {
    const bool own = queries.empty();
    const int64_t n = own ? Len() : (int64_t)queries.size();
    CovariancesResult r;
    r.cov.resize((size_t)n);
    r.normals.resize((size_t)n);
    r.counts.resize((size_t)n);
    check(pcgx_kdtree_covariances(h_.get(), own ? nullptr : queries[0].data(), n, k, maxRange, mode, epsilon,
                                  viewpoint.data(), n ? r.cov[0].data() : nullptr, n ? r.normals[0].data() : nullptr,
                                  r.counts.data()));
    return r;
  }
  const pcgx_kdtree *handle() const { return h_.get(); }

 private:
  KDTree(const KDTree &) = default;
  static size_t RayCount(const std::vector<Vec3> &origins, const std::vector<Vec3> &directions,
                         const std::vector<float> &sMin, const std::vector<float> &sMax) {
    const size_t nr = origins.size();
    if (directions.size() != nr || (!sMin.empty() && sMin.size() != nr) || (!sMax.empty() && sMax.size() != nr))
      throw Error(PCGX_E_INVALID, "one direction (and one sMin, sMax where given) per origin is required");
    return nr;
  }
  std::shared_ptr<pcgx_kdtree> h_;
};

// M3C2's finish (extension: no reference parity; include/pcgx.h, pcgx_m3c2_finish) on the cylinder statistics of two
// epochs (KDTree::CylinderStats with the same cores, axes, radius and half length against each epoch's tree): per core
// the signed distance along the axis, epoch 2 minus epoch 1, the level of detection at 95 % and whether |distance|
// exceeds it.  Fewer than minCount points in either cylinder, or an unusable axis: NaN, NaN, 0.
struct M3C2Result {
  std::vector<double> distance, lod;
  std::vector<uint8_t> significant;
};
inline M3C2Result M3C2Finish(const std::vector<Vec3> &axes, const KDTree::CylinderStatsResult &epoch1,
                             const KDTree::CylinderStatsResult &epoch2, double registrationError = 0.0,
                             int32_t minCount = 4) {
  const size_t m = axes.size();
  if (epoch1.counts.size() != m || epoch2.counts.size() != m || epoch1.sums.size() != 2 * m || epoch2.sums.size() != 2 * m)
    throw Error(PCGX_E_INVALID, "one count and two sums per axis and epoch are required");
  M3C2Result r;
  r.distance.resize(m);
  r.lod.resize(m);
  r.significant.resize(m);
  check(pcgx_m3c2_finish(m ? axes[0].data() : nullptr, epoch1.counts.data(), epoch1.sums.data(), epoch2.counts.data(),
                         epoch2.sums.data(), (int64_t)m, registrationError, minCount, r.distance.data(), r.lod.data(),
                         r.significant.data()));
  return r;
}

// Matching of FPFH descriptors (extension: no reference parity; include/pcgx.h, "FPFH matching").  Rows as
// KDTree::FPFH returns them.  ids: the nearest usable row of b per row of a (-1: none), distSq its float32 squared
// distance, secondDistSq the runner-up's (+inf: none).
using FPFHRow = std::array<float, 33>;
struct FPFHMatchResult {
  std::vector<int64_t> ids;
  std::vector<float> distSq, secondDistSq;
};
inline FPFHMatchResult fpfh_match(const std::vector<FPFHRow> &a, const std::vector<FPFHRow> &b) {
  const int64_t na = (int64_t)a.size(), nb = (int64_t)b.size();
  FPFHMatchResult r;
  r.ids.resize((size_t)na);
  r.distSq.resize((size_t)na);
  r.secondDistSq.resize((size_t)na);
  check(pcgx_fpfh_match(na ? a[0].data() : nullptr, na, nb ? b[0].data() : nullptr, nb, r.ids.data(), r.distSq.data(),
                        r.secondDistSq.data()));
  return r;
}
// The matches of a in b that pass the ratio test distSq <= maxRatio^2 secondDistSq (maxRatio in (0, 1], 1 keeps all)
// and, with mutual, whose row of b matches back to the same row of a: {row of a, row of b}, ascending in the first.
inline std::vector<std::array<int64_t, 2>> fpfh_correspondences(const std::vector<FPFHRow> &a,
                                                               const std::vector<FPFHRow> &b, float maxRatio = 1.0f,
                                                               bool mutual = true) {
  const int64_t na = (int64_t)a.size(), nb = (int64_t)b.size();
  std::vector<int64_t> src((size_t)na), dst((size_t)na);
  int64_t m = 0;
  check(pcgx_fpfh_correspondences(na ? a[0].data() : nullptr, na, nb ? b[0].data() : nullptr, nb, maxRatio * maxRatio,
                                  mutual ? 1 : 0, src.data(), dst.data(), &m));
  std::vector<std::array<int64_t, 2>> out((size_t)m);
  for (size_t i = 0; i < (size_t)m; i++) out[i] = {src[i], dst[i]};
  return out;
}

// The rigid pose most pairs of a correspondence list agree on, by sample consensus (extension: no reference parity;
// include/pcgx.h, "pose from correspondences").  pairs: {index into src, index into dst}, e.g. fpfh_correspondences';
// samples: three random 32-bit words per hypothesis, drawn by the caller (word u names pair (u * m) >> 32).  pose takes
// src onto dst: the best hypothesis's, or with refine the least-squares pose over its inliers where that keeps at least
// as many.  inliers: the pairs within maxDist under it, ascending.
struct PoseResult {
  bool found = false, refined = false;
  int64_t best = -1, bestCount = 0;
  Mat4 pose{};
  std::vector<int64_t> inliers;
};
inline PoseResult pose_from_correspondences(const std::vector<Vec3> &src, const std::vector<Vec3> &dst,
                                            const std::vector<std::array<int64_t, 2>> &pairs,
                                            const std::vector<std::array<uint32_t, 3>> &samples, float maxDist,
                                            float edgeSimilarity = 0.9f, bool refine = true) {
  const int64_t m = (int64_t)pairs.size(), n = (int64_t)samples.size();
  std::vector<int64_t> s((size_t)m), d((size_t)m), ids((size_t)m);
  for (size_t k = 0; k < (size_t)m; k++) {
    s[k] = pairs[k][0];
    d[k] = pairs[k][1];
  }
  PoseResult r;
  int32_t found = 0, refined = 0;
  int64_t nIn = 0;
  check(pcgx_pose_from_correspondences(src.empty() ? nullptr : src[0].data(), (int64_t)src.size(),
                                       dst.empty() ? nullptr : dst[0].data(), (int64_t)dst.size(), s.data(), d.data(), m,
                                       n ? samples[0].data() : nullptr, n, maxDist * maxDist, edgeSimilarity,
                                       refine ? 1 : 0, &found, &r.best, &r.bestCount, r.pose.data(), &refined, &nIn,
                                       ids.data(), nullptr, nullptr, nullptr));
  r.found = found != 0;
  r.refined = refined != 0;
  r.inliers.assign(ids.begin(), ids.begin() + nIn);
  return r;
}

// K poses scored on the whole clouds (extension: no reference parity; include/pcgx.h, "score poses"): for each pose the
// number of points of src that land within maxDist of the tree's cloud and the float64 sum of their DistSq; best: the
// live pose with the largest count (the smallest k among equals, -1 if none is live: a pose of sixteen zeros is dead).
struct ScoreResult {
  std::vector<int64_t> counts;
  std::vector<double> sums;
  int64_t best = -1;
  Mat4 pose{};
};
inline ScoreResult score_poses(const KDTree &tree, const std::vector<Vec3> &src, const std::vector<Mat4> &poses,
                               float maxDist) {
  ScoreResult r;
  const int64_t n = (int64_t)src.size(), K = (int64_t)poses.size();
  r.counts.assign((size_t)K, 0);
  r.sums.assign((size_t)K, 0.0);
  check(pcgx_kdtree_score_poses(tree.handle(), n ? src[0].data() : nullptr, n, K ? poses[0].data() : nullptr, K, maxDist,
                                K ? r.counts.data() : nullptr, K ? r.sums.data() : nullptr, &r.best, r.pose.data()));
  return r;
}

// The K best hypotheses of a pose_from_correspondences call (status 0, count >= 3; by count descending, then by index):
// ids[j] and poses[j], -1 and a dead pose in the slots behind the last one.
struct PoseSelection {
  std::vector<int64_t> ids;
  std::vector<Mat4> poses;
  int64_t selected = 0;
};
inline PoseSelection pose_select(const std::vector<int32_t> &status, const std::vector<int64_t> &counts,
                                 const std::vector<Mat4> &poses, int64_t K) {
  PoseSelection r;
  const int64_t n = (int64_t)status.size();
  if (counts.size() != status.size() || poses.size() != status.size())
    throw Error(PCGX_E_INVALID, "pose_select: status, counts and poses must have one entry per hypothesis");
  r.ids.assign((size_t)(K > 0 ? K : 0), -1);
  r.poses.assign((size_t)(K > 0 ? K : 0), Mat4{});
  check(pcgx_pose_select(n ? status.data() : nullptr, n ? counts.data() : nullptr, n ? poses[0].data() : nullptr, n, K,
                         K > 0 ? r.ids.data() : nullptr, K > 0 ? r.poses[0].data() : nullptr, &r.selected));
  return r;
}

class VoxelGrid {  // pc/filter/voxelgrid/voxelgrid.go:23-33 + option.go:14-18
 public:
  Vec3 LeafSize;
  std::array<int32_t, 3> ChunkSize{0, 0, 0};
  explicit VoxelGrid(Vec3 leaf) : LeafSize(leaf) {}
  VoxelGrid &WithChunkSize(std::array<int32_t, 3> s) { ChunkSize = s; return *this; }
  // Filter: returns the output records (Width = size()/stride, Height = 1).
  std::vector<uint8_t> Filter(const CloudView &c) const {
    std::vector<uint8_t> out((size_t)c.points * c.stride);
    int64_t m = 0;
    check(pcgx_voxel_filter(c.data, c.points, c.stride, c.xyz_offset, LeafSize.data(), ChunkSize.data(), out.data(), &m));
    out.resize((size_t)m * c.stride);
    return out;
  }
  // This rank's share of Filter(c) over the ranks of `comm` (every rank passes the same cloud); the
  // ranks' results, rank 0's first, are Filter's output record for record.  Collective.
  std::vector<uint8_t> FilterSharded(const CloudView &c, const Comm &comm) const {
    std::vector<uint8_t> out((size_t)c.points * c.stride);
    int64_t m = 0;
    check(pcgx_voxel_filter_sharded(comm.handle(), c.data, c.points, c.stride, c.xyz_offset, LeafSize.data(),
                                    ChunkSize.data(), out.data(), &m));
    out.resize((size_t)m * c.stride);
    return out;
  }
};

// Statistical outlier removal (extension: no reference counterpart; PCL's StatisticalOutlierRemoval) in the shape of
// filter.Filter (include/pcgx.h, pcgx_sor_filter).  Keeps the points whose mean distance to their MeanK nearest
// others is at most mu + StddevMul * sigma (WithNegative(true): the others); non-finite points are dropped.
class StatisticalOutlierRemoval {
 public:
  int32_t MeanK;
  float StddevMul;
  bool Negative = false;
  std::vector<double> MeanDist;  // after Filter: by input index, NaN for non-finite points
  std::array<double, 3> Stats{0.0, 0.0, 0.0};  // after Filter: {mu, sigma, threshold}
  StatisticalOutlierRemoval(int32_t meanK, float stddevMul) : MeanK(meanK), StddevMul(stddevMul) {}
  StatisticalOutlierRemoval &WithNegative(bool negative) { Negative = negative; return *this; }
  // Filter: returns the kept records in input order (Width = size()/stride, Height = 1).
  std::vector<uint8_t> Filter(const CloudView &c) {
    std::vector<uint8_t> out((size_t)c.points * c.stride);
    MeanDist.assign((size_t)c.points, 0.0);
    int64_t m = 0;
    check(pcgx_sor_filter(c.data, c.points, c.stride, c.xyz_offset, MeanK, StddevMul, Negative ? 1 : 0, out.data(), &m,
                          MeanDist.data(), Stats.data()));
    out.resize((size_t)m * c.stride);
    return out;
  }
};

// Radius outlier removal (extension: no reference counterpart; PCL's RadiusOutlierRemoval; include/pcgx.h,
// pcgx_ror_filter).  Keeps the finite points with at least MinNeighbors finite points within Radius, themselves
// included (WithNegative(true): the other finite points); non-finite points are dropped.
class RadiusOutlierRemoval {
 public:
  float Radius;
  int32_t MinNeighbors;
  bool Negative = false;
  RadiusOutlierRemoval(float radius, int32_t minNeighbors) : Radius(radius), MinNeighbors(minNeighbors) {}
  RadiusOutlierRemoval &WithNegative(bool negative) { Negative = negative; return *this; }
  // Filter: returns the kept records in input order (Width = size()/stride, Height = 1).
  std::vector<uint8_t> Filter(const CloudView &c) {
    std::vector<uint8_t> out((size_t)c.points * c.stride);
    int64_t m = 0;
    check(pcgx_ror_filter(c.data, c.points, c.stride, c.xyz_offset, Radius, MinNeighbors, Negative ? 1 : 0, out.data(), &m));
    out.resize((size_t)m * c.stride);
    return out;
  }
};

// pc/storage/voxelgrid.VoxelGrid (voxelgrid.go:7-122) filled with Add(point i, i) for a whole
// cloud, plus pc/segmentation/voxelgrid's Segment (voxelgrid.go:39-73).
class BucketVoxelGrid {
 public:
  BucketVoxelGrid(float resolution, std::array<int64_t, 3> size, Vec3 origin, const CloudView &c) {
    check(pcgx_bucket_grid_build(c.data, c.points, c.stride, c.xyz_offset, resolution, size.data(), origin.data(), &h_));
  }
  ~BucketVoxelGrid() { pcgx_bucket_grid_free(h_); }
  BucketVoxelGrid(const BucketVoxelGrid &) = delete;
  BucketVoxelGrid &operator=(const BucketVoxelGrid &) = delete;
  int64_t Len() const { int64_t n; check(pcgx_bucket_grid_counts(h_, &n, nullptr, nullptr)); return n; }
  // Get(p): false = nil (p outside the grid), else the ids of p's voxel in insertion order
  bool Get(const Vec3 &p, std::vector<int64_t> *ids) const {
    int64_t cnt = 0;
    check(pcgx_bucket_grid_get(h_, p.data(), nullptr, 0, &cnt));
    if (cnt < 0) return false;
    ids->resize((size_t)cnt);
    if (cnt > 0) check(pcgx_bucket_grid_get(h_, p.data(), ids->data(), cnt, &cnt));
    return true;
  }
  // Segment(p) in the reference's order (voxelgrid.go:39-73)
  std::vector<int64_t> Segment(const Vec3 &p) {
    int64_t cnt = 0;
    check(pcgx_bucket_grid_segment_bfs(h_, p.data(), nullptr, 0, &cnt));
    std::vector<int64_t> out((size_t)cnt);
    if (cnt > 0) check(pcgx_bucket_grid_segment_bfs(h_, p.data(), out.data(), cnt, &cnt));
    return out;
  }
  const pcgx_bucket_grid *handle() const { return h_; }

 private:
  pcgx_bucket_grid *h_ = nullptr;
};

// pc/segmentation/regiongrowing.RegionGrowing (regiongrowing.go:13-56): New(search, propertyIter)
class RegionGrowing {
 public:
  RegionGrowing(const KDTree &search, std::vector<uint32_t> property) : t_(search), labels_(std::move(property)) {
    if ((int64_t)labels_.size() != t_.Len()) throw Error(PCGX_E_INVALID, "one property value per point is required");
  }
  // Segment(p, maxRange) in the reference's order (regiongrowing.go:23-56)
  std::vector<int64_t> Segment(const Vec3 &p, float maxRange) {
    std::vector<int64_t> out(labels_.size());
    int64_t cnt = 0;
    check(pcgx_region_growing_segment_bfs(t_.handle(), labels_.data(), p.data(), maxRange, out.data(),
                                          (int64_t)out.size(), &cnt));
    out.resize((size_t)cnt);
    return out;
  }
  // the same set for many seeds: regions of the whole cloud labelled once per maxRange, ascending id
  std::vector<int64_t> SegmentById(const Vec3 &p, float maxRange) {
    if (comp_.empty() || maxRange != range_) {
      comp_.resize(labels_.size());
      check(pcgx_region_growing_components(t_.handle(), labels_.data(), maxRange, comp_.data()));
      range_ = maxRange;
    }
    std::vector<int64_t> out(labels_.size());
    int64_t cnt = 0;
    check(pcgx_region_growing_segment(t_.handle(), labels_.data(), comp_.data(), p.data(), maxRange, out.data(),
                                      (int64_t)out.size(), &cnt));
    out.resize((size_t)cnt);
    return out;
  }

 private:
  const KDTree &t_;
  std::vector<uint32_t> labels_;
  std::vector<int64_t> comp_;
  float range_ = 0.0f;
};

// icp.PointToPointCorrespondence / NearestPointCorresponder (correspondence.go:8-37): Pairs over pcgx_icp_pairs --
// one batched nearest-neighbour pass, the matched targets compacted in target order.
struct PointToPointCorrespondence {
  int64_t BaseID, TargetID;
  float SquaredDistance;
};
struct NearestPointCorresponder {
  float MaxDist = 0.0f;
  std::vector<PointToPointCorrespondence> Pairs(const KDTree &base, const std::vector<Vec3> &target) const {
    const size_t n = target.size();
    std::vector<int64_t> b(n), t(n);
    std::vector<float> d(n);
    int64_t np = 0;
    check(pcgx_icp_pairs(base.handle(), n ? target[0].data() : nullptr, (int64_t)n, MaxDist, base.MinDistSq, b.data(), t.data(),
                         d.data(), &np));
    std::vector<PointToPointCorrespondence> out((size_t)np);
    for (size_t i = 0; i < out.size(); i++) out[i] = PointToPointCorrespondence{b[i], t[i], d[i]};
    return out;
  }
};

struct Stat {  // icp/stat.go:3-6
  pcgx_icp_evaluated Evaluated;
  int NumIteration;
};

// PointToPointEvaluator.WeightFn (evaluator.go:19-23,72): the reference takes any closure, the device
// one of the built-in forms (include/pcgx.h PCGX_WEIGHT_*); Kind 0 = DefaultEvaluateWeightFn (w = 1).
struct WeightFn {
  int32_t Kind = PCGX_WEIGHT_ONE;
  float A = 0.0f;
};

class PointToPointICP {  // icp.go:18-67 with evaluator.go:69-73 and updater.go:18-22 options
 public:
  float MaxDist = 0.0f;
  int MinPairs = 0;
  WeightFn EvaluateWeight;  // evaluator.go:72
  std::array<float, 6> Weight{}, Threshold{};
  int MaxIteration = 0;
  // Sums (include/pcgx.h PCGX_SUMS_*).  Default PCGX_SUMS_REFERENCE: the evaluator's sums as the reference
  // forms them (sequential float32 additions in target order, evaluator.go:122-145): Evaluated and every
  // pose bit-identical to the Go code's.  PCGX_SUMS_F64_TREE: float64 reductions of the same float32 terms
  // (faster; equal up to the reference's own rounding noise; what FitSharded computes over several ranks).
  int32_t Sums = PCGX_SUMS_REFERENCE;
  std::pair<Mat4, Stat> Fit(const KDTree &base, const std::vector<Vec3> &target) const {
    const pcgx_icp_params p = params(base);
    Mat4 t;
    pcgx_icp_stat st{};
    const float *tp = target.empty() ? nullptr : target[0].data();
    check(pcgx_icp_fit(base.handle(), tp, (int64_t)target.size(), &p, t.data(), &st));
    return {t, Stat{st.evaluated, st.num_iteration}};
  }
  // Fit with the target spread over the device slots of THIS process (pcgx_init_devices): bases[r] the replica built
  // with slot r current, tiles[r] slot r's part.  Default sums: the reference's Fit of the tiles one after the other.
  std::pair<Mat4, Stat> FitMulti(const std::vector<const KDTree *> &bases, const std::vector<std::vector<Vec3>> &tiles) const {
    const pcgx_icp_params p = params(*bases.at(0));
    std::vector<const pcgx_kdtree *> hb;
    std::vector<const float *> ht;
    std::vector<int64_t> hn;
    for (size_t r = 0; r < bases.size(); r++) {
      hb.push_back(bases[r]->handle());
      ht.push_back(tiles.at(r).empty() ? nullptr : tiles[r][0].data());
      hn.push_back((int64_t)tiles[r].size());
    }
    Mat4 t;
    pcgx_icp_stat st{};
    check(pcgx_icp_fit_multi((int32_t)bases.size(), hb.data(), ht.data(), hn.data(), &p, t.data(), &st));
    return {t, Stat{st.evaluated, st.num_iteration}};
  }
  // Fit on this rank's tile of the target; every rank returns the same transform (default sums: the reference's over
  // the ranks' tiles one after the other; PCGX_SUMS_F64_TREE: one all-reduce of float64 sums per iteration; one
  // rank: Fit).  Collective.
  std::pair<Mat4, Stat> FitSharded(const KDTree &base, const std::vector<Vec3> &tile, const Comm &comm) const {
    const pcgx_icp_params p = params(base);
    Mat4 t;
    pcgx_icp_stat st{};
    check(pcgx_icp_fit_sharded(base.handle(), tile.empty() ? nullptr : tile[0].data(), (int64_t)tile.size(), &p,
                               comm.handle(), t.data(), &st));
    return {t, Stat{st.evaluated, st.num_iteration}};
  }

 private:
  pcgx_icp_params params(const KDTree &base) const {
    pcgx_icp_params p{};
    p.max_dist = MaxDist;
    p.min_dist_sq = base.MinDistSq;
    p.min_pairs = MinPairs;
    p.weight_fn = EvaluateWeight.Kind;
    p.weight_fn_param = EvaluateWeight.A;
    p.sums_mode = Sums;
    std::memcpy(p.weight, Weight.data(), sizeof p.weight);
    std::memcpy(p.threshold, Threshold.data(), sizeof p.threshold);
    p.max_iteration = MaxIteration;
    return p;
  }
};

// Extension (no counterpart in the reference; include/pcgx.h "point-to-plane ICP (extension)"):
// the Fit loop with the point-to-plane evaluator (fills Evaluated.Hessian) and a Gauss-Newton updater.
struct PlaneStat {
  pcgx_icp_evaluated Evaluated;
  std::array<float, 36> Hessian;  // Evaluated.Hessian (mat.Mat6)
  int NumIteration;
};

class PointToPlaneICP {
 public:
  float MaxDist = 0.0f;
  int MinPairs = 0;
  std::array<float, 6> Threshold{};
  int MaxIteration = 0;
  float Damping = 0.0f;
  bool HasGradient() const { return true; }
  bool HasHessian() const { return true; }
  // baseNormals: one unit normal per base point, in the tree's id order.
  std::pair<Mat4, PlaneStat> Fit(const KDTree &base, const std::vector<Vec3> &baseNormals,
                                 const std::vector<Vec3> &target) const {
    if ((int64_t)baseNormals.size() != base.Len()) throw Error(PCGX_E_INVALID, "one normal per base point is required");
    pcgx_icp_params p{};
    p.max_dist = MaxDist;
    p.min_pairs = MinPairs;
    std::memcpy(p.threshold, Threshold.data(), sizeof p.threshold);
    p.max_iteration = MaxIteration;
    Mat4 t;
    PlaneStat ps{};
    pcgx_icp_stat st{};
    check(pcgx_icp_plane_fit(base.handle(), baseNormals[0].data(), target.empty() ? nullptr : target[0].data(),
                             (int64_t)target.size(), &p, Damping, t.data(), &st, ps.Hessian.data()));
    ps.Evaluated = st.evaluated;
    ps.NumIteration = st.num_iteration;
    return {t, ps};
  }
};

// Extension (no counterpart in the reference; include/pcgx.h "Generalized ICP"): the Fit loop with the Generalized ICP
// evaluator -- r = p - b weighed by (C_b + R C_t R^T)^-1, the consumer of KDTree::Covariances -- and the Gauss-Newton
// updater.  Pairs whose covariances cannot be inverted are dropped and are not counted as pairs.
class GeneralizedICP {
 public:
  float MaxDist = 0.0f;
  int MinPairs = 0;
  std::array<float, 6> Threshold{};
  int MaxIteration = 0;
  float Damping = 0.0f;
  bool HasGradient() const { return true; }
  bool HasHessian() const { return true; }
  // baseCov: xx, xy, xz, yy, yz, zz per base point in the tree's id order; targetCov: per target point, in the target's
  // own frame (KDTree::Covariances(k).cov of a tree over each cloud).
  std::pair<Mat4, PlaneStat> Fit(const KDTree &base, const std::vector<std::array<float, 6>> &baseCov,
                                 const std::vector<Vec3> &target,
                                 const std::vector<std::array<float, 6>> &targetCov) const {
    if ((int64_t)baseCov.size() != base.Len()) throw Error(PCGX_E_INVALID, "one covariance per base point is required");
    if (targetCov.size() != target.size()) throw Error(PCGX_E_INVALID, "one covariance per target point is required");
    const pcgx_icp_params p = params();
    Mat4 t;
    PlaneStat ps{};
    pcgx_icp_stat st{};
    check(pcgx_icp_gicp_fit(base.handle(), baseCov.empty() ? nullptr : baseCov[0].data(),
                            target.empty() ? nullptr : target[0].data(), targetCov.empty() ? nullptr : targetCov[0].data(),
                            (int64_t)target.size(), &p, Damping, t.data(), &st, ps.Hessian.data()));
    ps.Evaluated = st.evaluated;
    ps.NumIteration = st.num_iteration;
    return {t, ps};
  }
  // The one call: both clouds' PLANE covariances from their k nearest neighbours, on the device, then the Fit.
  std::pair<Mat4, PlaneStat> FitKNN(const KDTree &base, const std::vector<Vec3> &target, int32_t k = 20,
                                    float epsilon = 1e-3f,
                                    float covMaxRange = std::numeric_limits<float>::infinity()) const {
    const pcgx_icp_params p = params();
    Mat4 t;
    PlaneStat ps{};
    pcgx_icp_stat st{};
    check(pcgx_icp_gicp_fit_knn(base.handle(), target.empty() ? nullptr : target[0].data(), (int64_t)target.size(), k,
                                covMaxRange, epsilon, &p, Damping, t.data(), &st, ps.Hessian.data()));
    ps.Evaluated = st.evaluated;
    ps.NumIteration = st.num_iteration;
    return {t, ps};
  }

 private:
  pcgx_icp_params params() const {
    pcgx_icp_params p{};
    p.max_dist = MaxDist;
    p.min_pairs = MinPairs;
    std::memcpy(p.threshold, Threshold.data(), sizeof p.threshold);
    p.max_iteration = MaxIteration;
    return p;
  }
};

// Extension (no counterpart in the reference; include/pcgx.h "Normal Distributions Transform"): the base cloud as one
// Gaussian per voxel of a BucketVoxelGrid.  The map copies what it needs: the grid and the cloud may go afterwards.
class NDTMap {
 public:
  struct CellList {  // the occupied voxels, ascending address; cov / icov: xx, xy, xz, yy, yz, zz, zero when invalid
    std::vector<int64_t> addr;
    std::vector<int32_t> count, valid;
    std::vector<Vec3> mean;
    std::vector<std::array<float, 6>> cov, icov;
  };
  NDTMap(const BucketVoxelGrid &vg, const CloudView &c, int32_t minPoints = 6, float minEigenRatio = 0.01f) {
    check(pcgx_ndt_map_create(vg.handle(), c.data, c.points, c.stride, c.xyz_offset, 0, minPoints, minEigenRatio, &h_));
  }
  ~NDTMap() { pcgx_ndt_map_free(h_); }
  NDTMap(const NDTMap &) = delete;
  NDTMap &operator=(const NDTMap &) = delete;
  int64_t Occupied() const { int64_t n; check(pcgx_ndt_map_counts(h_, &n, nullptr)); return n; }
  int64_t Valid() const { int64_t n; check(pcgx_ndt_map_counts(h_, nullptr, &n)); return n; }
  CellList Cells() const {
    CellList c;
    const size_t m = (size_t)Occupied();
    c.addr.resize(m); c.count.resize(m); c.valid.resize(m); c.mean.resize(m); c.cov.resize(m); c.icov.resize(m);
    if (m > 0)
      check(pcgx_ndt_map_cells(h_, c.addr.data(), c.count.data(), c.valid.data(), c.mean[0].data(), c.cov[0].data(),
                               c.icov[0].data()));
    return c;
  }
  // The 30 float64 sums {sum e, sum g [6], sum H upper triangle [21], sum omega, pairs} at pose trans (nullptr: identity)
  std::array<double, 30> Evaluate(const std::vector<Vec3> &target, const Mat4 *trans = nullptr, int32_t neighbors = 7,
                                  float outlierRatio = 0.55f) const {
    std::array<double, 30> s{};
    check(pcgx_ndt_evaluate(h_, target.empty() ? nullptr : target[0].data(), (int64_t)target.size(),
                            trans ? trans->data() : nullptr, neighbors, outlierRatio, s.data()));
    return s;
  }
  const pcgx_ndt_map *handle() const { return h_; }

 private:
  pcgx_ndt_map *h_ = nullptr;
};

// The NDT Fit: evaluate, the plane Fit's tail, the Gauss-Newton update, on the device with one read-back.
class NDT {
 public:
  int32_t Neighbors = 7;  // 1, 7 or 27 candidate voxels per point
  float OutlierRatio = 0.55f;
  int MinPairs = 0;
  std::array<float, 6> Threshold{};
  int MaxIteration = 0;
  float Damping = 0.0f;
  bool HasGradient() const { return true; }
  bool HasHessian() const { return true; }
  std::pair<Mat4, PlaneStat> Fit(const NDTMap &map, const std::vector<Vec3> &target, const Mat4 *init = nullptr) const {
    pcgx_icp_params p{};
    p.min_pairs = MinPairs;
    std::memcpy(p.threshold, Threshold.data(), sizeof p.threshold);
    p.max_iteration = MaxIteration;
    Mat4 t;
    PlaneStat ps{};
    pcgx_icp_stat st{};
    check(pcgx_ndt_fit(map.handle(), target.empty() ? nullptr : target[0].data(), (int64_t)target.size(), 0, &p, Damping,
                       Neighbors, OutlierRatio, init ? init->data() : nullptr, t.data(), &st, ps.Hessian.data()));
    ps.Evaluated = st.evaluated;
    ps.NumIteration = st.num_iteration;
    return {t, ps};
  }
};

// ---- the reference's package surface, name for name ------------------------------------------------------------
// What go/pc/storage/kdtree, go/pc/filter/voxelgrid and go/pc/registration/icp are to a Go caller (see go/README.md):
// the exported names of the three reference packages over the classes above, so that code written against
// kdtree.New(ra, opts...), voxelgrid.New(leaf, voxelgrid.WithChunkSize(s)), icp.PointToPointICPGradient{Evaluator,
// UpdaterFactory}.Fit(base, target) reads the same here.  tests/test_cpp_host.py runs them.
namespace kdtree {  // pc/storage/kdtree/kdtree.go:14-65
using KDTree = ::pcgx::KDTree;
using KDTreeOption = ::pcgx::KDTreeOption;
inline KDTree New(const std::vector<Vec3> &ra, std::initializer_list<KDTreeOption> opts = {}) { return KDTree(ra, opts); }
inline KDTree New(const CloudView &ra, std::initializer_list<KDTreeOption> opts = {}) { return KDTree(ra, opts); }
inline KDTreeOption WithMinDistSq(float d) { return KDTree::WithMinDistSq(d); }
}  // namespace kdtree

namespace voxelgrid {  // pc/filter/voxelgrid/voxelgrid.go:23-33, option.go:7-18
struct Options {
  Vec3 LeafSize{};
  std::array<int32_t, 3> ChunkSize{0, 0, 0};
};
using Option = std::function<void(Options &)>;
inline Option WithChunkSize(std::array<int32_t, 3> s) { return [s](Options &o) { o.ChunkSize = s; }; }
// filter.Filter (pc/filter/filter.go:7-9): Filter(cloud) -> the output records
inline ::pcgx::VoxelGrid New(Vec3 leafSize, std::initializer_list<Option> opts = {}) {
  Options o;
  o.LeafSize = leafSize;
  for (const auto &f : opts) f(o);
  ::pcgx::VoxelGrid vg(o.LeafSize);
  vg.WithChunkSize(o.ChunkSize);
  return vg;
}
}  // namespace voxelgrid

namespace icp {  // pc/registration/icp
using PointToPointCorrespondence = ::pcgx::PointToPointCorrespondence;  // correspondence.go:8-12
using NearestPointCorresponder = ::pcgx::NearestPointCorresponder;      // correspondence.go:18-37
using Stat = ::pcgx::Stat;                                              // stat.go:3-6
using Evaluated = pcgx_icp_evaluated;                                   // evaluator.go:25-30
using Weight = ::pcgx::WeightFn;
// PointToPointEvaluator (evaluator.go:69-73); WeightFn closures cannot cross to the device: Weight names a built-in form
struct PointToPointEvaluator {
  NearestPointCorresponder Corresponder;
  int MinPairs = 0;
  icp::Weight Weight;
  int32_t Sums = PCGX_SUMS_REFERENCE;
  bool HasGradient() const { return true; }
  bool HasHessian() const { return false; }
  Evaluated Evaluate(const KDTree &base, const std::vector<Vec3> &target) const {  // evaluator.go:91-189
    pcgx_icp_params p{};
    p.max_dist = Corresponder.MaxDist;
    p.min_dist_sq = base.MinDistSq;
    p.min_pairs = MinPairs;
    p.weight_fn = Weight.Kind;
    p.weight_fn_param = Weight.A;
    p.sums_mode = Sums;
    Evaluated ev{};
    check(pcgx_icp_evaluate_params(base.handle(), target.empty() ? nullptr : target[0].data(), (int64_t)target.size(), &p, &ev));
    return ev;
  }
};
struct GradientDescentUpdaterFactory {  // updater.go:18-37 (zero values: the reference's defaults)
  std::array<float, 6> Weight{}, Threshold{};
  int MaxIteration = 0;
};
struct PointToPointICPGradient {  // icp.go:18-67
  PointToPointEvaluator Evaluator;
  GradientDescentUpdaterFactory UpdaterFactory;
  std::pair<Mat4, Stat> Fit(const KDTree &base, const std::vector<Vec3> &target) const { return impl().Fit(base, target); }
  std::pair<Mat4, Stat> FitSharded(const KDTree &base, const std::vector<Vec3> &tile, const Comm &comm) const {
    return impl().FitSharded(base, tile, comm);
  }
  std::pair<Mat4, Stat> FitMulti(const std::vector<const KDTree *> &bases, const std::vector<std::vector<Vec3>> &tiles) const {
    return impl().FitMulti(bases, tiles);
  }

 private:
  PointToPointICP impl() const {
    PointToPointICP r;
    r.MaxDist = Evaluator.Corresponder.MaxDist;
    r.MinPairs = Evaluator.MinPairs;
    r.EvaluateWeight = Evaluator.Weight;
    r.Sums = Evaluator.Sums;
    r.Weight = UpdaterFactory.Weight;
    r.Threshold = UpdaterFactory.Threshold;
    r.MaxIteration = UpdaterFactory.MaxIteration;
    return r;
  }
};
}  // namespace icp

// pc/sac (sac.go, randomsample.go, surface.go).  Compute(n) draws the 3n ids from the Sampler first, in the
// reference's order, and fits and evaluates every hypothesis in one device call (include/pcgx.h).
namespace sac {

struct Sampler {  // sac.go:7-9
  virtual ~Sampler() = default;
  virtual int64_t Sample() = 0;
};

// randomsample.go:7-12: uniform ids in [0, n) (std::mt19937_64; Go's math/rand sequence is Go's own)
class RandomSampler : public Sampler {
 public:
  explicit RandomSampler(int64_t n, uint64_t seed = std::random_device{}()) : rng_(seed), dist_(0, n - 1) {}
  int64_t Sample() override { return dist_(rng_); }

 private:
  std::mt19937_64 rng_;
  std::uniform_int_distribution<int64_t> dist_;
};
inline std::unique_ptr<Sampler> NewRandomSampler(int64_t n) { return std::unique_ptr<Sampler>(new RandomSampler(n)); }

class VoxelGridSurfaceModel;
using ModelHandle = std::shared_ptr<pcgx_sac_plane_model>;

// voxelGridSurfaceModelCoefficients (surface.go:191-240)
class Coefficients {
 public:
  Coefficients(ModelHandle m, const pcgx_sac_plane &c, int64_t score) : m_(std::move(m)), c_(c), score_(score) {}
  int64_t Evaluate() const { return score_; }  // computed by the call that fitted these coefficients
  std::vector<int64_t> Inliers(float d) const {
    int64_t cnt = 0;
    check(pcgx_sac_plane_inliers(m_.get(), &c_, d, nullptr, 0, &cnt));
    std::vector<int64_t> out((size_t)cnt);
    if (cnt > 0) check(pcgx_sac_plane_inliers(m_.get(), &c_, d, out.data(), cnt, &cnt));
    return out;
  }
  bool IsIn(const Vec3 &p, float d) const {
    int32_t in = 0;
    check(pcgx_sac_plane_is_in(m_.get(), &c_, p.data(), d, &in));
    return in != 0;
  }
  const pcgx_sac_plane &plane() const { return c_; }

 private:
  ModelHandle m_;
  pcgx_sac_plane c_;
  int64_t score_;
};

// voxelGridSurfaceModel (surface.go:9-34): copies the cloud and the grid's buckets at construction
class VoxelGridSurfaceModel {
 public:
  VoxelGridSurfaceModel(const BucketVoxelGrid &vg, const CloudView &ra, bool on_device = false) {
    pcgx_sac_plane_model *h = nullptr;
    check(pcgx_sac_plane_model_create(vg.handle(), ra.data, ra.points, ra.stride, ra.xyz_offset, on_device ? 1 : 0, &h));
    h_ = ModelHandle(h, [](pcgx_sac_plane_model *p) { pcgx_sac_plane_model_free(p); });
  }
  std::pair<int, int> NumRange() const { return {3, 3}; }
  struct Result {
    bool found = false;
    int64_t best = -1, best_score = 0;
    std::unique_ptr<Coefficients> best_coeff;
    std::vector<int32_t> ok;
    std::vector<pcgx_sac_plane> coeff;
    std::vector<int64_t> score;
  };
  // Fit + Evaluate of ids.size() / 3 hypotheses
  Result Compute(const std::vector<int64_t> &ids) const {
    if (ids.size() % 3) throw Error(PCGX_E_INVALID, "three ids per hypothesis");
    const int64_t n = (int64_t)ids.size() / 3;
    Result r;
    r.ok.resize((size_t)n);
    r.coeff.resize((size_t)n);
    r.score.resize((size_t)n);
    int32_t found = 0;
    pcgx_sac_plane bc{};
    check(pcgx_sac_plane_compute(h_.get(), ids.data(), n, &found, &r.best, &r.best_score, &bc, r.ok.data(),
                                 r.coeff.data(), r.score.data()));
    r.found = found != 0;
    if (r.found) r.best_coeff.reset(new Coefficients(h_, bc, r.best_score));
    return r;
  }
  // surface.go:36-181: nullptr when the three points give no plane
  std::unique_ptr<Coefficients> Fit(const std::vector<int64_t> &ids) const {
    if (ids.size() != 3) return nullptr;
    Result r = Compute(ids);
    if (!r.ok[0]) return nullptr;
    return std::unique_ptr<Coefficients>(new Coefficients(h_, r.coeff[0], r.score[0]));
  }

 private:
  ModelHandle h_;
};

class SAC {  // sac.go:23-63
 public:
  SAC(Sampler &s, const VoxelGridSurfaceModel &m) : sampler_(&s), model_(&m) {}
  // false keeps the previous Coefficients()
  bool Compute(int n) {
    std::vector<int64_t> ids;
    ids.reserve((size_t)(n > 0 ? n : 0) * 3);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < model_->NumRange().first; j++) ids.push_back(sampler_->Sample());
    auto r = model_->Compute(ids);
    if (!r.found) return false;
    best_ = std::move(r.best_coeff);
    return true;
  }
  const sac::Coefficients *Coefficients() const { return best_.get(); }  // nullptr before the first success

 private:
  Sampler *sampler_;
  const VoxelGridSurfaceModel *model_;
  std::unique_ptr<sac::Coefficients> best_;
};

}  // namespace sac

}  // namespace pcgx
