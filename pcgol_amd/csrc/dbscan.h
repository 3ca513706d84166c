// dbscan.h -- what cluster.hip and dbscan.hip ask of each other.  Density clustering (include/pcgx.h, "density
// clusters") is cluster extraction with the core flags in place of the usable flags and the border points attached before
// the per-root counts: cluster.hip keeps the stages, the union-find and the whole tail (one body), dbscan.hip brings the
// two passes that are new and the entry points.
#pragma once
#include "pcgx_internal.h"

namespace pcgx {

// What density adds to a clusters call.  min_pts == 1 is Euclidean clustering (every usable point is core): no count
// pass, no border pass, only kind.
struct ClusterDensity {
  int32_t min_pts;   // >= 1
  bool count_all;    // the flag pass counts the whole neighbourhood instead of stopping at min_pts (measurements)
  uint8_t *d_kind;   // [n] by id, may be nullptr
};

// cluster.hip: Len() > 0, everything device resident; temporaries from ctx().arena, which the caller has begun.
// a: the tree the neighbourhoods come from (resolve_tree; nullptr: every point was deleted); n: the handle's Len().
// density: nullptr for pcgx_kdtree_clusters.
pcgx_status clusters_enqueue(const pcgx_kdtree *a, int64_t n, float radius, const float *d_normals, float min_cos,
                             int32_t oriented, const float *d_curvature, float max_curvature, int64_t min_size,
                             int64_t max_size, const ClusterDensity *density, int32_t *d_labels, int32_t *d_n_clusters,
                             int32_t *d_sizes, int32_t *d_ids, hipStream_t st);
pcgx_status clusters_check(const char *fn, const pcgx_kdtree *t, float radius, const void *normals, float min_cos,
                           const void *curvature, float max_curvature, int64_t min_size, int64_t max_size,
                           const void *labels, const void *n_clusters);

// dbscan.hip.  Positions: the grid's cell order where on_grid, else ids (core and kindp zeroed by the caller: an id
// without a node stays 0).
// core[pos] = 1 where the point there is core, else 0.
void dbscan_flags_launch(const pcgx_kdtree *a, bool on_grid, int64_t n, float bound, int32_t min_pts, bool count_all,
                         uint8_t *core, hipStream_t st);
// kindp[pos] = 2 core, 1 border, 0 neither; parent[pos] = the position of a border point's nearest core neighbour (a
// store to the lane's own word; the component passes are done, pointer jumping follows).
void dbscan_border_launch(const pcgx_kdtree *a, bool on_grid, int64_t n, float bound, const uint8_t *core, uint8_t *kindp,
                          uint32_t *parent, hipStream_t st);
// kind[id] = kindp[pos], or with all_core 2 wherever kindp[pos] != 0.  pts: the grid's records, nullptr: positions are ids.
void dbscan_kind_launch(const float4 *pts, int64_t n, const uint8_t *kindp, bool all_core, uint8_t *kind, hipStream_t st);
// core_by_id[id] = 1 where point id of the tree (no deletions) is core, else 0; temporaries from ctx().arena, which
// the caller has begun.  (radius outlier removal, sor.hip)
pcgx_status dbscan_core_by_id_enqueue(const pcgx_kdtree *t, float radius, int32_t min_pts, uint8_t *d_core_by_id,
                                      hipStream_t st);

}  // namespace pcgx
