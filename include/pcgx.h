/*
 * pcgx.h -- C ABI of libpcgx.so, the MI355X (gfx950) point-cloud hot path that
 * plugs in behind seqsense/pcgol's Go interfaces.
 *
 * The reference has NO FFI of its own (pure Go); its seams are Go interfaces.
 * Every entry point below names the reference interface / function it
 * replaces (paths relative to the reference repository root).  A cgo shim
 * (go/) implements those Go interfaces by calling these
 * symbols.  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *  - every function returns a pcgx_status (0 = OK); pcgx_last_error() gives
 *    the message of the last failure on the calling thread.
 *  - "host" pointers are ordinary process memory owned by the caller (Go
 *    slices); the library copies in/out before returning and never retains
 *    them (cgo pointer rules).
 *  - "_dev" entry points take DEVICE pointers (hipMalloc / pcgx_dev_alloc /
 *    torch tensor .data_ptr()) and a HIP stream passed as void* (NULL = the
 *    library's own stream); they only enqueue work.
 *  - point clouds are the reference's AoS little-endian records
 *    (pc/pointcloud.go:64-78): record i = data + i*stride, xyz = three
 *    consecutive float32 at byte offset xyz_off (pc/pointcloud.go:130-163).
 *  - Mat4 is column-major float[16] (mat/mat4.go:8-10).
 *  - ids are indices into the accessor the tree was built from
 *    (Vec3At(id), pc/storage/search.go:8-11); -1 = not found.
 */
#ifndef PCGX_H
#define PCGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCGX_API __attribute__((visibility("default")))

typedef int32_t pcgx_status;
enum {
  PCGX_OK = 0,
  PCGX_E_NO_POINT = 1,         /* pc/minmax.go:10-12 errors.New("no point") */
  PCGX_E_NOT_ENOUGH_PAIRS = 2, /* icp/evaluator.go:16 ErrNotEnoughPairs */
  PCGX_E_BAD_FIELD = 3,        /* pc/pointcloud.go:115 "invalid field name" / bad stride, offset */
  PCGX_E_HIP = 4,              /* HIP runtime failure (no GPU, launch error, ...) */
  PCGX_E_OOM = 5,              /* host or device allocation failed */
  PCGX_E_INVALID = 6,          /* invalid argument (NULL handle, negative count, ...) */
  PCGX_E_OUT_OF_RANGE = 7,     /* voxel index outside the dense grid: the Go code panics here
                                  (pc/filter/voxelgrid/voxelgrid.go:151); we return an error */
  PCGX_E_TOO_LARGE = 8,        /* tree larger than 2^26 points (traversal frame encoding) */
  PCGX_E_NEED_GRADIENT = 9,    /* icp/icp.go:15 ErrNeedGradient (kept for the Go shim's mapping) */
  PCGX_E_SINGULAR = 10,        /* point-to-plane extension: 6x6 normal equations not positive definite */
  PCGX_E_SYNTAX = 11,          /* PCD: strconv.ErrSyntax / ErrRange from a header or ascii token (pc/io.go) */
  PCGX_E_EOF = 12,             /* PCD: io.EOF / io.ErrUnexpectedEOF */
  PCGX_E_CORRUPT = 13,         /* PCD: lzf.ErrDataCorruption / lzf.ErrInsufficientBuffer */
  PCGX_E_BAD_HEADER = 14,      /* PCD: the errors.New cases of pc/io.go:55,119,125-133,202 */
  PCGX_E_RCCL = 15             /* the exchange of the sharded ICP path failed (RCCL missing / error, callback error) */
};

/* ------------------------------------------------------------ lifecycle */

/* Selects HIP device `device` for this process (one process per GPU) and
 * creates the library stream.  Idempotent. */
PCGX_API pcgx_status pcgx_init(int32_t device);
PCGX_API pcgx_status pcgx_shutdown(void);
/* One process, several GPUs (threading row: "one process drives all 8 GPUs" -- the reference is one
 * process, icp.go:23).  The library keeps one set of streams, workspaces and call contexts per DEVICE SLOT; slot k
 * works on HIP device device_ids[k] (NULL: device k; the same device may be named several times, which is how the
 * several-GPU paths run on a one-GPU test box).  A host thread names the slot its calls are for with
 * pcgx_set_device (default 0, per thread, like HIP's current device); a handle (tree, session, communicator)
 * belongs to the slot it was made on and is used from threads that have that slot current.
 * pcgx_icp_fit_multi below needs nothing else from the caller: it starts a thread per slot itself. */
PCGX_API pcgx_status pcgx_init_devices(int32_t n, const int32_t *device_ids);
PCGX_API pcgx_status pcgx_set_device(int32_t slot);
PCGX_API pcgx_status pcgx_get_device(int32_t *slot, int32_t *hip_device);
/* Copies the last error message of the calling thread; returns its length. */
PCGX_API int32_t pcgx_last_error(char *buf, size_t cap);
PCGX_API const char *pcgx_version(void);
/* The layout version of this header's structs and fixed-size output arrays (pcgx_icp_params gained sums_mode in 3;
 * pcgx_debug_icp_strict_stats writes 64 words since 3; 4: device slots, pcgx_icp_fit_multi, pcgx_debug_voxel_stats;
 * 5: pcgx_debug_shard_stats, pcgx_prof_read_max, words 48 .. 63 of pcgx_debug_icp_strict_stats re-assigned;
 * 6: pcgx_debug_ring_kinds, pcgx_debug_host_walks, pcgx_debug_icp_one_launch;
 * 7: pcgx_debug_grid_runner, pcgx_debug_icp_runner_pairs).
 * A binding built against another version of the header must not call into the library: the mirrors (go/pcgx,
 * host/pcgx.hpp, pcgol_amd/_lib.py) compare PCGX_ABI_VERSION with pcgx_abi_version() when they load it.
 * pcgx_icp_params_init zeroes a parameter block of THIS version (all defaults); sizeof_params is the caller's
 * sizeof(pcgx_icp_params): a mismatch is PCGX_E_INVALID instead of a read past a shorter struct. */
#define PCGX_ABI_VERSION 7
PCGX_API int32_t pcgx_abi_version(void);
/* Block until all work enqueued on `stream` (NULL = library stream) is done. */
PCGX_API pcgx_status pcgx_sync(void *stream);
/* Threading.  Handles are immutable after build (DeletePoint excepted, as in the reference,
 * kdtree.go:322-332).  The blocking host-pointer entry points -- pcgx_kdtree_build, _nearest_batch,
 * _range_count / _range_fill, pcgx_voxel_filter, pcgx_minmax, pcgx_icp_fit / _evaluate / _pairs --
 * may be called from any number of threads at once: each call works on a stream and workspace of
 * its own (a pool of 4; a fifth caller waits) and they overlap on the GPU.  Entry points with a
 * `stream` argument (the `_dev` calls, ICP sessions) and everything else run one caller at a time
 * in the library's context, so that work given to the NULL stream stays ordered.
 * Measurement aid: out = {largest number of pooled calls in flight at once, pooled calls} since the
 * last reset. */
PCGX_API pcgx_status pcgx_debug_call_stats(int64_t out[2], int32_t reset);
/* Measurement / test aid: queries answered on the HOST since the last reset.  pcgx_kdtree_nearest_batch, _range_count
 * and _range_fill with at most 32 queries (PCGX_HOST_WALK_MAX; 0: never) -- what storage.Search.Nearest / Range for one
 * point come to (pc/storage/search.go:13-17) -- are answered by the reference-order walk (kdtree.go:83-222) on the
 * handle's host mirror of the tree, the one DeletePoint patches: no launch, no PCIe round trip; ids, DistSq bits, tie
 * winners and MinDistSq > 0 answers are those of the device path (csrc/knn_explicit.hip). */
PCGX_API pcgx_status pcgx_debug_host_walks(int64_t *queries, int32_t reset);
/* Measurement / test aid: launches of the ONE-LAUNCH Fit since the last reset (csrc/icp_small.hip: PointToPointICPGradient.Fit,
 * icp.go:23-67, for small clouds -- every iteration of the loop inside one launch).  out = {launches, of them with
 * the tree's chunks looked at only below chunks that could not be ruled out (a queue, or band by band), of them with the
 * targets grouped by place}. */
PCGX_API pcgx_status pcgx_debug_icp_one_launch(int64_t out[3], int32_t reset);
/* Measurement / test aid: which path the VoxelGrid filter calls took since the last reset.  The filter
 * (voxelgrid.go:136-187) has two device paths with identical output: the bucket path (the coordinates travel
 * with the sort keys, a workgroup per bucket of cells; csrc/voxel_bucket.hip) and the radix path (stable sort of
 * (key, index) pairs + gather; csrc/voxel.hip), which also takes what the bucket path gives up on.
 * out = {calls the bucket path answered, bucket attempts given up (a bucket or a cell too crowded),
 *        flags of the last attempt given up (1 bucket, 2 cell, 4 exchange), low key bits of the last plan}. */
PCGX_API pcgx_status pcgx_debug_voxel_stats(int64_t out[4], int32_t reset);
/* Measurement / test aid: how the sharded steps with the reference's sums were exchanged since the last reset
 * (see "The sharded ICP path" below).  out = {steps enqueued in the ring form, steps in the collective form,
 * rings made (shared memory of the node's processes, or the one process's pinned block), ring set-ups that
 * ended with the collective form (no shared memory between the ranks, PCGX_SHARD_RING=0)}. */
PCGX_API pcgx_status pcgx_debug_shard_stats(int64_t out[4], int32_t reset);
/* ... and where the rings made since the last reset keep their inboxes' data words: out = {rings whose inboxes live
 * in the ranks' DEVICE memory, mapped by their peers (hipIpcOpenMemHandle between processes, peer access between the
 * device slots of one process: a hop is one store over xGMI and a poll of local HBM), rings whose data words stay in
 * host-coherent memory (a rank could not export / map an inbox, PCGX_RING_MEM=host: a PCIe round trip per poll)}.
 * Counted once per communicator, by its rank 0 (pcgx_icp_fit_multi: by slot 0). */
PCGX_API pcgx_status pcgx_debug_ring_kinds(int64_t out[2], int32_t reset);

/* Optional in-library kernel timing (HIP events on the launch stream around
 * the named kernel class).  Used by bench.py for the live roofline figure. */
enum {
  PCGX_PROF_ICP_WALK = 0,   /* icp_corr_kernel (tree walk of the targets the grid pass left + reduce;
                               every target when the base tree has no grid) */
  PCGX_PROF_KNN_WALK = 1,   /* nearest_kernel */
  PCGX_PROF_VOXEL_ALL = 2,  /* whole voxel-filter pipeline of one call */
  PCGX_PROF_SORT_SCATTER = 3, /* rs_scatter_kernel (radix sort passes) */
  PCGX_PROF_ICP_GRID = 4,   /* icp_grid_kernel (re-projection + certified nearest + sums) */
  PCGX_PROF_KNN_GRID = 5,   /* grid_nearest_kernel */
  PCGX_PROF_STRICT_TERMS = 6, /* strict_tilesum_kernel (sessions whose correspondence kernel does not form the tile sums) */
  PCGX_PROF_STRICT_SUM = 7,   /* strict_sum_kernel (terms into LDS, parity summaries, one record per (sum, tile)) */
  PCGX_PROF_STRICT_CHAIN = 8, /* strict_chain_kernel (runs applied in order + pose update) */
  PCGX_PROF_STRICT_JOB = 9,   /* strict_job_kernel (tiles that cross a level / have no window) */
  PCGX_PROF_ICP_LEFTOVER = 10, /* icp_corr_kernel behind the grid pass (leftover walk; strict: + tile sums) */
  PCGX_PROF_KINDS = 11
};
/* on: 0 = off, 1 = every launch, n > 1 = every n-th launch of each kind (a pair of events around a
 * 30 us kernel costs several us of stream time: sampling keeps the timed run close to the untimed one). */
PCGX_API pcgx_status pcgx_prof_enable(int32_t on);
/* Resolves pending events; returns accumulated milliseconds and launch count
 * of `kind` since the last pcgx_prof_reset(). */
PCGX_API pcgx_status pcgx_prof_read(int32_t kind, double *total_ms, int64_t *launches);
/* ... and the longest single launch of `kind` since the last reset (the iteration a latency-bound kernel took longest in) */
PCGX_API pcgx_status pcgx_prof_read_max(int32_t kind, double *max_ms);
PCGX_API pcgx_status pcgx_prof_reset(void);

/* Profiling aid (not part of the drop-in surface): counters of the instrumented exact-mode walk
 * over device-resident queries: {loop iterations, active lanes summed, node fetches, emit/refill
 * sections, chunks prepared, queries verified to the leaf, first-descent levels kept, queries,
 * fetches while descending, explicit pops, passing, first-descent pops, passing, leaves,
 * iterations after the last hand-out, most iterations of a wave, 100 MHz ticks summed over waves
 * before / after the last hand-out, longest wave in ticks, waves, kernel ns, queries finished
 * inside the preparation, lane-steps / iterations of its descent loop, ticks per phase (6), -, -}. */
typedef struct pcgx_kdtree pcgx_kdtree;
PCGX_API pcgx_status pcgx_debug_walk_stats(const pcgx_kdtree *t, const float *d_q, int64_t nq, float max_range,
                                           int32_t presort, const float *d_hint_xyz, uint32_t *d_leaf_io,
                                           uint64_t stats32[32]);

/* Tuning aid (not part of the drop-in surface): out = {queries of the batch the grid pass leaves to
 * the tree walk, grid cells, 1000 x mean number of other points in a point's cell, grid in use,
 * lane-slots the scan loops ran (64 per round of 4 records per wave, idle lanes included),
 * queries per reason 1..7 (csrc/knn_grid.h), point records read, cell-bound words read}. */
PCGX_API pcgx_status pcgx_debug_grid_stats(const pcgx_kdtree *t, const float *d_q, int64_t nq, float max_range,
                                           int64_t out[14]);

/* Test aid: where the grid's cells lie: geom = {lo.x, lo.y, lo.z, h, 1 / h}, dims = {nx, ny, nz}.  A point's cell along
 * an axis is (int)clamp((v - lo) * (1 / h), 0, n - 1), evaluated in float32; a grid row is the cells of one (y, z).
 * PCGX_E_INVALID for a tree without a grid. */
PCGX_API pcgx_status pcgx_debug_grid_geometry(const pcgx_kdtree *t, float geom[5], int32_t dims[3]);

/* Test aid: the points' certificates (csrc/knn_grid.hip, grid_cert_kernel), by point id, n floats into host memory.
 * A query whose DistSq to point i is below cert[i] has i as its one nearest base point; 0: no certificate (a point
 * with a twin).  PCGX_E_INVALID when the tree has none (no grid, labelled points). */
PCGX_API pcgx_status pcgx_debug_grid_cert(const pcgx_kdtree *t, float *cert, int64_t n);
/* ... and their runner-up records, made beside the certificates: runner[4 i ..] = {the nearest other point n1 of point
 * i, cert2}, runner_id[i] = n1's id.  A query whose DistSq to point i is below cert2 has i or n1 as its nearest base
 * point, whichever computes nearer; cert2 = 0: no record.  *below: ICP pairs carry the record where cert[i] is below it
 * (PCGX_GRID_RUNNER_BELOW, in cell edges; +inf: every pair).  +20 bytes of device memory per base point. */
PCGX_API pcgx_status pcgx_debug_grid_runner(const pcgx_kdtree *t, float *runner, uint32_t *runner_id, float *below, int64_t n);

/* Measurement aid: what the grid pass of the session's NEXT iteration would read, without changing
 * the session: out = {targets, targets left to the walk, point records read, cell-bound words read,
 * lane-slots its scan loops run (64 per round of 4 records per wave, idle lanes included), targets that keep last
 * iteration's partner on its certificate and are not searched for at all (the counts before it are those of searching
 * for every target)}. */
typedef struct pcgx_icp_session pcgx_icp_session;
PCGX_API pcgx_status pcgx_debug_icp_grid_stats(pcgx_icp_session *s, void *stream, int64_t out[6]);

/* Measurement aid: counters of the strict sums (set_strict 1) since the last call: out = {runs
 * applied, runs whose record did not cover the state, tiles recomputed exactly, leaves of those added
 * term by term, tile records that did not cover the state, -...}; words [48 .. 57]: states that missed their
 * tile's candidate table by log2 of the distance ([57]: other sign), [58]: plain tiles the repair pass of a Fit's first
 * Evaluate turned into jobs, [60] / [61]: ticks later chunks' walkers waited for their start state (all / the rows' last
 * chunks), [62]: walkers that gave up that wait and walked the earlier chunks alone, [63]: workgroups of the summary
 * kernel that gave up its exchange (both 0 in a healthy run: the tests require it). */
PCGX_API pcgx_status pcgx_debug_icp_strict_stats(pcgx_icp_session *s, void *stream, int64_t out[64]);
/* Words [47] and [59] of the above belong to the certified steps (the summary kernel tests every pair against its
 * partner's certificate): [47] low word = certified steps, high word = those enqueued again; [59] = targets searched
 * inside them.
 * Test / measurement aid for level 2 of those certificates (PCGX_ICP_CERT2): a strict session's pairs in the caller's
 * target order, {partner, its certificate (-1: no pair)}, and the runner words beside them (4 nt floats, 4 nt floats, nt
 * words into host memory; all three NULL: none), and counts (may be NULL) = since the last call {targets that failed
 * their certificate and kept their partner on its runner-up's record, targets moved to the runner-up, all that failed
 * their certificate while level 2 was on} -- the third less the first two is what [59] counted in those steps.
 * PCGX_E_INVALID for a session that keeps no runner words. */
PCGX_API pcgx_status pcgx_debug_icp_runner_pairs(pcgx_icp_session *s, void *stream, float *match_caller, float *runner_caller,
                                                 uint32_t *runner_id_caller, int64_t nt, int64_t counts[3]);

/* The strict-sum pipeline in plain host loops (no GPU): *out = the sequential float32 sum
 * 0 + t0 + t1 + ... computed the way the strict kernels compute it; stats as in csrc/strict_sum.h
 * (ss_host_model).  For tests of the arithmetic.  mode bit 0: general leaf form only; bit 1: no
 * error-prefix refinement. */
PCGX_API pcgx_status pcgx_debug_strict_sum_host(const float *terms, int64_t n, int32_t mode, float *out,
                                                int64_t stats[8]);

/* The same on the device: the strict_sum / strict_job / strict_chain kernels (csrc/strict.hip) run on terms given
 * as they are -- terms[9][n] (row-major, host memory), out[k] = 0.0f + terms[k][0] + terms[k][1] + ... in sequential
 * float32 -- instead of on the terms of a session's pairs.  For GPU tests with rows no registration produces (a tie
 * at every step, cancellation to zero, subnormals, overflow, NaN).  stats (may be NULL): the counters of
 * pcgx_debug_icp_strict_stats. */
PCGX_API pcgx_status pcgx_debug_strict_sum_dev(const float *terms, int64_t n, float out[9], int64_t stats[64]);

/* Device memory helpers for hosts that have no HIP binding of their own. */
PCGX_API pcgx_status pcgx_dev_alloc(size_t bytes, void **dptr);
PCGX_API pcgx_status pcgx_dev_free(void *dptr);
PCGX_API pcgx_status pcgx_dev_upload(void *dptr, const void *host, size_t bytes);
PCGX_API pcgx_status pcgx_dev_download(void *host, const void *dptr, size_t bytes);

/* --------------------------------------------------------------- KD-tree
 * replaces pc/storage/kdtree: kdtree.New (kdtree.go:33-56, newNode :348-370),
 * KDTree.Nearest (:83-146, searchLeafNode :199-222), MinDistSq field (:22),
 * behind storage.Search (pc/storage/search.go:13-17).
 */
typedef struct pcgx_kdtree pcgx_kdtree;

/* kdtree.New(ra): builds the median-split tree (dim = depth%3, upper median,
 * ties on the split axis ordered stably by current position) and uploads it.
 * n == 0 -> PCGX_E_NO_POINT (the Go code panics, kdtree.go:355-356). */
PCGX_API pcgx_status pcgx_kdtree_build(const void *data, int64_t n, int32_t stride,
                                       int32_t xyz_off, pcgx_kdtree **out);
PCGX_API pcgx_status pcgx_kdtree_free(pcgx_kdtree *t);
/* Len() of the accessor the tree indexes (pc/randomaccess.go:9). */
PCGX_API pcgx_status pcgx_kdtree_len(const pcgx_kdtree *t, int64_t *n);
/* node.maxDepth(0) (kdtree.go:385-395). */
PCGX_API pcgx_status pcgx_kdtree_max_depth(const pcgx_kdtree *t, int32_t *depth);
/* In-order point ids (child0, node, child1): the final state of the
 * reference's in-place sorted indice slice; defines the whole tree.  After DeletePoint: the
 * remaining ids (live_count of them) in the in-order sequence of the canonical tree over them. */
PCGX_API pcgx_status pcgx_kdtree_inorder(const pcgx_kdtree *t, int64_t *ids /* [n] host */);
/* Vec3At(id) for a batch of ids (pc/randomaccess.go:8). */
PCGX_API pcgx_status pcgx_kdtree_points(const pcgx_kdtree *t, const int64_t *ids, int64_t m,
                                        float *xyz /* [3m] host */);

/* The tree as the reference holds it (kdtree.go:25-29), pre-order: node k = {id, dim, index of
 * child0, index of child1} in the dump (-1 = nil); after DeletePoint the patched tree.  *n_nodes =
 * nodes in the tree, the first min(n_nodes, cap_nodes) quadruples are written. */
PCGX_API pcgx_status pcgx_kdtree_dump(const pcgx_kdtree *t, int64_t *out4, int64_t cap_nodes, int64_t *n_nodes);

/* KDTree.DeletePoint (kdtree.go:322-332) for a batch of ids.  An id outside [0, Len()) is
 * PCGX_E_OUT_OF_RANGE (the reference's "does not correspond to any point in the tree",
 * :323-325) and deletes nothing; deleting a point twice is a no-op (kdtree_test.go:576-650).
 * Len() / Vec3At() keep describing the accessor (all points), as in the reference.
 * The handle then keeps the reference's own patched tree (findMinimumImpl / deleteNodeImpl,
 * :224-320, applied in call order on a host mirror) and Nearest / Range walk an explicit device
 * copy of it in the reference's visit order: ids and DistSq as the Go code returns them, exact ties
 * and MinDistSq > 0 included (slower than the implicit tree: no speculative descent).  max_depth
 * and pcgx_kdtree_dump describe the patched tree.  ICP sessions created on such a handle walk the
 * patched tree as well (and see later deletions); a session created before the first deletion keeps
 * the tree it was created on.  Region growing uses a canonical tree rebuilt over the remaining points
 * (Range hits are a set: same components). */
PCGX_API pcgx_status pcgx_kdtree_delete_points(pcgx_kdtree *t, const int64_t *ids, int64_t m);
/* Points still in the tree (Len() minus deleted). */
PCGX_API pcgx_status pcgx_kdtree_live_count(const pcgx_kdtree *t, int64_t *n_live);

/* Batched KDTree.Nearest: for each query i the exact result of
 * k.Nearest(q[i], max_range) with k.MinDistSq = min_dist_sq, i.e.
 * {ID, DistSq} or {-1, max_range^2} (kdtree.go:84-86,100-103).
 * q is packed xyz float32 [3*nq]. */
PCGX_API pcgx_status pcgx_kdtree_nearest_batch(const pcgx_kdtree *t, const float *q, int64_t nq,
                                               float max_range, float min_dist_sq,
                                               int64_t *ids /* [nq] */, float *dist_sq /* [nq] */);

/* Batched KDTree.Range (kdtree.go:148-197): all points with DistSq < max_range^2, per query
 * sorted by DistSq (ties: discovery order of the reference walk; Go's sort leaves them
 * unspecified).  The result length is data dependent, hence two calls:
 *   count: counts[i] = number of neighbours of q[i];
 *   fill:  offsets[0..nq] = exclusive prefix sum of the counts (offsets[nq] = total); query i's
 *          neighbours are written to ids / dist_sq [offsets[i], offsets[i+1]). */
PCGX_API pcgx_status pcgx_kdtree_range_count(const pcgx_kdtree *t, const float *q, int64_t nq,
                                             float max_range, int64_t *counts /* [nq] */);
PCGX_API pcgx_status pcgx_kdtree_range_fill(const pcgx_kdtree *t, const float *q, int64_t nq,
                                            float max_range, const int64_t *offsets /* [nq+1] */,
                                            int64_t *ids, float *dist_sq);

#define PCGX_KNN_PRESORT 1u /* Morton-order the queries inside the call (results are
                               returned in the caller's order either way) */
/* Same, device resident: d_q packed xyz [3*nq], d_ids int32 [nq], d_dist_sq [nq]. */
PCGX_API pcgx_status pcgx_kdtree_nearest_batch_dev(const pcgx_kdtree *t, const float *d_q,
                                                   int64_t nq, float max_range,
                                                   float min_dist_sq, uint32_t flags,
                                                   int32_t *d_ids, float *d_dist_sq,
                                                   void *stream);

/* ------------------------------------------------------------- VoxelGrid
 * replaces pc/filter/voxelgrid: voxelgrid.New(leaf, WithChunkSize(chunk))
 * .Filter(pp) (voxelgrid.go:23-187, option.go:14-18) behind filter.Filter
 * (pc/filter/filter.go:7-9), incl. pc.MinMaxVec3 (pc/minmax.go:9-26).
 */

/* pc.MinMaxVec3 over an AoS cloud. n == 0 -> PCGX_E_NO_POINT. */
PCGX_API pcgx_status pcgx_minmax(const void *data, int64_t n, int32_t stride, int32_t xyz_off,
                                 float vmin[3], float vmax[3]);

/* Filter: out_data must hold n*stride bytes (worst case); *out_n = number of
 * output records (Width of the returned cloud, Height = 1).  chunk = {0,0,0}
 * (any product == 0) selects the non-chunked path (voxelgrid.go:45-47).
 * A non-finite coordinate (NaN, +-inf) or a point whose cell lies outside the
 * dense grid ends the call with PCGX_E_OUT_OF_RANGE, as the Go code panics. */
PCGX_API pcgx_status pcgx_voxel_filter(const void *data, int64_t n, int32_t stride,
                                       int32_t xyz_off, const float leaf[3],
                                       const int32_t chunk[3], void *out_data, int64_t *out_n);
/* Device resident: d_data/d_out are device buffers (d_out >= n*stride bytes);
 * *out_n is known when the call returns (it synchronises internally for the grid set-up and
 * the count), but the kernels that fill d_out may still be running on `stream`. */
PCGX_API pcgx_status pcgx_voxel_filter_dev(const void *d_data, int64_t n, int32_t stride,
                                           int32_t xyz_off, const float leaf[3],
                                           const int32_t chunk[3], void *d_out,
                                           int64_t *out_n, void *stream);

/* ------------------------------------------------------------------- ICP
 * replaces pc/registration/icp: NearestPointCorresponder.Pairs
 * (correspondence.go:22-37), PointToPointEvaluator.Evaluate (evaluator.go:91-189,
 * default weight w == 1), gradientDescentUpdater.Update (updater.go:44-71,
 * rodrigues.go:11-33) and PointToPointICPGradient.Fit (icp.go:23-67).
 */

/* icp.Evaluated (evaluator.go:25-30); Hessian is never written by the
 * reference (HasHessian() == false, :76) and is omitted. */
typedef struct {
  float value;
  float gradient[6];
  float dist_rms;
  int64_t num_pairs;
} pcgx_icp_evaluated;

/* NearestPointCorresponder{MaxDist}, PointToPointEvaluator{MinPairs},
 * KDTree.MinDistSq, GradientDescentUpdaterFactory{Weight,Threshold,MaxIteration}
 * (zero values select the reference defaults 6 / 0.3 / 0.01 / 20,
 * evaluator.go:92-95, updater.go:15-37). */
typedef struct {
  float max_dist;
  float min_dist_sq;
  int32_t min_pairs;
  float weight[6];
  float threshold[6];
  int32_t max_iteration;
  /* PointToPointEvaluator.WeightFn (evaluator.go:19-23,72,110-113,130): the reference takes any Go
   * closure w = WeightFn(distSq); arbitrary host code cannot run on the device, so the weight is
   * one of the built-in forms below, each evaluated in float32 exactly as the Go expression next to
   * it (the Go shim hands out the matching closure, go/pcgx: WeightFn.Func()).  0 = the reference's
   * default.  Not offered for the point-to-plane extension. */
  int32_t weight_fn;
  float weight_fn_param; /* a */
  /* How the evaluator's nine sums (evaluator.go:122-145) are formed: PCGX_SUMS_* below.  0 = the
   * reference's own sums wherever they are defined (one GPU: bit-identical Evaluated and pose). */
  int32_t sums_mode;
} pcgx_icp_params;

PCGX_API pcgx_status pcgx_icp_params_init(pcgx_icp_params *p, size_t sizeof_params);

/* pcgx_icp_params.sums_mode.  The reference adds float32 terms pair after pair in target order; its
 * result carries that chain's rounding (~1.6e-5 on the final transform at 1M pairs), so only a sum
 * formed the same way meets "within 1e-5 of the Go code" at every size.
 *  PCGX_SUMS_REFERENCE  (0, default) the reference's sequential float32 additions, evaluated exactly by
 *                       the whole GPU (csrc/strict_sum.h) -- pcgx_icp_fit / _evaluate / sessions on one
 *                       GPU, and sharded sessions (pcgx_icp_session_step_sharded, pcgx_icp_fit_sharded,
 *                       pcgx_icp_fit_multi: the order is the ranks' tiles one after the other).  The
 *                       point-to-plane extension has no reference sums to reproduce: float64 sums.
 *  PCGX_SUMS_F64_TREE   fixed-order float64 reduction of the same float32 terms: more accurate than the
 *                       reference, equal to it up to ITS rounding noise; what a sharded sum computes.
 *  PCGX_SUMS_REFERENCE_CHAIN  the reference's additions by ONE wave, term after term (milliseconds per
 *                       1M pairs): the on-device cross-check of PCGX_SUMS_REFERENCE. */
enum {
  PCGX_SUMS_REFERENCE = 0,
  PCGX_SUMS_F64_TREE = 1,
  PCGX_SUMS_REFERENCE_CHAIN = 2,
  PCGX_SUMS_KINDS = 3
};

enum {
  PCGX_WEIGHT_ONE = 0,      /* DefaultEvaluateWeightFn: return 1 */
  PCGX_WEIGHT_CONSTANT = 1, /* return a */
  PCGX_WEIGHT_INVERSE = 2,  /* return 1 / (a + d)                                   (Cauchy-like) */
  PCGX_WEIGHT_HUBER = 3,    /* if d <= a { return 1 }; return float32(math.Sqrt(float64(a / d)))   (k^2 = a) */
  PCGX_WEIGHT_TUKEY = 4,    /* if !(d < a) { return 0 }; u := 1 - d/a; return u * u               (c^2 = a) */
  PCGX_WEIGHT_KINDS = 5
};

/* icp.Stat (stat.go:3-6) */
typedef struct {
  pcgx_icp_evaluated evaluated;
  int32_t num_iteration;
} pcgx_icp_stat;

/* Pairs(): order-preserving compaction of matched targets.  Output arrays
 * hold nt entries (worst case, correspondence.go:24). */
PCGX_API pcgx_status pcgx_icp_pairs(const pcgx_kdtree *base, const float *target, int64_t nt,
                                    float max_dist, float min_dist_sq, int64_t *base_id,
                                    int64_t *target_id, float *dist_sq, int64_t *npairs);

/* Evaluate(base, target): fused correspondence + reduction on the GPU.
 * Fewer than min_pairs (0 -> 6) pairs -> PCGX_E_NOT_ENOUGH_PAIRS. */
PCGX_API pcgx_status pcgx_icp_evaluate(const pcgx_kdtree *base, const float *target, int64_t nt,
                                       float max_dist, float min_dist_sq, int32_t min_pairs,
                                       pcgx_icp_evaluated *out);

/* Host-only pieces (no GPU needed), exposed so a host can run the reference's
 * loop around its own exchange step:
 *  sums10 = {sum w*d2, G0..G5 sums, sum w*|pt|^2, sum w, pair count} (f64);
 *  finish = evaluator.go:156-186 (normalise, sqrt, rotation limiter). */
PCGX_API pcgx_status pcgx_icp_finish_evaluate(const double sums10[10], int32_t min_pairs,
                                              pcgx_icp_evaluated *out);
/* Update(trans, ev): *iter is the updater's iteration counter u.i;
 * *converged receives the bool result (updater.go:44-71). */
PCGX_API pcgx_status pcgx_icp_update(const pcgx_icp_params *p, int32_t *iter,
                                     const float gradient[6], float trans16[16],
                                     int32_t *converged);
/* rodriguesToRotation (rodrigues.go:11-33) and Mat4 helpers used by Fit. */
PCGX_API pcgx_status pcgx_rodrigues(const float v[3], float out16[16]);
PCGX_API pcgx_status pcgx_mat4_mul(const float m[16], const float a[16], float out16[16]);
PCGX_API pcgx_status pcgx_mat4_transform(const float m[16], const float *xyz, int64_t n,
                                         float *out_xyz);

/* Evaluate with every parameter of pcgx_icp_params that concerns it (max_dist, min_dist_sq, min_pairs,
 * weight_fn, weight_fn_param). */
PCGX_API pcgx_status pcgx_icp_evaluate_params(const pcgx_kdtree *base, const float *target, int64_t nt,
                                              const pcgx_icp_params *params, pcgx_icp_evaluated *out);

/* Fit(base, target): the whole loop stays on the device (evaluate + update
 * kernels, one download at the end).  On PCGX_E_NOT_ENOUGH_PAIRS trans16 and
 * stat->num_iteration hold the state at failure, like icp.go:49-53. */
PCGX_API pcgx_status pcgx_icp_fit(const pcgx_kdtree *base, const float *target, int64_t nt,
                                  const pcgx_icp_params *params, float trans16[16],
                                  pcgx_icp_stat *stat);

/* Device-resident ICP session: the same loop, cut at the per-iteration
 * exchange so that N processes (one per GPU, each with a replica of the base
 * tree and its own tile of the target) can all-reduce the 10 partial sums
 * between `partials` and `update`.  d_sums10 is a device
 * buffer of 10 doubles owned by the caller (e.g. a torch tensor handed to
 * torch.distributed.all_reduce == RCCL). */
typedef struct pcgx_icp_session pcgx_icp_session;
PCGX_API pcgx_status pcgx_icp_session_create(const pcgx_kdtree *base, const float *target,
                                             int64_t nt, int32_t target_on_device,
                                             const pcgx_icp_params *params, double *d_sums10,
                                             pcgx_icp_session **out);
PCGX_API pcgx_status pcgx_icp_session_free(pcgx_icp_session *s);
/* Restart the loop on the same target: trans = identity, counters cleared
 * (a new Fit, icp.go:46-47). */
PCGX_API pcgx_status pcgx_icp_session_reset(pcgx_icp_session *s, void *stream);
/* Overwrite the loop state's transform and updater counter (host-driven loops:
 * evaluate this rank's partial sums at a given pose).  iter == 0 means "no
 * re-projection yet" (the first Evaluate of Fit sees the raw target, icp.go:27-30). */
PCGX_API pcgx_status pcgx_icp_session_set_pose(pcgx_icp_session *s, const float trans16[16],
                                               int32_t iter, void *stream);
/* Copy the session's d_sums10 to the host (synchronises the stream). */
PCGX_API pcgx_status pcgx_icp_session_read_sums(pcgx_icp_session *s, double sums10[10], void *stream);
/* Enqueue transform(original target, current trans) + nearest + reduction of
 * this rank's tile into d_sums10.  No-op once the session has converged. */
PCGX_API pcgx_status pcgx_icp_session_partials(pcgx_icp_session *s, void *stream);
/* Enqueue evaluate-tail + Update from the (all-reduced) d_sums10 on the device. */
PCGX_API pcgx_status pcgx_icp_session_update(pcgx_icp_session *s, void *stream);
/* partials + update back to back, for a single GPU (no exchange in between): fewer launches. */
PCGX_API pcgx_status pcgx_icp_session_step(pcgx_icp_session *s, void *stream);

/* ---- the exchange of the sharded path -------------------------------------------
 * One process per GPU; every rank holds a replica of the base tree and one spatial tile of the
 * target.  A communicator is made from an id that rank 0 generates (pcgx_comm_unique_id) and the
 * host hands to every rank over any channel it has (a file, a socket, MPI, torch's store);
 * pcgx_comm_init is collective.  RCCL (xGMI inside a node) is bound at run time: a process that
 * never shards needs none.  pcgx_comm_init_callback is the same exchange through a host function
 * that sums `count` float64 in place over the ranks (the sums then make a round trip through host
 * memory): for hosts with a transport of their own, and for tests that run several ranks on one GPU.
 * pcgx_icp_session_step_sharded is one iteration on every rank, pcgx_icp_fit_sharded the whole Fit (icp.go:23-67) on
 * this rank's tile: every rank returns the same transform.  The sums (pcgx_icp_params.sums_mode):
 *  PCGX_SUMS_REFERENCE (default)  the reference's sequential float32 additions (evaluator.go:122-145) over the ranks'
 *      tiles ONE AFTER THE OTHER, rank 0's first: the sharded Fit returns what the reference's Fit returns on that
 *      concatenated target, bit for bit.  Correspondence, summaries and jobs run on all ranks at once; the ranks before
 *      a rank hand it two float64 totals per sum and the states their walk ended in (the walk is one dependent
 *      chain: it goes round the ranks).  Where the ranks can share host memory -- the processes of one node (a POSIX
 *      shared-memory segment every rank maps and registers with HIP, agreed on through the communicator's own
 *      all-reduce on first use), or the device slots of one process -- that is the RING form: no collective per
 *      iteration; every rank owns an inbox of tagged 64-bit words that the other GPUs' kernels write and its own
 *      kernels poll -- in its OWN GPU's memory, mapped by the peers (hipIpcGetMemHandle / hipIpcOpenMemHandle between
 *      processes, hipDeviceEnablePeerAccess between the slots of one: a store over xGMI, a poll of local HBM; the
 *      handles ride on the same set-up all-reduce; the mappings are tried out with a round of tagged words before a
 *      Fit depends on them), or in the host-coherent block where a rank cannot export or map one or the trial fails
 *      (pcgx_debug_ring_kinds says which); the abort words stay in the host block, hosts write them.  Every rank's
 *      kernels are resident at once and only the walkers wait, each for
 *      one word from the rank before it (csrc/strict.hip, strict_enqueue_ring).  Elsewhere (ranks on several nodes,
 *      PCGX_SHARD_RING=0): 2 + world collectives of <= 16 x world doubles per iteration.  Same bits either way.
 *      Several sessions on ONE communicator: allowed, stepped in any interleaving (A's step k, then B's step k, or
 *      one Fit after the other), as long as every rank makes its sharded calls on that communicator in the same
 *      order.  Each session's Fit is then its own, bit for bit: a ring word's tag names the communicator's step,
 *      not the session's.  A session's first step since it was made or reset begins a Fit on the communicator.  A
 *      rank that fails a step aborts the ring for every session on the communicator until one of them begins a Fit.
 *  PCGX_SUMS_F64_TREE  partials -> ONE all-reduce of the 10 (plane: 30) float64 sums -> update: faster, and off the
 *      reference by the reference's own rounding noise (1.6e-5 on the transform at 1M pairs).
 * Every collective also carries the ranks' error flag: a rank whose step fails keeps calling the collectives with its
 * flag up, and all ranks end the Fit in that same iteration (PCGX_E_RCCL on the others) -- none is left inside an
 * all-reduce.  Callers that drive the exchange themselves (pcgx_icp_session_partials -> their own all-reduce ->
 * pcgx_icp_session_update) MUST create the session with PCGX_SUMS_F64_TREE: sums of float32 chains cannot be added
 * across ranks.
 * In the ring form a failing rank raises an abort word in every inbox instead; a wait for a state that never comes is
 * bounded (10 s) and raises it too.
 * One process, several GPUs: pcgx_icp_fit_multi (a host thread per device slot, pcgx_init_devices; the ring in pinned
 * host memory, or the exchange in host memory, sums in rank order) -- the Go shim's FitMulti needs no second
 * process.  (Kernels that wait for one another must not queue up behind each other in one hardware queue: where slots
 * share ONE HIP device -- a test box -- pcgx_init_devices gives every slot's stream a hardware queue of its own.) */
typedef struct pcgx_comm pcgx_comm;
typedef struct { char internal[128]; } pcgx_comm_id;   /* == ncclUniqueId */
typedef int32_t (*pcgx_allreduce_fn)(double *host_buf, int32_t count, void *user);
PCGX_API pcgx_status pcgx_comm_unique_id(pcgx_comm_id *id);
PCGX_API pcgx_status pcgx_comm_init(int32_t rank, int32_t world, const pcgx_comm_id *id, pcgx_comm **out);
PCGX_API pcgx_status pcgx_comm_init_callback(int32_t rank, int32_t world, pcgx_allreduce_fn fn, void *user,
                                             pcgx_comm **out);
PCGX_API pcgx_status pcgx_comm_free(pcgx_comm *c);
PCGX_API pcgx_status pcgx_comm_rank(const pcgx_comm *c, int32_t *rank, int32_t *world);
PCGX_API pcgx_status pcgx_comm_allreduce_f64(pcgx_comm *c, double *d_buf, int32_t count, void *stream);
PCGX_API pcgx_status pcgx_icp_session_step_sharded(pcgx_icp_session *s, pcgx_comm *c, void *stream);
PCGX_API pcgx_status pcgx_icp_fit_sharded(const pcgx_kdtree *base, const float *tile, int64_t nt,
                                          const pcgx_icp_params *params, pcgx_comm *c, float trans16[16],
                                          pcgx_icp_stat *stat);
/* bases[r]: the tree replica built with slot r current; tiles[r] / nt[r]: slot r's part of the target (host memory). */
PCGX_API pcgx_status pcgx_icp_fit_multi(int32_t n, const pcgx_kdtree *const *bases, const float *const *tiles,
                                        const int64_t *nt, const pcgx_icp_params *params, float trans16[16],
                                        pcgx_icp_stat *stat);
/* all-reduce of a few doubles in host memory through `c` (set-up exchanges of the sharded paths) */
PCGX_API pcgx_status pcgx_comm_allreduce_host_f64(pcgx_comm *c, double *h_buf, int32_t count);
/* The voxel filter over several GPUs (second half).  Every rank holds the same cloud
 * in device memory.  Each runs the min/max pass (pc/minmax.go:9-26) over its n / world slice; the six
 * floats are exchanged through `c` (one all-reduce of 7 x world float64) and folded in rank order with
 * the reference's comparisons.  Each rank then keeps the points whose place in the reference's output
 * order -- chunk id, then cell (voxelgrid.go:49-116,137-151) -- lies in its contiguous share of that
 * key range and filters them: *out_n records in d_out (>= n * stride bytes).  The ranks' outputs,
 * rank 0's first, ARE the output of pcgx_voxel_filter_dev on one GPU, byte for byte; putting them
 * together is the caller's (a variable-length gather, or one copy per rank into the host cloud).
 * Collective: every rank of `c` must call it with the same cloud and options.  Errors as
 * pcgx_voxel_filter_dev on every rank alike. */
PCGX_API pcgx_status pcgx_voxel_filter_sharded_dev(pcgx_comm *c, const void *d_data, int64_t n, int32_t stride,
                                                   int32_t xyz_off, const float leaf[3], const int32_t chunk[3],
                                                   void *d_out, int64_t *out_n, void *stream);
/* The same with host buffers (upload, this rank's share, download of its *out_n records). */
PCGX_API pcgx_status pcgx_voxel_filter_sharded(pcgx_comm *c, const void *data, int64_t n, int32_t stride,
                                               int32_t xyz_off, const float leaf[3], const int32_t chunk[3],
                                               void *out_data, int64_t *out_n);
/* Change a session's sums after its creation (pcgx_icp_params.sums_mode sets them at creation; the
 * default is the reference's).  With strict on, the sums are the reference's: float32 additions in
 * target order, every rounding included, so Evaluated and the resulting pose are bit-identical to
 * the Go code's at any size.
 * on = 1: PCGX_SUMS_REFERENCE -- evaluated by the whole GPU (csrc/strict_sum.h: the additions of a
 *         stretch act on the state as a translation of its mantissa that is proven per rounding
 *         class, stretches are composed, one wave applies them; exact by construction);
 * on = 2: PCGX_SUMS_REFERENCE_CHAIN -- one wave adds the terms one after the other (~7 ms per 1M pairs);
 * on = 0: PCGX_SUMS_F64_TREE -- the float64 reduction.
 * Single-GPU sessions only (a sharded sum has no sequential order: step_sharded with world > 1
 * refuses a session whose strict sums were asked for explicitly and runs a default one with float64
 * sums).  Environment PCGX_ICP_STRICT=0 / 1 / 2 overrides sums_mode for every new session
 * (experiments). */
PCGX_API pcgx_status pcgx_icp_session_set_strict(pcgx_icp_session *s, int32_t on);
/* Synchronise and read back trans / stat / converged flag.  Returns
 * PCGX_E_NOT_ENOUGH_PAIRS if an iteration failed. */
PCGX_API pcgx_status pcgx_icp_session_result(pcgx_icp_session *s, void *stream,
                                             float trans16[16], pcgx_icp_stat *stat,
                                             int32_t *converged);

/* ------------------------------------------------ bucket voxel grid + segmentation
 * replaces pc/storage/voxelgrid.VoxelGrid (voxelgrid.go:7-122: dense [][]int buckets addressed by
 * int(pos*resolutionInv + 0.5)), pc/segmentation/voxelgrid.VoxelGrid.Segment (26-neighbour flood
 * fill, segmentation/voxelgrid/voxelgrid.go:39-73) and pc/segmentation/regiongrowing
 * .RegionGrowing.Segment (regiongrowing.go:23-56).  The device computes the buckets with one
 * stable sort and the connected components of the whole grid / cloud with a union-find; a seed
 * query is then a lookup (ids ascending by voxel address / point id).  The *_bfs variants return
 * the same set in the reference's own discovery order (its FIFO search replayed over the
 * device-built buckets / device Range batches); the reference's tests sort before comparing. */
typedef struct pcgx_bucket_grid pcgx_bucket_grid;
/* New(resolution, size, origin) followed by Add(point i, i) for every record of the cloud
 * (voxelgrid.go:15-23,37-45); points outside the grid are not added. */
PCGX_API pcgx_status pcgx_bucket_grid_build(const void *data, int64_t n, int32_t stride, int32_t xyz_off,
                                            float resolution, const int64_t size[3], const float origin[3],
                                            pcgx_bucket_grid **out);
PCGX_API pcgx_status pcgx_bucket_grid_free(pcgx_bucket_grid *g);
/* Len() (voxelgrid.go:110-112), points accepted by Add, occupied voxels; any pointer may be NULL */
PCGX_API pcgx_status pcgx_bucket_grid_counts(const pcgx_bucket_grid *g, int64_t *len, int64_t *n_added,
                                             int64_t *n_occupied);
/* Addr(p) (voxelgrid.go:64-79): *ok = 0 outside the grid */
PCGX_API pcgx_status pcgx_bucket_grid_addr(const pcgx_bucket_grid *g, const float p[3], int64_t *addr, int32_t *ok);
/* voxel address of every offered point, -1 where Add returned false */
PCGX_API pcgx_status pcgx_bucket_grid_point_addrs(const pcgx_bucket_grid *g, int64_t *addrs /* [n] */);
/* GetByAddr / Get (voxelgrid.go:52-62): *count = bucket length (Get: -1 = nil, p outside the grid);
 * the first min(count, cap) ids are written in insertion order.  An address outside
 * [0, Len()) is PCGX_E_OUT_OF_RANGE (the reference panics). */
PCGX_API pcgx_status pcgx_bucket_grid_get_by_addr(const pcgx_bucket_grid *g, int64_t addr, int64_t *out, int64_t cap,
                                                  int64_t *count);
PCGX_API pcgx_status pcgx_bucket_grid_get(const pcgx_bucket_grid *g, const float p[3], int64_t *out, int64_t cap,
                                          int64_t *count);
/* Indice() (voxelgrid.go:114-120): out holds n_added ids */
PCGX_API pcgx_status pcgx_bucket_grid_indice(const pcgx_bucket_grid *g, int64_t *out);
/* Segment(p) for every seed at once: point_comp[i] = smallest voxel address of the 26-connected
 * set of occupied voxels point i's voxel belongs to, -1 for points outside the grid. */
PCGX_API pcgx_status pcgx_bucket_grid_components(pcgx_bucket_grid *g, int64_t *point_comp /* [n] */);
/* Segment(p) (segmentation/voxelgrid/voxelgrid.go:39-73): *count = result length, the first
 * min(count, cap) ids are written; empty when p is outside the grid or its voxel is empty. */
PCGX_API pcgx_status pcgx_bucket_grid_segment(pcgx_bucket_grid *g, const float p[3], int64_t *out, int64_t cap,
                                              int64_t *count);

/* Segment(p) with the ids in the reference's own (FIFO flood-fill) order: the Go algorithm run on the
 * host over the device-built buckets.  Same set as pcgx_bucket_grid_segment. */
PCGX_API pcgx_status pcgx_bucket_grid_segment_bfs(pcgx_bucket_grid *g, const float p[3], int64_t *out, int64_t cap,
                                                  int64_t *count);

/* RegionGrowing (regiongrowing.go:18-56).  labels = the property accessor (Uint32At(id), id in
 * [0, Len())).  _components answers every seed at once for one max_range: comp[i] = smallest id of
 * the points reachable from i through steps with DistSq < max_range^2 between points of i's
 * property value.  _segment is Segment(p, maxRange) given those components. */
PCGX_API pcgx_status pcgx_region_growing_components(const pcgx_kdtree *t, const uint32_t *labels, float max_range,
                                                    int64_t *comp /* [Len()] */);
PCGX_API pcgx_status pcgx_region_growing_segment(const pcgx_kdtree *t, const uint32_t *labels, const int64_t *comp,
                                                 const float p[3], float max_range, int64_t *out, int64_t cap,
                                                 int64_t *count);

/* Segment(p, maxRange) with the ids in the reference's own (FIFO) order: the Range() calls of one
 * BFS level are one device batch, the queue logic runs on the host as in regiongrowing.go:33-54.
 * Same set as pcgx_region_growing_segment; needs no components. */
PCGX_API pcgx_status pcgx_region_growing_segment_bfs(const pcgx_kdtree *t, const uint32_t *labels, const float p[3],
                                                     float max_range, int64_t *out, int64_t cap, int64_t *count);

/* ------------------------------------------------ sample consensus plane detection
 * replaces pc/sac (sac.go:33-59 SAC.Compute, surface.go:36-240 the voxel-grid plane model, Fit / Evaluate /
 * Inliers / IsIn) over a bucket voxel grid.  Neither Fit nor Evaluate draws random numbers: the caller's sampler
 * draws the 3n ids of n hypotheses first, in the order sac.go:40-43 draws them, and ONE call fits and evaluates
 * them all on the device -- the same hypotheses give the reference's result bit for bit (float32 arithmetic left
 * to right, no contraction).
 * Model creation copies what the model reads into library-owned device memory before it returns: the cloud's xyz
 * (data: host records, or device records with on_device = 1; stride / xyz_off as pcgx_bucket_grid_build), the
 * grid's occupied voxels and their bucket lengths, vg.MinMax() and Resolution().  The caller's buffers and the
 * grid may change or go afterwards. */
typedef struct pcgx_sac_plane_model pcgx_sac_plane_model;
/* voxelGridSurfaceModelCoefficients (surface.go:191-200) */
typedef struct {
  float origin[3], v1[3], v2[3];
  float l1, l2;
  float norm[3];
  float d;
} pcgx_sac_plane;
PCGX_API pcgx_status pcgx_sac_plane_model_create(const pcgx_bucket_grid *g, const void *data, int64_t n, int32_t stride,
                                                 int32_t xyz_off, int32_t on_device, pcgx_sac_plane_model **out);
PCGX_API pcgx_status pcgx_sac_plane_model_free(pcgx_sac_plane_model *m);
/* Compute(n) over the pre-drawn ids[3n] (Fit(ids) alone is n = 1).  *found = 0 when no hypothesis scores above 0
 * (then *best = -1, *best_score = 0 and best_coeff is not written); else the FIRST hypothesis of the largest
 * score (sac.go:49: e > bestE).  ok[n], coeff[n] (zero where Fit failed) and score[n] (Evaluate(), 0 where Fit
 * failed) may each be NULL.  An id outside [0, n_points) is PCGX_E_OUT_OF_RANGE (the reference panics), n < 0 or
 * a NULL argument PCGX_E_INVALID; nothing is written then.  A lattice with more than 8192 values along one of its
 * two axes (the serial a / b accumulators, surface.go:206-207) is PCGX_E_TOO_LARGE, nothing written. */
PCGX_API pcgx_status pcgx_sac_plane_compute(pcgx_sac_plane_model *m, const int64_t *ids, int64_t n, int32_t *found,
                                            int64_t *best, int64_t *best_score, pcgx_sac_plane *best_coeff,
                                            int32_t *ok, pcgx_sac_plane *coeff, int64_t *score);
/* Inliers(d) (surface.go:222-235): every point of the model's cloud, ids ascending, with
 * -d < norm . (p - vgMin) - c->d < d (points outside the grid included).  *count = result length; the first
 * min(count, cap) ids are written. */
PCGX_API pcgx_status pcgx_sac_plane_inliers(pcgx_sac_plane_model *m, const pcgx_sac_plane *c, float d, int64_t *out,
                                            int64_t cap, int64_t *count);
/* IsIn(p, d) (surface.go:237-240), on the host */
PCGX_API pcgx_status pcgx_sac_plane_is_in(const pcgx_sac_plane_model *m, const pcgx_sac_plane *c, const float p[3], float d,
                                          int32_t *in);

/* ---------------------------------------------------------------- PCD files
 * replaces pc.UnmarshalHeader / pc.Unmarshal / pc.Marshal (pc/io.go:24-45,47-230,232-285) with a
 * device-resident output: the records of an ascii / binary / binary_compressed file land in HBM
 * (one upload; compressed files: LZF decode on the host, the SoA -> AoS de-interleave on the
 * device) ready for the *_dev entry points.  The reference's de-interleave quirk is kept (COUNT > 1
 * fields of compressed files: only element 0 is filled, io.go:217-226). */
#define PCGX_PCD_MAX_FIELDS 64
enum { PCGX_PCD_ASCII = 0, PCGX_PCD_BINARY = 1, PCGX_PCD_BINARY_COMPRESSED = 2 }; /* pc.Format, io.go:16-22 */
typedef struct {            /* pc.PointCloudHeader (pc/pointcloud.go:9-18) + what Unmarshal derives */
  float version;
  int32_t n_fields;
  char fields[PCGX_PCD_MAX_FIELDS][32]; /* NUL-terminated names */
  int32_t size[PCGX_PCD_MAX_FIELDS];
  char type[PCGX_PCD_MAX_FIELDS];       /* 'F', 'U', 'I' */
  int32_t count[PCGX_PCD_MAX_FIELDS];
  int64_t width, height;
  int32_t n_viewpoint;
  float viewpoint[16];
  int64_t points;                       /* POINTS */
  int32_t format;                       /* PCGX_PCD_* */
  int64_t stride;                       /* sum size*count (pointcloud.go:64-70) */
  int64_t data_offset;                  /* byte offset of the payload in the file */
} pcgx_pcd_header;
PCGX_API pcgx_status pcgx_pcd_unmarshal_header(const void *file, size_t len, pcgx_pcd_header *h);
/* out_data: host buffer of h->points * h->stride bytes */
PCGX_API pcgx_status pcgx_pcd_unmarshal(const void *file, size_t len, const pcgx_pcd_header *h, void *out_data);
/* d_out: DEVICE buffer of h->points * h->stride bytes; returns when the records are in HBM */
PCGX_API pcgx_status pcgx_pcd_unmarshal_dev(const void *file, size_t len, const pcgx_pcd_header *h, void *d_out,
                                            void *stream);
/* Marshal (always "DATA binary"): *out_len = file size; out == NULL only sizes */
PCGX_API pcgx_status pcgx_pcd_marshal(const pcgx_pcd_header *h, const void *data, void *out, size_t cap,
                                      size_t *out_len);

/* ------------------------------------------- point-to-plane ICP (extension)
 * NOT in the reference: pcgol declares only the slots -- Evaluated.Hessian mat.Mat6
 * (evaluator.go:28), Evaluator.HasHessian (evaluator.go:35,76), mat.Mat6 (mat/mat6.go:3),
 * UpdaterGradient (updater.go:11-13).  This fills them: an evaluator whose residual is the
 * point-to-plane distance r = n . (pt - pb) with the 6x6 Gauss-Newton normal equations
 * (J = {n, pt x n}, parameters {t, w} ordered like Evaluated.Gradient), and a Gauss-Newton
 * updater with the reference updater's flat test, pose composition
 * trans = Translate(d0..2) * (Rodrigues(d3..5) * trans) and iteration cap.
 * No reference parity exists; tests check against the CPU oracle's float64 restatement.
 *
 * base_normals: packed xyz float32 per base point, in the tree's id order (unit length).
 * A plane session is a pcgx_icp_session whose exchange vector has 30 doubles:
 *   {sum r^2, sum J r [6], upper triangle of sum J J^T row-major [21], sum w, pair count}.
 * partials / update / step / result / reset / set_pose / free are the session calls above;
 * params->weight is unused, params->threshold / max_iteration / min_pairs / max_dist as above.
 * params->min_dist_sq has no meaning here either: a plane session always searches exactly (MinDistSq = 0), and
 * pcgx_icp_plane_session_create answers a min_dist_sq > 0 with PCGX_E_INVALID instead of ignoring it silently
 * (so does pcgx_icp_plane_fit): pass 0 whatever MinDistSq the tree handle was made with. */
PCGX_API pcgx_status pcgx_icp_plane_session_create(const pcgx_kdtree *base, const float *base_normals,
                                                   const float *target, int64_t nt, int32_t on_device,
                                                   const pcgx_icp_params *params, float damping,
                                                   double *d_sums30, pcgx_icp_session **out);
/* 10 or 30: length of the session's exchange vector. */
PCGX_API pcgx_status pcgx_icp_session_sums_count(const pcgx_icp_session *s, int32_t *count);
PCGX_API pcgx_status pcgx_icp_session_read_sums_n(pcgx_icp_session *s, double *sums, int32_t cap, void *stream);
/* Evaluated.Hessian of the last evaluation (2/sum(w) * sum J J^T, symmetric 6x6). */
PCGX_API pcgx_status pcgx_icp_session_hessian(pcgx_icp_session *s, void *stream, float hessian36[36]);
/* Whole Fit on the device; hessian36 may be NULL.  PCGX_E_SINGULAR if the normal equations
 * are not positive definite (e.g. all normals parallel). */
PCGX_API pcgx_status pcgx_icp_plane_fit(const pcgx_kdtree *base, const float *base_normals, const float *target,
                                        int64_t nt, const pcgx_icp_params *params, float damping,
                                        float trans16[16], pcgx_icp_stat *stat, float hessian36[36]);
/* Host-only pieces for a host-driven exchange loop. */
PCGX_API pcgx_status pcgx_icp_plane_finish_evaluate(const double sums30[30], int32_t min_pairs,
                                                    pcgx_icp_evaluated *out, float hessian36[36]);
PCGX_API pcgx_status pcgx_icp_gauss_newton_update(const pcgx_icp_params *p, float damping, int32_t *iter,
                                                  const float gradient[6], const float hessian36[36],
                                                  float trans16[16], int32_t *converged);

/* ------------------------------------------- surface normals (extension: no reference parity)
 * NOT in the reference: pcgol has no normal estimation.  The normals of the point-to-plane extension above, from
 * KD-tree radius neighbourhoods.  For query q, radius r, viewpoint v (NULL: the origin) and min_neighbors (below 3
 * counts as 3):
 *   N(q)  = the points p of the tree with DistSq(p, q) < r*r (the reference's float32 expression): exactly the set
 *           pcgx_kdtree_range_count counts, with or without a grid, after DeletePoint too; a tree point counts itself;
 *   count = |N(q)| (exact);
 *   count < min_neighbors, or all of N(q) coincide: normal (0, 0, 0), curvature NaN;
 *   else, in float64 with d = p - q: C = sum d d^T / count - mean mean^T (mean = sum d / count), eigenvalues
 *   l0 <= l1 <= l2; normal = unit eigenvector of l0, negated if normal . (v - q) < 0, rounded to float32;
 *   curvature = max(l0, 0) / (l0 + l1 + l2) (PCL's surface variation).
 *   Cancelled trace: when the float64 trace of C rounds to <= 0 the query is answered as if degenerate: normal
 *   (0, 0, 0), curvature NaN.  sum d d^T / count - mean mean^T is within (2 count + 4) 2^-53 sum |d|^2 / count of the
 *   exact C, so this happens only where the neighbours' spread is below ~1e-8 of their distance from the query.
 * q == NULL: the tree's own points (deleted ones included), nq must equal Len(); the output is in the tree's id
 * order, i.e. exactly the base_normals pcgx_icp_plane_session_create / pcgx_icp_plane_fit take.  curvature and
 * counts may be NULL.  A radius that is not finite and > 0, q == NULL with nq != Len() or normals == NULL with
 * nq > 0 is PCGX_E_INVALID.  Always computed on the device.
 * Fed to a plane session: a degenerate point's zero normal gives its pairs r = 0 and J = 0, but they still count in
 * the pair count and in sum w.  pcgx_icp_plane_session_create reads device normals asynchronously on its stream:
 * the buffer must stay alive until the session's first synchronising call.
 * Cost is the sum over the queries of the records in the cells (or tree nodes) their radius covers, as for Range:
 * a radius far above the point spacing, or thousands of coincident queries, is paid for in full. */
PCGX_API pcgx_status pcgx_kdtree_normals(const pcgx_kdtree *t, const float *q, int64_t nq, float radius,
                                         const float viewpoint[3], int32_t min_neighbors,
                                         float *normals /* [3nq] */, float *curvature /* [nq] */,
                                         int32_t *counts /* [nq] */);
/* Same, every array device resident, enqueued on `stream` (NULL: the library's); returns without waiting. */
PCGX_API pcgx_status pcgx_kdtree_normals_dev(const pcgx_kdtree *t, const float *d_q, int64_t nq, float radius,
                                             const float viewpoint[3], int32_t min_neighbors, float *d_normals,
                                             float *d_curvature, int32_t *d_counts, void *stream);

/* ------------------------------------------- moving least squares (extension: no reference parity)
 * NOT in the reference.  Moving-least-squares smoothing (Alexa et al. 2003; PCL's MovingLeastSquares with the SIMPLE
 * projection): every query is projected onto a low-order polynomial fitted to its radius neighbourhood and comes back
 * with the polynomial's normal -- what puts noisy points back onto the surface every other stage assumes they lie on.
 * This comment is the contract; tests/mls_oracle.py restates it in float64 NumPy.
 * Queries and neighbourhood: pcgx_kdtree_normals' conventions.  q == NULL: the tree's own points, nq must equal Len(),
 *   output in id order, deleted ids included.  N(q) is exactly the set pcgx_kdtree_range_count counts on that handle
 *   (float32 DistSq < radius^2); count = |N(q)| (exact).  Outputs must not alias q.
 * Unchanged (kind 0): count < max(min_neighbors, 3), or all neighbours coincide (the exact box test of normals), or the
 *   float64 trace of C is <= 0.  points holds the query's own bits (a NaN query stays NaN), normals 0.
 * Plane (kind 1): C, mean and the eigenvectors of C's eigenvalues l0 <= l1 <= l2 exactly as normals compute them, with
 *   d = p - q in float64.  n: the unit eigenvector of l0; u, v: the other two, unit and orthogonal.  The origin is the
 *   query's projection onto the plane through the centroid, d0 = (mean . n) n.  Output q + d0, normal n.  order == 1
 *   stops here.
 * Polynomial (kind 2): order == 2 and count >= 6.  Per neighbour, all float64: e = d - d0, h = e . n,
 *   a = (e . u) / radius, b = (e . v) / radius, w = exp(-|e|^2 / sigma^2).  Basis, in this order:
 *   B = (1, a, b, a^2, a b, b^2); normal equations M = sum w B B^T, g = sum w B h.  The solve is Cholesky in the basis'
 *   order; it fails when sum w is not > 0, or when a pivot s_k = M_kk - sum_j L_kj^2 is not greater than 1e-10 M_kk
 *   (the smallest s_k / M_kk is the pivot ratio).  A failed solve gives kind 1.  With c = M^-1 g: |c0| > radius (the
 *   fitted height at the query lies outside its own neighbourhood) gives kind 1; otherwise the output is
 *   q + d0 + c0 n and the normal n - (c1 / radius) u - (c2 / radius) v, normalised.
 * Every kind: normals of kind 1 and 2 are turned towards the viewpoint (NULL: the origin) as pcgx_kdtree_normals
 *   turns them.  Positions and normals are computed in float64 and rounded to float32 once.  The result does not
 *   depend on which u, v the eigen-solve returns (the basis spans all polynomials of degree <= 2, the weight depends
 *   on |e| only); only the pivot ratio does, so a solve at the threshold may fall either way.  The same input gives
 *   the same bits on every call: no float atomics.
 * PCGX_E_INVALID: radius or sigma not finite and > 0, order outside {1, 2}, a NULL tree, nq < 0, q == NULL with
 *   nq != Len(), NULL points with nq > 0.  nq == 0 is PCGX_OK.  normals, kinds and counts may be NULL.  Always
 *   computed on the device.  Cost: pcgx_kdtree_normals' enumeration twice for order 2, once for order 1. */
enum { PCGX_MLS_UNCHANGED = 0, PCGX_MLS_PLANE = 1, PCGX_MLS_POLY = 2 };
PCGX_API pcgx_status pcgx_kdtree_mls(const pcgx_kdtree *t, const float *q, int64_t nq, float radius, float sigma,
                                     int32_t order, int32_t min_neighbors, const float viewpoint[3],
                                     float *points /* [3nq] */, float *normals /* [3nq], may be NULL */,
                                     int32_t *kinds /* [nq], may be NULL */, int32_t *counts /* [nq], may be NULL */);
/* Same, every array device resident, enqueued on `stream` (NULL: the library's); returns without waiting. */
PCGX_API pcgx_status pcgx_kdtree_mls_dev(const pcgx_kdtree *t, const float *d_q, int64_t nq, float radius, float sigma,
                                         int32_t order, int32_t min_neighbors, const float viewpoint[3],
                                         float *d_points, float *d_normals, int32_t *d_kinds, int32_t *d_counts,
                                         void *stream);

/* ------------------------------------------- FPFH descriptors (extension: no reference parity)
 * NOT in the reference.  The Fast Point Feature Histogram (Rusu, Blodow, Beetz 2009) of every point of the tree: 33
 * numbers per point, the input of feature-based coarse alignment, which finds the starting pose every ICP here needs.
 * Close to PCL's and Open3D's FPFH, pinned to neither: this comment is the contract, tests/fpfh_oracle.py restates it.
 * Queries: the tree's own points only, deleted ids included (the q == NULL convention of pcgx_kdtree_normals, _knearest
 * and _covariances); normals[3 Len()] is in id order -- what pcgx_kdtree_normals(q == NULL) writes -- and so is every
 * output.
 * Neighbourhood: N(q) = the points p of the tree with DistSq(p, q) < radius^2, DistSq the reference's float32
 * expression: exactly the set pcgx_kdtree_range_count counts on that handle (grid, forced walk, after DeletePoint).
 * Deleted points are nobody's neighbour.
 * Pair features of query s (normal ns) and neighbour t (normal nt), in float64 from the float32 inputs widened:
 *   d = pt - ps, f4 = |d|, a1 = ns . d / f4, a2 = nt . d / f4;
 *   if |a1| < |a2| the roles swap: (n1, n2, d, f3) = (nt, ns, -d, -a2), else (n1, n2, d, f3) = (ns, nt, d, a1)
 *   (no acos: comparing the magnitudes is the same decision);
 *   v = d x n1, v /= |v|;  w = n1 x v;  f2 = v . n2;  f1 = atan2(w . n2, n1 . n2);
 *   eleven bins per feature: b1 = clamp(floor(11 (f1 + pi) / 2 pi), 0, 10), b2 = clamp(floor(11 (f2 + 1) / 2), 0, 10),
 *   b3 = clamp(floor(11 (f3 + 1) / 2), 0, 10).
 *   Normals are used as given and are expected to be unit length.  A pair is invalid and contributes nothing when the
 *   float32 DistSq == 0 (the point itself, exact duplicates), when either normal is zero or not finite (how degenerate
 *   points come out of pcgx_kdtree_normals), or when |v| == 0.
 * SPFH: c_q[f][b] = the number of valid pairs of q whose feature f falls in bin b (exact 32-bit integers), m_q = the
 *   number of valid pairs; S_q = 100 c_q / m_q, and 0 where m_q == 0.  spfh_counts (may be NULL) returns c, feature
 *   major 3 x 11 per point; pair_counts (may be NULL) returns m.
 * FPFH: with w_i = 1 / DistSq(i, q), the float32 DistSq widened and the quotient taken in float64,
 *   W_f[b] = sum over i in N(q) with DistSq > 0 of w_i S_i[f][b],   T_f = sum over b of W_f[b],
 *   F_q[f][b] = S_q[f][b] + (T_f > 0 ? 100 W_f[b] / T_f : 0), rounded to float32; fpfh[33 q + 11 f + b].
 *   The sums are float64, in any order (every term is >= 0: the order matters far below float32).  The result is
 *   within 2^-22 relative of the real-number value; a bin whose real-number value is 0 is exactly 0; an isolated
 *   point gives 33 zeros.  The same input gives the same bits on every call.
 * PCGX_E_INVALID: a radius that is not finite and > 0, NULL normals or NULL fpfh with Len() > 0, a NULL tree.
 * Len() == 0 is PCGX_OK and does nothing.  Always computed on the device; the cost is two enumerations of every
 * neighbourhood (pcgx_kdtree_normals' cost, twice) plus an atan2 and a 12-byte read by id per pair in the first and a
 * 144-byte read by id per pair in the second.  144 Len() bytes of temporaries. */
PCGX_API pcgx_status pcgx_kdtree_fpfh(const pcgx_kdtree *t, const float *normals /* [3 Len()], id order */,
                                      float radius, float *fpfh /* [33 Len()] */,
                                      int32_t *spfh_counts /* [33 Len()], may be NULL */,
                                      int32_t *pair_counts /* [Len()], may be NULL */);
/* Same, every array device resident, enqueued on `stream` (NULL: the library's); returns without waiting. */
PCGX_API pcgx_status pcgx_kdtree_fpfh_dev(const pcgx_kdtree *t, const float *d_normals, float radius, float *d_fpfh,
                                          int32_t *d_spfh_counts, int32_t *d_pair_counts, void *stream);

/* ------------------------------------------- FPFH at chosen points (extension: no reference parity)
 * NOT in the reference.  pcgx_kdtree_fpfh's rows at a list of point ids -- keypoints -- without describing the rest
 * of the cloud: a descriptor is needed only at a listed point, an SPFH record only at a listed point or at one of its
 * neighbours.  The outputs are compact, one slot per list entry, with a fixed capacity on the device, so that the
 * chain keypoints -> descriptors -> match -> pose runs on one stream with nothing read back.
 * Slots: on the device form n = clamp(*d_n_ids, 0, cap), read on the device (d_n_ids == NULL: n = cap); on the host
 *   form n = n_ids.  Slot s is live iff s < n and 0 <= ids[s] < Len().  Ids may repeat and need not be sorted; deleted
 *   ids are allowed, exactly as pcgx_kdtree_fpfh computes their rows.  The host form, which can read the list, rejects
 *   an id out of range (as pcgx_pose_from_correspondences does); on the device form such an id makes its slot dead:
 *   that covers the -1 pcgx_kdtree_local_maxima_dev pads with, so its d_ids and d_n_ids can be passed on as they are.
 * Live slot s: fpfh[33 s ..], spfh_counts[33 s ..] and pair_counts[s] are what pcgx_kdtree_fpfh's contract defines
 *   for point ids[s] on that handle (the counts exact, F within 2^-22 relative of the real-number value and its zeros
 *   exact; in fact the bits pcgx_kdtree_fpfh writes, the sums being taken in its order); xyz[3 s ..] (may be NULL)
 *   holds the point's three float32 bit for bit.
 * Dead slot: 33 zeros, a zero xyz, zero counts: the row pcgx_fpfh_match never takes as a candidate and never answers
 *   as a query, so a matcher given na = cap sees the padding as nothing.  Every slot of [0, cap) is written on every
 *   call.
 * n_spfh (may be NULL; one int32 on the device): the number of distinct points whose SPFH record the call computed:
 *   the ids of the live slots and every member of their N(.).  Exact; it says, without a clock, how much of the cloud
 *   was left alone.
 * The same input gives the same bits on every call (no float atomics).  n_ids == 0 or cap == 0 is PCGX_OK.
 * PCGX_E_INVALID: a radius that is not finite and > 0, a NULL tree, a negative count, NULL ids or NULL fpfh with a
 * positive count, NULL normals with a positive count and Len() > 0, more than 2^31 - 1 ids or points; on the host
 * form an id outside [0, Len()).  Always computed on the device.  Temporaries: Len() bytes of flags, cleared inside
 * the call, and the 144 Len() bytes of records, of which only the n_spfh needed ones are written.  The first call on
 * a handle without deletions builds the handle's id -> node map and waits for it, once. */
PCGX_API pcgx_status pcgx_kdtree_fpfh_at(const pcgx_kdtree *t, const float *normals /* [3 Len()], id order */,
                                         float radius, const int64_t *ids /* [n_ids] */, int64_t n_ids,
                                         float *fpfh /* [33 n_ids] */, float *xyz /* [3 n_ids], may be NULL */,
                                         int32_t *spfh_counts /* [33 n_ids], may be NULL */,
                                         int32_t *pair_counts /* [n_ids], may be NULL */,
                                         int64_t *n_spfh /* may be NULL */);
/* Same, every array device resident, enqueued on `stream` (NULL: the library's); returns without waiting. */
PCGX_API pcgx_status pcgx_kdtree_fpfh_at_dev(const pcgx_kdtree *t, const float *d_normals, float radius,
                                             const int32_t *d_ids /* [cap] */, int64_t cap,
                                             const int32_t *d_n_ids /* one int32; NULL: cap ids */,
                                             float *d_fpfh /* [33 cap] */, float *d_xyz /* [3 cap], may be NULL */,
                                             int32_t *d_spfh_counts, int32_t *d_pair_counts,
                                             int32_t *d_n_spfh /* one int32, may be NULL */, void *stream);

/* ------------------------------------------- FPFH matching (extension: no reference parity)
 * NOT in the reference.  For every row of one descriptor array, the nearest and the second nearest row of another,
 * brute force over all pairs, and the correspondence list made from them: what feature-based coarse alignment
 * estimates its pose from.  This comment is the contract, tests/match_oracle.py restates it.
 * A descriptor array is float32 [33 n], row i at 33 i: what pcgx_kdtree_fpfh writes.
 * Usable row: all 33 values finite and at least one not zero (-0.0 is zero).  An all-zero row is how FPFH says "no
 *   descriptor" (an isolated point, a degenerate normal).  Unusable rows are never candidates and find nothing as
 *   queries; a caller who wants a point left out (a deleted id) zeroes its row.
 * Distance: float32, left to right, nothing fused (the rule of DistSq):
 *     acc = 0;  for k = 0 .. 32:  d = a[k] - b[k];  acc = acc + d * d;     D(a, b) = acc
 *   every operation rounded to float32.  Between usable rows D is never NaN; it can be +inf, and a candidate at
 *   D == +inf is not a match.  D(a, b) and D(b, a) have the same bits.
 * Match: for query row i of A, over the usable rows j of B with finite D(i, j): ids[i] = the j with the smallest
 *   (D, j) in lexicographic order (ties go to the smaller id, as in pcgx_kdtree_knearest), dist_sq[i] = that D,
 *   second_dist_sq[i] = the D of the runner-up in the same order (another j; it may equal dist_sq[i]), +inf with one
 *   such candidate.  With none, or an unusable query: {-1, +inf, +inf}.
 * Correspondences: i is kept when ids[i] >= 0, and dist_sq[i] <= max_ratio_sq * second_dist_sq[i] (a float32 product:
 *   Lowe's ratio test on squared distances, 1.0f keeps every match), and, if mutual != 0, the match of B's row ids[i]
 *   in A is i (the same rule, roles swapped).  src_ids[] / dst_ids[] hold the kept pairs (i, ids[i]) in ascending i,
 *   *n_pairs their number, the slots from n_pairs to na are -1.  0 < max_ratio_sq <= 1, else PCGX_E_INVALID.
 * All four: na == 0 is PCGX_OK and writes nothing except *n_pairs = 0; nb == 0 is PCGX_OK with every query unmatched.
 *   PCGX_E_INVALID: NULL a with na > 0, NULL b with nb > 0, NULL ids / dist_sq / src_ids / dst_ids / n_pairs with
 *   na > 0, a negative count, more than 2^31 - 1 rows.  The same input gives the same bits on every call.  Always
 *   computed on the device: 99 na nb float32 operations (twice that with mutual: two passes); 12 S na + 4 (na + nb)
 *   bytes of temporaries, S the number of chunks B is split into to fill the chip (the library's choice; PCGX_MATCH_SPLIT=<n>
 *   in the environment, read per call, forces it -- any n gives the same bits). */
PCGX_API pcgx_status pcgx_fpfh_match(const float *a /* [33 na] */, int64_t na, const float *b /* [33 nb] */, int64_t nb,
                                     int64_t *ids /* [na] */, float *dist_sq /* [na] */,
                                     float *second_dist_sq /* [na], may be NULL */);
/* Same, every array device resident (ids and counts are int32 there), enqueued on `stream` (NULL: the library's);
 * returns without waiting. */
PCGX_API pcgx_status pcgx_fpfh_match_dev(const float *d_a, int64_t na, const float *d_b, int64_t nb, int32_t *d_ids,
                                         float *d_dist_sq, float *d_second_dist_sq /* may be NULL */, void *stream);
PCGX_API pcgx_status pcgx_fpfh_correspondences(const float *a, int64_t na, const float *b, int64_t nb,
                                               float max_ratio_sq, int32_t mutual, int64_t *src_ids /* [na] */,
                                               int64_t *dst_ids /* [na] */, int64_t *n_pairs);
PCGX_API pcgx_status pcgx_fpfh_correspondences_dev(const float *d_a, int64_t na, const float *d_b, int64_t nb,
                                                   float max_ratio_sq, int32_t mutual, int32_t *d_src_ids /* [na] */,
                                                   int32_t *d_dst_ids /* [na] */, int32_t *d_n_pairs, void *stream);
/* Queries per workgroup of the match kernel (a wave, two queries per lane): the boundary the tests put rows across. */
PCGX_API int32_t pcgx_fpfh_match_tile(void);

/* ------------------------------------------- keypoints (extension: no reference parity)
 * NOT in the reference.  The matcher above is brute force over all pairs, so coarse alignment of large clouds describes
 * and matches a few thousand keypoints instead of every point.  Two operations, both over the tree's own points only
 * (the q == NULL convention of pcgx_kdtree_normals, _fpfh and _knearest), every array in id order, deleted ids
 * included.  This comment is the contract, tests/keypoints_oracle.py restates it.
 * Neighbourhood: N(i) = the points p of the tree with DistSq(p, point i) < radius^2, DistSq the reference's float32
 *   expression: exactly the set pcgx_kdtree_range_count counts on that handle (grid, forced walk, after DeletePoint).
 *   Deleted points are nobody's neighbour.
 * Local maxima of score[Len()] at `radius`: id i is a maximum iff
 *   score[i] > 0 (a NaN, zero or negative score never qualifies; +inf does), and
 *   i is in N(i) (so a deleted id, or a point with a NaN coordinate, is never a maximum), and
 *   no other j in N(i) has score[j] > score[i], or score[j] == score[i] with j < i (ties go to the smaller id, as in
 *   pcgx_kdtree_knearest; a NaN neighbour beats nobody; coincident points with equal scores leave one maximum, the
 *   smallest id).
 *   ids[Len()] holds the maxima in ascending id, then -1 in every remaining slot (the convention of
 *   pcgx_fpfh_correspondences); *n_ids their number.
 * ISS keypoints (Zhong 2009), in Open3D's form: for every id, C = pcgx_kdtree_normals' covariance over N(i) at
 *   salient_radius (float64, centred on the query, about the mean, a tree point counting itself);
 *   (l0, l1, l2) = C's eigenvalues in ascending order, unscaled, l0 clamped at 0, each rounded to float32;
 *   (0, 0, 0) when count < max(min_neighbors, 3), when all neighbours coincide, or when the float64 trace is <= 0 (the
 *   three cases in which normals answer "degenerate").  eigenvalues[3 i ..] holds them.
 *   Salient iff l0 > 0 and l1 < gamma_21 * l2 and l0 < gamma_32 * l1, decided on the float32 values with float32
 *   products rounded once each (as max_ratio_sq is applied above).  saliency[i] = l0 if salient, else 0.
 *   Keypoints = the local maxima of saliency at non_max_radius, by the rule above exactly.
 *   eigenvalues and saliency may each be NULL.
 *   Not Open3D's or PCL's bits: Open3D breaks a tie by dropping both points and also asks for a minimum count in the
 *   suppression neighbourhood; PCL scatters about the query point instead of the mean.
 * PCGX_E_INVALID: a radius, or a gamma, that is not finite and > 0; a NULL tree; NULL score, ids or n_ids with
 *   Len() > 0.  Len() == 0 is PCGX_OK and writes nothing except *n_ids = 0.  The same input gives the same bits on every
 *   call.  Always computed on the device: one enumeration of every neighbourhood whose own score is > 0 plus a 4-byte
 *   read by id per neighbour, and for ISS pcgx_kdtree_normals' cost before it.  Temporaries: Len() bytes of flags and
 *   4 ceil(Len() / 2048) bytes of tile counts; ISS adds 4 Len() bytes when saliency is NULL. */
PCGX_API pcgx_status pcgx_kdtree_local_maxima(const pcgx_kdtree *t, float radius, const float *score /* [Len()] */,
                                              int64_t *ids /* [Len()] */, int64_t *n_ids);
/* Same, every array device resident (ids and the count are int32 there), enqueued on `stream` (NULL: the library's);
 * returns without waiting. */
PCGX_API pcgx_status pcgx_kdtree_local_maxima_dev(const pcgx_kdtree *t, float radius, const float *d_score,
                                                  int32_t *d_ids /* [Len()] */, int32_t *d_n_ids, void *stream);
PCGX_API pcgx_status pcgx_kdtree_iss_keypoints(const pcgx_kdtree *t, float salient_radius, float non_max_radius,
                                               float gamma_21, float gamma_32, int32_t min_neighbors,
                                               float *eigenvalues /* [3 Len()], may be NULL */,
                                               float *saliency /* [Len()], may be NULL */, int64_t *ids /* [Len()] */,
                                               int64_t *n_ids);
PCGX_API pcgx_status pcgx_kdtree_iss_keypoints_dev(const pcgx_kdtree *t, float salient_radius, float non_max_radius,
                                                   float gamma_21, float gamma_32, int32_t min_neighbors,
                                                   float *d_eigenvalues, float *d_saliency, int32_t *d_ids /* [Len()] */,
                                                   int32_t *d_n_ids, void *stream);

/* ------------------------------------------- clusters (extension: no reference parity)
 * NOT in the reference.  The connected components of the radius graph over the tree's own points -- PCL's
 * EuclideanClusterExtraction -- optionally cut where the normals turn or the curvature is high (smooth faces), kept
 * inside a size range, ranked, and returned as labels, sizes and grouped member ids.  Every array is in id order over
 * the tree's own points, deleted ids included (the q == NULL convention of pcgx_kdtree_normals, _fpfh and
 * _local_maxima).  This comment is the contract, tests/cluster_oracle.py restates it.
 * Neighbourhood: N(i) = the points p of the tree with DistSq(p, point i) < radius^2, DistSq the reference's float32
 *   expression: exactly the set pcgx_kdtree_range_count counts on that handle (grid, forced walk, after DeletePoint).
 *   Deleted points are nobody's neighbour.
 * Usable point: i is usable when all three hold:
 *   i is in N(i) (this excludes a deleted id and a point with a NaN or infinite coordinate);
 *   if normals != NULL, its three normal components are finite and not all zero (the zero normal is what
 *     pcgx_kdtree_normals answers for a degenerate neighbourhood);
 *   if curvature != NULL, curvature[i] <= max_curvature (a NaN curvature fails: again the degenerate answer).
 *   An unusable point gets label -1, belongs to no cluster and carries no edge.
 * Edge: {i, j} with i != j is an edge when both points are usable, j is in N(i) (the expression is symmetric bit for
 *   bit), and, if normals != NULL, the normals agree: with the float32 components widened to float64,
 *   c = (nx_i nx_j + ny_i ny_j) + nz_i nz_j (the products are exact, the two additions rounded in this order, nothing
 *   contracted); the edge holds iff c >= (double)min_cos when oriented != 0, else iff fabs(c) >= (double)min_cos.
 *   Normals are taken as given, not normalised.  With normals == NULL, min_cos and oriented are ignored; with
 *   curvature == NULL, max_curvature is ignored.
 * Clusters: a cluster is a connected component of the usable points under these edges whose size s satisfies
 *   max(min_size, 1) <= s, and also s <= max_size when max_size > 0 (max_size == 0: no upper limit).  A usable point
 *   without an edge is a component of size 1.  The clusters are numbered 0 .. C-1 by decreasing size, equal sizes by the
 *   smallest member id, ascending.
 * Outputs: labels[i] = the cluster's number, or -1 for an unusable point or a point of a component outside the size
 *   range.  *n_clusters = C.  sizes[0 .. C) holds the sizes and is 0 in every remaining slot.  ids holds the members of
 *   cluster 0 in ascending id, then those of cluster 1, and so on, then -1 in every remaining slot (the padding of
 *   pcgx_kdtree_local_maxima); cluster c starts at the sum of the sizes before it.
 * PCGX_E_INVALID: a radius that is not finite and > 0; a NaN min_cos with normals given; a NaN max_curvature with
 *   curvature given; min_size < 0 or max_size < 0; 0 < max_size < max(min_size, 1); a NULL tree; NULL labels or
 *   n_clusters with Len() > 0.  Len() == 0 is PCGX_OK and writes only *n_clusters = 0.  A component is a property of a
 *   set: the same input gives the same bits on every call.
 * Always computed on the device.  Cost: the sum over the usable points of the records in the cells (or tree nodes) that
 *   their radius covers, as for Range, twice on a handle with a grid (a hook pass and a union pass), plus two radix sorts
 *   of Len() keys of ceil(log2(Len() + 1)) bits (one when ids is NULL).  What the edge test reads of a neighbour lies
 *   beside the grid's cell-ordered points (1 byte a record, 16 more with normals), not behind its id.  There is no
 *   wave-shared path for a grid row of thousands of coincident points (region growing has none either): such a row is one
 *   lane's loop for each of its points.
 *   Temporaries: 9 arrays of 4 Len() bytes, Len() bytes of flags, 16 Len() bytes with normals, and the radix sort's
 *   workspace; the host form stages its inputs and 4 (3 Len() + 1) bytes of outputs beside them. */
PCGX_API pcgx_status pcgx_kdtree_clusters(const pcgx_kdtree *t, float radius,
                                          const float *normals /* [3 Len()], may be NULL */, float min_cos,
                                          int32_t oriented, const float *curvature /* [Len()], may be NULL */,
                                          float max_curvature, int64_t min_size, int64_t max_size,
                                          int64_t *labels /* [Len()] */, int64_t *n_clusters,
                                          int64_t *sizes /* [Len()], may be NULL */,
                                          int64_t *ids /* [Len()], may be NULL */);
/* Same, every array device resident (labels, sizes, ids and the count are int32 there), enqueued on `stream` (NULL: the
 * library's); returns without waiting, reads nothing back. */
PCGX_API pcgx_status pcgx_kdtree_clusters_dev(const pcgx_kdtree *t, float radius, const float *d_normals, float min_cos,
                                              int32_t oriented, const float *d_curvature, float max_curvature,
                                              int64_t min_size, int64_t max_size, int32_t *d_labels /* [Len()] */,
                                              int32_t *d_n_clusters, int32_t *d_sizes /* [Len()], may be NULL */,
                                              int32_t *d_ids /* [Len()], may be NULL */, void *stream);

/* ------------------------------------------- density clusters (extension: no reference parity)
 * NOT in the reference.  DBSCAN (Ester, Kriegel, Sander and Xu 1996; Open3D's cluster_dbscan, scikit-learn's DBSCAN)
 * over the tree's own points: the components of the radius graph over the points whose neighbourhood is dense, plus the
 * points on their rim.  A single stray return between two objects joins them in "clusters" above; here it joins nobody
 * unless it has min_pts points around it.  Every array is in id order over the tree's own points, deleted ids included,
 * as in "clusters".  This comment is the contract, tests/dbscan_oracle.py restates it.
 * Neighbourhood: N(i) is the N(i) of "clusters": the points p of the tree with DistSq(p, point i) < radius^2, strict,
 *   DistSq the reference's float32 expression: exactly the set pcgx_kdtree_range_count counts on that handle (grid,
 *   forced walk, after DeletePoint).  Deleted points are nobody's neighbour and count for nobody.
 * Usable point: i is usable iff i is in N(i) (this excludes a deleted id and a point with a NaN or infinite
 *   coordinate).  There are no normals and no curvature in this call: no cut of either kind.
 * Core point: i is core iff it is usable and |N(i)| >= min_pts.  The point counts itself (as in Open3D and
 *   scikit-learn), and every member of N(i) counts, core or not.  min_pts >= 1.
 * Core edge: {i, j} with i != j is an edge iff both points are core and j is in N(i) (symmetric bit for bit).
 * Border point: a usable point that is not core and has at least one core point in N(i).  It belongs to the component
 *   of its nearest core neighbour: the one of the smallest float32 DistSq, of equal ones the one of the smallest id.
 *   (The textbook rule, "whichever cluster reaches it first", depends on the visit order and cannot be pinned; this one
 *   is a property of the point set, and it is local: no component's name is needed to decide it.)  A border point
 *   carries no edge and joins nobody else.
 * Noise: every other point: the unusable ones, and the points that are not core and have no core point in N(i).
 * Clusters: a cluster is a connected component of the core points under the core edges, plus its border points.  Its
 *   size counts both, and its smallest member id is taken over both.  It is kept when max(min_size, 1) <= size, and
 *   also size <= max_size when max_size > 0 (max_size == 0: no upper limit).  The clusters are numbered 0 .. C-1 by
 *   decreasing size, equal sizes by the smallest member id, ascending.
 * Outputs: labels[i] = the cluster's number, or -1 for a noise point or a point of a cluster outside the size range.
 *   *n_clusters = C.  sizes[0 .. C) holds the sizes and is 0 in every remaining slot.  ids holds the members of cluster
 *   0 in ascending id, then those of cluster 1, and so on, then -1 in every remaining slot; cluster c starts at the sum
 *   of the sizes before it.  (Word for word the outputs of pcgx_kdtree_clusters[_dev], int64 in the host form, int32 in
 *   the device form: d_ids, d_sizes and d_n_clusters can be passed on to pcgx_kdtree_group_stats_dev and
 *   pcgx_kdtree_group_hulls_dev as they are.)
 *   kind[i], uint8_t in both forms, optional: 0 noise or unusable, 1 border, 2 core.  kind does not depend on the size
 *   range: a core point of a cluster that is dropped for its size keeps kind 2 and gets label -1.
 * min_pts == 1: every usable point is core, and labels, *n_clusters, sizes and ids equal those of pcgx_kdtree_clusters
 *   with normals == NULL and curvature == NULL on that handle bit for bit; no count pass runs.
 * PCGX_E_INVALID: a radius that is not finite and > 0; min_size < 0 or max_size < 0; 0 < max_size < max(min_size, 1);
 *   a NULL tree; NULL labels or n_clusters with Len() > 0; min_pts < 1.  Nothing is written then.  Len() == 0 is
 *   PCGX_OK and writes only *n_clusters = 0.  The same input gives the same bits on every call.
 * Always computed on the device.  Cost: what pcgx_kdtree_clusters costs, plus with min_pts >= 2 two more enumerations:
 *   a flag pass (per point the records of the cells, or tree nodes, that its radius covers, on a grid only until min_pts
 *   of them are in reach) and a border pass (the same records, whole, for the usable points that are not core).  There
 *   is no wave-shared path for a grid row of thousands of coincident points, as in clusters: such a row is one lane's
 *   loop for each of its points.  Temporaries: those of pcgx_kdtree_clusters and Len() more bytes of flags. */
PCGX_API pcgx_status pcgx_kdtree_dbscan(const pcgx_kdtree *t, float radius, int32_t min_pts, int64_t min_size,
                                        int64_t max_size, int64_t *labels /* [Len()] */, int64_t *n_clusters,
                                        int64_t *sizes /* [Len()], may be NULL */,
                                        int64_t *ids /* [Len()], may be NULL */,
                                        uint8_t *kind /* [Len()], may be NULL */);
/* Same, every array device resident (labels, sizes, ids and the count are int32 there, kind stays uint8_t), enqueued on
 * `stream` (NULL: the library's); returns without waiting, reads nothing back. */
PCGX_API pcgx_status pcgx_kdtree_dbscan_dev(const pcgx_kdtree *t, float radius, int32_t min_pts, int64_t min_size,
                                            int64_t max_size, int32_t *d_labels /* [Len()] */, int32_t *d_n_clusters,
                                            int32_t *d_sizes /* [Len()], may be NULL */,
                                            int32_t *d_ids /* [Len()], may be NULL */,
                                            uint8_t *d_kind /* [Len()], may be NULL */, void *stream);

/* ------------------------------------------- group geometry (extension: no reference parity)
 * NOT in the reference.  What a user takes from clusters next: per group of a grouped id list over the tree's own
 * points -- the shape pcgx_kdtree_clusters writes, and what region growing's components, a plane's inliers or a keypoint
 * list are -- the count, the axis-aligned box, centroid and covariance, the covariance's eigenvalues and axes (the fitted
 * plane and the principal frame) and the oriented box in that frame.  This comment is the contract,
 * tests/group_oracle.py restates it.
 *   pcgx_kdtree_group_stats    (t, ids[n_ids] i64, n_ids, sizes[n_groups] i64, n_groups, outputs...)
 *   pcgx_kdtree_group_stats_dev(t, d_ids[cap_ids] i32, cap_ids, d_sizes[cap_groups] i32, cap_groups,
 *                               d_n_groups (one int32; NULL: cap_groups), outputs... [cap_groups rows], stream)
 * Groups: on the device form G = clamp(*d_n_groups, 0, cap_groups), read on the device; on the host form G = n_groups.
 *   Group g owns the slots [o_g, o_g + max(sizes[g], 0)) of ids, o_g = the sum of the earlier (clamped) sizes: the
 *   layout pcgx_kdtree_clusters writes.  Slots at or beyond cap_ids do not exist: the list is clipped there.  The labels
 *   array is not an input.  d_ids, d_sizes and d_n_clusters of pcgx_kdtree_clusters_dev can be passed on as they are,
 *   with cap_ids = cap_groups = Len().
 * Live member: a slot is live when 0 <= id < Len() and the point's three coordinates are finite.  Ids may repeat and
 *   are then counted each time.  Deleted ids are allowed and use the stored coordinates (as pcgx_kdtree_fpfh_at allows).
 *   A dead slot is skipped; this covers the -1 padding.  The host form rejects an id outside [0, Len()) and a size sum
 *   above n_ids, as pcgx_kdtree_fpfh_at does, and then writes nothing.
 * Outputs: each may be NULL.  Every row of [0, cap_groups) is written on every call; rows >= G, and rows of groups
 *   without a live member, are all zero.
 *   count[g]        the number of live members (int32 on the device, int64 on the host).
 *   aabb[6 g ..]    float32: lo x, y, z then hi x, y, z over the live members.  Exact.
 *   centroid[3 g ..], cov[6 g ..]  float64: the mean of the members, and sum d d^T / n - m m^T in the order (xx, xy, xz,
 *                   yy, yz, zz) (csrc/cov3.h), both evaluated in float64 with the sums centred on a pivot inside the
 *                   group's own box: the box centre (lo + hi) / 2 widened to double.  d = p - pivot in float64, the sums
 *                   with one rounding per term (the products are fused into the additions), in an order fixed by the
 *                   group's place in the list alone: per run of the group inside 64 consecutive slots, then the runs in
 *                   slot order (a group of more than four such runs: lanes striding the runs, then a butterfly over the
 *                   64 partial sums); centroid = pivot + s / n,
 *                   cov = q / n - (s / n)(s / n)^T (csrc/group_terms.h).
 *                   Bounds, n the live count, D the diagonal of the group's box: each element of cov within
 *                   (2 n + 4) 2^-53 D^2 of the exact value (tests/cov_exact.py's bound B with S <= D^2; it holds for any
 *                   pivot inside the box and any order), each component c of the centroid within
 *                   (n + 2) 2^-53 D + 2^-53 |c| of the exact mean (n - 1 additions of terms bounded by D, the division,
 *                   the addition of the pivot).  Both take p - pivot to be exact in float64, which it is whenever a
 *                   group's nonzero coordinates along an axis differ by less than 2^28 in magnitude.
 *   eig[3 g ..]     float64: the eigenvalues of cov, descending.
 *   axes[9 g ..]    float64: the three unit eigenvectors as rows, in that order.  Axis 2 is the fitted plane's normal,
 *                   the plane passes through the centroid, and eig[2] / (eig[0] + eig[1] + eig[2]) is the surface
 *                   variation pcgx_kdtree_normals calls curvature.  Sign: axis 0 and axis 1 are each turned so that their
 *                   component of largest magnitude is positive (on a tie the first such component decides);
 *                   axis 2 = axis 0 x axis 1, so the frame is right-handed.  If the trace is 0 or not finite (all
 *                   members at one place), eig = 0 and axes = identity.  Equal eigenvalues keep the order of their
 *                   diagonal positions (x, y, z) in the solve: cyclic Jacobi at unit trace, as csrc/cov3.h.
 *   obb[6 g ..]     float64: with e-_k and e+_k the least and greatest of (p - centroid) . axis_k over the live members,
 *                   evaluated in float64: the centre centroid + sum_k ((e+_k + e-_k) / 2) axis_k as x, y, z, then the
 *                   half-extents h_k = (e+_k - e-_k) / 2.  The principal-axes box, not the box of smallest volume.
 * PCGX_E_INVALID: a NULL tree; negative counts or capacities; NULL ids or sizes with a positive count; more than
 *   2^31 - 1 slots (or groups); on the host form an id outside [0, Len()) or a size sum above n_ids.  G = 0 or
 *   cap_groups = 0 is PCGX_OK.
 * Determinism: the same input gives the same bits on every call.  No floating-point atomic feeds a sum; min / max are
 *   combined with integer atomics on order-preserving keys, in any order.
 * Always computed on the device (csrc/group_stats.hip), nothing read back in the device form.  Cost: three gathers of
 *   16 B per slot (box, moments, extents; two when obb is NULL), 16 B of reads per slot and pass for the slot -> group
 *   map and the ids, one record of 80 B per run of a group inside 64 consecutive slots in an array of
 *   ceil(cap_ids / 64) + cap_groups records, and per group 24 + 48 B of keys, 96 B of frame and a Jacobi solve in one
 *   lane.  The id -> node map of the handle is made on first use (as pcgx_kdtree_fpfh_at makes it). */
PCGX_API pcgx_status pcgx_kdtree_group_stats(const pcgx_kdtree *t, const int64_t *ids /* [n_ids] */, int64_t n_ids,
                                             const int64_t *sizes /* [n_groups] */, int64_t n_groups,
                                             int64_t *count /* [n_groups] */, float *aabb /* [6 n_groups] */,
                                             double *centroid /* [3 n_groups] */, double *cov /* [6 n_groups] */,
                                             double *eig /* [3 n_groups] */, double *axes /* [9 n_groups] */,
                                             double *obb /* [6 n_groups] */);
/* Same, every array device resident (ids, sizes and counts are int32 there), enqueued on `stream` (NULL: the library's);
 * returns without waiting, reads nothing back. */
PCGX_API pcgx_status pcgx_kdtree_group_stats_dev(const pcgx_kdtree *t, const int32_t *d_ids /* [cap_ids] */,
                                                 int64_t cap_ids, const int32_t *d_sizes /* [cap_groups] */,
                                                 int64_t cap_groups, const int32_t *d_n_groups /* may be NULL */,
                                                 int32_t *d_count, float *d_aabb, double *d_centroid, double *d_cov,
                                                 double *d_eig, double *d_axes, double *d_obb, void *stream);
/* Slots per tile of the slot -> group map; the gathers cut a run of a group every 64 slots and take four tiles to a
 * workgroup (the boundaries the tests put groups across). */
PCGX_API int32_t pcgx_group_stats_tile(void);

/* ------------------------------------------- group footprints (extension: no reference parity)
 * NOT in the reference.  What a tracker or planner takes from a cluster of an upright scene: per group of a grouped id
 * list, the polygon the group stands on -- the exact convex hull of its members' (x, y) -- that polygon's area, and the
 * smallest upright rectangle with a side along one of its edges (a car seen from one corner is an L of points: the
 * principal-axes box of "group geometry" runs along the L's diagonal, this one along the car).  This comment is the
 * contract, tests/hull_oracle.py restates it.
 *   pcgx_kdtree_group_hulls    (t, ids[n_ids] i64, n_ids, sizes[n_groups] i64, n_groups,
 *                               hull_sizes[n_groups] i64, hull_ids[n_ids] i64, area[n_groups] f64, rect[6 n_groups] f64)
 *   pcgx_kdtree_group_hulls_dev(t, d_ids[cap_ids] i32, cap_ids, d_sizes[cap_groups] i32, cap_groups, d_n_groups,
 *                               d_hull_sizes[cap_groups] i32, d_hull_ids[cap_ids] i32, d_area, d_rect, stream)
 * Inputs: the groups, the clip at cap_ids, the live-member test, G, the error codes and what the host form rejects are
 *   those of pcgx_kdtree_group_stats[_dev] above, word for word (the same checks, the same messages under these names).
 *   cap_groups = 0 is PCGX_OK.  A tree of no points gives all-zero rows and an all -1 hull_ids.  Every output may be
 *   NULL, and a NULL output changes no bit of the others.
 * Footprint: the set of (x, y) of the group's live members, as stored, z dropped (other up-axes are out of scope).
 *   Two members are at the same place when both coordinates compare ==, so -0 equals +0.  A place is represented by the
 *   smallest id among the group's live members at it.
 * Vertices: a place is a vertex exactly when it is a strict extreme point of the convex hull of the group's places, in
 *   exact real arithmetic on the float32 values.  A place on the boundary between two others is not a vertex.  A group
 *   with one place has 1 vertex; a group whose places all lie on one line has 2, its lexicographically least and greatest
 *   (x, then y); a group without a live member has 0.
 *   hull_sizes[g]   h_g, the number of vertices of group g (int32 on the device, int64 on the host); 0 for rows >= G.
 *   hull_ids        again a grouped id list: group g's vertices stand at [H_g, H_g + h_g), H_g the sum of the earlier
 *                   hull_sizes, counter-clockwise, starting at the lexicographically least place; everything from the
 *                   total to the capacity (cap_ids, n_ids) is -1.  (hull_ids, hull_sizes) can go straight into
 *                   pcgx_kdtree_group_stats or back into this call, which returns them unchanged.
 *   area[g]         float64: half the sum over k = 1 .. h - 2 of cross(v_k - v_0, v_{k+1} - v_0), the differences in
 *                   float64, each term (a - v0)_x (b - v0)_y - (a - v0)_y (b - v0)_x (csrc/hull_terms.h), the terms added
 *                   in that order; 0 for h < 3.  Within 2 h 2^-53 D^2 of the exact area, D the diagonal of the group's
 *                   xy box (each term: two products and a difference of values bounded by D^2; h - 3 additions of
 *                   partial sums bounded by D^2), the differences taken to be exact as in "group geometry".
 *   rect[6 g ..]    float64: the minimum-area enclosing rectangle with one side along a hull edge: the centre x, y; the
 *                   unit direction u of that edge; the half-extents along u and along n = (-u_y, u_x).  For every edge k
 *                   in order (from v_k to v_{k+1}, the last one back to v_0): u = (v_{k+1} - v_k) / |v_{k+1} - v_k| in
 *                   float64, the least and greatest of s = (p - v_k) . u and t = (p - v_k) . n over all h vertices p, and
 *                   the product of the two widths; the first edge with the smallest product wins.  centre = v_k +
 *                   ((s+ + s-) / 2) u + ((t+ + t-) / 2) n, half-extents (s+ - s-) / 2 and (t+ - t-) / 2.
 *                   h = 2: u along the segment from vertex 0 to vertex 1, second half-extent 0.  h = 1: the centre at the
 *                   point, u = (1, 0), half-extents 0.  h = 0: zeros.  The rectangle's area is within 32 2^-53 D^2 of
 *                   the exact minimum over the edges (u: four roundings; a projection: three more; a width within
 *                   13 2^-53 D; the product of two widths bounded by D).
 * PCGX_E_INVALID: as pcgx_kdtree_group_stats[_dev].
 * Determinism: the same input gives the same bits on every call.  No floating-point atomic feeds a result; the extremes
 *   are combined with integer atomics on order-preserving keys, every other order is fixed by the input.
 * Always computed on the device (csrc/group_hull.hip), nothing read back in the device form, which returns without
 *   waiting.  A member is dropped from consideration only on exact evidence that it is no vertex: the sign of an
 *   orientation determinant against real input points, from a float64 evaluation under a static error bound and, where
 *   that does not certify it, from the exact sum of the six products (csrc/hull_terms.h).  Cost: two gathers of 16 B per
 *   slot, four stable radix sorts of 32-bit pairs over cap_ids (id, y, x, group), 53 B of temporaries per slot and 80 B
 *   per group; a group whose members are nearly all vertices is chained by one lane. */
PCGX_API pcgx_status pcgx_kdtree_group_hulls(const pcgx_kdtree *t, const int64_t *ids /* [n_ids] */, int64_t n_ids,
                                             const int64_t *sizes /* [n_groups] */, int64_t n_groups,
                                             int64_t *hull_sizes /* [n_groups] */, int64_t *hull_ids /* [n_ids] */,
                                             double *area /* [n_groups] */, double *rect /* [6 n_groups] */);
/* Same, every array device resident (ids and sizes are int32 there), enqueued on `stream` (NULL: the library's);
 * returns without waiting, reads nothing back. */
PCGX_API pcgx_status pcgx_kdtree_group_hulls_dev(const pcgx_kdtree *t, const int32_t *d_ids /* [cap_ids] */,
                                                 int64_t cap_ids, const int32_t *d_sizes /* [cap_groups] */,
                                                 int64_t cap_groups, const int32_t *d_n_groups /* may be NULL */,
                                                 int32_t *d_hull_sizes /* [cap_groups] */,
                                                 int32_t *d_hull_ids /* [cap_ids] */, double *d_area, double *d_rect,
                                                 void *stream);
/* Survivors a lane of the hull's reduce rounds takes at a time (a boundary the tests put hulls across). */
PCGX_API int32_t pcgx_group_hulls_chunk(void);

/* ------------------------------------------- pose from correspondences (extension: no reference parity)
 * NOT in the reference.  The rigid motion (a proper rotation and a translation, no scale) that most pairs of a
 * correspondence list agree on, by sample consensus: the starting pose every Fit here needs, from what
 * pcgx_fpfh_correspondences returns.  As in pcgx_sac_plane_compute the caller draws every random number first; one call
 * fits and scores all hypotheses and returns the first best.  This comment is the contract, tests/pose_oracle.py
 * restates it.
 * Pairs: pair k < m is (point src_ids[k] of src_xyz, point dst_ids[k] of dst_xyz); p_k and q_k are its two points.
 * Samples: a sample is a random 32-bit word u; the pair it names is (uint64(u) * m) >> 32, computed on the device, so one
 *   sample array serves the host form and the device form, where m is not known to the host.  Hypothesis h uses
 *   samples[3h], [3h + 1], [3h + 2]: pairs i0, i1, i2.
 * Hypothesis h, in this order:
 *   status 1 (bad sample): m < 3, or two of i0, i1, i2 are equal, or one of the three pairs names an id outside
 *     [0, ns) / [0, nd).
 *   status 2 (degenerate): the source triangle or the target triangle is degenerate.  With e1 = x1 - x0, e2 = x2 - x0 in
 *     float64 from the float32 points, c = e1 x e2, norms as (x x + y y) + z z: degenerate unless
 *     |c|^2 > (1e-12 * |e1|^2) * |e2|^2 (a comparison that fails on a NaN counts as degenerate).
 *   status 3 (edge): edge_similarity s > 0 and, for one of the edges (0,1), (0,2), (1,2), the source length ls and the
 *     target length ld (float64, a correctly rounded sqrt) fail ls >= s * ld or ld >= s * ls.  s = 0 switches the test off.
 *   status 0 otherwise.  Its pose is the proper rotation R and the translation t that minimise sum |R p_i + t - q_i|^2
 *     over the three pairs, computed in float64 from the float32 inputs, each of the twelve numbers rounded once to
 *     float32 into a column-major 4 x 4 (m[4 col + row], the layout of pcgx_mat4_transform), bottom row 0 0 0 1.
 *     count[h] = the number of pairs k < m with both ids in range and DistSq < max_dist_sq, where
 *     x' = pcgx_mat4_transform(pose, p_k), d = q_k - x', DistSq = (dx dx + dy dy) + dz dz: all float32, nothing fused;
 *     given the pose's bits the count has no tolerance.  A NaN is not an inlier.
 *   A rejected hypothesis (status != 0) has count 0 and an all-zero pose.
 * Best: the status-0 hypothesis with the largest count, the smallest h among equals; best = -1 when there is none.
 *   found = (that count >= 3).  pose, n_inliers and inlier_ids describe the pose that is kept (the best's, or its
 *   refinement): the inliers' k in ascending order, -1 from n_inliers to m.  With best = -1 the pose is all zero.
 * Refinement (refine != 0 and found): I = the best's inliers in ascending k.  The refined pose is the same minimiser over
 *   I, from float64 moments {n, sum p, sum q, sum p q^T} taken about the first inlier's two points (small cancellation)
 *   and summed in a fixed order without float atomics: the same input gives the same bits on every call.  The pairs are
 *   counted again under the refined pose; it replaces the best's when its count is >= best_count (then refined = 1 and
 *   n_inliers, inlier_ids are its own; best and best_count keep describing the hypothesis).
 *   Too degenerate to refit (refined = 0, the hypothesis's pose is kept): fewer than three inliers, or l1 - l2 <=
 *   1e-9 * l1, where l1 >= l2 are the two largest eigenvalues of the symmetric 4 x 4 matrix N of Horn's closed form
 *   whose top eigenvector is the rotation (the solve has them).  In terms of the singular values s1 >= s2 >= s3 of the
 *   centred sum p q^T and d = the sign of its determinant: l1 = s1 + s2 + d s3 and l1 - l2 = 2 (s2 + d s3), which is
 *   zero when the inliers of either cloud lie on a line: the rotation about the line is then free.
 * Arguments: PCGX_E_INVALID for a NULL array with a positive count, a NULL scalar output, a negative count, more than
 *   2^31 - 1 points, pairs or hypotheses, max_dist_sq not finite or not > 0, edge_similarity outside [0, 1] or NaN, and
 *   -- on the host path only, where the list can be read -- a pair that names an id out of range.  On the device path
 *   such a pair is never an inlier and a hypothesis that draws it has status 1.  n_hyp == 0 or m == 0 is PCGX_OK with
 *   found = 0, best = -1 (every status 1).  inlier_ids [m], status [n_hyp], counts [n_hyp] and poses [16 n_hyp] may be
 *   NULL.  Always computed on the device: about 30 m n_hyp float32 operations; 32 m + 72 n_hyp bytes of temporaries at
 *   most.  The pairs are split into S chunks to fill the chip (the library's choice; PCGX_POSE_SPLIT=<n> in the
 *   environment, read per call, forces it -- any n gives the same bits). */
PCGX_API pcgx_status pcgx_pose_from_correspondences(const float *src_xyz /* [3 ns] */, int64_t ns,
                                                    const float *dst_xyz /* [3 nd] */, int64_t nd,
                                                    const int64_t *src_ids /* [m] */, const int64_t *dst_ids /* [m] */,
                                                    int64_t m, const uint32_t *samples /* [3 n_hyp] */, int64_t n_hyp,
                                                    float max_dist_sq, float edge_similarity, int32_t refine,
                                                    int32_t *found, int64_t *best, int64_t *best_count, float pose16[16],
                                                    int32_t *refined, int64_t *n_inliers, int64_t *inlier_ids,
                                                    int32_t *status, int64_t *counts, float *poses);
/* Same, every array device resident, enqueued on `stream` (NULL: the library's); returns without waiting.  Ids, status
 * and counts are int32.  The list is the first *d_n_pairs (held to [0, m_cap]) of d_src_ids / d_dst_ids [m_cap], read on
 * the device -- pcgx_fpfh_correspondences_dev's outputs feed it with nothing read back; d_n_pairs == NULL: m_cap pairs.
 * d_inlier_ids is [m_cap].  The scalar outputs go to d_result, PCGX_POSE_RESULT_WORDS 4-byte words: int32 found, best,
 * best_count, refined, n_inliers, m (the list's length as used), 0, 0, then the float32 pose in words 8..23. */
#define PCGX_POSE_RESULT_WORDS 24
PCGX_API pcgx_status pcgx_pose_from_correspondences_dev(const float *d_src_xyz, int64_t ns, const float *d_dst_xyz,
                                                        int64_t nd, const int32_t *d_src_ids, const int32_t *d_dst_ids,
                                                        int64_t m_cap, const int32_t *d_n_pairs,
                                                        const uint32_t *d_samples, int64_t n_hyp, float max_dist_sq,
                                                        float edge_similarity, int32_t refine, void *d_result,
                                                        int32_t *d_inlier_ids /* may be NULL */,
                                                        int32_t *d_status /* may be NULL */,
                                                        int32_t *d_counts /* may be NULL */,
                                                        float *d_poses /* may be NULL */, void *stream);
/* Hypotheses per workgroup of the count kernel (a wave, two hypotheses per lane): the boundary the tests put n_hyp
 * across. */
PCGX_API int32_t pcgx_pose_tile(void);

/* ------------------------------------------- planes (extension: no reference parity)
 * NOT in the reference (its plane detector is the voxel-grid surface patch, pcgx_sac_plane_compute).  Plane segmentation
 * as Open3D's segment_plane or PCL's SACSegmentation in a loop with ExtractIndices: the infinite plane most points lie
 * within max_dist of, optionally roughly perpendicular to an axis and agreeing with the points' normals; its inliers are
 * taken out and the next plane is looked for, up to max_planes times.  As in pcgx_pose_from_correspondences the caller
 * draws every random word first; one call fits and scores all hypotheses of every round, the first best of a round wins.
 * This comment is the contract, tests/plane_oracle.py restates it.
 *   pcgx_kdtree_planes    (t, samples[3 n_hyp max_planes] u32, n_hyp, max_planes, max_dist, min_inliers,
 *                          axis[3] | NULL, min_axis_cos, normals[3 Len()] | NULL, min_normal_cos, refine,
 *                          n_planes*, planes[4 max_planes] f32, sizes[max_planes] i64, refined[max_planes] i32,
 *                          best[max_planes] i64, labels[Len()] i64, ids[Len()] i64 | NULL,
 *                          status[max_planes n_hyp] i32 | NULL, counts[...] i64 | NULL, hyp_planes[4 ...] f32 | NULL)
 *   pcgx_kdtree_planes_dev(... every array device resident, ids / sizes / labels / counts / best int32,
 *                          d_n_planes one int32, stream)
 * Live point: not deleted (pcgx_kdtree_delete_point[s]), its three coordinates finite and, with normals != NULL, its three
 *   normal components finite and not all zero (the zero normal is pcgx_kdtree_normals' answer for a degenerate
 *   neighbourhood).  A point that is not live is never sampled and never an inlier; its label is -1.
 * Rounds: A_0 = the live ids in ascending order, R_r = |A_r|.  Round r runs iff r < max_planes, every earlier round
 *   found a plane and R_r >= 3.  Hypothesis h of round r uses samples[3 (r n_hyp + h) + j], j = 0, 1, 2; word u names the
 *   point A_r[(uint64(u) * R_r) >> 32], computed on the device: one sample array serves both forms.
 * Hypothesis, in this order: status 1 (bad sample): two of the three indices are equal.  Status 2 (degenerate): the
 *   triangle test of pcgx_pose_from_correspondences on the three points (the same expression, the same 1e-12).  Status 3
 *   (axis): `axis` is given and the plane fails the axis test.  Status 0 otherwise.  A rejected hypothesis has count 0 and
 *   a zero plane; the rows of a round that did not run hold status -1, count 0 and a zero plane.
 * Plane of a status-0 hypothesis, in float64 from the float32 points, each operation rounded once, nothing contracted:
 *   e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2, n = c / sqrt((cx cx + cy cy) + cz cz).  Axis test, on this n:
 *   |(nx ax + ny ay) + nz az| >= (double)min_axis_cos * |a|, |a| = sqrt((ax ax + ay ay) + az az) in float64 from the
 *   float32 axis.  Sign: with an axis n is turned so that (nx ax + ny ay) + nz az >= 0; where that expression is 0, and
 *   without an axis, so that its component of largest magnitude is positive, the first such component on a tie (the rule
 *   of pcgx_kdtree_group_stats' axes).  d = -((nx p0x + ny p0y) + nz p0z).  The four numbers are rounded once to float32.
 * Inlier of plane (n, d): a point of A_r with fabsf(((nx px + ny py) + nz pz) + d) < max_dist, all float32, nothing
 *   fused, the comparison strict; with normals also fabsf((nx mx + ny my) + nz mz) >= min_normal_cos for the point's
 *   normal m as given.  A NaN is not an inlier.  Given the plane's bits the count has no tolerance.
 * Best of a round: the status-0 hypothesis with the largest count, the smallest h among equals.  The round FINDS a plane
 *   iff that count >= max(min_inliers, 3); otherwise this round and all later ones did not.  n_planes = the number of
 *   rounds that found one.
 * Refinement (refine != 0, the round found a plane): I = the best's inliers in ascending id.  The refitted plane has the
 *   centroid c and axis 2, a, that pcgx_kdtree_group_stats returns for the one-group list I (the same kernels: the same
 *   bits); a is signed by the rule above, n = float32(a), d = float32(-((ax cx + ay cy) + az cz)) in float64.  No refit
 *   when group geometry answers the degenerate frame (eig[0] is not > 0) or the refitted normal fails the axis test.  The
 *   points of A_r are counted again under the refitted plane; it replaces the hypothesis's iff its count >= the best's
 *   count: then refined[r] = 1 and the round's inliers are its own.  One refit, not an iteration.
 * Outputs: planes[4 r ..] the kept plane, best[r] the winning h, sizes[r] the kept plane's inlier count, labels[i] the
 *   round that took point i or -1, ids: round 0's inliers ascending, then round 1's, ..., -1 in the remaining slots (what
 *   pcgx_kdtree_group_stats[_dev] and pcgx_kdtree_group_hulls[_dev] take, with sizes and n_planes).  From n_planes on,
 *   sizes, planes and refined are 0 and best is -1.  A_{r+1} = A_r minus the inliers of round r's kept plane.  Every row
 *   of every output is written on every call.
 * PCGX_E_INVALID (nothing is written): a NULL tree, n_hyp < 0, max_planes outside [1, 256], max_dist not finite or not
 *   > 0, min_inliers < 0, an axis that is not finite or all zero, min_axis_cos (with an axis) or min_normal_cos (with
 *   normals) outside [0, 1] or NaN, NULL samples with n_hyp > 0, a NULL mandatory output (labels only where Len() > 0),
 *   n_hyp * max_planes above 2^31 - 1.  n_hyp == 0 or Len() == 0 is PCGX_OK with n_planes = 0.
 * Always computed on the device (csrc/planes.hip).  The same input gives the same bits on every call: no float atomic
 *   anywhere, counts are added by integer atomics.  The points are split into chunks to fill the chip (the library's
 *   choice; PCGX_PLANES_SPLIT=<n> in the environment, read per call, forces it -- any n gives the same bits). */
PCGX_API pcgx_status pcgx_kdtree_planes(const pcgx_kdtree *t, const uint32_t *samples /* [3 n_hyp max_planes] */,
                                        int64_t n_hyp, int32_t max_planes, float max_dist, int64_t min_inliers,
                                        const float *axis /* [3] or NULL */, float min_axis_cos,
                                        const float *normals /* [3 Len()] or NULL */, float min_normal_cos, int32_t refine,
                                        int64_t *n_planes, float *planes, int64_t *sizes, int32_t *refined, int64_t *best,
                                        int64_t *labels, int64_t *ids /* may be NULL */, int32_t *status /* may be NULL */,
                                        int64_t *counts /* may be NULL */, float *hyp_planes /* may be NULL */);
/* Same, every array device resident (`axis` alone stays three floats in HOST memory: it is an argument, checked before
 * anything is enqueued), enqueued on `stream` (NULL: the library's); returns without waiting and reads nothing back.
 * Ids, sizes, labels, counts and best are int32, d_n_planes is one int32.  All max_planes rounds are enqueued at once; a
 * round reads from device words how many points are left and whether an earlier round failed.  d_ids, d_sizes and
 * d_n_planes can be passed on to pcgx_kdtree_group_stats_dev and pcgx_kdtree_group_hulls_dev as they are (cap_ids =
 * Len(), cap_groups = max_planes).  A handle with deleted points has its deleted flags copied to the device first, and
 * that copy alone is waited for. */
PCGX_API pcgx_status pcgx_kdtree_planes_dev(const pcgx_kdtree *t, const uint32_t *d_samples, int64_t n_hyp,
                                            int32_t max_planes, float max_dist, int64_t min_inliers,
                                            const float *axis /* HOST [3] or NULL */, float min_axis_cos,
                                            const float *d_normals /* may be NULL */, float min_normal_cos, int32_t refine,
                                            int32_t *d_n_planes, float *d_planes, int32_t *d_sizes, int32_t *d_refined,
                                            int32_t *d_best, int32_t *d_labels, int32_t *d_ids /* may be NULL */,
                                            int32_t *d_status /* may be NULL */, int32_t *d_counts /* may be NULL */,
                                            float *d_hyp_planes /* may be NULL */, void *stream);
/* Hypotheses per workgroup of the count kernel (a wave, two hypotheses per lane): the boundary the tests put n_hyp
 * across. */
PCGX_API int32_t pcgx_planes_tile(void);

/* ------------------------------------------- shapes (extension: no reference parity)
 * NOT in the reference.  Cylinder and sphere segmentation as PCL's SACSegmentationFromNormals with SACMODEL_CYLINDER /
 * SACMODEL_SPHERE in a loop with ExtractIndices, the hypotheses made from TWO oriented points (Schnabel, Wahl, Klein
 * 2007), the second drawn from the first's radius neighbourhood: a pole holds a thousandth of a cloud, and two points
 * drawn from all of it lie on the same pole once in a million draws.  The rounds, the samples, the first best, the
 * peeling and the outputs are pcgx_kdtree_planes'; where a point is not stated here, that contract holds word for word.
 * This comment is the contract, tests/shape_oracle.py restates it.
 *   pcgx_kdtree_shapes    (t, kind, samples[2 n_hyp max_shapes] u32, n_hyp, max_shapes, max_dist, min_inliers,
 *                          sample_radius, r_min, r_max, axis[3] | NULL, min_axis_cos, normals[3 Len()], min_normal_cos,
 *                          refine, n_shapes*, shapes[8 max_shapes] f32, sizes[max_shapes] i64, refined[max_shapes] i32,
 *                          best[max_shapes] i64, labels[Len()] i64, ids[Len()] i64 | NULL,
 *                          status[max_shapes n_hyp] i32 | NULL, counts[...] i64 | NULL, hyp_shapes[8 ...] f32 | NULL)
 *   pcgx_kdtree_shapes_dev(... every array device resident, ids / sizes / labels / counts / best int32,
 *                          d_n_shapes one int32, stream; axis stays a host argument)
 * kind: PCGX_SHAPE_SPHERE (0) or PCGX_SHAPE_CYLINDER (1).  Normals are mandatory: the hypotheses are made from them.
 * Live point, A_r, R_r and how a word names an index: pcgx_kdtree_planes' with normals given.  Round r runs iff
 *   r < max_shapes, every earlier round found a shape and R_r >= 2.
 * Sampling: hypothesis h of round r uses u0 = samples[2 (r n_hyp + h)] and u1 = samples[2 (r n_hyp + h) + 1].  The seed
 *   is i0 = A_r[(u0 R_r) >> 32].  With sample_radius == 0 the partner is i1 = A_r[(u1 R_r) >> 32]; status 1 if i1 == i0.
 *   With sample_radius > 0 the candidates are the points of A_r other than i0 in the set pcgx_kdtree_range_count counts
 *   for the seed and that radius on that handle (strict bound, deleted points absent; points taken by earlier rounds are
 *   not in A_r).  The partner is the candidate with the smallest (x, id), x in uint32 arithmetic:
 *   x = u1 ^ (id * 0x9E3779B1); x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16.  No candidate:
 *   status 1.  The choice is a property of the set, not of the order it is enumerated in: the grid, the tree walk
 *   (PCGX_RANGE_WALK=1) and the patched walk of a handle with deletions give the same partner.
 * Hypothesis of (p0, n0), (p1, n1), in float64 from the float32 numbers, each operation rounded once, nothing contracted,
 *   dots as (x x + y y) + z z:  w = p0 - p1, A = n0.n0, B = n0.n1, C = n1.n1, D = n0.w, E = n1.w, den = A C - B B.
 *   Status 2 (degenerate) unless den > 1e-12 (A C) (a comparison that fails on NaN is degenerate).  s = (B E - C D) / den,
 *   t = (A E - B D) / den: c0 = p0 + s n0 and c1 = p1 + t n1 are the closest points of the two normal lines,
 *   m = 0.5 (c0 + c1).  Sphere: the centre is m, r = 0.5 (|p0 - m| + |p1 - m|).  Cylinder: a = n0 x n1 divided by
 *   sqrt((ax ax + ay ay) + az az); axis test, status 3, as the planes' on this a: |a . axis| >= (double)min_axis_cos |axis|
 *   (the cylinder's axis PARALLEL to `axis`: poles along z); a is signed by the planes' rule; q = m - (m.a) a, the axis
 *   point nearest the origin; r = 0.5 (rho(p0) + rho(p1)), rho(p) = sqrt(max(0, |v|^2 - (v.a)^2)), v = p - q (max(0, x)
 *   is x where x > 0, else 0).  Status 4 (radius): !(r >= r_min && r <= r_max) on the float64 r, or a number of the
 *   record is not finite once rounded to float32.  Status 0 otherwise.
 * Record, 8 float32, each number rounded once: sphere {cx, cy, cz, r, 0, 0, 0, 0}, cylinder {qx, qy, qz, r, ax, ay, az,
 *   0}.  A rejected hypothesis has count 0 and a zero record; rows of a round that did not run hold status -1.
 * Inlier: float32 throughout, nothing fused, no square root: given the record's bits the count has no tolerance.  Once
 *   per record lo = r - max_dist, hi = r + max_dist, hi2 = hi hi, lo2 = lo lo if lo > 0 else -1,
 *   c2 = min_normal_cos min_normal_cos.  Per point p with normal m, v = p - centre (or p - q):
 *   sphere d2 = (vx vx + vy vy) + vz vz, g = (mx vx + my vy) + mz vz; cylinder t = (vx ax + vy ay) + vz az,
 *   d2 = ((vx vx + vy vy) + vz vz) - t t, g = ((mx vx + my vy) + mz vz) - t ((mx ax + my ay) + mz az).  Inlier iff
 *   d2 < hi2 && d2 > lo2 and, unless min_normal_cos == 0, g g >= c2 d2.  A NaN is not an inlier.
 * Best, found (count >= max(min_inliers, 2)), peeling, labels, sizes, ids and their padding: pcgx_kdtree_planes'.  Every
 *   row of every output is written on every call.
 * Refinement (refine != 0, the round found a shape): I = the best's inliers in ascending id, the pivot the record's own
 *   centre (sphere) or q (cylinder) widened to float64.  x = p - pivot in three dimensions (sphere), or
 *   x = ((p - pivot).e1, (p - pivot).e2) in two (cylinder: the record's axis a is kept; e1 = the unit vector of a x the
 *   coordinate axis of a's smallest |component|, the first on a tie; e2 = a x e1).  |x|^2 - 2 x.u - k is fitted to zero by
 *   linear least squares (Kasa) in float64: unknowns (u, k), rows (2 x, 1), so the normal matrix is
 *   [[4 sum x x^T, 2 sum x], [2 sum x^T, n]] and the right side (2 sum |x|^2 x, sum |x|^2), solved by Cholesky in that
 *   order of unknowns.  The sums are added in a fixed order with no float atomic: the same bits on every call and under
 *   every split.  No refit when a pivot of the factorisation is not > 1e-12 times the largest diagonal entry, k + |u|^2 is
 *   not > 0, the new radius r = sqrt(k + |u|^2) fails the radius test, or a number of the new record is not finite.  The
 *   new centre is the pivot plus u (plus u1 e1 + u2 e2, q made canonical again).  The points of A_r are counted again
 *   under the refitted record; it replaces the hypothesis's iff its count >= the best's count.  One refit, not an
 *   iteration; the cylinder's axis is not refitted.
 * PCGX_E_INVALID (nothing is written): pcgx_kdtree_planes' list (min_normal_cos always checked), and kind not 0 or 1,
 *   NULL normals with Len() > 0, sample_radius negative or not finite, r_min or r_max NaN or negative, r_min > r_max
 *   (r_max may be +inf).  n_hyp == 0 or Len() == 0 is PCGX_OK with n_shapes = 0.
 * Always computed on the device (csrc/shapes.hip).  The points are split into chunks to fill the chip (the library's
 *   choice; PCGX_SHAPES_SPLIT=<n> in the environment, read per call, forces it -- any n gives the same bits). */
#define PCGX_SHAPE_SPHERE 0
#define PCGX_SHAPE_CYLINDER 1
PCGX_API pcgx_status pcgx_kdtree_shapes(const pcgx_kdtree *t, int32_t kind,
                                        const uint32_t *samples /* [2 n_hyp max_shapes] */, int64_t n_hyp,
                                        int32_t max_shapes, float max_dist, int64_t min_inliers, float sample_radius,
                                        float r_min, float r_max, const float *axis /* [3] or NULL */, float min_axis_cos,
                                        const float *normals /* [3 Len()] */, float min_normal_cos, int32_t refine,
                                        int64_t *n_shapes, float *shapes, int64_t *sizes, int32_t *refined, int64_t *best,
                                        int64_t *labels, int64_t *ids /* may be NULL */, int32_t *status /* may be NULL */,
                                        int64_t *counts /* may be NULL */, float *hyp_shapes /* may be NULL */);
/* Same, every array device resident (`axis` alone stays three floats in HOST memory), enqueued on `stream` (NULL: the
 * library's); returns without waiting and reads nothing back.  Ids, sizes, labels, counts and best are int32, d_n_shapes
 * is one int32.  d_ids, d_sizes and d_n_shapes can be passed on to pcgx_kdtree_group_stats_dev and
 * pcgx_kdtree_group_hulls_dev as they are (cap_ids = Len(), cap_groups = max_shapes).  A handle with deleted points has
 * its deleted flags copied to the device first, and that copy alone is waited for. */
PCGX_API pcgx_status pcgx_kdtree_shapes_dev(const pcgx_kdtree *t, int32_t kind, const uint32_t *d_samples, int64_t n_hyp,
                                            int32_t max_shapes, float max_dist, int64_t min_inliers, float sample_radius,
                                            float r_min, float r_max, const float *axis /* HOST [3] or NULL */,
                                            float min_axis_cos, const float *d_normals, float min_normal_cos,
                                            int32_t refine, int32_t *d_n_shapes, float *d_shapes, int32_t *d_sizes,
                                            int32_t *d_refined, int32_t *d_best, int32_t *d_labels,
                                            int32_t *d_ids /* may be NULL */, int32_t *d_status /* may be NULL */,
                                            int32_t *d_counts /* may be NULL */, float *d_hyp_shapes /* may be NULL */,
                                            void *stream);
/* Hypotheses per workgroup of the count kernel (a wave, two hypotheses per lane). */
PCGX_API int32_t pcgx_shapes_tile(void);

/* ------------------------------------------- ground (extension: no reference parity)
 * NOT in the reference.  Ground segmentation for terrain that no plane holds: the grid form of the progressive
 * morphological filter (Zhang et al. 2003; PCL's ApproximateProgressiveMorphologicalFilter).  The minimum surface of the
 * points over the caller's grid is opened with squares that grow by the caller's schedule; a point is ground while it
 * stays within the schedule's height of every opened surface.  The up axis is z.  The caller gives the grid (as
 * StorageVoxelGrid's resolution, size and origin) and the window schedule (as it gives the random words elsewhere): this
 * contract holds no floating-point formula for either.  Every step is a min, a max or one float32 subtraction, so the
 * result is a property of the point set.  This comment is the contract, tests/ground_oracle.py restates it.
 *   pcgx_kdtree_ground    (t, origin[2] f32, dims[2] i32 (nx, ny), cell, n_win, half[n_win] i32, height[n_win] f32,
 *                          labels[Len()] i64, sizes[2] i64, ids[Len()] i64, n_groups*, window[Len()] i32 | NULL,
 *                          surface[nx ny] f32 | NULL, hag[Len()] f32 | NULL)
 *   pcgx_kdtree_ground_dev(... origin, dims, half and height stay in HOST memory; labels, sizes, ids int32, d_n_groups
 *                          one int32, every output device resident, stream)
 * Cell of a point, all float32, each operation rounded once: fx = floorf((x - ox) / cell), fy = floorf((y - oy) / cell).
 * Live point: not deleted (pcgx_kdtree_delete_point[s]), x, y and z finite, 0 <= fx < nx and 0 <= fy < ny compared as
 *   floats before any conversion; then c = (int)fy * nx + (int)fx.  A point that is not live has label -1 and takes no part.
 * Minimum surface: S_0[c] = the smallest z of the live points of cell c, by the order-preserving key of group geometry's
 *   min / max combines, so -0.0 lies below +0.0.  A cell without a live point is EMPTY.
 * Window k = 0 .. n_win - 1, h = half[k]; the window of cell (i, j) is the in-grid cells with |di| <= h and |dj| <= h:
 *   E[c] = the key-minimum of S_k over the non-empty cells of c's window, empty if there are none;
 *   S_{k+1}[c] = the key-maximum of E over the non-empty cells of c's window, empty if there are none
 *   (a grey opening with a (2 h + 1)^2 square; the next window opens the opened surface; empty cells take no part in
 *   either half).
 * Ground test: a live point survives window k iff z - S_{k+1}[c] < height[k] (float32, one subtraction, strict).  It is
 *   GROUND iff it survives every window; window[i] = the first k it fails, -1 for ground points and points that are not
 *   live.  The surfaces depend on S_0 alone, not on which points have failed so far.
 * Outputs, every row written on every call: labels[i] 0 ground, 1 not ground, -1 not live; sizes[2] their counts; ids:
 *   the ground ascending, then the rest ascending, then -1 in the remaining slots; n_groups = 2 (a grouped list for
 *   pcgx_kdtree_group_stats[_dev] and pcgx_kdtree_group_hulls[_dev]); surface = S_{n_win}, +inf at an empty cell (the
 *   terrain model); hag[i] = z - S_{n_win}[c], bits 0x7fc00000 where the point is not live (the height above ground).
 * PCGX_E_INVALID (nothing is written): a NULL tree, origin or dims; cell not finite or not > 0; an origin that is not
 *   finite; nx or ny outside [1, 8192]; n_win outside [0, 64]; a half[k] outside [1, 8192]; a height[k] not finite or
 *   not > 0; NULL half or height with n_win > 0; a NULL mandatory output (labels and ids only where Len() > 0).
 *   n_win == 0 is PCGX_OK: every live point is ground and surface = S_0.  Len() == 0 is PCGX_OK with sizes 0, 0.
 * Always computed on the device (csrc/ground.hip).  The same input gives the same bits on every call: no float atomic
 *   anywhere, the minimum surface is an unsigned atomicMin over keys. */
PCGX_API pcgx_status pcgx_kdtree_ground(const pcgx_kdtree *t, const float *origin /* [2] */, const int32_t *dims /* [2] */,
                                        float cell, int32_t n_win, const int32_t *half, const float *height,
                                        int64_t *labels, int64_t *sizes /* [2] */, int64_t *ids, int64_t *n_groups,
                                        int32_t *window /* may be NULL */, float *surface /* may be NULL */,
                                        float *hag /* may be NULL */);
/* Same, every output device resident (origin, dims, half and height stay in HOST memory: they are arguments, checked
 * before anything is enqueued), enqueued on `stream` (NULL: the library's); returns without waiting and reads nothing
 * back: every window is enqueued at once.  d_ids, d_sizes and d_n_groups can be passed on to pcgx_kdtree_group_stats_dev
 * and pcgx_kdtree_group_hulls_dev as they are (cap_ids = Len(), cap_groups = 2).  A handle with deleted points has its
 * deleted flags copied to the device first, and that copy alone is waited for. */
PCGX_API pcgx_status pcgx_kdtree_ground_dev(const pcgx_kdtree *t, const float *origin /* HOST [2] */,
                                            const int32_t *dims /* HOST [2] */, float cell, int32_t n_win,
                                            const int32_t *half /* HOST */, const float *height /* HOST */,
                                            int32_t *d_labels, int32_t *d_sizes, int32_t *d_ids, int32_t *d_n_groups,
                                            int32_t *d_window /* may be NULL */, float *d_surface /* may be NULL */,
                                            float *d_hag /* may be NULL */, void *stream);
/* Cells of a grid row that one pass of the morphology kernel's workgroup handles at once, and the largest half-width
 * that takes its plain loop (above it: doubling in LDS): the boundaries the tests put nx, ny and half across. */
PCGX_API int32_t pcgx_ground_tile(void);
PCGX_API int32_t pcgx_ground_loop_max(void);

/* ------------------------------------------- boundary points (extension: no reference parity)
 * NOT in the reference.  A scan is a surface with edges: the rim where the sensor's view ends, shadows, holes.  A point
 * sits on such an edge when its neighbours, seen in its tangent plane, leave a wide angular gap -- PCL's
 * BoundaryEstimation, Open3D's compute_boundary_points.  Over the tree's own points only (the q == NULL convention of
 * _fpfh and _local_maxima), every array in id order, deleted ids included.  This comment is the contract,
 * tests/boundary_oracle.py restates it.
 * Arguments: normals[3 Len()] in id order (what pcgx_kdtree_normals(q == NULL) writes), min_gap in sectors (1..64),
 *   min_neighbors.
 * Neighbourhood: N(i) = exactly the set pcgx_kdtree_range_count counts on that handle (float32 DistSq < radius^2, the
 *   bound strict; grid, forced walk, after DeletePoint).  A deleted point is nobody's neighbour.  count = |N(i)|, a tree
 *   point counting itself.
 * Evaluated: point i is evaluated iff i is in N(i) (so a deleted id or a NaN coordinate never is), and its normal's
 *   three components are finite and not all zero, and count >= max(min_neighbors, 1).  Otherwise mask = 0, gap = -1 and
 *   the point is no boundary point.  counts[i] is |N(i)| where i is in N(i) and the normal is usable (so also where only
 *   min_neighbors failed), else 0: nothing is enumerated for a normal that gives no frame.
 * Frame, float64 from the float32 normal n widened, not normalised, no square root anywhere: e = the unit vector of the
 *   axis where |n| is smallest (a tie: the lowest axis); u = n x e; v = n x u; each component a difference of two
 *   products in the cross product's written order.  Normals are expected to be of unit length, which is what the library
 *   writes: a normal of length L stretches v by L beside u and skews the sectors accordingly.
 * Direction of a neighbour p seen from q = point i, all float64, fixed order, nothing fused: d = p - q;
 *   a = (d.x u.x + d.y u.y) + d.z u.z; b likewise with v.  Both are finite, the members of N(i) being finite.
 *   a == 0 and b == 0: the neighbour has no sector and sets no bit (the point itself, a coincident point, a point on the
 *   normal's line).
 * Sector, 64 of 5.625 degrees, each owning its lower border: the quarter turn Q and the rotated (x, y), x > 0, y >= 0:
 *   Q0: a > 0, b >= 0 -> (a, b);  Q1: a <= 0, b > 0 -> (b, -a);  Q2: a < 0, b <= 0 -> (-a, -b);  Q3: a >= 0, b < 0 ->
 *   (-b, a).  s = #{k in 1..15 : y >= x T[k]}, each product rounded once, T[k] the float64 nearest tan(k pi / 32), T[8]
 *   = 1 exactly (csrc/boundary_terms.h writes them out).  sector = 16 Q + s.
 * Mask and gap: mask = OR of 1 << sector over N(i).  gap = the longest cyclic run of zero bits of mask: 0..63 for a
 *   non-zero mask, 64 for an evaluated point whose mask is 0.  Point i is a boundary point iff it is evaluated and
 *   gap >= min_gap.
 * What the gap means: for a true angular opening g between neighbouring directions and w = 5.625 degrees,
 *   g / w - 2 < gap < g / w.  So a point flagged at min_gap has an opening wider than min_gap w, and every opening of at
 *   least (min_gap + 2) w is flagged: with min_gap = 16 (PCL's pi / 2) nothing below 90 degrees and everything from
 *   101.25 degrees.  Not PCL's or Open3D's bits: they sort angles from atan2 and compare with a float threshold.
 * Outputs: ids[Len()] holds the boundary points in ascending id, then -1 in every remaining slot
 *   (pcgx_kdtree_local_maxima's convention), *n_ids their number; gaps[Len()] int32, masks[Len()] uint64 and
 *   counts[Len()] int32 may each be NULL.
 * PCGX_E_INVALID: a NULL tree; a radius that is not finite and > 0; min_gap outside 1..64; NULL normals, ids or n_ids
 *   with Len() > 0.  Len() == 0 is PCGX_OK and writes only *n_ids = 0.  The same input gives the same bits on every call
 *   (OR and integer + over the set: the visit's order does not enter).  Always computed on the device
 *   (csrc/boundary.hip): pcgx_kdtree_normals' enumeration once.  Temporaries: Len() bytes of flags and
 *   4 ceil(Len() / 2048) bytes of tile counts. */
PCGX_API pcgx_status pcgx_kdtree_boundary(const pcgx_kdtree *t, float radius, const float *normals /* [3 Len()] */,
                                          int32_t min_gap, int32_t min_neighbors, int64_t *ids /* [Len()] */,
                                          int64_t *n_ids, int32_t *gaps /* [Len()], may be NULL */,
                                          uint64_t *masks /* [Len()], may be NULL */,
                                          int32_t *counts /* [Len()], may be NULL */);
/* Same, every array device resident (ids and the count are int32 there), enqueued on `stream` (NULL: the library's);
 * returns without waiting.  d_normals can be what pcgx_kdtree_normals_dev wrote on the same stream. */
PCGX_API pcgx_status pcgx_kdtree_boundary_dev(const pcgx_kdtree *t, float radius, const float *d_normals, int32_t min_gap,
                                              int32_t min_neighbors, int32_t *d_ids /* [Len()] */, int32_t *d_n_ids,
                                              int32_t *d_gaps, uint64_t *d_masks, int32_t *d_counts, void *stream);

/* ------------------------------------------- ray queries (extension: no reference parity)
 * NOT in the reference.  Every other query is about a point and its surroundings; these are about a line: which map
 * points later beams passed through (free-space carving), which points are seen from a viewpoint, the point under a
 * cursor, a range image of a map.  One primitive: for a batch of rays, the tree's points inside a thin tube around
 * each, and of that set the first point along the ray or a count of how often each point was pierced.  This comment is
 * the contract, tests/rays_oracle.py restates it.
 * A ray: an origin o, a direction d (NOT normalised: any finite non-zero vector) and a parameter range [s_min, s_max];
 *   its point at s is o + s d.  For a beam that ended at e: d = e - o and s_max = 1 - margin.  origins and directions are
 *   [3 nr] float32, s_min and s_max [nr] float32; s_min == NULL means 0, s_max == NULL means +inf.
 * Member: all float64 from the float32 inputs widened, fixed order, each product rounded once, nothing fused, no square
 *   root and no division.  For a live tree point p with three finite coordinates: w = p - o;
 *   a = (w.x d.x + w.y d.y) + w.z d.z;  dd = (d.x d.x + d.y d.y) + d.z d.z;  c = w x d = (w.y d.z - w.z d.y,
 *   w.z d.x - w.x d.z, w.x d.y - w.y d.x);  cc = (c.x c.x + c.y c.y) + c.z c.z;  rr = radius radius.
 *   p is a member iff cc <= rr dd and s_min dd <= a <= s_max dd: the tube's surface and both ends belong to it.
 *   A deleted point is no ray's member.  A ray has no members if o or d has a non-finite component, if dd == 0, if s_min
 *   or s_max is NaN, or if s_min > s_max.  A negative s_min is allowed, and so are -inf and +inf.
 * First hit (pcgx_kdtree_raycast): per ray the member with the smallest a, a tie going to the smallest id.  ids[nr]
 *   (-1: none), along[nr] = a, off_sq[nr] = cc, both float64, written as 0 for a miss, each may be NULL.  The caller
 *   derives s = a / dd and the metric offset sqrt(cc / dd).
 * Pierced counts (pcgx_kdtree_ray_pierce): counts[Len()] in id order; every (ray, member) pair adds 1 to counts[id].
 *   The host form returns this call's counts; the _dev form ADDS into the caller's int32 array, so successive scans
 *   accumulate on one stream with nothing read back.
 * A minimum under a total order and an integer sum over a set: the same bits on every call, on every kind of handle
 *   (grid, PCGX_RANGE_WALK=1, after DeletePoint) and however the work is split.
 * PCGX_E_INVALID: a NULL tree; a radius that is not finite and > 0; nr < 0 (or above 2^31 - 16); NULL origins,
 *   directions or ids / counts with nr > 0 (counts: and Len() > 0); a tree whose finite points span 2^62 or more along
 *   an axis (float32 squared distances overflow there: csrc/ray_terms.h).  nr == 0 or Len() == 0 is PCGX_OK; with an
 *   empty tree every ray is a miss.
 * Always computed on the device (csrc/rays.hip): a wave per ray; the ray's range, clipped to the box of the tree's
 *   finite points, is cut into slabs of about 2 radius (no shorter than a grid cell, at most 4096 per ray: longer slabs
 *   beyond, never a shorter ray), each one ball query of pcgx_kdtree_range_count's enumeration whose candidates the
 *   float64 member test filters.  csrc/ray_terms.h proves the balls cover the members.  No temporaries.  A tree with a
 *   NaN or infinite coordinate among its points has no such enumeration to rely on (the reference's build has no
 *   consistent order for a NaN): there a wave tests its ray against every point, from a copy of the handle's points
 *   uploaded in the call (12 Len() bytes, Len() more after DeletePoint). */
PCGX_API pcgx_status pcgx_kdtree_raycast(const pcgx_kdtree *t, const float *origins /* [3 nr] */,
                                         const float *directions /* [3 nr] */, const float *s_min /* [nr] or NULL */,
                                         const float *s_max /* [nr] or NULL */, int64_t nr, float radius,
                                         int64_t *ids /* [nr] */, double *along /* [nr], may be NULL */,
                                         double *off_sq /* [nr], may be NULL */);
/* Same, every array device resident (ids are int32 there), enqueued on `stream` (NULL: the library's); returns without
 * waiting. */
PCGX_API pcgx_status pcgx_kdtree_raycast_dev(const pcgx_kdtree *t, const float *d_origins, const float *d_directions,
                                             const float *d_s_min, const float *d_s_max, int64_t nr, float radius,
                                             int32_t *d_ids, double *d_along, double *d_off_sq, void *stream);
PCGX_API pcgx_status pcgx_kdtree_ray_pierce(const pcgx_kdtree *t, const float *origins /* [3 nr] */,
                                            const float *directions /* [3 nr] */, const float *s_min /* [nr] or NULL */,
                                            const float *s_max /* [nr] or NULL */, int64_t nr, float radius,
                                            int32_t *counts /* [Len()] */);
/* Same on the device, ADDING into d_counts int32 [Len()] (the caller zeroes it before the first scan). */
PCGX_API pcgx_status pcgx_kdtree_ray_pierce_dev(const pcgx_kdtree *t, const float *d_origins, const float *d_directions,
                                                const float *d_s_min, const float *d_s_max, int64_t nr, float radius,
                                                int32_t *d_counts, void *stream);

/* ------------------------------------------- cylinder statistics (extension: no reference parity)
 * NOT in the reference.  What moved between two registered epochs, and by how much: M3C2 (Lague, Brodu and Leroux
 * 2013) takes, for a core point with a normal, the points of each epoch inside a cylinder along the normal and compares
 * their mean positions along it.  The primitive: for a batch of cylinders over one tree, how many of the tree's points
 * lie in each and the sums of their positions along the axis and of the squares.  This comment is the contract,
 * tests/m3c2_oracle.py restates it.
 * A cylinder: a core o, an axis d (NOT normalised: any finite non-zero vector), a radius and a half length L, the last
 *   two the same for the whole batch.  cores and axes are [3 m] float32.
 * Member: all float64 from the float32 inputs widened, fixed order, each product rounded once, nothing fused, no square
 *   root and no division.  w, a, dd, cc and rr are the ray queries' expressions above, with o the core and d the axis;
 *   ll = half_length half_length.  A live tree point p with three finite coordinates is a member iff cc <= rr dd and
 *   a a <= ll dd: the side surface and both end caps belong to the cylinder, and its metric size does not depend on |d|.
 *   A deleted point is in no cylinder.  A cylinder is unusable, and has no members, if o or d has a non-finite component
 *   or dd == 0.
 * counts[m] int32: the number of members.  A property of the point set: the same on every kind of handle (grid,
 *   PCGX_RANGE_WALK=1, after DeletePoint) and on every call.
 * sums[2 m] float64: sums[2 i] = S1 = the sum of a over cylinder i's members, sums[2 i + 1] = S2 = the sum of a a.
 *   Every term has its contract bits.  The order of the additions is the library's: the same handle, arguments and
 *   build give the same bits on every call (lanes in the order of the visit, shuffles in a fixed tree, no floating-point
 *   atomics); across handles, or against the exact sum, a value differs by at most n 2^-53 times the sum of the terms'
 *   magnitudes, n the count -- the bound of any summation order while n n < 2^53, derived, not measured.
 *   The sums are UNNORMALISED: the caller derives the metric mean S1 / n / sqrt(dd) and the metric variance, the sample
 *   variance of a over dd (pcgx_m3c2_finish does both).  An unusable cylinder writes 0, 0, 0.
 * PCGX_E_INVALID: a NULL tree; a radius or half_length that is not finite and > 0; m < 0 (or above 2^31 - 16); a NULL
 *   array with m > 0; a tree whose finite points span 2^62 or more along an axis (csrc/ray_terms.h).  m == 0 is
 *   PCGX_OK.  A tree with no live point gives zeros.
 * Always computed on the device (csrc/m3c2.hip), in one launch: the enumeration of the ray queries -- the axis' range
 *   [-L, L], clipped to the box of the tree's finite points, cut into slabs of about 2 radius (no shorter than a grid
 *   cell), each one ball query whose candidates the float64 member test filters (csrc/m3c2_terms.h hands
 *   csrc/ray_terms.h a range that holds every member, so its cover proof applies) -- with 8, 16 or 64 lanes per
 *   cylinder, the fewest that hold the slabs 2 L / max(2 radius, cell) can make.  No temporaries.  A tree with a NaN or
 *   infinite coordinate among its points is answered by a wave per cylinder over all points, from a copy of the
 *   handle's points uploaded in the call (12 Len() bytes, Len() more after DeletePoint). */
PCGX_API pcgx_status pcgx_kdtree_cylinder_stats(const pcgx_kdtree *t, const float *cores /* [3 m] */,
                                                const float *axes /* [3 m] */, int64_t m, float radius,
                                                float half_length, int32_t *counts /* [m] */, double *sums /* [2 m] */);
/* Same, every array device resident, enqueued on `stream` (NULL: the library's); returns without waiting, reads
 * nothing back. */
PCGX_API pcgx_status pcgx_kdtree_cylinder_stats_dev(const pcgx_kdtree *t, const float *d_cores, const float *d_axes,
                                                    int64_t m, float radius, float half_length, int32_t *d_counts,
                                                    double *d_sums, void *stream);

/* ------------------------------------------- M3C2 (extension: no reference parity)
 * NOT in the reference.  The finish of M3C2 on the cylinder statistics of two epochs (the same cores, axes, radius and
 * half length against the tree of each): per core the signed distance along the normal, the level of detection at 95 %
 * and whether the change is significant.  tests/m3c2_oracle.py restates it.
 * All float64 in the written order, division and square root IEEE (so the device's values equal a NumPy restatement's
 *   bit for bit, given the sums): dd from the axis as above; for epoch c, n = counts_c[i], S1 = sums_c[2 i],
 *   S2 = sums_c[2 i + 1]:  mean_c = S1 / n;  v = (S2 - (S1 S1) / n) / (n - 1);  var_c = (v > 0 ? v : 0) / dd.
 *   distance = (mean_2 - mean_1) / sqrt(dd);  lod = 1.96 (sqrt(var_1 / n_1 + var_2 / n_2) + registration_error);
 *   significant = |distance| > lod.
 * A core with counts_1 < min_count or counts_2 < min_count, or with an unusable axis (a non-finite component, dd == 0),
 *   gets distance = lod = NaN and significant = 0.
 * PCGX_E_INVALID: m < 0 (or above 2^31 - 1); registration_error not >= 0; min_count < 2; a NULL array with m > 0.
 *   m == 0 is PCGX_OK.  Left out: median / IQR statistics, multi-scale normals, a radius per core, the members' ids. */
PCGX_API pcgx_status pcgx_m3c2_finish(const float *axes /* [3 m] */, const int32_t *counts1 /* [m] */,
                                      const double *sums1 /* [2 m] */, const int32_t *counts2 /* [m] */,
                                      const double *sums2 /* [2 m] */, int64_t m, double registration_error,
                                      int32_t min_count, double *distance /* [m] */, double *lod /* [m] */,
                                      uint8_t *significant /* [m] */);
/* Same, every array device resident, enqueued on `stream` (NULL: the library's); returns without waiting.  The inputs
 * can be what two pcgx_kdtree_cylinder_stats_dev calls wrote on the same stream. */
PCGX_API pcgx_status pcgx_m3c2_finish_dev(const float *d_axes, const int32_t *d_counts1, const double *d_sums1,
                                          const int32_t *d_counts2, const double *d_sums2, int64_t m,
                                          double registration_error, int32_t min_count, double *d_distance,
                                          double *d_lod, uint8_t *d_significant, void *stream);

/* ------------------------------------------- score poses (extension: no reference parity)
 * NOT in the reference.  pcgx_pose_from_correspondences picks its pose by the inliers among the CORRESPONDENCES; on a
 * scene with repeated structure a wrong pose can collect more of them than the right one.  This call counts, for each of
 * K poses, how many points of the WHOLE source cloud land within max_dist of the tree's cloud ("fitness"), and sums
 * their squared distances ("inlier RMSE" = sqrt(sum / count)), in one call, with nothing written per pair.  This comment
 * is the contract, tests/score_oracle.py restates it.
 * Dead pose: a pose whose 16 numbers all compare equal to 0 (what a rejected hypothesis has, what pcgx_pose_select pads
 *   with).  Its count is 0, its sum is 0, it is never the best.  Every other pose is live (one with a NaN too).
 * Pair rule: for a live pose k and point i, x' = pcgx_mat4_transform(pose_k, p_i): float32, nothing fused, the division
 *   by w included.  The pair is found iff x' is finite in all three coordinates and
 *   pcgx_kdtree_nearest_batch(t, x', 1, max_dist, 0, ...) returns an id >= 0 -- on every handle that call accepts
 *   (after DeletePoint, PCGX_GRID=0 / 2, every point deleted), its rule at DistSq == max_dist^2 included; its DistSq is
 *   the one that call returns (which of several tied points it names does not matter).
 * counts[k]: the number of found pairs; exact, the same on every call.
 * sum_dist_sq[k]: the float64 sum of the found pairs' float32 DistSq.  The order is the library's: two conforming
 *   values differ by summation rounding only.  This implementation adds in a fixed order (lanes by a fixed tree, the
 *   waves of a workgroup, then the workgroups' partials in tile order; no floating-point atomics): the same handle,
 *   points, poses and chunk give the same bits on every call.
 * best: the live pose with the largest count, the smallest k among equals; -1 when no pose is live.  pose16: its 16
 *   numbers as given, or all zero.
 * Errors (PCGX_E_INVALID): a NULL array with a positive count, NULL scalar outputs, negative counts, n or K above
 *   2^31 - 1, max_dist not finite or not > 0.  K == 0 and n == 0 are PCGX_OK (counts 0; best the first live pose).
 * Temporaries (the library's arena): 36 n bytes for the source in Morton order over its own box, and per round of
 *   `chunk` poses 24 chunk n bytes for the pairs the grid cannot certify (ties, DistSq == max_dist^2, sparse regions) --
 *   sized for the worst case, a tree of coincident points, where that is every pair -- plus 48 bytes per workgroup.
 *   chunk = max(1, min(K, 65535, 2^22 / n)): at most max(96 MiB, 24 n bytes).  PCGX_SCORE_CHUNK=<poses> in the
 *   environment, read per call, forces the chunk (held to what an int32 slot index allows); counts do not depend on it.
 *   Handles with deletions or without a grid take one pose at a time through the handle's own search: 20 n bytes. */
PCGX_API pcgx_status pcgx_kdtree_score_poses(const pcgx_kdtree *t, const float *src_xyz /* [3 n] */, int64_t n,
                                             const float *poses /* [16 K], column-major */, int64_t K, float max_dist,
                                             int64_t *counts /* [K] */, double *sum_dist_sq /* [K], may be NULL */,
                                             int64_t *best, float pose16[16]);
/* Same, every array device resident, enqueued on `stream` (NULL: the library's); returns without waiting, reads nothing
 * back.  Counts are int32.  The scalar outputs go to d_result, PCGX_SCORE_RESULT_WORDS 4-byte words: int32 best,
 * best_count, the number of live poses, n; the best's sum as one float64 in words 4..5 (0 without a best); words 6..7
 * zero; the float32 pose in words 8..23.  Every word is written on every call, K == 0 and n == 0 included. */
#define PCGX_SCORE_RESULT_WORDS 24
PCGX_API pcgx_status pcgx_kdtree_score_poses_dev(const pcgx_kdtree *t, const float *d_src_xyz, int64_t n,
                                                 const float *d_poses, int64_t K, float max_dist,
                                                 int32_t *d_counts /* [K], may be NULL */,
                                                 double *d_sums /* [K], may be NULL */, void *d_result, void *stream);
/* Source points per workgroup of the scoring kernels: the boundary the tests put n across. */
PCGX_API int32_t pcgx_score_tile(void);

/* The hypotheses of a pcgx_pose_from_correspondences call worth scoring: among those with status 0 and count >= 3, by
 * count descending, then by h ascending.  Slot j < K gets the j-th: ids[j] = h and its 16 pose numbers; the slots behind
 * the last such hypothesis get id -1 and an all-zero (dead) pose.  *n_selected = min(K, the number of such hypotheses).
 * Every slot of [0, K) is written on every call.  PCGX_E_INVALID: negative counts, n_hyp or K above 2^31 - 1, a NULL
 * input with n_hyp > 0, a NULL output with K > 0, NULL n_selected.  The host form is plain host code. */
PCGX_API pcgx_status pcgx_pose_select(const int32_t *status /* [n_hyp] */, const int64_t *counts /* [n_hyp] */,
                                      const float *poses /* [16 n_hyp] */, int64_t n_hyp, int64_t K,
                                      int64_t *ids /* [K] */, float *out_poses /* [16 K] */, int64_t *n_selected);
/* Same on the device: int32 status and counts, exactly what pcgx_pose_from_correspondences_dev writes; int32 ids;
 * n_selected is a device word.  Enqueued on `stream`, nothing read back. */
PCGX_API pcgx_status pcgx_pose_select_dev(const int32_t *d_status, const int32_t *d_counts, const float *d_poses,
                                          int64_t n_hyp, int64_t K, int32_t *d_ids, float *d_out_poses,
                                          int32_t *d_n_selected, void *stream);

/* ------------------------------------------- k nearest neighbours (extension: no reference parity)
 * NOT in the reference: pcgol's KD-tree answers Nearest (k = 1) and Range (a fixed radius).  For each query i: the k
 * points p of the tree with the smallest (DistSq(p, q[i]), id) in lexicographic order, among those with
 * DistSq < max_range^2 (Range's rule, kdtree.go:166,178; DistSq is the reference's float32 expression
 * (dx*dx + dy*dy) + dz*dz).  Ascending in that order.  counts[i] = how many were found (<= k).  Slots past counts[i]
 * are {-1, max_range^2}, Nearest's not-found value.
 * q == NULL: the queries are the tree's own points in id order (nq must equal Len()); each point finds itself at
 * DistSq 0.  Deleted points are never neighbours.  A deleted point's own row is still computed when q == NULL.
 * 1 <= k <= 64.  max_range >= 0 or +inf.  Anything else (NaN max_range, NULL ids / dist_sq with nq > 0) is
 * PCGX_E_INVALID.  Non-finite queries find nothing.
 * Ties are broken by id, not by visit order, so the result is a function of the cloud alone, whichever way the
 * device enumerates (grid, tree walk, patched tree after DeletePoint).  Consequences:
 *   - the result equals the prefix Range(q, max_range)[:k] whenever no two of Range's first k+1 entries have equal
 *     DistSq; on a tie it can differ, because Range orders ties by the walk's discovery order;
 *   - k = 1 equals Nearest except on ties and at DistSq == max_range^2 (Nearest's leaf rule admits that one).
 * Always computed on the device.  The cost is that of the cells (or tree nodes) the k-th distance covers; a heap of
 * coincident points is scanned by a whole wave for every query that reaches it. */
PCGX_API pcgx_status pcgx_kdtree_knearest(const pcgx_kdtree *t, const float *q, int64_t nq, int32_t k,
                                          float max_range, int64_t *ids /* [nq*k] */,
                                          float *dist_sq /* [nq*k] */, int32_t *counts /* [nq], may be NULL */);
/* Same, every array device resident (ids int32), enqueued on `stream` (NULL: the library's); returns without
 * waiting. */
PCGX_API pcgx_status pcgx_kdtree_knearest_dev(const pcgx_kdtree *t, const float *d_q, int64_t nq, int32_t k,
                                              float max_range, int32_t *d_ids, float *d_dist_sq,
                                              int32_t *d_counts, void *stream);

/* ------------------------------------------- k-NN covariances (extension: no reference parity)
 * NOT in the reference.  The per-point covariances Generalized ICP (Segal, Haehnel, Thrun 2009) takes, from k nearest
 * neighbourhoods, which adapt to the point density by themselves.  For each query i:
 *   N(q)  = exactly the list pcgx_kdtree_knearest(t, q, k, max_range) returns: the same sources (grid, forced walk,
 *           patched tree after DeletePoint), the same (DistSq, id) order, the same count; a tree point is its own
 *           neighbour.  n = |N(q)|.
 *   C     = sum d d^T / n - m m^T with d = p - q and m = sum d / n, in float64, summed in N(q)'s order
 *           (pcgx_kdtree_normals' moments and formula).
 *   PCGX_COV_RAW:   C as it is.
 *   PCGX_COV_PLANE: I - (1 - epsilon) u u^T = V diag(epsilon, 1, 1) V^T, u the unit eigenvector of C's smallest
 *                   eigenvalue (pcgx_kdtree_normals' Jacobi solve): Segal's regularisation, fast_gicp's PLANE.
 *   Degenerate: n < 3, or all of N(q) at one place (the normals' exact box test): I for PLANE, 0 for RAW.
 *   Cancelled trace: when the float64 trace of C rounds to <= 0 (only where the neighbours' spread is below ~1e-8 of
 *   their distance from the query: each entry of C is within (2 n + 4) 2^-53 sum |d|^2 / n of the exact one) nothing
 *   can be solved: PLANE is I and the normal 0 as if degenerate, RAW is C as computed (then not positive definite).
 *   cov6[6i .. 6i+5] = xx, xy, xz, yy, yz, zz in float32.
 *   normals (may be NULL): u turned towards the viewpoint (NULL: the origin) as pcgx_kdtree_normals turns it; 0 where
 *   degenerate.  counts (may be NULL): n.
 * q == NULL: the queries are the tree's own points (nq must equal Len()), the output in id order -- one covariance per
 * base id, deleted ids included.  PCGX_E_INVALID: k outside [1, 64], epsilon outside (0, 1], an unknown mode, a NaN or
 * negative max_range, q == NULL with nq != Len(), cov6 == NULL with nq > 0.  Always computed on the device; the cost is
 * pcgx_kdtree_knearest's plus k reads by id per query and the 3 x 3 solve, which PCGX_COV_RAW skips when normals is
 * NULL.  On a handle without deletions the first call builds an id -> node map once and waits for it. */
enum { PCGX_COV_RAW = 0, PCGX_COV_PLANE = 1 };
PCGX_API pcgx_status pcgx_kdtree_covariances(const pcgx_kdtree *t, const float *q, int64_t nq, int32_t k,
                                             float max_range, int32_t mode, float epsilon, const float viewpoint[3],
                                             float *cov6 /* [6nq] */, float *normals /* [3nq], may be NULL */,
                                             int32_t *counts /* [nq], may be NULL */);
/* Same, every array device resident, enqueued on `stream` (NULL: the library's); returns without waiting. */
PCGX_API pcgx_status pcgx_kdtree_covariances_dev(const pcgx_kdtree *t, const float *d_q, int64_t nq, int32_t k,
                                                 float max_range, int32_t mode, float epsilon,
                                                 const float viewpoint[3], float *d_cov6, float *d_normals,
                                                 int32_t *d_counts, void *stream);

/* ------------------------------------------- Generalized ICP (extension: no reference parity)
 * NOT in the reference: pcgol has nothing like it.  Generalized ICP (Segal, Haehnel, Thrun 2009; fast_gicp, PCL's
 * GeneralizedIterativeClosestPoint) as a third kind of session and Fit beside point-to-point and point-to-plane: the
 * consumer of pcgx_kdtree_covariances.  Tests check against a NumPy float64 restatement (tests/gicp_oracle.py).
 * Inputs: a base tree; base_cov6[6 * Len()], float32 xx, xy, xz, yy, yz, zz per base id in id order -- exactly what
 * pcgx_kdtree_covariances(q == NULL) writes, deleted ids included; the target, nt points; target_cov6[6 * nt] in the
 * caller's target order, computed in the target's own frame.
 * Pairs: at pose T (the session's float32 trans) exactly the pairs the reference corresponder finds for the
 * re-projected target p_i = Mat4.Transform(T, target_i) (float32, the bits pcgx_mat4_transform gives): the partner is
 * Nearest(p_i, MaxDist) on the base, after DeletePoint too.  MinDistSq > 0 is refused, as for plane sessions.  Before
 * the first update (iter == 0) the target is a plain copy and T counts as the identity, as for the other kinds.
 * Per pair (i -> base id j), everything float64 from the float32 inputs widened, R the upper-left 3 x 3 of T, the pose
 * increment p' = p + t + w x p with parameters {t0, t1, t2, w0, w1, w2} as everywhere here:
 *   r   = p_i - b_j
 *   S   = C_b[j] + R C_t[i] R^T                           (symmetric 3 x 3)
 *   M   = S^-1                                            (held fixed within an iteration: its dependence on R is
 *                                                          not differentiated -- GICP as Segal and fast_gicp have it)
 *   J_k = e_k (k = 0..2),  J_{3+k} = e_k x p_i            (d r / d parameter k)
 *   e   = r^T M r;  g_k = J_k^T M r;  H_kl = J_k^T M J_l  (k <= l)
 * The exchange vector has the plane session's 30 doubles: {sum e, sum g [6], upper triangle of sum H row-major [21],
 * sum w, pair count} with w = 1; Evaluated.Value is the mean squared Mahalanobis distance.  Evaluate tail, Gauss-Newton
 * update (flat test, damping, pose composition, iteration cap, PCGX_E_SINGULAR), sums_count / read_sums_n / hessian /
 * result / reset / set_pose / partials / update / step / step_sharded and the host pieces
 * pcgx_icp_plane_finish_evaluate / pcgx_icp_gauss_newton_update are the plane session's, unchanged.
 * Pairs that cannot be inverted are DROPPED, and counted: a pair is used only if S is positive definite by the rule the
 * Gauss-Newton solve uses -- trace(S) > 0 and every pivot of its float64 Cholesky factorisation > 1e-12 trace(S).  NaN
 * or negative covariances fail that by themselves.  A dropped pair is in none of the 30 sums, the pair count included:
 * MinPairs tests the pairs actually used.  pcgx_icp_gicp_session_dropped returns how many pairs the session's last
 * evaluation dropped (on a sharded target: of this rank's tile).
 *   PCGX_COV_PLANE covariances never drop a pair: S then has eigenvalues in [2 epsilon, 2], cond(S) <= 1 / epsilon
 *   (degenerate points give I).
 *   PCGX_COV_RAW covariances of a locally flat surface make S singular along the shared normal, and the pairs are
 *   dropped: RAW is the caller's to regularise before it comes here.
 * Restrictions, as for plane sessions: the default weight only; sums_mode is ignored (float64 sums in a fixed order:
 * two runs are bit-identical); pcgx_icp_session_set_strict is refused; no one-launch small Fit.
 * on_device covers the target and BOTH covariance arrays.  Device buffers: base_cov6 has been read when create
 * returns; target and target_cov6 are read asynchronously on the library's stream and must stay alive until the
 * session's first synchronising call (result, read_sums_n, dropped, ...).
 * Sharded (pcgx_icp_session_step_sharded, the 30-double float64 exchange): a rank holds a tile of the target and that
 * tile's covariances -- computed over the WHOLE target before it is cut into tiles, else the neighbourhoods at the
 * tile borders differ from the unsharded Fit's.  pcgx_icp_fit_multi and the ring form are not offered. */
PCGX_API pcgx_status pcgx_icp_gicp_session_create(const pcgx_kdtree *base, const float *base_cov6, const float *target,
                                                  const float *target_cov6, int64_t nt, int32_t on_device,
                                                  const pcgx_icp_params *params, float damping, double *d_sums30,
                                                  pcgx_icp_session **out);
/* Pairs the last evaluation dropped (0 before the first). */
PCGX_API pcgx_status pcgx_icp_gicp_session_dropped(pcgx_icp_session *s, void *stream, int64_t *n);
/* Whole Fit on the device from host arrays; hessian36 may be NULL.  PCGX_E_NOT_ENOUGH_PAIRS counts used pairs;
 * PCGX_E_SINGULAR if sum H is not positive definite. */
PCGX_API pcgx_status pcgx_icp_gicp_fit(const pcgx_kdtree *base, const float *base_cov6, const float *target,
                                       const float *target_cov6, int64_t nt, const pcgx_icp_params *params,
                                       float damping, float trans16[16], pcgx_icp_stat *stat, float hessian36[36]);
/* The same from the clouds alone: builds a tree over the target (host memory), runs pcgx_kdtree_covariances_dev(k,
 * cov_max_range, PCGX_COV_PLANE, epsilon) on both clouds and the Fit; the covariances never leave the device, and the
 * result equals pcgx_kdtree_covariances on both clouds followed by pcgx_icp_gicp_fit bit for bit.  Returns the tree
 * build's and the covariance calls' errors unchanged; nt == 0 is PCGX_E_NOT_ENOUGH_PAIRS. */
PCGX_API pcgx_status pcgx_icp_gicp_fit_knn(const pcgx_kdtree *base, const float *target, int64_t nt, int32_t k,
                                           float cov_max_range, float epsilon, const pcgx_icp_params *params,
                                           float damping, float trans16[16], pcgx_icp_stat *stat, float hessian36[36]);

/* ------------------------------------------- statistical outlier removal (extension: no reference parity)
 * PCL's StatisticalOutlierRemoval / Open3D's remove_statistical_outlier over an AoS cloud (stride / xyz_off as
 * pcgx_voxel_filter).
 *   F   = the points whose x, y, z are all finite (the others are dropped and are nobody's neighbour); m = |F|.
 *   d_i = (1/mean_k) * sum of sqrt((double)DistSq) over the mean_k points of F \ {i} with the smallest
 *         (DistSq, id) (pcgx_kdtree_knearest's order, ids = positions in F).  The sum is float64 in that order.
 *         Coincident duplicates of i count; i itself does not.
 *   mu  = sum d_i / m;  sigma = sqrt(sum (d_i - mu)^2 / (m - 1));  T = mu + std_mul * sigma   (all float64;
 *         deterministic: the same bits on every call for the same input).
 *   keep i iff d_i <= T (negative != 0: iff d_i > T).  Output: the kept records, byte for byte, in input order;
 *   *out_n of them (out_data must hold n*stride bytes).
 * 1 <= mean_k <= 64 else PCGX_E_INVALID; n == 0 or m <= mean_k -> PCGX_E_NO_POINT; a stride / offset that does not
 * hold an xyz triple -> PCGX_E_BAD_FIELD.  mean_dist (n doubles by input index, NaN for dropped points) and
 * stats = {mu, sigma, T} are optional (NULL).  A tree over F is built inside the call (pcgx_kdtree_build). */
PCGX_API pcgx_status pcgx_sor_filter(const void *data, int64_t n, int32_t stride, int32_t xyz_off, int32_t mean_k,
                                     float std_mul, int32_t negative, void *out_data, int64_t *out_n,
                                     double *mean_dist, double stats[3]);
/* Device resident: d_data, d_out (>= n*stride bytes) and d_mean_dist (may be NULL) are device buffers; out_n and
 * stats (may be NULL) are host memory.  Returns when everything is done on `stream` (the tree build in between needs
 * the finite count on the host, and the tree is freed before the call returns). */
PCGX_API pcgx_status pcgx_sor_filter_dev(const void *d_data, int64_t n, int32_t stride, int32_t xyz_off,
                                         int32_t mean_k, float std_mul, int32_t negative, void *d_out,
                                         int64_t *out_n, double *d_mean_dist, double stats[3], void *stream);

/* ------------------------------------------- radius outlier removal (extension: no reference parity)
 * PCL's RadiusOutlierRemoval / Open3D's remove_radius_outlier over an AoS cloud (stride / xyz_off as
 * pcgx_voxel_filter), in the shape of pcgx_sor_filter.
 *   F = the points whose x, y, z are all finite (the others are dropped in both modes and are nobody's neighbour).
 *   keep i of F iff |{p in F : DistSq(p, i) < radius^2}| >= min_neighbors, DistSq the reference's float32 expression,
 *   strict.  The point itself is counted: PCL's radius search returns the query point too, so min_neighbors = k here
 *   keeps what PCL's setMinNeighborsInRadius(k) keeps for a cloud without duplicates of the query; Open3D's nb_points
 *   counts the same way.  min_neighbors == 1 keeps exactly F.
 *   negative != 0 keeps the other points of F.
 *   Output: the kept records, byte for byte, in input order; *out_n of them (out_data must hold n*stride bytes).
 * By definition the kept set is kind == 2 of pcgx_kdtree_dbscan on a tree over F with min_pts = min_neighbors: one
 * kernel decides both.  A tree over F is built inside the call (pcgx_kdtree_build).
 * PCGX_E_INVALID: a radius that is not finite and > 0, or min_neighbors < 1; a stride / offset that does not hold an
 * xyz triple -> PCGX_E_BAD_FIELD; n == 0 or F empty -> PCGX_E_NO_POINT. */
PCGX_API pcgx_status pcgx_ror_filter(const void *data, int64_t n, int32_t stride, int32_t xyz_off, float radius,
                                     int32_t min_neighbors, int32_t negative, void *out_data, int64_t *out_n);
/* Device resident: d_data and d_out (>= n*stride bytes) are device buffers; out_n is host memory.  Returns when
 * everything is done on `stream` (the tree build in between needs the finite count on the host, and the tree is freed
 * before the call returns). */
PCGX_API pcgx_status pcgx_ror_filter_dev(const void *d_data, int64_t n, int32_t stride, int32_t xyz_off, float radius,
                                         int32_t min_neighbors, int32_t negative, void *d_out, int64_t *out_n,
                                         void *stream);

/* ------------------------------------------- minimum-distance subsampling (extension: no reference parity)
 * NOT in the reference.  CloudCompare's "subsample by space", Poisson-disk sampling, greedy non-maximum suppression:
 * a subset of the tree's ORIGINAL points no two of which are within `radius` of each other, maximal (every dropped
 * point has a kept one within `radius`), and for every dropped point the kept point that stands for it.  Unlike the
 * voxel filter the output points are input points, so ids, normals, labels and descriptors carry over; unlike
 * pcgx_kdtree_local_maxima the selection is greedy and the spacing is guaranteed.  This comment is the contract,
 * tests/thin_oracle.py restates it.
 * Eligible points E: the live points (not deleted) whose x, y, z are finite and, in score mode, whose score is no NaN.
 *   The others are never kept, suppress nobody and have owner -1.
 * Neighbours: pcgx_kdtree_range_count's set on that handle, DistSq(p_i, p_j) < radius * radius, DistSq the reference's
 *   float32 expression, the product float32, the bound STRICT: two kept points have DistSq >= the bound, and a point at
 *   exactly DistSq == bound suppresses nothing.
 * Priority, a total order on E.  score == NULL (hash mode): the smaller ((uint64)mix(seed, id) << 32) | id comes first,
 *   mix the partner rule's of "shapes" (csrc/shape_terms.h: shape_mix).  Score mode: j comes before i iff
 *   score[j] > score[i], or they are equal (-0 == +0) and j < i; scores <= 0 and +-inf are ordinary values here.
 * Kept set K: what visiting E in priority order and keeping a point iff no kept point is its neighbour keeps -- the
 *   lexicographically first maximal independent set of the radius graph on E.  Given the order it is unique, so the
 *   result is a property of the point set: the same bits on every call, on every kind of handle (grid,
 *   PCGX_RANGE_WALK=1, after DeletePoint) and whatever the schedule.
 * Outputs: ids[Len()] = K ascending, -1 in every remaining slot; *n_ids = |K|; owner[Len()] (may be NULL) = the point
 *   itself for a kept point, for a dropped point of E its kept neighbour with the smallest (DistSq, id) (the rule of
 *   "density clusters" for a border point), -1 for every other point.
 * Rounds (csrc/thin.hip).  One round decides every still undecided point i of E from the states AS THE PREVIOUS ROUND
 *   LEFT THEM: a neighbour before i is KEPT -> i is DROPPED; else no neighbour before i is UNDECIDED -> i is KEPT; else
 *   i stays.  Rounds to completion give K; the states after R rounds are a property of the set as well.  Hash mode needs
 *   O(log n) rounds; a smooth score gives chains as long as the cloud is wide in radii.
 * The host form always finishes: it enqueues batches of pcgx_thin_default_rounds() rounds and reads one count word per
 *   batch until it is zero.
 * PCGX_E_INVALID: a NULL tree; a radius that is not finite and > 0, or whose float32 square is not (a bound of 0 holds
 *   nobody, not a point itself); NULL ids or n_ids with Len() > 0; more than 2^31 - 1 points; max_rounds < 0.
 *   Len() == 0: *n_ids = 0, PCGX_OK. */
PCGX_API pcgx_status pcgx_kdtree_thin(const pcgx_kdtree *t, float radius, uint32_t seed,
                                      const float *score /* [Len()] or NULL */, int64_t *ids /* [Len()] */,
                                      int64_t *n_ids, int64_t *owner /* [Len()], may be NULL */);
/* Same, every array device resident (ids and owners are int32 there), enqueued on `stream` (NULL: the library's);
 * returns without waiting and reads nothing back.  It enqueues max_rounds rounds (0: pcgx_thin_default_rounds()), each
 * of which returns at once when nothing is undecided.  *d_n_left (may be NULL) receives the number of points still
 * undecided.  0: the outputs are the contract's.  > 0: d_ids / d_n_ids hold the points decided KEPT so far -- a subset
 * of K, pairwise at least `radius` apart, not yet maximal -- and d_owner is -2 in every slot. */
PCGX_API pcgx_status pcgx_kdtree_thin_dev(const pcgx_kdtree *t, float radius, uint32_t seed,
                                          const float *d_score /* [Len()] or NULL */, int32_t max_rounds,
                                          int32_t *d_ids /* [Len()] */, int32_t *d_n_ids,
                                          int32_t *d_owner /* [Len()], may be NULL */, int32_t *d_n_left, void *stream);
PCGX_API int32_t pcgx_thin_default_rounds(void);
/* The filter form over an AoS cloud (stride / xyz_off as pcgx_voxel_filter), in the shape of pcgx_ror_filter: F = the
 * records whose x, y, z are all finite; a tree over F is built inside the call; the kept records are hash mode's K
 * over that tree (ids: positions in F), byte for byte, in input order; *out_n of them (out_data must hold n*stride
 * bytes).  PCGX_E_INVALID: a radius that is not finite and > 0; a stride / offset that does not hold an xyz triple ->
 * PCGX_E_BAD_FIELD; n == 0 or F empty -> PCGX_E_NO_POINT. */
PCGX_API pcgx_status pcgx_thin_filter(const void *data, int64_t n, int32_t stride, int32_t xyz_off, float radius,
                                      uint32_t seed, void *out_data, int64_t *out_n);
/* Device resident: d_data and d_out (>= n*stride bytes) are device buffers; out_n is host memory.  Returns when
 * everything is done on `stream`. */
PCGX_API pcgx_status pcgx_thin_filter_dev(const void *d_data, int64_t n, int32_t stride, int32_t xyz_off, float radius,
                                          uint32_t seed, void *d_out, int64_t *out_n, void *stream);

/* ------------------------------------------- farthest-point sampling (extension: no reference parity)
 * NOT in the reference.  PointNet++'s sampling layer, Open3D's farthest_point_down_sample: `count` of the tree's
 * ORIGINAL points, each as far as possible from the ones picked before it, in pick order.  Where the voxel filter takes a
 * leaf and pcgx_kdtree_thin a radius, this takes a target count.  This comment is the contract, tests/fps_oracle.py
 * restates it.
 * Eligible points E: the live points (not deleted) whose x, y, z are all finite.  Every other point is never picked
 *   and has owner -1.
 * Distance: DistSq, the reference's float32 expression (dx dx + dy dy) + dz dz of d = p - q, never contracted.  It is
 *   symmetric in its two points bit for bit; on E it is never NaN, it is >= +0, and it may be +inf on overflow.
 * Start: start >= 0 is the first pick and must lie in E; start = -1 means the smallest id in E.
 * Pick j + 1: among the points of E not yet picked, the one with the largest d_j(p) = the minimum of
 *   DistSq(p, pick_i) over the picks 1 .. j; ties go to the smallest id.  A picked point is never a candidate again;
 *   coincident points have d = 0 and come last, in id order.
 * Stop: after min(count, |E|) picks.
 * Outputs: ids[count] = the picks in pick order, then -1; *n_ids = how many.  dist_sq[count] (may be NULL) = d of each
 *   pick at the moment it was picked: the first +inf, the tail -1.0f; from the second entry on it does not increase.
 *   *cover_sq (may be NULL) = the d the next pick would have had, the largest d among the unpicked points of E: every
 *   point of E lies within it of a pick; -1.0f when none is left.  owner[Len()] (may be NULL) = for a point of E the
 *   id of the pick nearest to it, among equal DistSq the EARLIER pick (an owner changes only when a later pick is
 *   strictly nearer: not pcgx_kdtree_thin's (DistSq, id) rule); -1 for every other point.
 * Prefix property: a maximum with a fixed tie rule does not depend on the schedule, so the result is a property of the
 *   point set -- the same bits on every call and every kind of handle -- and ids and dist_sq for `count` are the first
 *   `count` entries of those for any larger count, and cover_sq is that call's dist_sq[count] (-1.0f where that is
 *   padding).  One call orders a cloud so that every prefix is a sampling of its own.
 * How (csrc/fps.hip): the points in Morton order, in tiles that carry their box and their largest d; a pick skips every
 *   tile whose box is at least that far away, which is exact in float32 (csrc/fps_terms.h states the lemma).  One
 *   launch per pick: the cost is a chain of `count` launches, so for a count above a fraction of Len() a radius and
 *   pcgx_kdtree_thin is the tool.
 * PCGX_E_INVALID, with nothing written: a NULL tree; count < 0 (or above 2^31 - 1); NULL ids or n_ids with Len() > 0
 *   and count > 0; start not in [-1, Len()); start not in E.
 *   Len() == 0, count == 0, or an empty E with start = -1: *n_ids = 0, every output slot holds its padding value,
 *   PCGX_OK. */
PCGX_API pcgx_status pcgx_kdtree_fps(const pcgx_kdtree *t, int64_t count, int64_t start, int64_t *ids /* [count] */,
                                     int64_t *n_ids, float *dist_sq /* [count], may be NULL */,
                                     float *cover_sq /* may be NULL */, int64_t *owner /* [Len()], may be NULL */);
/* Same, every array device resident (ids and owners are int32 there), enqueued on `stream` (NULL: the library's);
 * returns without waiting and reads nothing back: `start` is checked against the handle's host copy. */
PCGX_API pcgx_status pcgx_kdtree_fps_dev(const pcgx_kdtree *t, int64_t count, int64_t start,
                                         int32_t *d_ids /* [count] */, int32_t *d_n_ids,
                                         float *d_dist_sq /* [count], may be NULL */, float *d_cover_sq /* may be NULL */,
                                         int32_t *d_owner /* [Len()], may be NULL */, void *stream);
/* Measurement hook (tools/fps_probe.py).  d_touched == NULL: the call's preparation alone -- the ordered copy of the
 * points, the tiles (rebuilt by every call, not kept on the handle) -- enqueued on `stream`, no output.  Else the steps
 * run too and d_touched[j] (device, uint32 [min(count, Len())]) = the tiles step j touched. */
PCGX_API pcgx_status pcgx_kdtree_fps_prep_dev(const pcgx_kdtree *t, int64_t count, uint32_t *d_touched, void *stream);
/* How a call over n points is cut up (csrc/fps_plan.h), for tests that want sizes at the seams: out4 = {points per
 * tile, tiles, tiles per workgroup of a pick launch, workgroups of a pick launch}; zeros for n == 0 or count == 0. */
PCGX_API pcgx_status pcgx_fps_plan(int64_t n, int64_t count, int64_t out4[4]);
/* The filter form over an AoS cloud (stride / xyz_off as pcgx_voxel_filter), in the shape of pcgx_thin_filter: F = the
 * records whose x, y, z are all finite; a tree over F is built inside the call; the output records are the picks over
 * that tree (start: -1, or a position in F), byte for byte, IN PICK ORDER -- not pcgx_thin_filter's input order: the
 * prefix property is the point; *out_n = min(count, |F|) of them (out_data must hold n*stride bytes).
 * PCGX_E_INVALID: count < 0, start not in [-1, |F|); a stride / offset that does not hold an xyz triple ->
 * PCGX_E_BAD_FIELD; n == 0 or F empty -> PCGX_E_NO_POINT. */
PCGX_API pcgx_status pcgx_fps_filter(const void *data, int64_t n, int32_t stride, int32_t xyz_off, int64_t count,
                                     int64_t start, void *out_data, int64_t *out_n);
/* Device resident: d_data and d_out (>= n*stride bytes) are device buffers; out_n is host memory.  Returns when
 * everything is done on `stream`. */
PCGX_API pcgx_status pcgx_fps_filter_dev(const void *d_data, int64_t n, int32_t stride, int32_t xyz_off, int64_t count,
                                         int64_t start, void *d_out, int64_t *out_n, void *stream);

/* ------------------------------------------- consistent normal orientation (extension: no reference parity)
 * NOT in the reference.  Hoppe et al. 1992; Open3D's orient_normals_consistent_tangent_plane; CloudCompare's "orient
 * normals with a minimum spanning tree".  pcgx_kdtree_normals turns every normal towards one viewpoint, which is right
 * for one scan from one pose and wrong for a merged map, a downsampled cloud or a closed object.  This call gives
 * neighbouring normals the same side instead: it propagates a sign along the minimum spanning forest of the radius graph,
 * whose edges are cheapest where two normals are most nearly parallel.  Over the tree's own points only; every array is in
 * id order over Len(), deleted ids included (the q == NULL convention).  This comment is the contract,
 * tests/orient_oracle.py restates it, csrc/orient_terms.h holds its expressions.
 * Neighbourhood N(i): the set pcgx_kdtree_range_count counts on that handle, float32 DistSq < radius * radius, STRICT.
 * Usable point: "clusters"' rule with normals given: i is in N(i) (not deleted, x, y, z finite, a bound above 0), and
 *   the three components of its normal are finite and not all zero.  Normals are taken as given, not normalised.
 * Edge {i, j}, i != j: both usable and j in N(i) (DistSq is symmetric bit for bit).  Its agreement is
 *   c = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in float64 from the float32 components, the products exact, the two additions
 *   rounded in this order, nothing contracted ("clusters"' expression); its sign is s = (c < 0).
 * Edge order, strict and total: e comes before f iff |c_e| > |c_f|, or they are equal and min(i, j) is smaller, or those
 *   are equal too and max(i, j) is smaller.  (Hoppe's weight 1 - |c|, the ties made explicit.)
 * Forest after R rounds: F_0 has no edges.  In a round every component of F_R that has an edge leaving it takes the
 *   first such edge in the edge order; all taken edges are added at once.  Under a strict order that makes no cycle, and
 *   F_inf is the minimum spanning forest, which is unique.  The components with a leaving edge at least halve each round:
 *   pcgx_orient_full_rounds(Len()) = max(1, ceil(log2 Len())) rounds always suffice.
 * Parity pi_i: the XOR of s along the forest's path from i to the smallest member id of its component.
 * Component sign sigma, by mode:
 *   0  sigma = 0: the smallest-id member keeps its given sign.  ref is not read.
 *   1  ref = a direction u.  The anchor is the member with the largest float32 h = (px ux + py uy) + pz uz, never
 *      contracted, compared after h + 0 (so -0 ties with +0; a NaN from an overflow is ordered by its bits), ties to the
 *      smallest id.  sigma = 1 iff the anchor's normal after pi, dotted with u the way c is formed, is < 0.  (Hoppe's
 *      rule: the topmost point looks up.)
 *   2  ref = a viewpoint v.  Member i votes "wrong" when t_i < 0 and "right" when t_i > 0, t_i = (n'x ex + n'y ey) +
 *      n'z ez in float64, e = (double)v - (double)p_i, n' the normal after pi; t_i == 0 (or NaN) abstains.  sigma = 1 iff
 *      wrong > right.
 * Outputs: flipped[i] = pi_i ^ sigma, 0 for an unusable point.  normals_out[3 i ..] = the given normal with the sign bit
 *   of all three components inverted where flipped[i], else the given bits (an unusable point's too); normals_out ==
 *   normals is allowed.  component[i] (may be NULL) = the smallest member id of i's component, -1 for an unusable point.
 *   *n_components = the components.  *n_open = the components that still had a leaving edge after the last round run: 0
 *   means the result is final.  Either of normals_out and flipped may be NULL, not both.
 * The host form always finishes.  The device form enqueues max_rounds rounds, 0 meaning pcgx_orient_full_rounds(Len());
 *   a round reads the number of still-active points from a device word and costs almost nothing once it is zero; nothing
 *   is read back.  With max_rounds = R too small every output is this contract applied to F_R, and *n_open > 0.
 * The same input gives the same bits on every call and on every kind of handle (grid, PCGX_RANGE_WALK=1, after
 *   DeletePoint): the forest is a property of the point set, not of a schedule.
 * A handle that holds a NaN coordinate: its tree is out of order, N is whatever Range gives on it, and j in N(i) need not
 *   mean i in N(j).  There "i in N(i)" is looked up, not assumed, and a component takes the first among the leaving edges
 *   {i, j} one of ITS members i sees (j in N(i)) and the edges other components took into it in that round; with
 *   symmetric neighbourhoods that is the rule above.  Still a property of the handle, the same bits on every call.
 * PCGX_E_INVALID, nothing written: a NULL tree; a radius that is not finite and > 0; a mode outside 0..2; in mode 1 or 2
 *   a NULL ref or one with a non-finite component; max_rounds < 0; NULL n_components or n_open; with Len() > 0, NULL
 *   normals, or NULL normals_out and flipped.  Len() == 0: PCGX_OK, the two counts are written (0), nothing else.
 * Always computed on the device (csrc/orient.hip).  Temporaries: 83 bytes per point. */
PCGX_API pcgx_status pcgx_kdtree_orient_normals(const pcgx_kdtree *t, float radius, const float *normals /* [3 Len()] */,
                                                int32_t mode, const float *ref /* [3]; mode 0: may be NULL */,
                                                float *normals_out /* [3 Len()] */, uint8_t *flipped /* [Len()] */,
                                                int64_t *component /* [Len()], may be NULL */, int64_t *n_components,
                                                int64_t *n_open);
/* Same, every array device resident (component and the counts are int32 there; ref stays host memory), enqueued on
 * `stream` (NULL: the library's); returns without waiting, reads nothing back. */
PCGX_API pcgx_status pcgx_kdtree_orient_normals_dev(const pcgx_kdtree *t, float radius, const float *d_normals, int32_t mode,
                                                    const float *ref, int32_t max_rounds, float *d_normals_out,
                                                    uint8_t *d_flipped, int32_t *d_component /* may be NULL */,
                                                    int32_t *d_n_components, int32_t *d_n_open, void *stream);
/* Rounds that finish a call over n points for certain: max(1, ceil(log2 n)); 0 for n <= 0. */
PCGX_API int32_t pcgx_orient_full_rounds(int64_t n);
/* Measurement hooks (tools/orient_probe.py).  The device form without `component`, and d_active (device, uint32
 * [rounds + 1], may be NULL) = the points still in the active list before each enqueued round and after the last.
 * pcgx_orient_active_list: 0 where the library was built with -DPCGX_ORIENT_ACTIVE_LIST=0 (every point stays in the list:
 * the same results, for comparison), else 1. */
PCGX_API pcgx_status pcgx_kdtree_orient_normals_probe_dev(const pcgx_kdtree *t, float radius, const float *d_normals,
                                                          int32_t mode, const float *ref, int32_t max_rounds,
                                                          float *d_normals_out, uint8_t *d_flipped,
                                                          int32_t *d_n_components, int32_t *d_n_open, uint32_t *d_active,
                                                          void *stream);
PCGX_API int32_t pcgx_orient_active_list(void);

/* ------------------------------------------- Normal Distributions Transform (extension: no reference parity)
 * NOT in the reference: pcgol has nothing like it.  NDT registration (Biber and Strasser 2003; Magnusson 2009; PCL's
 * NormalDistributionsTransform) as a fourth Fit beside point-to-point, point-to-plane and Generalized ICP.  It needs
 * no nearest-neighbour search: the BASE cloud (fixed) becomes a map of one Gaussian per voxel of a bucket voxel grid,
 * and the TARGET (the cloud that moves) is scored against the Gaussians of the voxels its points fall into.  Its basin
 * of convergence is about the voxel size, not the point spacing.  Tests check against a NumPy float64 restatement
 * (tests/ndt_oracle.py).
 *
 * The map.  data / n / stride / xyz_off are the cloud the grid was built from (as pcgx_sac_plane_model_create takes
 * them; on_device = 1: device records); creation copies what it needs into library-owned device memory, the grid and
 * the caller's buffers may go afterwards.  Per occupied voxel with integer coordinates v, whose points are the ids
 * whose pcgx_bucket_grid_addr names it (count of them), everything float64 from the float32 inputs widened:
 *   centre      o_k = origin_k + v_k * resolution      (the address arithmetic rounds, so voxel v is centred there)
 *   offsets     d = p - o;  mean_d = sum d / count
 *   covariance  C = (sum d d^T - count * mean_d mean_d^T) / (count - 1)
 *   mean        o + mean_d, rounded to float32 once
 * A voxel is INVALID when count < max(min_points, 3) (min_points below 3 counts as 3), when all its points coincide (the
 * exact min / max box test of pcgx_kdtree_normals), or when the float64 trace of C is <= 0.  Invalid voxels are listed
 * with valid = 0 and zero cov6 / icov6, and take no part in an evaluation.  A valid voxel is regularised: with
 * eigenvalues l0 <= l1 <= l2 and eigenvectors V of C (the Jacobi solve of normals and covariances),
 *   l'_k = max(l_k, min_eigen_ratio * l2),  cov6 = V diag(l') V^T,  icov6 = V diag(1 / l') V^T,
 * each rounded to float32 once: cond <= 1 / min_eigen_ratio, collinear and coplanar voxels stay usable.  The sums of a
 * voxel are taken in a fixed order (one wave over its ids in bucket order, no float atomics): the same call gives the
 * same bits.  PCGX_E_INVALID: a NULL grid or out, n different from the grid's, min_eigen_ratio outside (0, 1].  An
 * empty grid gives a map with no voxels, which is no error.
 * pcgx_ndt_map_cells lists the occupied voxels in ascending voxel address (n_occupied entries each; every array may be
 * NULL); cov6 / icov6 in the order xx, xy, xz, yy, yz, zz of pcgx_kdtree_covariances. */
typedef struct pcgx_ndt_map pcgx_ndt_map;
PCGX_API pcgx_status pcgx_ndt_map_create(const pcgx_bucket_grid *g, const void *data, int64_t n, int32_t stride,
                                         int32_t xyz_off, int32_t on_device, int32_t min_points, float min_eigen_ratio,
                                         pcgx_ndt_map **out);
PCGX_API pcgx_status pcgx_ndt_map_free(pcgx_ndt_map *m);
PCGX_API pcgx_status pcgx_ndt_map_counts(const pcgx_ndt_map *m, int64_t *n_occupied, int64_t *n_valid);
PCGX_API pcgx_status pcgx_ndt_map_cells(const pcgx_ndt_map *m, int64_t *addr, int32_t *count, int32_t *valid,
                                        float *mean3, float *cov6, float *icov6);

/* One evaluation at pose T (trans16, column-major; NULL: the identity).
 * Pairs: p_i = Mat4.Transform(T, target_i) in float32 (the bits pcgx_mat4_transform gives; always applied, for the
 * identity too).  The grid's address arithmetic names p_i's voxel v; a point it refuses (outside the grid, NaN, Inf)
 * contributes nothing.  The candidate voxels are v itself (neighbors = 1), v and its six face neighbours (7), or the
 * 3 x 3 x 3 block round v (27); a candidate is used if it lies inside the grid on every axis -- a neighbour beyond
 * size[k] is NOT the voxel whose address happens to follow -- and is a valid voxel of the map.  Every (point, valid
 * voxel) is a pair.
 * Constants (Magnusson 2009, as PCL's ndt.hpp; res the grid's float32 resolution), formed in extended precision on the
 * host and rounded to float64 once:
 *   c1 = 10 (1 - outlier_ratio);  c2 = outlier_ratio / res^3;  d3 = -log c2;  d1 = -log(c1 + c2) - d3;
 *   k2 = -2 log((-log(c1 e^-1/2 + c2) - d3) / d1)
 * Per pair, all float64; mu and M the voxel's float32 mean and icov6 widened; the pose increment is
 * p' = p + t + w x p with parameters {t0, t1, t2, w0, w1, w2} as everywhere here:
 *   q = p - mu;  m = q^T M q;  omega = exp(-k2 m / 2);  J_k = e_k,  J_{3+k} = e_k x p
 *   e = (2 / k2) (1 - omega);  g_k = omega J_k^T M q;  H_kl = omega J_k^T M J_l  (k <= l)
 * The 30 sums have the plane session's layout {sum e, sum g [6], upper triangle of sum H row-major [21], sum omega,
 * pair count}: unlike Generalized ICP the weight slot holds sum omega, NOT the count, so pcgx_icp_plane_finish_evaluate
 * yields the omega-weighted mean gradient 2 sum g / sum omega, which does not fade with the weights when the clouds
 * are far apart.  This is iteratively reweighted Gauss-Newton on Magnusson's score; the negative-curvature term
 * -k2 g g^T of the full Newton Hessian is left out on purpose, so sum H stays positive semi-definite and the Cholesky
 * rule of the plane Fit applies.  There is no cut-off on distant pairs: omega underflows by itself.  The sums are
 * reduced in a fixed order (lanes, waves, workgroup rows, one final reduce): two calls give the same bits.  nt == 0
 * gives thirty zeros.  PCGX_E_INVALID: outlier_ratio outside (0, 1), k2 not finite or not > 0, neighbors outside
 * {1, 7, 27}, a NULL map, nt < 0, a NULL target with nt > 0, NULL sums. */
PCGX_API pcgx_status pcgx_ndt_evaluate(const pcgx_ndt_map *m, const float *target, int64_t nt,
                                       const float trans16[16] /* NULL: identity */, int32_t neighbors,
                                       float outlier_ratio, double sums30[30]);
/* Same, d_target and d_sums30 device resident, enqueued on `stream` (NULL: the library's); returns without waiting. */
PCGX_API pcgx_status pcgx_ndt_evaluate_dev(const pcgx_ndt_map *m, const float *d_target, int64_t nt,
                                           const float trans16[16], int32_t neighbors, float outlier_ratio,
                                           double *d_sums30, void *stream);

/* The Fit.  From init16 (NULL: the identity) the loop repeats: evaluate; the plane session's tail (the min_pairs test
 * on the pair count, 0 -> 6, then pcgx_icp_plane_finish_evaluate's arithmetic); pcgx_icp_gauss_newton_update's
 * arithmetic (flat test, damping, Translate * (Rodrigues * trans), iteration cap).  Of params only min_pairs, threshold
 * and max_iteration are read.  The whole loop runs on the device behind a `done` flag with one read-back at the end,
 * and equals a host loop of pcgx_ndt_evaluate -> pcgx_icp_plane_finish_evaluate -> pcgx_icp_gauss_newton_update bit for
 * bit.  PCGX_E_NOT_ENOUGH_PAIRS and PCGX_E_SINGULAR as for plane Fits (trans16 is then the pose the failing iteration
 * started from); stat is filled as there, with dist_rms = 0; hessian36 may be NULL; target: host floats, or device
 * floats with on_device = 1.
 * PCGX_E_INVALID: what pcgx_ndt_evaluate refuses, NULL params or trans16, a negative min_pairs or max_iteration.
 * When no point sees a valid voxel with omega > 0 (and min_pairs lets the evaluation pass), the gradient is 0, the flat
 * test holds and the input pose comes back as converged: the caller reads sum omega from an evaluation to tell. */
PCGX_API pcgx_status pcgx_ndt_fit(const pcgx_ndt_map *m, const float *target, int64_t nt, int32_t on_device,
                                  const pcgx_icp_params *params, float damping, int32_t neighbors, float outlier_ratio,
                                  const float init16[16] /* NULL: identity */, float trans16[16], pcgx_icp_stat *stat,
                                  float hessian36[36] /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PCGX_H */
