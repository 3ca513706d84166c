"""Coarse alignment (extension: no reference counterpart; include/pcgx.h, "pose from correspondences"): the rigid pose
most pairs of a correspondence list agree on, by sample consensus on the GPU -- the starting pose every Fit needs, from
what features.Correspondences returns.  The sampler stays on the host (as in pc/sac): every random word is drawn before
the one call that fits and scores all hypotheses."""
import ctypes as C

import numpy as np

from . import _lib as L

OK, BAD_SAMPLE, DEGENERATE, EDGE = 0, 1, 2, 3  # a hypothesis's status
RESULT_WORDS = 24                               # PCGX_POSE_RESULT_WORDS


def PoseTile():
    """Hypotheses per workgroup of the count kernel (the boundary the tests put n across)."""
    return int(L.lib().pcgx_pose_tile())


def Samples(n, seed=None):
    """(n, 3) uint32 random words, three per hypothesis: word u names pair (u * m) >> 32 of a list of m."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, (int(n), 3), dtype=np.uint64).astype(np.uint32)


def _xyz(a, what):
    a = L.f32c(a)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s: an (n, 3) array of points is required" % what)
    return a


def EstimatePose(P, Q, pairs, n, MaxDist, EdgeSimilarity=0.9, Refine=True, seed=None, samples=None,
                 per_hypothesis=False):
    """-> (found, pose, inlier_ids, info).  P (ns, 3), Q (nd, 3) float32; pairs (m, 2) integer rows (index into P, index
    into Q); n hypotheses from `seed`, or the (n, 3) uint32 `samples` as given.  pose: the column-major float32 [16] that
    takes P onto Q (mat.Transform(pose, P)), the best hypothesis's or -- with Refine, where it keeps at least as many
    inliers -- the least-squares pose over that hypothesis's inliers.  inlier_ids: the pairs within MaxDist under it,
    ascending.  info: best, best_count, refined and, with per_hypothesis, status (n,) int32, counts (n,) int64,
    poses (n, 16) float32.  found is False when no hypothesis agrees with three pairs."""
    p, q = _xyz(P, "P"), _xyz(Q, "Q")
    pairs = np.asarray(pairs)
    if pairs.ndim != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs: an (m, 2) array of ids is required")
    src = np.ascontiguousarray(pairs[:, 0], np.int64)
    dst = np.ascontiguousarray(pairs[:, 1], np.int64)
    if samples is None:
        samples = Samples(n, seed)
    samples = np.ascontiguousarray(samples, np.uint32).reshape(-1, 3)
    nh, m = len(samples), len(src)
    d = np.float32(MaxDist)
    found, refined = C.c_int32(0), C.c_int32(0)
    best, best_count, n_in = C.c_int64(-1), C.c_int64(0), C.c_int64(0)
    pose = np.zeros(16, np.float32)
    ids = np.full(m, -1, np.int64)
    status = np.empty(nh, np.int32) if per_hypothesis else None
    counts = np.empty(nh, np.int64) if per_hypothesis else None
    poses = np.empty((nh, 16), np.float32) if per_hypothesis else None
    L.check(L.lib().pcgx_pose_from_correspondences(
        L.ptr(p), len(p), L.ptr(q), len(q), L.ptr(src), L.ptr(dst), m, L.ptr(samples), nh, float(d * d),
        float(np.float32(EdgeSimilarity)), 1 if Refine else 0, C.byref(found), C.byref(best), C.byref(best_count),
        L.ptr(pose), C.byref(refined), C.byref(n_in), L.ptr(ids), L.ptr(status), L.ptr(counts), L.ptr(poses)))
    info = dict(best=best.value, best_count=best_count.value, refined=bool(refined.value))
    if per_hypothesis:
        info.update(status=status, counts=counts, poses=poses)
    return bool(found.value), pose, ids[:n_in.value], info


def EstimatePoseDev(d_src_xyz, ns, d_dst_xyz, nd, d_src_ids, d_dst_ids, m_cap, d_samples, n, d_result, MaxDist,
                    EdgeSimilarity=0.9, Refine=True, d_n_pairs=0, d_inlier_ids=0, d_status=0, d_counts=0, d_poses=0,
                    stream=0):
    """Device-resident EstimatePose: raw device addresses (e.g. torch .data_ptr()).  d_src_xyz float32 [3 ns], d_dst_xyz
    float32 [3 nd], d_src_ids / d_dst_ids int32 [m_cap] of which the first *d_n_pairs (int32 [1], read on the device;
    0: all m_cap) are the list -- what features.CorrespondencesDev writes; d_samples uint32 [3 n]; d_result
    RESULT_WORDS 4-byte words: int32 found, best, best_count, refined, n_inliers, m, 0, 0, then the float32 pose [16];
    optional d_inlier_ids int32 [m_cap], d_status int32 [n], d_counts int32 [n], d_poses float32 [16 n].  Enqueued on
    `stream`, returns without waiting."""
    d = np.float32(MaxDist)

    def opt(a):
        return L.ptr(int(a)) if a else None

    L.check(L.lib().pcgx_pose_from_correspondences_dev(
        opt(d_src_xyz), int(ns), opt(d_dst_xyz), int(nd), opt(d_src_ids), opt(d_dst_ids), int(m_cap), opt(d_n_pairs),
        opt(d_samples), int(n), float(d * d), float(np.float32(EdgeSimilarity)), 1 if Refine else 0, opt(d_result),
        opt(d_inlier_ids), opt(d_status), opt(d_counts), opt(d_poses), L.ptr(stream) if stream else None))


def ReadResult(words):
    """the record EstimatePoseDev writes, from its host copy (24 int32 words) -> dict"""
    w = np.ascontiguousarray(words, np.int32).reshape(RESULT_WORDS)
    return dict(found=bool(w[0]), best=int(w[1]), best_count=int(w[2]), refined=bool(w[3]), n_inliers=int(w[4]),
                m=int(w[5]), pose=w[8:24].view(np.float32).copy())


# ---- verification on the whole clouds (include/pcgx.h, "score poses")

def ScoreTile():
    """Source points per workgroup of the scoring kernels (the boundary the tests put n across)."""
    return int(L.lib().pcgx_score_tile())


def _poses(a):
    a = L.f32c(a).reshape(-1, 16)
    return a


def ScorePoses(tree, P, poses, MaxDist):
    """-> (counts, sums, best, pose).  tree: the KDTree over the target cloud; P (n, 3) float32; poses (K, 16) float32,
    column-major.  counts (K,) int64: the points of P that land within MaxDist of the tree's cloud under each pose; sums
    (K,) float64: the sum of their DistSq; best: the live pose with the largest count (the smallest k among equals, -1
    if none is live -- a pose of sixteen zeros is dead); pose: its sixteen numbers, or zeros."""
    p = _xyz(P, "P") if len(P) else np.zeros((0, 3), np.float32)
    m = _poses(poses)
    K = len(m)
    counts = np.zeros(K, np.int64)
    sums = np.zeros(K, np.float64)
    best = C.c_int64(-1)
    pose = np.zeros(16, np.float32)
    L.check(L.lib().pcgx_kdtree_score_poses(tree._h, L.ptr(p) if len(p) else None, len(p), L.ptr(m) if K else None, K,
                                            float(np.float32(MaxDist)), L.ptr(counts) if K else None,
                                            L.ptr(sums) if K else None, C.byref(best), L.ptr(pose)))
    return counts, sums, best.value, pose


def ScorePosesDev(tree, d_src_xyz, n, d_poses, K, MaxDist, d_result, d_counts=0, d_sums=0, stream=0):
    """Device-resident ScorePoses: raw device addresses.  d_src_xyz float32 [3 n], d_poses float32 [16 K], d_result
    RESULT_WORDS 4-byte words (ReadScore); optional d_counts int32 [K], d_sums float64 [K].  Enqueued on `stream`,
    returns without waiting, reads nothing back."""

    def opt(a):
        return L.ptr(int(a)) if a else None

    L.check(L.lib().pcgx_kdtree_score_poses_dev(tree._h, opt(d_src_xyz), int(n), opt(d_poses), int(K),
                                                float(np.float32(MaxDist)), opt(d_counts), opt(d_sums), opt(d_result),
                                                L.ptr(stream) if stream else None))


def ReadScore(words):
    """the record ScorePosesDev writes, from its host copy (24 int32 words) -> dict"""
    w = np.ascontiguousarray(words, np.int32).reshape(RESULT_WORDS)
    return dict(best=int(w[0]), best_count=int(w[1]), live=int(w[2]), n=int(w[3]), sum=float(w[4:6].view(np.float64)[0]),
                pose=w[8:24].view(np.float32).copy())


def SelectPoses(status, counts, poses, K):
    """-> (ids, poses, n_selected): the K best hypotheses of an EstimatePose(per_hypothesis=True) call -- status 0 and
    count >= 3, by count descending, then by index ascending; ids (K,) int64 and poses (K, 16) float32, -1 and zeros
    in the slots behind the last one."""
    st = np.ascontiguousarray(status, np.int32)
    ct = np.ascontiguousarray(counts, np.int64)
    m = _poses(poses)
    if not (len(st) == len(ct) == len(m)):
        raise ValueError("status, counts and poses must have one row per hypothesis")
    K = int(K)
    ids = np.empty(max(K, 0), np.int64)
    out = np.empty((max(K, 0), 16), np.float32)
    n_sel = C.c_int64(0)
    nh = len(st)
    L.check(L.lib().pcgx_pose_select(L.ptr(st) if nh else None, L.ptr(ct) if nh else None, L.ptr(m) if nh else None, nh,
                                     K, L.ptr(ids) if K > 0 else None, L.ptr(out) if K > 0 else None, C.byref(n_sel)))
    return ids, out, n_sel.value


def SelectPosesDev(d_status, d_counts, d_poses, n, K, d_ids, d_out_poses, d_n_selected, stream=0):
    """Device-resident SelectPoses over what EstimatePoseDev writes: d_status int32 [n], d_counts int32 [n], d_poses
    float32 [16 n] -> d_ids int32 [K], d_out_poses float32 [16 K], d_n_selected int32 [1].  Enqueued on `stream`."""

    def opt(a):
        return L.ptr(int(a)) if a else None

    L.check(L.lib().pcgx_pose_select_dev(opt(d_status), opt(d_counts), opt(d_poses), int(n), int(K), opt(d_ids),
                                         opt(d_out_poses), opt(d_n_selected), L.ptr(stream) if stream else None))


def EstimatePoseVerified(tree_Q, P, Q, pairs, n, MaxDist, K=16, VerifyDist=None, EdgeSimilarity=0.9, Refine=True, seed=None,
                         samples=None):
    """-> (found, pose, info).  EstimatePose over the pairs, then its K best hypotheses scored on the whole clouds: the
    pose under which most points of P land within VerifyDist (default MaxDist) of Q, the cloud tree_Q was built over.
    info: `estimate` (EstimatePose's own found, pose and info: its best is the one most CORRESPONDENCES agree on),
    `ids` (the selected hypotheses), `counts` and `sums` (their whole-cloud scores), `best_slot`, `best` (the verified
    hypothesis's index, -1 if none) and `agree` (the two name the same hypothesis).  found is False when no hypothesis
    agrees with three pairs."""
    found, pose, inl, est = EstimatePose(P, Q, pairs, n, MaxDist, EdgeSimilarity=EdgeSimilarity, Refine=Refine, seed=seed,
                                         samples=samples, per_hypothesis=True)
    ids, sel, n_sel = SelectPoses(est["status"], est["counts"], est["poses"], K)
    counts, sums, slot, vpose = ScorePoses(tree_Q, P, sel, MaxDist if VerifyDist is None else VerifyDist)
    best = int(ids[slot]) if slot >= 0 else -1
    info = dict(estimate=dict(found=found, pose=pose, inliers=inl, **est), ids=ids, n_selected=n_sel, counts=counts,
                sums=sums, best_slot=slot, best=best, agree=best == est["best"])
    return slot >= 0, vpose, info
