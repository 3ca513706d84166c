"""NumPy restatement of keypoint detection (include/pcgx.h, "keypoints"; csrc/keypoints.hip, csrc/keypoint_terms.h).

No reference counterpart exists: this is the contract itself, by brute force.
  N(i)    = the points p of the cloud (deleted ones left out) with DistSq(p, point i) < r*r, DistSq the reference's
            float32 (dx*dx + dy*dy) + dz*dz;
  maximum = score[i] > 0, and i in N(i), and no other j in N(i) with score[j] > score[i] or (score[j] == score[i] and
            j < i);
  ISS     = (l0, l1, l2): the eigenvalues of normals_oracle's covariance at salient_radius, ascending, l0 clamped at 0,
            rounded to float32, (0, 0, 0) where normals are degenerate; salient iff l0 > 0, l1 < g21 * l2, l0 < g32 * l1
            in float32; saliency = l0 if salient else 0; keypoints = the maxima of saliency at non_max_radius.
Three statements of the suppression, pinned to one another in tests/test_keypoints_oracle.py: local_maxima_direct (all
pairs, small clouds), maxima_from_lists (CSR neighbour lists: brute force or the library's Range batch) and
maxima_from_sites (coincident points share one distance row: clouds with heaps of thousands of coincident points)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_oracle as NO  # noqa: E402

f32 = np.float32


def beats(sj, j, si, i):
    """does neighbour j (score sj) beat point i (score si)?  NaN beats nobody and is beaten by nobody"""
    sj, si = np.asarray(sj, f32), np.asarray(si, f32)
    with np.errstate(invalid="ignore"):
        return (sj > si) | ((sj == si) & (np.asarray(j) < np.asarray(i)))


def candidate(s):
    with np.errstate(invalid="ignore"):
        return np.asarray(s, f32) > f32(0.0)


def saliency(eig, gamma_21, gamma_32):
    """float32 saliency of float32 eigenvalue triples (m, 3)"""
    e = np.asarray(eig, f32).reshape(-1, 3)
    l0, l1, l2 = e[:, 0], e[:, 1], e[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        t21 = f32(gamma_21) * l2
        t32 = f32(gamma_32) * l1
        sal = (l0 > f32(0.0)) & (l1 < t21) & (l0 < t32)
    return np.where(sal, l0, f32(0.0)).astype(f32)


def _live_points(points, deleted):
    p = np.array(points, f32).reshape(-1, 3)
    if deleted is not None and len(deleted):
        p[np.asarray(deleted, np.int64)] = np.nan  # never DistSq < bound: nobody's neighbour, not its own either
    return p


def local_maxima_direct(points, score, radius, deleted=None):
    """every pair, as the contract reads (small clouds) -> ids int64 ascending"""
    p = _live_points(points, deleted)
    s = np.asarray(score, f32).reshape(-1)
    n = len(p)
    bound = f32(radius) * f32(radius)
    out = []
    for i in range(n):
        with np.errstate(invalid="ignore"):
            nb = NO.dist_sq_f32(p, p[i]) < bound
        if not (candidate(s[i]) and nb[i]):
            continue
        j = np.nonzero(nb)[0]
        j = j[j != i]
        if not np.any(beats(s[j], j, s[i], i)):
            out.append(i)
    return np.array(out, np.int64)


def brute_lists(points, radius, deleted=None):
    """CSR (offsets, ids) of N(i) for every id, by looking at every point"""
    p = _live_points(points, deleted)
    with np.errstate(invalid="ignore"):
        return NO.brute_force_lists(p, p, radius)


def maxima_from_lists(score, offs, ids, deleted=None):
    """the rule over CSR neighbour lists of every id (list i = N(i), deleted ids already out of them, or named in
    `deleted`) -> ids int64 ascending"""
    s = np.asarray(score, f32).reshape(-1)
    n = len(s)
    offs, ids = np.asarray(offs, np.int64), np.asarray(ids, np.int64)
    qi = np.repeat(np.arange(n), np.diff(offs))
    keep = np.ones(len(ids), bool)
    if deleted is not None and len(deleted):
        gone = np.zeros(n, bool)
        gone[np.asarray(deleted, np.int64)] = True
        keep = ~gone[ids] & ~gone[qi]
    met = np.bincount(qi[keep & (ids == qi)], minlength=n) > 0
    beaten = np.bincount(qi[keep & (ids != qi) & beats(s[ids], ids, s[qi], qi)], minlength=n) > 0
    return np.nonzero(candidate(s) & met & ~beaten)[0].astype(np.int64)


def sites(points, radius, only=None, deleted=None):
    """[(members, neighbours)]: the ids `only` (a mask; default all) grouped by coincident position, each group with
    the ids of its common neighbourhood -- one distance row per distinct position"""
    p = _live_points(points, deleted)
    n = len(p)
    sel = np.arange(n) if only is None else np.nonzero(only)[0]
    sel = sel[~np.isnan(p[sel]).any(axis=1)]
    bound = f32(radius) * f32(radius)
    _, first, inv = np.unique(p[sel], axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(inv, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(np.bincount(inv))])
    out = []
    for g in range(len(first)):
        members = sel[order[cuts[g]:cuts[g + 1]]]
        with np.errstate(invalid="ignore"):
            nb = np.nonzero(NO.dist_sq_f32(p, p[members[0]]) < bound)[0]
        out.append((members, nb))
    return out


def sites_without(groups, deleted, n):
    """sites() groups of the same cloud after the ids `deleted` have left it"""
    gone = np.zeros(n, bool)
    gone[np.asarray(deleted, np.int64)] = True
    out = [(m[~gone[m]], nb[~gone[nb]]) for m, nb in groups]
    return [(m, nb) for m, nb in out if len(m)]


def maxima_from_sites(score, groups):
    """the rule over sites() groups -> ids int64 ascending.  Ids outside every group are not maxima (the caller left
    out only ids whose score cannot qualify).  Coincident points share N, so a group holds at most one maximum: with
    smax the largest non-NaN score in N and jmin the smallest id in N that has it, every other i in N is beaten (by a
    larger score if score[i] < smax, else by jmin), and jmin by nobody."""
    s = np.asarray(score, f32).reshape(-1)
    out = []
    for members, nb in groups:
        sn = s[nb]
        ok = ~np.isnan(sn)
        if not ok.any():
            continue
        smax = sn[ok].max()
        jmin = nb[sn == smax].min()
        if candidate(smax) and np.any(members == jmin):
            out.append(jmin)
    return np.sort(np.array(out, np.int64))


def eigenvalues_from_lists(points, offs, ids, min_neighbors=5):
    """-> (float32 (n, 3) as the contract rounds them, float64 (n, 3) before rounding, counts)"""
    ref = NO.normals_from_lists(points, points, offs, ids, min_neighbors=min_neighbors)
    lam = np.where(ref["degenerate"][:, None], 0.0, ref["lam"])
    lam[:, 0] = np.maximum(lam[:, 0], 0.0)
    return lam.astype(f32), lam, ref["counts"]


def iss_keypoints(points, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """brute force end to end (small clouds) -> dict(ids, eigenvalues f32, lam f64, saliency f32, counts)"""
    points = np.asarray(points, f32).reshape(-1, 3)
    offs, ids = brute_lists(points, salient_radius)
    eig, lam, counts = eigenvalues_from_lists(points, offs, ids, min_neighbors)
    sal = saliency(eig, gamma_21, gamma_32)
    o2, i2 = brute_lists(points, non_max_radius)
    return dict(ids=maxima_from_lists(sal, o2, i2), eigenvalues=eig, lam=lam, saliency=sal, counts=counts)


def eigenvalue_bound(ref64, counts, radius):
    """|library - oracle| allowed per eigenvalue: float32 rounding of the value plus the moments' bound of
    pcgx_kdtree_normals' contract and a few ulps of the trace for the solve, taken twice (the oracle rounds too)"""
    c = np.asarray(counts, np.float64)[:, None]
    return 2.0 ** -23 * np.abs(ref64) + (2.0 * c + 16.0) * 2.0 ** -52 * float(radius) ** 2
