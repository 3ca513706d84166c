"""Scenes and the reference of the point-to-plane route tests (tests/test_plane_icp_scenes.py on the CPU,
tests/test_gpu_icp_plane_routes.py on the GPU).

scene()     a base of 2 977 points -- a dyadic 24 x 24 lattice patch in z = 0 (step 2^-2) and a jittered curved sheet of
            49 x 49 points beside it -- with a pseudo-random unit normal per point, unrelated to its neighbours': a wrong
            partner id changes every sum.  5 000 targets in groups (GROUPS), interleaved so that scene.cut(nt) = the first
            nt targets holds every group from nt = 7 on:
              ordinary   base points plus jitter, well inside MaxDist;
              tie2/tie4  lattice edge midpoints / face centres (some lifted by multiples of 2^-4): exactly equidistant
                         from 2 / 4 base points -- the grid gives them to the walk, the walk's visit order decides;
              limit      lattice points lifted by exactly MaxDist: DistSq == MaxDist^2, where the reference accepts a leaf
                         and not a pivot (kdtree.go:100-103, :117);
              beyond     just outside MaxDist (lattice points lifted by MaxDist + 2^-10, sheet points lifted by 0.75);
              far        a cluster 6.6 .. 7.4 above the lattice: more than 9 grid cells from every base point, with no
                         pair at MAX_DIST and one at MAX_DIST_LARGE;
              nonfinite  NaN, +inf and -inf coordinates.
            Every special coordinate is a multiple of 2^-10 below 16: differences, squares and their sums are exact in
            float32, and so is adding a dyadic translation (scene.shifted).
fit_scene() a rigidly moved, jittered copy of part of the sheet: a real Fit, partners change between iterations.
singular_scene()  a flat part whose normals are all (0, 0, 1) and twelve points with horizontal normals whose targets
            leave MaxDist with the first update: the normal equations turn singular at the second Evaluate.

Non-finite targets.  The reference pairs a NaN target (its DistSq is not greater than MaxDist^2) and all its sums turn
NaN; the device leaves such a target without a pair and fits the rest ("Non-finite input");
an infinite target turns NaN when it is re-projected.  finite_rows() is that rule: the reference below is the oracle
over the targets whose projected coordinates are finite.

The reference.  oracle_ids() are the oracle's pairs (O.KDTree.nearest_batch: the reference's walk); pair_terms() forms
the 30 float32 terms of each pair in NumPy, every product and every sum an operation of its own in the order
oracle/plane_oracle.c documents; fsum30() adds them with math.fsum -- the exactly rounded sum -- and returns
A_k = sum |term_k| beside it.  Device and oracle add the same float32 terms in float64 in some order: either is within
(N - 1) 2^-53 A_k of the exact sum of its N terms, so |d - s| <= N 2^-53 A_k per component (assert_sums); the pair
count and the weight are exact."""
import math

import numpy as np

f32 = np.float32

MAX_DIST = 0.375           # 3 * 2^-3: MaxDist^2 = 0.140625 exactly
MAX_DIST_LARGE = 8.0
LAT_N, LAT_STEP = 24, 0.25
SHEET_N, SHEET_STEP, SHEET_Y0, SHEET_JITTER = 49, 0.125, 7.0, 0.04
N_TARGETS = 5000
GROUPS = ("ordinary", "tie2", "tie4", "limit", "beyond", "far", "nonfinite")
SPECIAL = ("tie2", "tie4", "limit", "beyond", "far", "nonfinite")
FAR_Z = (6.6, 7.4)
GRID_OCC = 1.5             # the documented rule: about 1.5 points per cell of the bounding box (include/pcgx.h, csrc/knn_grid.hip)
SHIFTS = ((0.0, 0.0, 0.0), (2.0, -1.5, 0.5), (-3.25, 4.0, -1.0))  # dyadic translations t_k of shifted(k)
# fit_scene(): the gradient is 0.06 at the second Evaluate and 1e-4 at the third -- the flat test stops the Fit there
FLAT_THRESHOLD = np.full(6, 0.003, f32)


def unit_normals(n, seed):
    """n pseudo-random directions, normalised in float32 (the extension asks for unit length only)"""
    v = np.random.default_rng(seed).normal(size=(n, 3)).astype(f32)
    nrm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(f32)).astype(f32)
    return np.ascontiguousarray((v / nrm[:, None]).astype(f32))


def sheet_height(x, y):
    return 0.5 * np.sin(x) * np.cos(y)


class Scene:
    def __init__(self, base, normals, target, group, lattice_ids, sheet_ids):
        self.base, self.normals, self.target, self.group = base, normals, target, group
        self.lattice_ids, self.sheet_ids = lattice_ids, sheet_ids
        self.max_dist, self.max_dist_large = MAX_DIST, MAX_DIST_LARGE

    def mask(self, *names):
        return np.isin(self.group, [GROUPS.index(n) for n in names])

    def dyadic(self):
        """the targets whose coordinates are multiples of 2^-10: the ties, the limit targets and the first 64 `beyond`"""
        m = self.mask("tie2", "tie4", "limit")
        m[np.flatnonzero(self.mask("beyond"))[:64]] = True
        return m

    def cut(self, nt):
        """the first nt targets (every group is in from nt = 7 on) and their group codes"""
        return np.ascontiguousarray(self.target[:nt]), self.group[:nt]

    def shifted(self, k):
        """-> (target + t_k, the pose Translate(-t_k)): the float32 projection of the special targets by that pose is
        the special targets of scene(), bit for bit"""
        t = np.array(SHIFTS[k], f32)
        pose = np.eye(4, dtype=f32)
        pose[3, :3] = -t  # (column-major: elements 12..14)
        return np.ascontiguousarray((self.target + t).astype(f32)), pose.reshape(-1)

    def grid_edge_estimate(self):
        """the cell edge the documented rule gives for this base: the grid only ever makes its cells smaller"""
        ext = self.base.max(axis=0).astype(np.float64) - self.base.min(axis=0).astype(np.float64)
        return float((np.prod(ext) / (len(self.base) / GRID_OCC)) ** (1.0 / 3.0))


_scene = None


def scene():
    """the one scene (built once; its arrays are shared: do not write into them)"""
    global _scene
    if _scene is None:
        _scene = _build_scene()
    return _scene


def _build_scene():
    rng = np.random.default_rng(20267)
    # ---- base
    i, j = np.meshgrid(np.arange(LAT_N), np.arange(LAT_N), indexing="ij")
    lat = np.stack([i.ravel() * LAT_STEP, j.ravel() * LAT_STEP, np.zeros(LAT_N * LAT_N)], axis=1)
    i, j = np.meshgrid(np.arange(SHEET_N), np.arange(SHEET_N), indexing="ij")
    sx = i.ravel() * SHEET_STEP + rng.uniform(-SHEET_JITTER, SHEET_JITTER, SHEET_N * SHEET_N)
    sy = SHEET_Y0 + j.ravel() * SHEET_STEP + rng.uniform(-SHEET_JITTER, SHEET_JITTER, SHEET_N * SHEET_N)
    sheet = np.stack([sx, sy, sheet_height(sx, sy)], axis=1)
    pts = np.concatenate([lat, sheet]).astype(f32)
    perm = rng.permutation(len(pts))  # ids unrelated to place
    base = np.ascontiguousarray(pts[perm])
    is_lat = perm < len(lat)
    lattice_ids, sheet_ids = np.flatnonzero(is_lat), np.flatnonzero(~is_lat)
    normals = unit_normals(len(base), 20268)
    # ---- targets, group by group
    g = {}
    pick = rng.integers(0, len(base), 3728)
    g["ordinary"] = base[pick].astype(np.float64) + rng.uniform(-0.03, 0.03, (len(pick), 3))
    lifts = np.array([0.0, 0.0625, -0.0625, 0.125, -0.125])
    ci, cj = np.meshgrid(np.arange(2, LAT_N - 3), np.arange(2, LAT_N - 3), indexing="ij")  # interior cells of the lattice
    cells = np.stack([ci.ravel(), cj.ravel()], axis=1)
    c = cells[rng.permutation(len(cells))]
    n2, n4, nl, nb = 48, 48, 64, 64
    edge = c[:n2]
    along_x = np.arange(n2) % 2 == 0
    g["tie2"] = np.stack([(edge[:, 0] + np.where(along_x, 0.5, 0.0)) * LAT_STEP,
                          (edge[:, 1] + np.where(along_x, 0.0, 0.5)) * LAT_STEP, lifts[np.arange(n2) % 5]], axis=1)
    face = c[n2:n2 + n4]
    g["tie4"] = np.stack([(face[:, 0] + 0.5) * LAT_STEP, (face[:, 1] + 0.5) * LAT_STEP, lifts[np.arange(n4) % 5]], axis=1)
    at = c[n2 + n4:n2 + n4 + nl]
    sign = np.where(np.arange(nl) % 2 == 0, 1.0, -1.0)
    g["limit"] = np.stack([at[:, 0] * LAT_STEP, at[:, 1] * LAT_STEP, sign * MAX_DIST], axis=1)
    out = c[n2 + n4 + nl:n2 + n4 + nl + nb]
    just = np.stack([out[:, 0] * LAT_STEP, out[:, 1] * LAT_STEP, sign[:nb] * (MAX_DIST + 2.0 ** -10)], axis=1)
    above = base[sheet_ids[rng.permutation(len(sheet_ids))[:400]]].astype(np.float64)
    above[:, 2] += np.where(np.arange(400) % 2 == 0, 0.75, -0.75)
    g["beyond"] = np.concatenate([just, above])
    mid = (LAT_N - 1) * LAT_STEP / 2
    g["far"] = np.stack([rng.uniform(mid - 1.0, mid + 1.0, 600), rng.uniform(mid - 1.0, mid + 1.0, 600),
                         rng.uniform(FAR_Z[0], FAR_Z[1], 600)], axis=1)
    nf = rng.uniform(0.0, 5.0, (48, 3))
    bad = (np.nan, np.inf, -np.inf)
    for r in range(48):
        nf[r, r % 3] = bad[(r // 3) % 3]
        if r % 8 == 7:
            nf[r, :] = bad[(r // 8) % 3]  # (all three coordinates)
    g["nonfinite"] = nf
    # ---- interleaved: round r takes the r-th target of every group that still has one
    rows, codes = [], []
    for r in range(max(len(v) for v in g.values())):
        for code, name in enumerate(GROUPS):
            if r < len(g[name]):
                rows.append(g[name][r])
                codes.append(code)
    target = np.ascontiguousarray(np.array(rows).astype(f32))
    assert len(target) == N_TARGETS
    return Scene(base, normals, target, np.array(codes, np.int32), lattice_ids, sheet_ids)


def no_grid_scenes():
    """-> {name: dict(base, normals, target, max_dist)}: bases that get no voxel grid.
    "63 points"        a 7 x 9 dyadic lattice (step 2^-2): below the 64 points a grid is built from;
    "all but one alike" 99 copies of one point and one point elsewhere: a point's cell holds 98 others, the grid is
                       given up as crowded -- and every target near the heap ties 99 ways: which id the reference's
                       walk returns decides whose normal enters the sums.
    Targets: jittered copies, exact ties (edge midpoints / the heap itself), targets at exactly MaxDist, beyond it, far
    away and non-finite ones."""
    rng = np.random.default_rng(20270)
    nonfinite = scene().target[scene().mask("nonfinite")][:6]
    out = {}
    i, j = np.meshgrid(np.arange(7), np.arange(9), indexing="ij")
    lat = np.stack([i.ravel() * LAT_STEP, j.ravel() * LAT_STEP, np.zeros(63)], axis=1)
    base = np.ascontiguousarray(lat[rng.permutation(63)].astype(f32))
    mids = lat[lat[:, 1] < 2.0][:20] + np.array([0.0, LAT_STEP / 2, 0.0625])  # (the midpoint of an edge along y, lifted)
    target = np.concatenate([base[rng.integers(0, 63, 150)] + rng.uniform(-0.05, 0.05, (150, 3)), mids,
                             lat[30:40] + np.array([0.0, 0.0, MAX_DIST]), lat[40:50] - np.array([0.0, 0.0, MAX_DIST + 2.0 ** -10]),
                             rng.uniform(20.0, 21.0, (10, 3)), nonfinite])
    out["63 points"] = dict(base=base, normals=unit_normals(63, 20271), max_dist=MAX_DIST,
                            target=np.ascontiguousarray(target[rng.permutation(len(target))].astype(f32)))
    heap, lone = np.array([1.5, -0.25, 2.0]), np.array([2.5, 0.5, 1.75])
    base = np.tile(heap, (100, 1))
    base[37] = lone
    target = np.concatenate([heap + rng.uniform(-0.2, 0.2, (150, 3)), np.tile(heap, (8, 1)), heap + np.array([[MAX_DIST, 0.0, 0.0]] * 4),
                             lone + rng.uniform(-0.2, 0.2, (40, 3)), (heap + lone) / 2 + rng.uniform(-0.1, 0.1, (20, 3)),
                             rng.uniform(20.0, 21.0, (10, 3)), nonfinite])
    out["all but one alike"] = dict(base=np.ascontiguousarray(base.astype(f32)), normals=unit_normals(100, 20272), max_dist=MAX_DIST,
                                    target=np.ascontiguousarray(target[rng.permutation(len(target))].astype(f32)))
    return out


def fit_scene():
    """-> dict(base, normals, target, max_dist): the scene's base and normals; the target a rigidly moved copy (0.012 rad
    about an oblique axis through the sheet, 0.05 along it) of 1 500 sheet points with 0.01 of jitter, eight non-finite
    targets among them"""
    s = scene()
    rng = np.random.default_rng(20269)
    ids = s.sheet_ids[rng.permutation(len(s.sheet_ids))[:1500]]
    p = s.base[ids].astype(np.float64) + rng.uniform(-0.01, 0.01, (1500, 3))
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    ang = 0.012
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K
    centre = np.array([3.0, 10.0, 0.0])
    moved = (p - centre) @ R.T + centre + np.array([0.03, -0.035, 0.02])
    moved[::200] = s.target[s.mask("nonfinite")][:8]
    return dict(base=s.base, normals=s.normals, target=np.ascontiguousarray(moved.astype(f32)), max_dist=MAX_DIST)


def singular_scene():
    """-> dict(base, normals, target, max_dist, n_flat, n_side).  The flat part (40 x 40, step 0.25, z = 0, normals
    (0, 0, 1)) has its targets 0.05 above it; the side part (12 points 2 below it, horizontal normals in twelve directions) has
    its targets 0.36 below their partners: their residual n . d is 0, so the first update is the flat part's -- 0.05 down
    -- and moves them to 0.41 > MaxDist from their partners.  From the second Evaluate on every pair's normal is
    (0, 0, 1): x, y and the rotation about z are unobservable."""
    i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    flat = np.stack([i.ravel() * 0.25, j.ravel() * 0.25, np.zeros(1600)], axis=1)
    k = np.arange(12)
    side = np.stack([1.0 + 0.75 * k, 9.0 - 0.5 * k, np.full(12, -2.0)], axis=1)
    base = np.concatenate([flat, side]).astype(f32)
    normals = np.zeros((1612, 3), f32)
    normals[:1600, 2] = 1.0
    normals[1600:, 0] = np.cos(2 * np.pi * k / 12 + 0.2).astype(f32)
    normals[1600:, 1] = np.sin(2 * np.pi * k / 12 + 0.2).astype(f32)
    nrm = np.sqrt((normals * normals).sum(axis=1, dtype=f32)).astype(f32)
    normals = np.ascontiguousarray((normals / nrm[:, None]).astype(f32))
    target = base.copy()
    target[:1600, 2] += f32(0.05)
    target[1600:, 2] -= f32(0.36)
    return dict(base=base, normals=normals, target=target, max_dist=MAX_DIST, n_flat=1600, n_side=12)


# ------------------------------------------------------------------ the reference

def finite_rows(pts):
    return np.all(np.isfinite(pts), axis=1)


def project(O, pose, it, target):
    """what the Fit loop evaluates at iteration `it` (icp.go:27-30, :62-64): the target itself before the first update,
    its float32 projection by the pose after it"""
    return target if it == 0 else O.mat4_transform(pose, target)


def oracle_ids(otree, pts, max_dist):
    """the oracle's partner per target (-1: none); a non-finite target has none (see the module's text)"""
    ids = np.full(len(pts), -1, np.int64)
    ok = finite_rows(pts)
    if ok.any():
        ids[ok] = otree.nearest_batch(np.ascontiguousarray(pts[ok]), max_dist)[0]
    return ids


def pair_terms(base, normals, pts, ids):
    """(N, 30) float32 terms of the N pairs (ids >= 0), in the order of the sums; each product and each sum rounds to
    float32 on its own (NumPy evaluates one operation per array expression: no fused multiply-add)"""
    on = ids >= 0
    t, pb, n = pts[on].astype(f32), base[ids[on]].astype(f32), normals[ids[on]].astype(f32)
    x0, y0, z0 = t[:, 0], t[:, 1], t[:, 2]
    dx, dy, dz = x0 - pb[:, 0], y0 - pb[:, 1], z0 - pb[:, 2]
    r = n[:, 0] * dx
    r = r + n[:, 1] * dy
    r = r + n[:, 2] * dz
    J = [n[:, 0], n[:, 1], n[:, 2],
         y0 * n[:, 2] - z0 * n[:, 1],
         z0 * n[:, 0] - x0 * n[:, 2],
         x0 * n[:, 1] - y0 * n[:, 0]]
    cols = [r * r] + [J[a] * r for a in range(6)] + [J[a] * J[b] for a in range(6) for b in range(a, 6)]
    one = np.ones(len(t), f32)
    out = np.stack(cols + [one, one], axis=1)
    assert out.dtype == f32 and out.shape == (len(t), 30)
    return out


def fsum30(terms):
    """-> (the exactly rounded sums, A = sum |term| per component, N)"""
    t64 = terms.astype(np.float64)
    s = np.array([math.fsum(t64[:, k]) for k in range(30)])
    a = np.array([math.fsum(np.abs(t64[:, k])) for k in range(30)])
    return s, a, len(terms)


def reference_sums(O, otree, base, normals, pts, max_dist):
    """-> (sums, A, N, ids) of one evaluation at the (already projected) targets"""
    ids = oracle_ids(otree, pts, max_dist)
    s, a, n = fsum30(pair_terms(base, normals, pts, ids))
    return s, a, n, ids


def assert_sums(got, ref, what=""):
    """got: 30 float64 sums formed in any order from the reference's float32 terms; ref: reference_sums' (s, A, N, ...)"""
    s, a, n = ref[0], ref[1], ref[2]
    got = np.asarray(got, np.float64)
    assert got[29] == s[29] == n and got[28] == s[28], (what, got[28:], s[28:], n)
    err, bound = np.abs(got[:28] - s[:28]), n * 2.0 ** -53 * a[:28]
    bad = np.flatnonzero(~(err <= bound))
    assert len(bad) == 0, (what, "components", bad.tolist(), "error", err[bad].tolist(), "bound", bound[bad].tolist())
