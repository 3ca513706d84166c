"""A float32 NumPy restatement of pc/sac (sac.go, surface.go) over pc/storage/voxelgrid (voxelgrid.go).

TEST INFRASTRUCTURE ONLY: the GPU's sample consensus (pcgol_amd.sac, csrc/sac.hip) is compared with it bit for bit.
Every operation is one float32 operation in the reference's order (NumPy float32 scalars and arrays round each
operation, nothing is fused); Norm is float32(sqrt(float64(NormSq))) (mat/vec3.go:22-28).  Evaluate's lattice is
vectorised over the serial float32 accumulators `a += l1`, `b += l2`; evaluate_literal is the per-sample loop of
surface.go:202-220 as written, the check of the vectorised one.
"""
import numpy as np

F = np.float32
EPSILON = F(0.01)              # surface.go:17, float32(0.01) where nearZero compares
EPSILON_SQ = F(0.0001)         # epsilon*epsilon: the exact constant 0.0001, rounded once
SQRT3 = F(1.732050808)         # surface.go:16
COEFF_FIELDS = ("origin", "v1", "v2", "l1", "l2", "norm", "d")  # pcgx_sac_plane

# surface.go:108-135, the listed (uncommented) candidates in order: (axis0, index0, axis1, index1)
EDGES = [
    (0, 0, 1, 0), (0, 0, 1, 2), (0, 0, 2, 0), (0, 0, 2, 2),
    (0, 1, 1, 1), (0, 1, 1, 3), (0, 1, 2, 0), (0, 1, 2, 2),
    (0, 2, 1, 0), (0, 2, 1, 2), (0, 2, 2, 1), (0, 2, 2, 3),
    (0, 3, 1, 1), (0, 3, 1, 3), (0, 3, 2, 1), (0, 3, 2, 3),
    (1, 0, 2, 0), (1, 0, 2, 1),
    (1, 1, 2, 0), (1, 1, 2, 1),
    (1, 2, 2, 2), (1, 2, 2, 3),
    (1, 3, 2, 2), (1, 3, 2, 3),
    (0, 0, 0, 2), (0, 0, 0, 1), (0, 1, 0, 3), (0, 3, 0, 2),
    (1, 0, 1, 2), (1, 0, 1, 1), (1, 1, 1, 3), (1, 3, 1, 2),
    (2, 0, 2, 2), (2, 0, 2, 1), (2, 1, 2, 3), (2, 3, 2, 2),
]


def vec(x, y, z):
    return (F(x), F(y), F(z))


def sub(a, b):
    return (F(a[0] - b[0]), F(a[1] - b[1]), F(a[2] - b[2]))


def add(a, b):
    return (F(a[0] + b[0]), F(a[1] + b[1]), F(a[2] + b[2]))


def mul(a, s):
    return (F(a[0] * s), F(a[1] * s), F(a[2] * s))


def norm_sq(v):
    return F(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2]))


def norm(v):
    return F(np.sqrt(np.float64(norm_sq(v))))


def dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def near_zero(a):
    return -EPSILON < a and a < EPSILON


def near_zero_sq(a):
    return a < EPSILON_SQ


class Grid:
    """voxelgrid.New(resolution, size, origin) with Add(point i, i) for every point: only what SAC reads (Addr, MinMax,
    Resolution and the bucket lengths)."""

    def __init__(self, resolution, size, origin, points):
        self.resolution = F(resolution)
        self.resolution_inv = F(F(1) / self.resolution)
        self.size = [int(s) for s in size]
        self.origin = tuple(F(v) for v in np.asarray(origin, np.float32).reshape(3))
        a, ok = self.addr_vec(np.asarray(points, np.float32).reshape(-1, 3))
        self.cell_addr, self.cell_count = np.unique(a[ok], return_counts=True)

    def Len(self):
        return self.size[0] * self.size[1] * self.size[2]

    def MinMax(self):  # voxelgrid.go:25-31
        ext = tuple(F(F(self.size[k]) * self.resolution) for k in range(3))
        return self.origin, add(self.origin, ext)

    def addr_vec(self, P):
        """Addr (voxelgrid.go:64-79) of every row of P (float32): (address, ok)."""
        P = np.asarray(P, np.float32).reshape(-1, 3)
        ok = np.ones(len(P), bool)
        v = np.zeros((len(P), 3), np.int64)
        with np.errstate(invalid="ignore"):
            for k in range(3):
                f = (P[:, k] - self.origin[k]) * self.resolution_inv + F(0.5)
                good = (f == f) & (f > F(-9.0e18)) & (f < F(9.0e18))
                v[:, k] = np.where(good, f, F(0)).astype(np.int64)   # Go's int(): truncation
                ok &= good & (v[:, k] >= 0) & (v[:, k] < self.size[k])
        a = v[:, 0] + (v[:, 1] + v[:, 2] * self.size[1]) * self.size[0]
        return np.where(ok, a, 0), ok

    def count_of(self, addrs):
        """len(GetByAddr(a)) of every address (0 for an empty voxel)."""
        addrs = np.asarray(addrs, np.int64)
        j = np.searchsorted(self.cell_addr, addrs)
        jj = np.minimum(j, max(len(self.cell_addr) - 1, 0))
        hit = (j < len(self.cell_addr)) & (self.cell_addr[jj] == addrs) if len(self.cell_addr) else np.zeros(len(addrs), bool)
        return np.where(hit, self.cell_count[jj] if len(self.cell_addr) else 0, 0)


class Coefficients:
    """voxelGridSurfaceModelCoefficients (surface.go:191-200)."""

    def __init__(self, model, origin, v1, v2, l1, l2, nrm, d):
        self.model = model
        self.origin, self.v1, self.v2, self.l1, self.l2, self.norm, self.d = origin, v1, v2, l1, l2, nrm, d

    def as_array(self):
        """the 15 float32 of pcgx_sac_plane"""
        return np.array([*self.origin, *self.v1, *self.v2, self.l1, self.l2, *self.norm, self.d], np.float32)

    def sequences(self, cap=None):
        """the values the accumulators a (+= l1) and b (+= l2) take while <= 1 (surface.go:206-207)"""
        out = []
        for step in (self.l1, self.l2):
            s, x = [], F(0)
            while x <= 1:
                s.append(x)
                if cap is not None and len(s) > cap:
                    break
                x = F(x + step)
            out.append(np.array(s, np.float32))
        return out

    def Evaluate(self):
        A, B = self.sequences()
        g = self.model.vg
        o, v1, v2 = self.origin, self.v1, self.v2
        P = np.empty((len(A), len(B), 3), np.float32)
        for k in range(3):
            P[:, :, k] = (o[k] + v1[k] * A)[:, None] + v2[k] * B[None, :]
        a, ok = g.addr_vec(P.reshape(-1, 3))
        return int(g.count_of(np.unique(a[ok])).sum())

    def evaluate_literal(self):
        """surface.go:202-220 sample by sample."""
        g = self.model.vg
        added = set()
        cnt = 0
        a = F(0)
        while a <= 1:
            b = F(0)
            while b <= 1:
                p = add(add(self.origin, mul(self.v1, a)), mul(self.v2, b))
                addr, ok = g.addr_vec(np.array([p], np.float32))
                if ok[0] and int(addr[0]) not in added:
                    added.add(int(addr[0]))
                    cnt += int(g.count_of(addr)[0])
                b = F(b + self.l2)
            a = F(a + self.l1)
        return cnt

    def Inliers(self, d):  # surface.go:222-235
        d = F(d)
        q = self.model.points - np.array(self.model.vg_min, np.float32)
        n = self.norm
        dd = ((n[0] * q[:, 0] + n[1] * q[:, 1]) + n[2] * q[:, 2]) - self.d
        return np.nonzero((-d < dd) & (dd < d))[0].astype(np.int64)

    def IsIn(self, p, d):  # surface.go:237-240
        d = F(d)
        dd = F(dot(self.norm, sub(tuple(F(v) for v in p), self.model.vg_min)) - self.d)
        return bool(-d < dd and dd < d)


class SurfaceModel:
    """voxelGridSurfaceModel (surface.go:9-30) over a Grid and the cloud it was filled from (or any other)."""

    def __init__(self, vg, points):
        self.vg = vg
        self.points = np.asarray(points, np.float32).reshape(-1, 3)
        self.vg_min, vg_max = vg.MinMax()
        self.vg_size = sub(vg_max, self.vg_min)

    def NumRange(self):
        return 3, 3

    def Fit(self, ids):  # surface.go:36-181
        if len(ids) != 3:
            return None, False
        p0, p1, p2 = (sub(tuple(self.points[i]), self.vg_min) for i in ids)
        v1, v2 = sub(p1, p0), sub(p2, p0)
        nrm = (F(F(v1[1] * v2[2]) - F(v1[2] * v2[1])), F(F(v1[2] * v2[0]) - F(v1[0] * v2[2])),
               F(F(v1[0] * v2[1]) - F(v1[1] * v2[0])))
        if near_zero_sq(norm_sq(nrm)):
            return None, False
        nrm = mul(nrm, F(F(1) / norm(nrm)))
        d = dot(nrm, p0)
        valid = [not near_zero(nrm[0]), not near_zero(nrm[1]), not near_zero(nrm[2])]
        vs = self.vg_size
        vgn = (F(nrm[0] * vs[0]), F(nrm[1] * vs[1]), F(nrm[2] * vs[2]))
        z = F(0)
        o = [[(z, z, z)] * 4 for _ in range(3)]
        if valid[0]:
            o[0] = [(F(F(F(d - vgn[1]) - vgn[2]) / nrm[0]), vs[1], vs[2]), (F(F(d - vgn[1]) / nrm[0]), vs[1], z),
                    (F(F(d - vgn[2]) / nrm[0]), z, vs[2]), (F(d / nrm[0]), z, z)]
        if valid[1]:
            o[1] = [(vs[0], F(F(F(d - vgn[0]) - vgn[2]) / nrm[1]), vs[2]), (vs[0], F(F(d - vgn[0]) / nrm[1]), z),
                    (z, F(F(d - vgn[2]) / nrm[1]), vs[2]), (z, F(d / nrm[1]), z)]
        if valid[2]:
            o[2] = [(vs[0], vs[1], F(F(F(d - vgn[0]) - vgn[1]) / nrm[2])), (vs[0], z, F(F(d - vgn[0]) / nrm[2])),
                    (z, vs[1], F(F(d - vgn[1]) / nrm[2])), (z, z, F(d / nrm[2]))]

        def inside(p):
            return not (p[0] < 0 or vs[0] < p[0] or p[1] < 0 or vs[1] < p[1] or p[2] < 0 or vs[2] < p[2])

        edge = [[[] for _ in range(4)] for _ in range(3)]
        for a0, i0, a1, i1 in EDGES:
            if not valid[a0] or not valid[a1]:
                continue
            if inside(o[a0][i0]) and inside(o[a1][i1]) and not near_zero_sq(norm_sq(sub(o[a0][i0], o[a1][i1]))):
                edge[a0][i0].append((a1, i1))
                edge[a1][i1].append((a0, i0))
        for a in range(3):
            for i in range(4):
                es = edge[a][i]
                edge[a][i] = [e for j, e in enumerate(es)
                              if not any(near_zero_sq(norm_sq(sub(o[e[0]][e[1]], o[f[0]][f[1]]))) for f in es[j + 1:])]
        aO = iO = 0
        max_len_sq = F(0)
        for a in range(3):
            for i in range(4):
                es = edge[a][i]
                if len(es) != 2:
                    continue
                ln = F(0)
                for e in es:
                    ln = F(ln + norm_sq(sub(o[a][i], o[e[0]][e[1]])))
                if ln > max_len_sq:
                    max_len_sq = ln
                    aO, iO = a, i
        if max_len_sq == 0:
            return None, False
        es = edge[aO][iO]
        o0, o1, o2 = o[es[0][0]][es[0][1]], o[aO][iO], o[es[1][0]][es[1][1]]
        ov1, ov2 = sub(o0, o1), sub(o2, o1)
        r = F(self.vg.resolution / SQRT3)
        return Coefficients(self, add(o1, self.vg_min), ov1, ov2, F(r / norm(ov1)), F(r / norm(ov2)), nrm, d), True


def compute(model, ids, n):
    """SAC.Compute(n) (sac.go:33-59) over the pre-drawn ids[3n], in draw order.
    -> (found, best index or -1, best score, [(coeff or None, ok, score)] per hypothesis)"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    best, best_e, per = -1, 0, []
    for h in range(n):
        c, ok = model.Fit([int(i) for i in ids[3 * h:3 * h + 3]])
        e = c.Evaluate() if ok else 0
        per.append((c, ok, e))
        if ok and e > best_e:
            best_e, best = e, h
    return best >= 0, best, best_e, per
