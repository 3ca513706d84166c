"""k-NN covariances and radius normals on the GPU (csrc/knearest.hip covariance mode, csrc/normals.hip, csrc/cov3.h)
on ill-conditioned neighbourhoods, against the exact reference (tests/cov_exact.py): no spectral-gap gate and no share
of the queries left out.  Every scene runs on the grid, the forced walk (PCGX_RANGE_WALK=1) and a handle after
DeletePoints, through Covariances RAW and PLANE and, with a radius, through Normals.

With C, tr, S, B = (2 n + 4) 2^-53 S and lambda (unit trace) from cov_exact, n the returned float32 normal and n_hat
the same renormalised in float64, every non-degenerate query must keep:
  counts                    equal to knn_oracle / the brute-force radius list
  RAW entry                 2^-24 (|C| + B) + B                  float32 store of a value within B
  n_hat^T C n_hat - l0 tr   6 B + 2e-14 tr                       entrywise B is a 2-norm perturbation <= 3 B, twice; the
                                                                 float32 normal is within sqrt(3) 2^-24 rad: 3 2^-48 tr;
                                                                 the Jacobi allowance J tr of tests/test_cov3_host.py
  | |n| - 1 |               2^-22                                three float32 roundings
  PLANE - (I - (1-eps) n n^T)  2^-22 per entry                   built from the returned n; the same, plus the store
  n . (v - q)               >= -2^-22 |v - q|                    the sign rule, to the normal's rounding
  curvature - max(l0, 0)    (6 B + 2e-14 tr) / tr + 2^-24        as the Rayleigh excess
  fallback (PLANE exactly I, normal exactly 0, curvature NaN, RAW still within its bound) only where tr <= 3 B: the
  guard `tr > 0.0` can fire only when rounding can cancel the trace.
Exact degenerates (n < 3, one place) stay bit-exact I / 0 / 0 / NaN; nothing else may be NaN or Inf."""
import os
import sys

import numpy as np
import pytest

from pcgol_amd import kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_exact as CE  # noqa: E402
import knn_oracle as KO  # noqa: E402
import normals_oracle as NO  # noqa: E402

pytestmark = pytest.mark.gpu

VP = (0.25, -2.0, 5.0)
EPS = 1e-3
F24, F22 = 2.0 ** -24, 2.0 ** -22
EYE6 = np.float32([1, 0, 0, 1, 0, 1])


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _sources(pts, monkeypatch, deleted):
    """(name, tree, excluded ids): the grid, the forced walk, a handle after DeletePoints"""
    t = kdtree.New(pts)
    yield "grid", t, None
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    yield "walk", t, None
    monkeypatch.delenv("PCGX_RANGE_WALK")
    td = kdtree.New(pts)
    td.DeletePoints(deleted)
    yield "deleted", td, np.asarray(deleted, np.int64)


class Worst:
    """the worst ratio of each figure to its bound, per scene (printed: DESIGN 3.8 quotes them)"""

    def __init__(self, scene):
        self.scene, self.r, self.fallbacks, self.queries = scene, {}, 0, 0

    def take(self, key, value, bound):
        ratio = np.max(np.where(bound > 0, value / np.where(bound > 0, bound, 1.0), np.where(value > 0, np.inf, 0.0)),
                       initial=0.0)
        self.r[key] = max(self.r.get(key, 0.0), float(ratio))

    def show(self):
        print("%s: %d non-degenerate results, %d fallbacks; worst / bound: %s"
              % (self.scene, self.queries, self.fallbacks, ", ".join("%s %.3g" % kv for kv in sorted(self.r.items()))))


def _judge(E, q, vp, normal, what, W, raw=None, plane=None, curvature=None, fallback_ok=False):
    """the table in the file's head on one result; E from cov_exact.from_lists.  -> mask of the fallbacks"""
    q64 = np.asarray(q, np.float32).astype(np.float64)
    deg = E["degenerate"]
    nd = int(deg.sum())
    assert np.isfinite(normal).all(), what
    assert np.array_equal(normal[deg], np.zeros((nd, 3), np.float32)), what
    if raw is not None:
        assert np.isfinite(raw).all() and np.array_equal(raw[deg], np.zeros((nd, 6), np.float32)), what
    if plane is not None:
        assert np.isfinite(plane).all() and np.array_equal(plane[deg], np.tile(EYE6, (nd, 1))), what
    if curvature is not None:
        assert np.all(np.isnan(curvature[deg])) and not np.any(np.isinf(curvature)), what
    C6, tr, B = E["cov6"], E["trace"], E["B"]
    if raw is not None:
        err = np.abs(raw.astype(np.float64) - C6)[~deg]
        bound = (F24 * (np.abs(C6) + B[:, None]) + B[:, None])[~deg]
        W.take("RAW", err, bound)
        bad = np.nonzero((err > bound).any(1))[0]
        assert len(bad) == 0, (what, "RAW", len(bad), bad[:3], err[bad[:1]], bound[bad[:1]])
    fb = ~deg & ~normal.any(1)
    if fb.any():
        assert fallback_ok, (what, "fallback outside the far-query scene", np.nonzero(fb)[0][:5])
        off = np.nonzero(fb & (tr > 3 * B))[0]
        assert len(off) == 0, (what, "fallback where tr > 3 B", off[:5], tr[off[:5]], B[off[:5]])
        if plane is not None:
            assert np.array_equal(plane[fb], np.tile(EYE6, (int(fb.sum()), 1))), what
        if curvature is not None:
            assert np.all(np.isnan(curvature[fb])), what
    ok = ~deg & ~fb
    W.queries += int(ok.sum())
    W.fallbacks += int(fb.sum())
    if not ok.any():
        return fb
    n = normal[ok].astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    W.take("|n|-1", np.abs(length - 1.0), np.full(len(n), F22))
    assert np.all(np.abs(length - 1.0) <= F22), (what, "unit length", float(np.max(np.abs(length - 1.0))))
    nh = n / length[:, None]
    excess = np.einsum("mi,mij,mj->m", nh, CE.full(C6[ok]), nh) - E["lam"][ok, 0] * tr[ok]
    allow = 6 * B[ok] + 2e-14 * tr[ok]
    W.take("Rayleigh", excess, allow)
    bad = np.nonzero(excess > allow)[0]
    assert len(bad) == 0, (what, "Rayleigh excess", len(bad), np.nonzero(ok)[0][bad[:3]], excess[bad[:3]],
                           allow[bad[:3]], E["lam"][ok][bad[:3]], normal[ok][bad[:3]])
    to_v = np.asarray(vp, np.float32).astype(np.float64)[None, :] - q64[ok]
    dot = np.sum(n * to_v, axis=1)
    assert np.all(dot >= -F22 * np.linalg.norm(to_v, axis=1)), (what, "sign rule")
    if plane is not None:
        f = 1.0 - float(np.float32(EPS))
        want = np.eye(3)[None, :, :] - f * n[:, :, None] * n[:, None, :]
        err = np.abs(plane[ok].astype(np.float64) - np.stack([want[:, a, b] for a, b in CE.UPPER], axis=1))
        W.take("PLANE", err, np.full(err.shape, F22))
        assert np.all(err <= F22), (what, "PLANE", float(err.max()))
    if curvature is not None:
        cv = curvature[ok].astype(np.float64)
        assert np.isfinite(cv).all(), (what, "curvature NaN on a solved query")
        err = np.abs(cv - np.maximum(E["lam"][ok, 0], 0.0))
        allow = allow / tr[ok] + F24
        W.take("curvature", err, allow)
        assert np.all(err <= allow), (what, "curvature", float(np.max(err / allow)))
    return fb


def _radius_lists(pts, q, r, ex):
    bound = np.float32(r) * np.float32(r)
    keep = np.ones(len(pts), bool)
    if ex is not None:
        keep[ex] = False
    with np.errstate(all="ignore"):
        return [np.nonzero((NO.dist_sq_f32(pts, x) < bound) & keep)[0] for x in _f32(q).reshape(-1, 3)]


def _cov(t, pts, q, k, r, E, what, W, vp=VP, fallback_ok=False):
    """Covariances RAW and PLANE of one handle against E (the exact reference of knn_oracle's lists) -> fallbacks"""
    raw, rn, rc = t.Covariances(k, r, Mode="raw", Queries=q, Viewpoint=vp)
    pl, pn, pc = t.Covariances(k, r, Mode="plane", Epsilon=EPS, Queries=q, Viewpoint=vp)
    assert np.array_equal(rc, E["n"]) and np.array_equal(pc, E["n"]), (what, "counts")
    assert np.array_equal(rn.view(np.uint32), pn.view(np.uint32)), (what, "the normal does not depend on the mode")
    return _judge(E, q, vp, pn, what, W, raw=raw, plane=pl, fallback_ok=fallback_ok)


def _exact_knn(pts, q, k, r, ex):
    oi, _, oc = KO.knearest(pts, q, k, r, exclude=ex)
    return CE.from_lists(pts, q, CE.knn_lists(oi, oc))


def _run(scene, pts, q, ks, radius, deleted, monkeypatch, max_range=np.inf, vp=VP, expect=None):
    """one scene on the three sources: Covariances for every k (lists cut by max_range), Normals with `radius`.
    expect(E, k): scene-specific assertions on the exact reference (k None: the radius lists).  -> Worst"""
    pts, q = _f32(pts), _f32(q)
    W = Worst(scene)
    cache = {}
    for name, t, ex in _sources(pts, monkeypatch, deleted):
        key = ex is not None
        for k in ks:
            if (key, k) not in cache:
                cache[(key, k)] = _exact_knn(pts, q, k, max_range, ex)
                if expect:
                    expect(cache[(key, k)], k)
            _cov(t, pts, q, k, max_range, cache[(key, k)], (scene, name, k), W, vp)
        if radius is not None:
            if (key, None) not in cache:
                cache[(key, None)] = CE.from_lists(pts, q, _radius_lists(pts, q, radius, ex))
                if expect:
                    expect(cache[(key, None)], None)
            E = cache[(key, None)]
            nrm, cv, cnt = t.Normals(radius, Viewpoint=vp, Queries=q)
            assert np.array_equal(cnt, E["n"]), (scene, name, "Normals counts")
            _judge(E, q, vp, nrm, (scene, name, "Normals"), W, curvature=cv)
    W.show()
    return W


# ---- exact structures on a 2^-4 lattice ---------------------------------------------------------------------------------

def _lattice(kind):
    a = np.arange(24)
    i, j = [x.ravel() for x in np.meshgrid(a, a, indexing="ij")]
    s = np.arange(200)
    if kind == "plane z":
        p = np.stack([i, j, np.full_like(i, 8)], 1)
    elif kind == "line x":
        p = np.stack([s, np.full_like(s, 4), np.full_like(s, 12)], 1)
    elif kind == "plane x+y+z":
        p = np.stack([i, j, 48 - i - j], 1)
    elif kind == "plane x=y":
        p = np.stack([i, i, j], 1)
    else:  # "line (1,1,1)"
        p = np.stack([s, s, s], 1)
    return _f32(p / 16.0)


@pytest.mark.parametrize("kind", ["plane z", "line x", "plane x+y+z", "plane x=y", "line (1,1,1)"])
def test_exact_planes_and_lines(kind, monkeypatch):
    """lattice points exactly on a plane (lambda0 = 0) or a line (lambda0 = lambda1 = 0): C has exact zeros on the
    axis-aligned ones (the apq == 0 and first-sweep-break paths), a repeated structure on x = y"""
    pts = _lattice(kind)
    off = pts[::7] + np.float32([1, 0, 2]) / 16  # queries off the structure, still on the lattice
    q = _f32(np.concatenate([pts, off]))
    rank = 1 if kind.startswith("line") else 2

    def expect(E, k):
        ok = ~E["degenerate"]
        assert ok.sum() >= 0.8 * len(q)
        assert np.all(np.abs(E["lam"][ok, 0]) <= 1e-15)
        if rank == 1:
            assert np.all(np.abs(E["lam"][ok, 1]) <= 1e-15)
    radius = (4.5 if kind == "line (1,1,1)" else 2.5) / 16  # two lattice steps along the structure
    _run(kind, pts, q, (3, 4, 9, 64), radius, np.arange(3, len(pts), 7), monkeypatch, expect=expect)


def test_isotropic_clusters(monkeypatch):
    """a centre with its six octahedron (eight cube-corner) lattice neighbours: C = c I, any unit normal is right"""
    octa = np.float32([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) / 16
    cube = np.float32([[0, 0, 0]] + [[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]) / 16
    g = np.arange(6) * 4.0
    centres = _f32(np.stack([x.ravel() for x in np.meshgrid(g, g, g, indexing="ij")], 1) + 1.0)  # 216, 4 apart
    co, cc, spare = centres[:90], centres[90:180], centres[180:]
    pts = _f32(np.concatenate([(co[:, None, :] + octa[None]).reshape(-1, 3), (cc[:, None, :] + cube[None]).reshape(-1, 3),
                               (spare[:, None, :] + octa[None]).reshape(-1, 3)]))
    deleted = np.arange(90 * 7 + 90 * 9, len(pts), 2)  # only from the clusters nobody asks about

    def expect(E, k):
        assert not E["degenerate"].any() and (k is None or np.all(E["n"] == k))
        assert np.max(np.abs(E["lam"] - 1.0 / 3.0)) <= 1e-15
    W = _run("isotropic octahedra", pts, co, (7,), 1.5 / 16, deleted, monkeypatch, expect=expect)
    assert W.queries == 3 * 2 * 90
    W = _run("isotropic cubes", pts, cc, (9,), 2.0 / 16, deleted, monkeypatch, expect=expect)
    assert W.queries == 3 * 2 * 90


# ---- thin slabs and a rod ----------------------------------------------------------------------------------------------

def _frame():
    nrm = np.array([1.0, -2.0, 2.0]) / 3.0
    e1 = np.array([2.0, 1.0, 0.0]) / np.sqrt(5.0)
    return nrm, e1, np.cross(nrm, e1)


@pytest.mark.parametrize("thick", [1e-3, 1e-5, 0.0])
def test_thin_slabs(thick, monkeypatch):
    """a tilted plane of extent 1 and thickness 1e-3, 1e-5 and float32 rounding only"""
    r = _rng(21)
    nrm, e1, e2 = _frame()
    ab = r.random((2500, 2))
    pts = _f32(1.0 + ab[:, :1] * e1 + ab[:, 1:] * e2 + thick * r.uniform(-0.5, 0.5, (2500, 1)) * nrm)
    q = _f32(np.concatenate([pts[:600], pts[600:700] + _f32(0.01 * r.normal(size=(100, 3)))]))

    def expect(E, k):
        ok = ~E["degenerate"]
        if k is not None:
            assert ok.all()
        assert np.median(E["lam"][ok, 0]) <= max(10 * thick ** 2, 1e-11) / 1e-3
    _run("slab %g" % thick, pts, q, (3, 20), 0.06, r.choice(2500, 250, replace=False), monkeypatch, expect=expect)


def test_rod_with_two_near_equal_small_eigenvalues(monkeypatch):
    """a tilted line rounded to float32: lambda0 and lambda1 both ~1e-9 lambda2 and as close to each other"""
    r = _rng(22)
    _, e1, _ = _frame()
    pts = _f32(1.0 + r.random((2500, 1)) * e1)
    q = _f32(np.concatenate([pts[:600], pts[600:700] + _f32(0.003 * r.normal(size=(100, 3)))]))

    def expect(E, k):
        if k == 20:
            own = slice(0, 600)
            assert np.median(E["lam"][own, 1] - E["lam"][own, 0]) <= 1e-8 and np.max(E["lam"][own, 1]) <= 1e-6
    _run("rod", pts, q, (3, 20), 0.01, r.choice(2500, 250, replace=False), monkeypatch, expect=expect)


# ---- the smallest lists and the launch shapes -------------------------------------------------------------------------

def test_three_neighbours_and_query_counts(monkeypatch):
    """k = 3, lists cut to exactly 3 by max_range, and nq around one wave (one lane per query, 64 per workgroup)"""
    pts = synth.uniform_cloud(3000, 1.0, 23)
    r = _rng(24)
    qall = _f32(np.concatenate([r.random((100, 3)), pts[:29]]))
    deleted = r.choice(3000, 300, replace=False)
    seen3 = []

    def expect(E, k):
        seen3.append(int((E["n"] == 3).sum()))
    for nq in (1, 63, 64, 65, 129):
        _run("nq %d, k 3" % nq, pts, qall[:nq], (3,), None, deleted, monkeypatch)
        seen3.clear()
        _run("nq %d, cut" % nq, pts, qall[:nq], (8,), 0.062, deleted, monkeypatch, max_range=0.062, expect=expect)
        if nq >= 63:
            assert min(seen3) > 0, "no list was cut to exactly 3"


# ---- far queries: the only place the fallback may appear ----------------------------------------------------------------

@pytest.mark.parametrize("spread,dist", [(1e-3, 1e3), (2e-7, 1e2), (2e-7, 1e4), (1e-3, 1e6)])
def test_far_queries(spread, dist, monkeypatch):
    """a cluster `spread` wide around (1, 1, 1) seen from `dist` away, max_range = inf: the moments cancel 12 to 22
    digits.  RAW stays within B; where the float64 trace rounds to <= 0 the fallback is taken, never where tr > 3 B"""
    r = _rng(25)
    fallback_ok = (spread, dist) != (1e-3, 1e3)
    taken = {"grid": 0, "walk": 0, "deleted": 0}
    for n in (3, 5, 17, 40, 64):
        own = _f32(1.0 + spread * r.uniform(-1, 1, (n, 3)))
        spare = _f32(1.0 + spread * r.uniform(-1, 1, (6, 3)))  # deleted again: the third source keeps the same cluster
        pts = _f32(np.concatenate([own, spare]))
        d = r.normal(size=(150, 3))
        q = _f32(1.0 + dist * d / np.linalg.norm(d, axis=1, keepdims=True))
        t = kdtree.New(own)
        td = kdtree.New(pts)
        td.DeletePoints(np.arange(n, n + 6))
        E = CE.from_lists(own, q, [np.arange(n)] * len(q))
        assert not E["degenerate"].any()
        W = Worst("far %g / %g, n = %d" % (spread, dist, n))
        for name, tree in (("grid", t), ("walk", t), ("deleted", td)):
            if name == "walk":
                monkeypatch.setenv("PCGX_RANGE_WALK", "1")
            what = (W.scene, name)
            fb = _cov(tree, own, q, 64, np.inf, E, what, W, fallback_ok=fallback_ok)
            nrm, cv, cnt = tree.Normals(2.0 * dist + 4.0, Viewpoint=VP, Queries=q)
            assert np.array_equal(cnt, E["n"]), what
            fbn = _judge(E, q, VP, nrm, what + ("Normals",), W, curvature=cv, fallback_ok=fallback_ok)
            if name == "walk":
                monkeypatch.delenv("PCGX_RANGE_WALK")
            taken[name] += int(fb.sum()) + int(fbn.sum())
        W.show()
    if fallback_ok:  # on every source: otherwise the guarded branch (trace rounds to <= 0) is still unrun
        assert min(taken.values()) > 0, taken
    else:
        assert max(taken.values()) == 0, taken


# ---- coincident heaps: Normals' wave-cooperative sums on ill-conditioned moments ---------------------------------------

@pytest.mark.parametrize("heaps", [2, 3])
def test_coincident_heaps(heaps, monkeypatch):
    """two heaps of 4097 points: rank 1; three: exactly coplanar with n in the thousands (fat grid rows summed by the
    whole wave: wave_sum, merge).  The exact reference takes each heap once, with its multiplicity."""
    sites = _f32([[0.3, 0.7, 0.1], [0.8, 0.45, 0.6], [0.15, 0.2, 0.9]])[:heaps]
    r = _rng(26)
    pts = _f32(np.repeat(sites, 4097, axis=0)[r.permutation(4097 * heaps)])
    q = _f32(np.concatenate([np.repeat(sites, 8, axis=0), r.random((70 - 8 * heaps, 3))]))
    monkeypatch.setenv("PCGX_GRID", "2")
    W = Worst("%d heaps" % heaps)
    for name, t, ex in _sources(pts, monkeypatch, np.arange(0, len(pts), 97)):
        E = CE.from_lists(pts, q, _radius_lists(pts, q, 2.0, ex))
        assert not E["degenerate"].any() and np.all(E["n"] == len(pts) - (0 if ex is None else len(ex)))
        assert np.all(np.abs(E["lam"][:, 0]) <= 1e-15) and (heaps == 3 or np.all(np.abs(E["lam"][:, 1]) <= 1e-15))
        nrm, cv, cnt = t.Normals(2.0, Viewpoint=VP, Queries=q)
        assert np.array_equal(cnt, E["n"]), name
        _judge(E, q, VP, nrm, (W.scene, name), W, curvature=cv)
        # a radius that reaches one heap only: one place, exactly degenerate
        nrm, cv, cnt = t.Normals(0.05, Viewpoint=VP, Queries=q[:8 * heaps])
        want = np.int32([len(x) for x in _radius_lists(pts, q[:8 * heaps], 0.05, ex)])
        assert np.array_equal(cnt, want) and np.all(want > 4000), name
        assert not nrm.any() and np.all(np.isnan(cv)), name
    W.show()


# ---- non-finite queries -------------------------------------------------------------------------------------------------

def test_non_finite_queries(monkeypatch):
    pts = synth.uniform_cloud(2000, 1.0, 27)
    bad = [np.nan, np.inf, -np.inf]
    q = _f32([[0.5, 0.5, 0.5]] + [np.where(np.arange(3) == a, v, 0.5) for a in range(3) for v in bad] +
             [[np.nan] * 3, [np.inf, -np.inf, np.nan], [0.25, 0.5, 0.75]])
    n = len(q) - 2
    for name, t, ex in _sources(pts, monkeypatch, np.arange(0, 2000, 5)):
        for k, r in ((8, np.inf), (64, 0.3)):
            raw, rn, rc = t.Covariances(k, r, Mode="raw", Queries=q, Viewpoint=VP)
            pl, pn, pc = t.Covariances(k, r, Mode="plane", Queries=q, Viewpoint=VP)
            assert rc[0] == pc[0] == k and rc[-1] == k and not rc[1:-1].any() and not pc[1:-1].any(), name
            assert np.array_equal(raw[1:-1], np.zeros((n, 6), np.float32)), name
            assert np.array_equal(pl[1:-1], np.tile(EYE6, (n, 1))), name
            assert not rn[1:-1].any() and not pn[1:-1].any(), name
            assert np.isfinite(raw).all() and np.isfinite(pl).all() and np.isfinite(pn).all(), name
            assert pn[0].any() and pn[-1].any(), name
        nrm, cv, cnt = t.Normals(0.3, Viewpoint=VP, Queries=q)
        assert cnt[0] > 3 and cnt[-1] > 3 and not cnt[1:-1].any(), name
        assert not nrm[1:-1].any() and np.all(np.isnan(cv[1:-1])) and np.isfinite(nrm).all(), name
        assert nrm[0].any() and np.isfinite(cv[[0, -1]]).all(), name


# ---- metamorphic, bit for bit -----------------------------------------------------------------------------------------

def _all_outputs(t, q, k, r, radius, vp):
    raw, n1, c1 = t.Covariances(k, r, Mode="raw", Queries=q, Viewpoint=vp)
    pl, n2, c2 = t.Covariances(k, r, Mode="plane", Epsilon=EPS, Queries=q, Viewpoint=vp)
    nrm, cv, cnt = t.Normals(radius, Viewpoint=vp, Queries=q)
    return dict(raw=raw, n_raw=n1, c_raw=c1, plane=pl, n_plane=n2, c_plane=c2, normals=nrm, curvature=cv, counts=cnt)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_power_of_two_scale_is_exact(monkeypatch):
    """points, queries and viewpoint on a 2^-16 lattice in [0, 1)^3, everything times 2^30 and 2^-30: float32 and
    float64 arithmetic commute with the scale (nothing under- or overflows), so the lists are the same and counts,
    normals, PLANE and curvature come back in the same bits; RAW the same after 2^-+60"""
    r = _rng(28)
    pts = _f32(r.integers(0, 1 << 16, (3000, 3)) / 65536.0)
    q = _f32(r.integers(0, 1 << 16, (200, 3)) / 65536.0)
    vp = _f32([0.5, -2.0, 5.0 + 2.0 ** -16])
    deleted = r.choice(3000, 300, replace=False)
    k = 20
    for mr in (np.inf, 2.0 ** -4):
        base = {}
        for s in (1.0, 2.0 ** 30, 2.0 ** -30):
            ps, qs, vs, mrs = _f32(pts * s), _f32(q * s), _f32(vp * s), mr * s
            assert np.array_equal(ps.astype(np.float64), pts.astype(np.float64) * s)
            for ex in (None, deleted):  # the lists are the same: only then does the rest follow
                i0, d0, c0 = KO.knearest(pts, q, k, mr, exclude=ex)
                i1, d1, c1 = KO.knearest(ps, qs, k, mrs, exclude=ex)
                assert np.array_equal(i0, i1) and np.array_equal(c0, c1)
                assert np.array_equal(d1.astype(np.float64), d0.astype(np.float64) * s * s)
            if mr != np.inf:
                assert c0.min() < 3 <= c0.max() and (c0 == 3).any()
            for name, t, ex in _sources(ps, monkeypatch, deleted):
                got = _all_outputs(t, qs, k, mrs, 2.0 ** -4 * s, vs)
                got["raw"] = (got["raw"].astype(np.float64) / (s * s)).astype(np.float32)
                if s == 1.0:
                    base[name] = got
                    assert np.array_equal(got["c_raw"], KO.knearest(pts, q, k, mr, exclude=ex)[2])
                    continue
                for key, val in got.items():
                    assert _same_bits(val, base[name][key]), ("scale %g" % s, mr, name, key)


def test_translation_is_exact(monkeypatch):
    """points, queries and viewpoint on a 2^-4 lattice in [0, 16)^3, shifted by (2^17, -2^18, 2^16): every difference
    is the same float, so every output is the same bits although grid and tree are built over very different boxes"""
    r = _rng(29)
    pts = _f32(r.integers(0, 256, (3000, 3)) / 16.0)
    q = _f32(r.integers(0, 256, (200, 3)) / 16.0)
    vp = _f32([0.5, -2.0, 20.0])
    shift = _f32([2.0 ** 17, -2.0 ** 18, 2.0 ** 16])
    deleted = r.choice(3000, 300, replace=False)
    k = 20
    ps, qs, vs = _f32(pts + shift), _f32(q + shift), _f32(vp + shift)
    for a, b in ((pts, ps), (q, qs), (vp, vs)):
        assert np.array_equal(b.astype(np.float64), a.astype(np.float64) + shift.astype(np.float64))
    for mr in (np.inf, 1.0):
        for ex in (None, deleted):
            i0, d0, c0 = KO.knearest(pts, q, k, mr, exclude=ex)
            i1, d1, c1 = KO.knearest(ps, qs, k, mr, exclude=ex)
            assert np.array_equal(i0, i1) and np.array_equal(c0, c1) and _same_bits(d0, d1)
        if mr != np.inf:
            assert c0.min() < 3 <= c0.max() and (c0 == 3).any()
        base = {name: _all_outputs(t, q, k, mr, 1.0, vp) for name, t, _ in _sources(pts, monkeypatch, deleted)}
        for name, t, ex in _sources(ps, monkeypatch, deleted):
            got = _all_outputs(t, qs, k, mr, 1.0, vs)
            assert np.array_equal(got["c_raw"], KO.knearest(pts, q, k, mr, exclude=ex)[2])
            for key, val in got.items():
                assert _same_bits(val, base[name][key]), ("translation", mr, name, key)


# ---- streams ----------------------------------------------------------------------------------------------------------

def test_first_call_on_other_streams():
    """a fresh handle's first covariance call is CovariancesDev on a non-default stream, at once followed by a second on
    another stream (both read the id -> slot map the first one builds): each equals the host entry's bits"""
    import torch
    dev = torch.device("cuda", 0)
    pts = synth.surface_cloud(40_000, 6.0, 30)[0]
    nq = len(pts)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    out = []
    for _ in range(2):
        out.append((torch.empty((nq, 6), dtype=torch.float32, device=dev),
                    torch.empty((nq, 3), dtype=torch.float32, device=dev),
                    torch.empty(nq, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    t = kdtree.New(pts)
    for s, (dc, dn, dk), mode in ((s1, out[0], "plane"), (s2, out[1], "raw")):
        t.CovariancesDev(20, dc.data_ptr(), dn.data_ptr(), dk.data_ptr(), Mode=mode, Viewpoint=VP,
                         stream=s.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    for (dc, dn, dk), mode in ((out[0], "plane"), (out[1], "raw")):
        host = t.Covariances(20, Mode=mode, Viewpoint=VP)
        for x, y in zip(host, (dc, dn, dk)):
            assert _same_bits(x, y.cpu().numpy()), mode
        assert np.all(host[2] == 20) and host[1].any(1).all()
