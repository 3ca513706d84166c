"""Scenes for the tests of cylinder and sphere segmentation (tests/test_shape_oracle.py, tests/test_gpu_shapes.py)."""
import numpy as np

f32, u32 = np.float32, np.uint32
FLOOR, POLE_A, POLE_B, PIPE, BALL, CLUTTER = range(6)


def samples(n_hyp, rounds, seed):
    """uint32 (rounds, n_hyp, 2): what KDTree.Shapes draws for Seed=seed"""
    return np.random.default_rng(seed).integers(0, 2 ** 32, (rounds, n_hyp, 2), dtype=np.uint64).astype(u32)


def _cylinder(rng, m, base, direction, radius, length, noise):
    a = np.asarray(direction, np.float64)
    a = a / np.linalg.norm(a)
    e1 = np.cross(a, [0, 1, 0] if abs(a[1]) < 0.9 else [1, 0, 0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    phi, s = rng.random(m) * 2 * np.pi, rng.random(m) * length
    nrm = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    pts = np.asarray(base, np.float64) + s[:, None] * a + (radius + rng.normal(0, noise, m))[:, None] * nrm
    return pts, nrm


def yard(seed=0):
    """-> (points float32 (10400, 3), normals float32, part int (10400,)): a 6 x 6 floor, two upright poles, a lying
    pipe, a ball and clutter, shuffled; analytic normals perturbed by N(0, 0.05) a component and renormalised."""
    rng = np.random.default_rng(seed)
    P, M, part = [], [], []

    def add(p, m, k):
        P.append(p)
        M.append(m)
        part.append(np.full(len(p), k))
    xy = rng.random((4000, 2)) * 6
    add(np.column_stack([xy, rng.normal(0, 0.004, 4000)]), np.tile([0.0, 0.0, 1.0], (4000, 1)), FLOOR)
    add(*_cylinder(rng, 1500, (1.5, 1.5, 0.0), (0, 0, 1), 0.10, 2.0, 0.003), POLE_A)
    add(*_cylinder(rng, 1800, (4.0, 2.0, 0.0), (0, 0, 1), 0.15, 2.5, 0.003), POLE_B)
    add(*_cylinder(rng, 900, (2.0, 4.5, 0.5), (1, 0, 0.05), 0.08, 1.5, 0.003), PIPE)
    d = rng.normal(size=(1200, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    add(np.array([4.8, 3.3, 0.8]) + (0.3 + rng.normal(0, 0.003, 1200))[:, None] * d, d, BALL)
    c = rng.normal(size=(1000, 3))
    add(rng.random((1000, 3)) * (6, 6, 2.5), c / np.linalg.norm(c, axis=1)[:, None], CLUTTER)
    P, M, part = np.concatenate(P), np.concatenate(M), np.concatenate(part)
    M = M + rng.normal(0, 0.05, M.shape)
    M /= np.linalg.norm(M, axis=1)[:, None]
    order = rng.permutation(len(P))
    return P[order].astype(f32), M[order].astype(f32), part[order]


# the three calls of the yard: keyword arguments of shape_oracle.segment (kind first), and the shapes each must find
CALLS = {
    "poles": (1, dict(sample_radius=0.3, r_min=0.03, r_max=0.3, axis=(0, 0, 1), min_axis_cos=0.95), (POLE_B, POLE_A)),
    "cylinders": (1, dict(sample_radius=0.3, r_min=0.03, r_max=0.3), (POLE_B, POLE_A, PIPE)),
    "spheres": (0, dict(sample_radius=0.4, r_min=0.1, r_max=0.6), (BALL,)),
}
YARD = dict(max_dist=0.02, min_normal_cos=0.8, min_inliers=600)
SEEDS = (1, 5, 7)  # of samples(): on these the oracle finds exactly the shapes above at 128 and at 256 hypotheses


def fat_site(seed=0):
    """A few hundred ordinary points about a unit sphere's patch, and one site taken 4200 times (a fat grid row) inside
    the radius of the seeds around it -> (points, normals)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(400, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    site = np.array([0.0, 0.6, 0.8])
    P = np.concatenate([d, np.tile(site, (4200, 1))])
    M = P.copy()
    order = rng.permutation(len(P))
    return P[order].astype(f32), M[order].astype(f32)


def word_for(i, R):
    """The smallest random word that names index i among R points: (u * R) >> 32 == i."""
    u = -((-int(i) << 32) // int(R))
    assert (u * int(R)) >> 32 == i and 0 <= u < 2 ** 32
    return u


def words(pairs, R):
    return np.array([[word_for(i, R) for i in t] for t in pairs], u32)


def refit_loses(kind, low=0.981):
    """Two sample points exactly on the unit sphere about the origin (kind 0) or the unit cylinder about z (kind 1) with
    exact normals, ten points at distance 1.019 around them and one at `low`: all thirteen are inliers of the unit shape
    at max_dist 0.02; the least-squares radius of the thirteen lies near 1.013 and loses the one at 0.981.  With
    low = 1.019 nothing is lost and the refit is kept.  Twenty far points keep the cloud from being one shape.
    -> (points, normals, words of the one hypothesis (0, 1) for sample_radius 0)"""
    rng = np.random.default_rng(3)
    d = rng.normal(size=(11, 3))
    if kind == 1:
        d[:, 2] = 0
    d /= np.linalg.norm(d, axis=1)[:, None]
    rho = np.concatenate([np.full(10, 1.019), [low]])
    ring = d * rho[:, None]
    if kind == 1:
        ring[:, 2] = rng.random(11)
    first = [[1, 0, 0], [0, 1, 0.5 if kind == 1 else 0]]
    far = rng.random((20, 3)) + (0, 0, 5)
    P = np.concatenate([first, ring, far])
    M = np.concatenate([[[1, 0, 0], [0, 1, 0]], d, np.tile([0.0, 0.0, 1.0], (20, 1))])
    return P.astype(f32), M.astype(f32), words([(0, 1)], len(P))
