"""Scenes of the plane segmentation tests (tests/test_plane_oracle.py, tests/test_gpu_planes.py): small enough that the
NumPy oracle answers in a moment, built so that each one does what its test is for."""
import numpy as np

f32 = np.float32


def word_for(i, R):
    """The smallest random word that names index i among R points: (u * R) >> 32 == i."""
    u = -((-int(i) << 32) // int(R))
    assert (u * int(R)) >> 32 == i and 0 <= u < 2 ** 32
    return u


def words(triples, R):
    return np.array([[word_for(i, R) for i in t] for t in triples], np.uint32)


def samples(n_hyp, max_planes, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, (max_planes, n_hyp, 3), dtype=np.uint64).astype(np.uint32)


def _patch(rng, m, origin, u, v, sigma=0.004):
    u, v = np.asarray(u, float), np.asarray(v, float)
    n = np.cross(u, v)
    n /= np.linalg.norm(n)
    return np.asarray(origin, float) + rng.random((m, 1)) * u + rng.random((m, 1)) * v + rng.normal(0, sigma, (m, 1)) * n


def room(seed=0):
    """13 700 points: a floor of 6000, walls of 3000 and 2000, a slanted patch of 1200 (noise 0.004 along the normal)
    and 1500 clutter points, shuffled.  max_dist 0.02, min_inliers 600: four planes, then a round that finds none."""
    rng = np.random.default_rng(seed)
    c, s = np.cos(np.radians(35)), np.sin(np.radians(35))
    parts = [_patch(rng, 6000, (0, 0, 0), (4, 0, 0), (0, 4, 0)),
             _patch(rng, 3000, (0, 0, 0), (0, 4, 0), (0, 0, 2.5)),
             _patch(rng, 2000, (0, 0, 0), (4, 0, 0), (0, 0, 2.5)),
             _patch(rng, 1200, (1.5, 1.5, 0.4), (1.6, 0, 0), (0, 1.3 * c, 1.3 * s)),
             rng.random((1500, 3)) * (4, 4, 2.5)]
    P = np.concatenate(parts)
    return P[rng.permutation(len(P))].astype(f32)


def lattice(max_dist=0.125):
    """8 x 8 points at multiples of 1/8 on z = 0, and the same again at z = max_dist exactly: not inliers of z = 0."""
    g = np.arange(8) / 8.0
    x, y = np.meshgrid(g, g, indexing="ij")
    low = np.stack([x.ravel(), y.ravel(), np.zeros(64)], 1)
    return np.concatenate([low, low + (0, 0, max_dist)]).astype(f32)


def box_on_floor(seed=1):
    """A floor of 3000 points (normal +z) and the four sides of a box standing on it (horizontal normals), 400 points a
    side down to z = 0: the feet of the sides lie within max_dist of the floor."""
    rng = np.random.default_rng(seed)
    P = [np.column_stack([rng.random(3000) * 4, rng.random(3000) * 4, rng.normal(0, 0.002, 3000)])]
    M = [np.tile([0.0, 0.0, 1.0], (3000, 1))]
    for k, (o, u, nrm) in enumerate((((1, 1, 0), (1, 0, 0), (0, -1, 0)), ((1, 2, 0), (1, 0, 0), (0, 1, 0)),
                                     ((1, 1, 0), (0, 1, 0), (-1, 0, 0)), ((2, 1, 0), (0, 1, 0), (1, 0, 0)))):
        a, z = rng.random((400, 1)), rng.random((400, 1)) * 0.8
        P.append(np.asarray(o, float) + a * np.asarray(u, float) + z * (0, 0, 1))
        M.append(np.tile(np.asarray(nrm, float), (400, 1)))
    P, M = np.concatenate(P), np.concatenate(M)
    p = rng.permutation(len(P))
    return P[p].astype(f32), M[p].astype(f32)


def refit_loses():
    """Three sample points on z = 0, ten points at z = 0.019 over them and one at z = -0.019: all fourteen are inliers of
    z = 0 at max_dist 0.02; the least-squares plane of the fourteen lies near z = 0.013 and loses the low one."""
    rng = np.random.default_rng(3)
    top = np.column_stack([rng.random(10), rng.random(10), np.full(10, 0.019)])
    P = np.concatenate([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], top, [[0.5, 0.5, -0.019]],
                        rng.random((20, 3)) + (0, 0, 5)])  # ... and twenty far above, so that the cloud is not one plane
    return P.astype(f32), words([(0, 1, 2)], len(P))
