"""The scenes of the group footprint tests (no test inside): built once, shared by tests/test_hull_terms_host.py, which
measures the host-compiled finish on them, and tests/test_gpu_group_hulls.py, which runs them on the device.  Each scene
is (points float32 (n, 3), ids int64, sizes int64); tests/group_scenes.py's ladder, slots and chain are scenes too."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_scenes as GS  # noqa: E402

f32 = np.float32
TILE = GS.TILE


def _scene(xy_parts, seed):
    """groups of xy rows -> a cloud in shuffled id order (z: noise), the ids group by group, the sizes"""
    rng = np.random.default_rng(seed)
    xy = np.concatenate(xy_parts).astype(f32)
    n = len(xy)
    perm = rng.permutation(n)  # row r of xy is point perm[r]
    pts = np.zeros((n, 3), f32)
    pts[perm, :2] = xy
    pts[:, 2] = rng.uniform(-1, 1, n).astype(f32)
    return pts, perm.astype(np.int64), np.array([len(p) for p in xy_parts], np.int64)


def parabola_pair(m):
    """the family as written: (i, i^2) and (i, -i^2) for integer i in [-a, b], m rows (the origin is there twice).  Its
    hull is the four end points: everything else is filtered or reduced away."""
    half = m // 2
    lo = np.arange(half) - half // 2
    up = np.arange(m - half) - (m - half) // 2
    return np.concatenate([np.stack([lo, lo * lo], axis=1), np.stack([up, -up * up], axis=1)]).astype(np.float64)


def lens(m):
    """m places that are ALL vertices: (i, i^2) below and (i, K - i^2) above, strictly inside the lower row's x range, K
    large enough that both ends turn strictly left (the two parabolas of parabola_pair moved apart until the polygon is
    convex).  Integers below 2^24: exact in float32."""
    n_lo = m - m // 2 + 1 if m > 2 else m
    n_up = m - n_lo
    lo = np.arange(n_lo) - n_lo // 2
    up = np.arange(n_up) - n_up // 2  # (n_up <= n_lo - 2: inside)
    K = 2 * int(max(abs(lo).max(), 1)) ** 2 + 1
    assert K + 1 < 2 ** 24
    return np.concatenate([np.stack([lo, lo * lo], axis=1), np.stack([up, K - up * up], axis=1)]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def all_vertices(T=TILE):
    """one group of 3 T + 5 and groups of 64 and 65, each a lens: h_g = members"""
    return _scene([lens(3 * T + 5) + [7, -3], lens(64) + [-40, 9], lens(65)], 31)


@functools.lru_cache(maxsize=None)
def parabolas(T=TILE):
    """the same sizes over the family as written"""
    return _scene([parabola_pair(3 * T + 5) + [7, -3], parabola_pair(64) + [-40, 9], parabola_pair(65)], 37)


@functools.lru_cache(maxsize=None)
def lattice_scene():
    """a 40 x 40 integer lattice (4 vertices, 156 boundary places that are none); the same with every point twice and
    the ids shuffled; a row of 500 collinear points (on a line that is no axis); 300 copies of one point"""
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
    row = np.stack([3 * np.arange(500) - 100, 200 - 2 * np.arange(500)], axis=1).astype(np.float64)
    one = np.tile([[12.5, -0.75]], (300, 1))
    return _scene([g, np.concatenate([g + [100, 0], g + [100, 0]]), row, one], 41)


NEAR_K = 26


@functools.lru_cache(maxsize=None)
def near_collinear(k=NEAR_K, step=1):
    """a = (0.5 + i 2^-24, 0.5 + j 2^-24), b = (12 2^k, 12 2^k), c = (24 2^k, 24 2^k) with two far points, once on the
    left of the diagonal and once on its right: b is a vertex exactly when it lies strictly on the other side of the line
    from a to c, which at k = 26 only the exact branch of hull_orient can tell"""
    s = 2.0 ** k
    parts = []
    for i in range(0, 32, step):
        for j in range(0, 32, step):
            abc = [[0.5 + i * 2.0 ** -24, 0.5 + j * 2.0 ** -24], [12 * s, 12 * s], [24 * s, 24 * s]]
            parts.append(np.array(abc + [[1.0, 20 * s], [6 * s, 30 * s]]))
            parts.append(np.array(abc + [[20 * s, 1.0], [30 * s, 6 * s]]))
    return _scene(parts, 43)


def ladder(reverse=False):
    return GS.boundaries(TILE, reverse)


def scenes():
    """every scene the device test compares area and rectangle on"""
    yield "ladder", ladder()
    yield "ladder reversed", ladder(True)
    yield "all vertices", all_vertices()
    yield "parabolas", parabolas()
    yield "lattices", lattice_scene()
    yield "near collinear", near_collinear()
    yield "slots", GS.slots()
    yield "chain", GS.chain()
