"""The scenes of the group geometry tests (no test inside): built once, shared by tests/test_group_terms_host.py, which
measures the eigen-solve's residuals on them on the CPU, and tests/test_gpu_group_stats.py, which runs them on the
device.  Each scene is (points float32 (n, 3), ids int64, sizes int64)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as CO  # noqa: E402

f32 = np.float32
TILE = 1024  # pcgx_group_stats_tile(); the device test asserts that it is


def boundary_sizes(T=TILE):
    """groups across every boundary of the kernels: the wave's row of 64 slots, the workgroup's tile of T, a group over
    four tiles, runs of empty groups, and a group that ends exactly where a tile ends, the next one starting there"""
    sizes = [0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 0, 0, 0]
    sizes.append(T - sum(sizes) % T)  # the filler: the list now ends on a tile boundary
    assert sum(sizes) % T == 0
    sizes += [7, 130, 0, 0, 1, 257 + 4 * 64, 5]  # (257 + 256: more than kGsLaneRows rows, not a tile)
    return np.array(sizes, np.int64)


@functools.lru_cache(maxsize=None)
def boundaries(T=TILE, reverse=False):
    sizes = boundary_sizes(T)
    rng = np.random.default_rng(19)
    n = int(sizes.sum()) + 500
    pts = (rng.uniform(-1, 1, (n, 3)) * [4, 2, 1] + [30, -20, 10]).astype(f32)
    ids = rng.permutation(n)[: int(sizes.sum())].astype(np.int64)
    if reverse:
        parts = np.split(ids, np.cumsum(sizes)[:-1])[::-1]
        ids, sizes = np.concatenate(parts), sizes[::-1].copy()
    return pts, ids, sizes


ROT = None


def rotation():
    """a fixed proper rotation (Rodrigues, axis (1, 2, 3) / sqrt(14), angle 0.7): its columns are the lattices' axes"""
    global ROT
    if ROT is None:
        k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        ROT = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)
    return ROT


SHIFT = np.array([60.0, -64.0, 48.0])  # 100 units from the origin
LATTICES = [(9, 5, 3), (33, 17, 5), (17, 9, 1)]  # unit spacing: half-extents (4, 2, 1), (16, 8, 2), and a flat patch (8, 4, 0)


@functools.lru_cache(maxsize=None)
def lattices():
    """-> points, ids, sizes, half-extents (3, 3); every lattice rotated by rotation(), then moved by SHIFT"""
    parts, half = [], []
    for nx, ny, nz in LATTICES:
        g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
        g = g - (np.array([nx, ny, nz]) - 1) / 2.0
        parts.append((g @ rotation().T + SHIFT).astype(f32))
        half.append([(nx - 1) / 2.0, (ny - 1) / 2.0, (nz - 1) / 2.0])
    pts = np.concatenate(parts)
    sizes = np.array([len(p) for p in parts], np.int64)
    rng = np.random.default_rng(23)
    ids = np.concatenate([o + rng.permutation(len(p)) for o, p in zip(np.cumsum([0] + [len(p) for p in parts[:-1]]), parts)])
    return pts, ids.astype(np.int64), sizes, np.array(half)


CHAIN_RADIUS = 0.032


def chain_cloud():
    from pcgol_amd import synth
    return synth.uniform_cloud(20_000, 1.0, 71)  # tests/test_gpu_clusters.py's cloud


@functools.lru_cache(maxsize=None)
def chain():
    """the clusters of the 20 000-point cloud at r = 0.032 by the NumPy oracle: 3070 clusters, the largest 1754"""
    pts = chain_cloud()
    _, c, sizes, ids = CO.clusters(pts, CHAIN_RADIUS)
    sizes = sizes[:c]
    return pts, ids[: int(sizes.sum())], sizes


@functools.lru_cache(maxsize=None)
def slots():
    """a small cloud with a NaN point (id 7) and an infinite one (id 11) among its members, a repeated id and a
    group that lists one id five times"""
    rng = np.random.default_rng(29)
    pts = (rng.uniform(-1, 1, (300, 3)) * [3, 1, 0.25] + [5, 5, -2]).astype(f32)
    pts[7, 1] = np.nan
    pts[11, 2] = -np.inf
    ids = np.concatenate([np.arange(0, 40), [50, 50, 51, 52, 50], [60] * 5, [7, 11], [7, 70, 71, 11, 72, 73, 73, 73],
                          np.arange(100, 300)]).astype(np.int64)
    sizes = np.array([40, 5, 5, 2, 8, 200], np.int64)
    assert sizes.sum() == len(ids)
    return pts, ids, sizes
