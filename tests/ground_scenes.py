"""Scenes for the ground segmentation tests: a hillside no plane holds, with things standing on it."""
import numpy as np

f32 = np.float32

HILL_CELL = 0.5
HILL_HALF = np.array([1, 2, 4, 8, 16], np.int32)
# slope 0.3, initial 0.15, max 2.5 over widths 3, 5, 9, 17, 33 cells of 0.5 m (segmentation.pmf_windows gives the same)
HILL_HEIGHT = np.array([0.15, 0.45, 0.75, 1.35, 2.5], f32)
HILL_ORIGIN = np.array([0.0, 0.0], f32)
HILL_DIMS = np.array([96, 64], np.int32)


def terrain(x, y):
    return 0.08 * x + 0.5 * np.sin(0.3 * y)


def _box(rng, x0, y0, lx, ly, top, wall_from, n_roof, n_wall):
    """a box standing on the terrain: its roof at `top` above the terrain under its centre, its walls from `wall_from`
    above the terrain under them"""
    zr = terrain(x0 + lx / 2, y0 + ly / 2) + top
    roof = np.stack([x0 + rng.random(n_roof) * lx, y0 + rng.random(n_roof) * ly, np.full(n_roof, zr)], axis=1)
    t = rng.random(n_wall) * 2 * (lx + ly)
    wx = np.where(t < lx, x0 + t, np.where(t < lx + ly, x0 + lx, np.where(t < 2 * lx + ly, x0 + (t - lx - ly), x0)))
    wy = np.where(t < lx, y0, np.where(t < lx + ly, y0 + (t - lx), np.where(t < 2 * lx + ly, y0 + ly, y0 + (t - 2 * lx - ly))))
    lo = terrain(wx, wy) + wall_from
    wz = lo + rng.random(n_wall) * (zr - lo)
    return np.concatenate([roof, np.stack([wx, wy, wz], axis=1)])


def hill(seed=7):
    """About 20k points on 48 m x 32 m: terrain z = 0.08 x + 0.5 sin(0.3 y) with 1 cm noise, none of it under an
    8 x 6 x 4 m building (roof plus walls from +0.3 m) or under a 4 x 2 x 1.5 m car, three 3 m poles of radius 0.15,
    the ids shuffled -> (points float32 (n, 3), is_terrain bool (n,))."""
    rng = np.random.default_rng(seed)
    n = 17000
    x, y = rng.random(n) * 48.0, rng.random(n) * 32.0
    under = ((x >= 10) & (x <= 18) & (y >= 10) & (y <= 16)) | ((x >= 30) & (x <= 34) & (y >= 20) & (y <= 22))
    x, y = x[~under], y[~under]
    ground = np.stack([x, y, terrain(x, y) + rng.normal(0.0, 0.01, len(x))], axis=1)
    things = [_box(rng, 10.0, 10.0, 8.0, 6.0, 4.0, 0.3, 1500, 1500), _box(rng, 30.0, 20.0, 4.0, 2.0, 1.5, 0.3, 400, 400)]
    for px, py in ((5.0, 25.0), (24.0, 6.0), (41.0, 14.0)):
        a, h = rng.random(150) * 2 * np.pi, rng.random(150) * 3.0
        things.append(np.stack([px + 0.15 * np.cos(a), py + 0.15 * np.sin(a), terrain(px, py) + h], axis=1))
    things = np.concatenate(things)
    pts = np.concatenate([ground, things]).astype(f32)
    is_terrain = np.arange(len(pts)) < len(ground)
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order]), is_terrain[order]
