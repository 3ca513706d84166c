"""The NumPy oracle of ground segmentation (tests/ground_oracle.py) on grids small enough to work by hand, the
properties every input has, and the purpose of the whole thing on the hill() scene: the terrain of a hillside is ground,
what stands on it is not, and it takes more than one window to say so.  No GPU: what tests/test_gpu_ground.py compares
the library with is checked here on its own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_oracle as GO  # noqa: E402
import ground_scenes as GS  # noqa: E402

f32 = np.float32
INF = f32(np.inf)


def _row(zs):
    """one point in the middle of each cell of a 1 x len(zs) grid of unit cells; None: an empty cell"""
    return np.array([[i + 0.5, 0.5, z] for i, z in enumerate(zs) if z is not None], f32)


def test_row_with_a_spike_and_a_hole():
    zs = [1.0, 1.0, 5.0, None, 1.0]
    pts = _row(zs)
    r = GO.ground(pts, (0, 0), (5, 1), 1.0, [1], [0.5])
    # erosion by 3: 1 1 1 1 1 (the hole takes no part; cell 3 sees 5 and 1); dilation: 1 everywhere, the hole included
    assert np.array_equal(r["surface"], np.full((1, 5), 1.0, f32))
    assert list(r["labels"]) == [0, 0, 1, 0] and list(r["window"]) == [-1, -1, 0, -1]
    assert list(r["sizes"]) == [3, 1] and list(r["ids"]) == [0, 1, 3, 2]
    assert np.array_equal(r["hag"], np.array([0, 0, 4, 0], f32))
    # without a window the surface is S_0: the hole is +inf and the spike is ground
    r0 = GO.ground(pts, (0, 0), (5, 1), 1.0, [], [])
    assert np.array_equal(r0["surface"], np.array([[1, 1, 5, INF, 1]], f32))
    assert list(r0["labels"]) == [0, 0, 0, 0] and list(r0["sizes"]) == [4, 0]


def test_empty_cells_stay_out_of_both_halves():
    # a hole wider than the window: its middle sees no cell with a point, in the erosion and in the dilation
    zs = [2.0, None, None, None, None, None, 3.0]
    r = GO.ground(_row(zs), (0, 0), (7, 1), 1.0, [1], [0.5])
    assert np.array_equal(r["surface"], np.array([[2, 2, 2, INF, 3, 3, 3]], f32))
    r = GO.ground(_row(zs), (0, 0), (7, 1), 1.0, [1, 3], [0.5, 0.5])
    # a window wider than the hole: the erosion is 2 up to cell 5, and the dilation brings the 3 back from cell 3 on
    assert np.array_equal(r["surface"], np.array([[2, 2, 2, 3, 3, 3, 3]], f32))


def test_window_wider_than_the_grid():
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.random((40, 2)) * [4, 3], rng.random((40, 1)) * 10], axis=1).astype(f32)
    r = GO.ground(pts, (0, 0), (4, 3), 1.0, [9], [0.25])
    lo = pts[:, 2].min()
    assert np.array_equal(r["surface"], np.full((3, 4), lo, f32))  # the opening of the whole grid: its minimum
    assert np.array_equal(r["labels"], (pts[:, 2] - lo >= f32(0.25)).astype(np.int64))


def test_signed_zeros_in_one_cell():
    pts = np.array([[0.5, 0.5, 0.0], [0.6, 0.5, -0.0], [0.7, 0.5, 0.0]], f32)
    r = GO.ground(pts, (0, 0), (1, 1), 1.0, [1], [1.0])
    assert r["surface"].view(np.uint32)[0, 0] == 0x80000000  # -0.0 lies below +0.0
    assert list(r["labels"]) == [0, 0, 0]
    assert GO.key(f32(-0.0)) < GO.key(f32(0.0)) and GO.unkey(GO.key(np.array([-0.0], f32))).view(np.uint32)[0] == 0x80000000


def test_not_live_points():
    pts = np.array([[0.5, 0.5, 1.0], [np.nan, 0.5, 1.0], [0.5, np.inf, 1.0], [0.5, 0.5, -np.inf], [-0.1, 0.5, 0.0],
                    [2.0, 0.5, 0.0], [0.5, -1e-3, 0.0], [0.5, 1.0, 0.0], [1.5, 0.5, 3.0]], f32)
    r = GO.ground(pts, (0, 0), (2, 1), 1.0, [1], [0.5])
    assert list(r["labels"]) == [0, -1, -1, -1, -1, -1, -1, -1, 1]
    assert list(r["ids"]) == [0, 8, -1, -1, -1, -1, -1, -1, -1]
    assert np.array_equal(r["hag"].view(np.uint32)[1:8], np.full(7, 0x7FC00000, np.uint32))
    d = GO.ground(pts, (0, 0), (2, 1), 1.0, [1], [0.5], deleted=[1, 0, 0, 0, 0, 0, 0, 0, 0])
    assert list(d["labels"]) == [-1] * 8 + [0] and np.array_equal(d["surface"], np.array([[3, 3]], f32))


def test_properties_on_random_inputs():
    rng = np.random.default_rng(11)
    for trial in range(6):
        nx, ny = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        n = int(rng.integers(1, 3000))
        pts = (rng.random((n, 3)) * [nx + 2, ny + 2, 20] - [1, 1, 10]).astype(f32)
        half = rng.integers(1, 12, 4)
        c, S = GO.surfaces(pts, (0, 0), (nx, ny), 1.0, half)
        for a, b in zip(S[:-1], S[1:]):
            full = a != GO.EMPTY
            assert np.all(b[full] <= a[full])  # S_{k+1} <= S_k cell by cell (an opening is anti-extensive)
            assert np.all(b[full] != GO.EMPTY)
        r = GO.ground(pts, (0, 0), (nx, ny), 1.0, half, [0.5, 1.0, 1.5, 2.0])
        live = c >= 0
        assert np.all(r["hag"][live] >= 0) and np.all(np.isnan(r["hag"][~live]))
        assert r["sizes"].sum() == live.sum() and np.all(r["ids"][live.sum():] == -1)


def test_the_hill():
    pts, is_terrain = GS.hill()
    assert 19000 < len(pts) < 22000
    r = GO.ground(pts, GS.HILL_ORIGIN, GS.HILL_DIMS, GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT)
    g = r["labels"] == 0
    terrain_kept = g[is_terrain].mean()
    things_kept = g[~is_terrain].mean()
    removed_at = np.unique(r["window"][r["window"] >= 0])
    one = GO.ground(pts, GS.HILL_ORIGIN, GS.HILL_DIMS, GS.HILL_CELL, [1], GS.HILL_HEIGHT[:1])
    things_kept_one = (one["labels"] == 0)[~is_terrain].mean()
    empty = np.isinf(GO.ground(pts, GS.HILL_ORIGIN, GS.HILL_DIMS, GS.HILL_CELL, [], [])["surface"]).mean()
    print("terrain kept %.4f, things kept %.4f, removed at windows %s, things kept by half = [1] alone %.4f, empty cells %.3f"
          % (terrain_kept, things_kept, list(removed_at), things_kept_one, empty))
    assert terrain_kept >= 0.99
    assert things_kept <= 0.05
    assert len(removed_at) >= 2
    assert things_kept_one > 0.20  # the progression is what removes the roofs
    # no plane within 0.15 m holds this terrain: the best least-squares plane leaves more than a fifth of it outside
    t = pts[is_terrain].astype(np.float64)
    A = np.c_[t[:, :2], np.ones(len(t))]
    res = t[:, 2] - A @ np.linalg.lstsq(A, t[:, 2], rcond=None)[0]
    assert (np.abs(res) > 0.15).mean() > 0.2
