"""GPU: farthest-point sampling at 1 000 000 surface points, count 64, against the oracle (64 NumPy passes over the
cloud): thousands of tiles, sixteen to a pick workgroup and four to a wave (a lane tests a tile), the early picks that
touch a large share of the tiles and the later ones that skip nearly all of them."""
import os
import sys

import numpy as np
import pytest

from pcgol_amd import kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_oracle as FO  # noqa: E402
from test_gpu_fps import _check, _plan  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def test_a_million_points():
    pts = np.ascontiguousarray(synth.surface_cloud(1_000_000, 30.0, 6)[0], f32)
    n = len(pts)
    p = _plan(n, 64)
    assert p["wg_tiles"] > 4 and p["workgroups"] > 64  # more tiles than a wave per workgroup, more workgroups than one
    t = kdtree.New(pts)
    want = FO.fps(pts, 64)
    assert want["n_ids"] == 64 and want["cover_sq"] > 0
    _check(t, 64, want, -1, "1M")
