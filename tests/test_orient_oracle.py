"""The NumPy oracle of consistent normal orientation (tests/orient_oracle.py) against itself: the literal simulation of
the rounds, run to completion, gives Kruskal's forest under the same edge order (the minimum spanning forest is unique
under a strict order, so this is an equality of edge sets); a sphere whose normals had every sign randomised comes out
with every normal outward under mode 1 with u = +z; the rounds needed stay within ceil(log2 n)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orient_oracle as OO  # noqa: E402

f32 = np.float32


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


@pytest.mark.parametrize("seed", range(20))
def test_rounds_run_to_completion_equal_kruskal(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(50, 401))
    pts = rng.uniform(0, 1, (n, 3)).astype(f32)
    nrm = _unit(rng, n)
    radius = float(rng.uniform(0.08, 0.3))
    usable, lo, hi, c = OO.graph(pts, nrm, radius)
    assert usable.all() and len(lo) > 0
    forest, rounds, n_open = OO.boruvka(n, lo, hi, c)
    assert n_open == 0
    assert np.array_equal(forest, OO.kruskal(n, lo, hi, c))
    assert rounds <= math.ceil(math.log2(n))
    # F_R for every R is a growing chain of subsets that ends in the forest
    prev = np.zeros(0, np.int64)
    for r in range(rounds + 1):
        part, done, left = OO.boruvka(n, lo, hi, c, rounds=r)
        assert done == r and np.isin(prev, part).all() and np.isin(part, forest).all()
        assert (left == 0) == (r == rounds)
        prev = part


def _sphere(n, seed):
    rng = np.random.default_rng(seed)
    out = _unit(rng, n)
    sign = np.where(rng.integers(0, 2, n) == 1, f32(-1), f32(1))
    return out.copy(), out, out * sign[:, None]


def test_a_sign_randomised_sphere_comes_out_outward():
    pts, outward, nrm = _sphere(2000, 7)
    res = OO.orient(pts, nrm, 0.15, mode=1, ref=(0, 0, 1))
    assert res["n_components"] == 1 and res["n_open"] == 0
    assert np.array_equal(res["normals_out"], outward)
    assert np.array_equal(res["flipped"] != 0, (nrm != outward).any(axis=1))
    assert res["rounds"] <= math.ceil(math.log2(len(pts)))
    # mode 2 from the centre: everything looks away from the viewpoint, so the vote turns the whole component inward
    inward = OO.orient(pts, nrm, 0.15, mode=2, ref=(0, 0, 0))
    assert np.array_equal(inward["normals_out"], -outward)
    # mode 0: the smallest id keeps its sign
    keep = OO.orient(pts, nrm, 0.15, mode=0)
    assert keep["flipped"][0] == 0 and np.array_equal(keep["normals_out"], outward * np.sign(nrm[0] @ outward[0]).astype(f32))


def test_unusable_points_take_no_part():
    rng = np.random.default_rng(3)
    pts = rng.uniform(0, 1, (120, 3)).astype(f32)
    nrm = _unit(rng, 120)
    pts[5] = np.nan
    pts[6, 1] = np.inf
    nrm[7] = 0
    nrm[8, 2] = np.nan
    res = OO.orient(pts, nrm, 0.3, mode=0, deleted=[9])
    for i in (5, 6, 7, 8, 9):
        assert res["component"][i] == -1 and res["flipped"][i] == 0
        assert np.array_equal(res["normals_out"][i].view(np.uint32), nrm[i].view(np.uint32))
    lo, hi = res["forest"]
    assert not np.isin([5, 6, 7, 8, 9], np.concatenate([lo, hi])).any()


def test_the_edge_order_is_the_sort():
    rng = np.random.default_rng(11)
    c = rng.choice(np.array([0.0, -0.0, 0.5, -0.5, 1.0, 0.25]), 200)
    lo = rng.integers(0, 20, 200)
    hi = lo + rng.integers(1, 20, 200)
    _, first = np.unique(np.stack([lo, hi]), axis=1, return_index=True)
    c, lo, hi = c[first], lo[first], hi[first]
    order = OO.edge_order(lo, hi, c)
    for a, b in zip(order[:-1], order[1:]):
        assert OO.edge_before(c[a], lo[a], hi[a], c[b], hi[b], lo[b])
        assert not OO.edge_before(c[b], lo[b], hi[b], c[a], lo[a], hi[a])
