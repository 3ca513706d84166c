"""The NDT oracle (tests/ndt_oracle.py) pinned on the prototype scene and on hand cases; no GPU needed.

The scenes and the hand cases defined here are the ones the host test (test_ndt_terms_host.py) and the GPU tests
(test_gpu_ndt.py) run the library on; each is built once (lru_cache) and never changed.

Figures of the prototype scene (float64 oracle, 7 neighbours, outlier ratio 0.55, threshold -1): 105 occupied voxels,
100 valid, k2 = 0.756363; translation error 1.23e-1 at the identity, 8.0e-2 after one iteration, 1.0e-3 after 21 and
from there on (1.02e-3 after 30; its smallest value, 4.2e-4, is passed at iteration 12: the two samplings' optimum is
not the truth pose).  With the single containing voxel it stalls at 1.0e-2; with 27 voxels it reaches 5.9e-4.  At the
truth pose the omega-weighted mean gradient is O(1) (largest component 2.0), against 4.5e2 at the identity: the
Mahalanobis gradient scales with 1 / l', and the default flat threshold 0.01 is met only near the optimum (16
iterations from the identity)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndt_oracle as NO  # noqa: E402

f32, f64 = np.float32, np.float64
ALL_RUN = np.full(6, -1, f32)  # threshold -1: every iteration runs

# pinned: the oracle's own figures on the prototype scene
PROTO_OCCUPIED, PROTO_VALID = 105, 100
PROTO_K2 = 0.7563627375996009
PROTO_ERR_21 = 1.00e-3   # translation error after 21 iterations, 7 neighbours
PROTO_ERR_30 = 1.02e-3   # ... after 30
PROTO_ERR_30_ONE = 1.02e-2   # ... with the single containing voxel
PROTO_ERR_30_27 = 5.92e-4    # ... with the 27 voxels


@functools.lru_cache(maxsize=None)
def prototype():
    sc = NO.prototype_scene()
    sc["map"] = NO.build_map(sc["grid"], sc["base"])
    return sc


@functools.lru_cache(maxsize=None)
def prototype_trace(neighbors=7, iters=30):
    """The oracle's Fit on the prototype scene, every iteration run: the poses after 1 ... iters iterations"""
    sc = prototype()
    trace = []
    r = NO.fit(sc["map"], sc["target"], neighbors, 0.55, threshold=ALL_RUN, max_iter=iters, trace=trace)
    poses = [t for t, _ in trace[1:]] + [r["trans"]]
    return dict(poses=poses, first=trace[0][1], result=r)


HAND_MIN_POINTS, HAND_RATIO = 6, 0.01
HAND_GRID = dict(resolution=1.0, size=(4, 3, 3), origin=(0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def hand_scene():
    """One grid of 4 x 3 x 3 voxels of edge 1 (voxel v is centred on v), filled by hand:
      (0,0,0) min_points - 1 points: invalid     (1,0,0) exactly min_points points: valid
      (2,0,0) eight coincident points: invalid   (3,0,0) seven collinear points: valid, l0 = l1 = ratio l2
      (0,1,0) a 3 x 3 coplanar lattice: valid, l0 = ratio l2      (3,2,2), (0,0,1), (3,1,0): general, valid
    plus a point outside the grid, a NaN and an Inf point, which belong to no voxel.  Voxel (3,0,0) has address 3 and
    (0,1,0) address 4: each is the other's neighbour by address, not in space."""
    rng = np.random.default_rng(5)

    def blob(v, k):
        return (np.asarray(v, f64) + rng.uniform(-0.4, 0.4, (k, 3))).astype(f32)

    line = np.array([3.0, 0.0, 0.0]) + np.outer(np.linspace(-0.3, 0.3, 7), [0.6, 0.64, 0.48])
    u, w = np.array([0.8, 0.0, 0.6]), np.array([0.0, 1.0, 0.0])
    lat = np.array([0.0, 1.0, 0.0]) + np.array([a * u + b * w for a in (-0.25, 0.0, 0.25) for b in (-0.3, 0.0, 0.3)])
    parts = [blob((0, 0, 0), HAND_MIN_POINTS - 1), blob((1, 0, 0), HAND_MIN_POINTS),
             np.tile(f32([2.1, -0.2, 0.3]), (8, 1)), line.astype(f32), lat.astype(f32), blob((3, 2, 2), 9),
             blob((0, 0, 1), 12), blob((3, 1, 0), 10),
             f32([[10.0, 10.0, 10.0], [np.nan, 0.0, 0.0], [np.inf, 1.0, 1.0]])]
    pts = np.ascontiguousarray(np.concatenate(parts), f32)
    pts = pts[np.random.default_rng(6).permutation(len(pts))]
    grid = NO.Grid(**HAND_GRID)
    # targets: one inside every valid voxel, two on the x borders, one outside, a NaN and a +Inf
    target = f32([[1.1, 0.1, -0.1], [3.05, 0.02, 0.01], [0.02, 1.03, 0.01], [3.1, 2.1, 1.9], [0.1, -0.1, 1.1],
                  [3.2, 1.1, 0.1], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-1.7, 0.0, 0.0], [9.0, 0.0, 0.0],
                  [np.nan, 0.5, 0.5], [np.inf, 0.5, 0.5], [0.5, 0.5, np.inf]])
    return dict(grid=grid, base=pts, target=target, map=NO.build_map(grid, pts, HAND_MIN_POINTS, HAND_RATIO))


@functools.lru_cache(maxsize=None)
def fat_scene():
    """One voxel of 5000 points (several strides of a wave) beside two ordinary ones"""
    rng = np.random.default_rng(9)
    grid = NO.Grid(0.5, (3, 2, 2), (1.0, -1.0, 0.25))
    c = grid.centre((1, 1, 0))
    pts = [c + rng.normal(0, 0.07, (5000, 3)) * [1.0, 0.4, 0.1], grid.centre((0, 0, 0)) + rng.uniform(-0.2, 0.2, (40, 3)),
           grid.centre((2, 1, 1)) + rng.uniform(-0.2, 0.2, (70, 3))]
    pts = np.ascontiguousarray(np.concatenate(pts), f32)
    target = (c + rng.normal(0, 0.1, (300, 3))).astype(f32)
    return dict(grid=grid, base=pts, target=target, map=NO.build_map(grid, pts))


@functools.lru_cache(maxsize=None)
def single_voxel_scene():
    rng = np.random.default_rng(10)
    grid = NO.Grid(2.0, (1, 1, 1), (5.0, 5.0, 5.0))
    pts = (5.0 + rng.uniform(-0.9, 0.9, (50, 3))).astype(f32)
    target = (5.0 + rng.uniform(-1.2, 1.2, (64, 3))).astype(f32)
    return dict(grid=grid, base=pts, target=target, map=NO.build_map(grid, pts))


def map_scenes():
    """name -> scene, for the map comparisons (min_points, ratio: the scene's, default 6 / 0.01)"""
    return dict(prototype=prototype(), hand=hand_scene(), fat=fat_scene(), single=single_voxel_scene())


def scene_params(name):
    return (HAND_MIN_POINTS, HAND_RATIO) if name == "hand" else (6, 0.01)


@functools.lru_cache(maxsize=None)
def order_sensitivity(name):
    """How far the oracle's cov6 / icov6 move, as a fraction of the voxel's largest entry, when each voxel's sums are
    dealt to 64 accumulators and merged"""
    sc = map_scenes()[name]
    mp, ratio = scene_params(name)
    other = NO.build_map(sc["grid"], sc["base"], mp, ratio, parts=64)
    v = sc["map"]["valid"] != 0
    worst = 0.0
    for k in ("cov6_64", "icov6_64"):
        a, b = sc["map"][k][v], other[k][v]
        if len(a):
            worst = max(worst, float(np.max(np.abs(a - b).max(axis=1) / np.abs(a).max(axis=1))))
    return worst


def map_delta(name):
    """The map tolerance's delta: max(4 x the measured order sensitivity, 64 / min_eigen_ratio * 2^-53)"""
    return max(4.0 * order_sensitivity(name), 64.0 / scene_params(name)[1] * 2.0 ** -53)


def check_map(got, ref, delta, what):
    """got: dict(addr, count, valid, mean, cov6, icov6) of the library (or the header on the host); ref: the oracle's."""
    assert np.array_equal(got["addr"], ref["addr"]), what
    assert np.array_equal(got["count"], ref["count"]), what
    assert np.array_equal(got["valid"], ref["valid"]), what
    if len(ref["addr"]) == 0:
        return
    assert np.all(np.abs(got["mean"].astype(f64) - ref["mean"].astype(f64)) <= np.spacing(np.abs(ref["mean"]))), what
    for k in ("cov6", "icov6"):
        r64 = ref[k + "_64"]
        bound = 2.0 ** -23 * np.abs(r64) + delta * np.abs(r64).max(axis=1, keepdims=True)
        err = np.abs(got[k].astype(f64) - r64)
        assert np.all(err <= bound), (what, k, float(np.max(err - bound)))
    inv = ref["valid"] == 0
    assert np.all(got["cov6"][inv] == 0) and np.all(got["icov6"][inv] == 0), what


def test_prototype_figures():
    sc = prototype()
    m = sc["map"]
    assert len(m["addr"]) == PROTO_OCCUPIED and int(m["valid"].sum()) == PROTO_VALID
    assert NO.k2_of(0.55, 0.5) == PROTO_K2
    tr = prototype_trace()
    errs = [NO.translation_error(p, sc["truth"]) for p in tr["poses"]]
    assert tr["result"]["num_iteration"] == 30
    assert abs(NO.translation_error(NO.IDENTITY, sc["truth"]) - 1.23e-1) < 1e-3
    assert abs(errs[0] - 8.0e-2) < 1e-3
    assert abs(errs[20] - PROTO_ERR_21) < 2e-5 and abs(errs[29] - PROTO_ERR_30) < 2e-5
    assert min(errs) == errs[11] and abs(errs[11] - 4.2e-4) < 2e-5
    # the first gradient does not fade with the weights: sum omega is 1.28 over 13560 pairs
    first = tr["first"]
    assert first["pairs"] == 13560 and abs(first["sums"][NO.P_WEIGHT] - 1.2828) < 1e-3
    assert np.max(np.abs(NO.finish(first["sums"])["gradient"])) > 100.0


def test_prototype_other_neighbourhoods():
    sc = prototype()
    e1 = NO.translation_error(prototype_trace(1)["poses"][-1], sc["truth"])
    e27 = NO.translation_error(prototype_trace(27)["poses"][-1], sc["truth"])
    assert abs(e1 - PROTO_ERR_30_ONE) < 2e-4   # the single containing voxel stalls ten times further out
    assert abs(e27 - PROTO_ERR_30_27) < 2e-5


def test_prototype_default_threshold_and_truth_start():
    sc = prototype()
    r = NO.fit(sc["map"], sc["target"], 7, 0.55)
    assert r["num_iteration"] == 16 and NO.translation_error(r["trans"], sc["truth"]) < 1e-3
    # at the truth pose the gradient is O(1): a flat test of 10 holds there at once, and fails at the identity
    s = NO.sums(sc["map"], sc["target"], sc["truth"], 7)
    g = NO.finish(s["sums"])["gradient"]
    assert 1.0 < np.max(np.abs(g)) < 3.0
    r = NO.fit(sc["map"], sc["target"], 7, 0.55, threshold=np.full(6, 10, f32), init=sc["truth"])
    assert r["num_iteration"] == 1 and np.array_equal(r["trans"], sc["truth"])


def _cell(m, grid, v):
    a = int(v[0] + (v[1] + v[2] * grid.size[1]) * grid.size[0])
    i = int(np.nonzero(m["addr"] == a)[0][0])
    return i


def test_hand_voxels():
    sc = hand_scene()
    m, g = sc["map"], sc["grid"]
    assert len(m["addr"]) == 8 and np.all(np.diff(m["addr"]) > 0)
    assert int(m["count"].sum()) == len(sc["base"]) - 3  # the outside point, the NaN and the Inf are nobody's
    few, enough, same = _cell(m, g, (0, 0, 0)), _cell(m, g, (1, 0, 0)), _cell(m, g, (2, 0, 0))
    assert m["count"][few] == HAND_MIN_POINTS - 1 and m["valid"][few] == 0
    assert m["count"][enough] == HAND_MIN_POINTS and m["valid"][enough] == 1
    assert m["count"][same] == 8 and m["valid"][same] == 0
    for i in (few, same):
        assert np.all(m["cov6"][i] == 0) and np.all(m["icov6"][i] == 0)
    assert np.array_equal(m["mean"][same], f32([2.1, -0.2, 0.3]))
    line, plane = _cell(m, g, (3, 0, 0)), _cell(m, g, (0, 1, 0))
    assert m["valid"][line] == 1 and m["valid"][plane] == 1
    ratio = f64(f32(HAND_RATIO))  # (the ratio is a float32 argument)
    el = np.linalg.eigvalsh(NO.sym6(m["cov6_64"][line])[0])
    assert np.all(np.abs(el[:2] / el[2] - ratio) <= 1e-12)  # collinear: both small eigenvalues sit on the floor
    ep = np.linalg.eigvalsh(NO.sym6(m["cov6_64"][plane])[0])
    assert abs(ep[0] / ep[2] - ratio) <= 1e-12 and ep[1] / ep[2] > 0.5
    for i in (line, plane):  # ... and the float32 records keep that to float32's rounding; icov is cov's inverse
        e32 = np.linalg.eigvalsh(NO.sym6(m["cov6"][i])[0])
        assert abs(e32[0] / e32[2] - HAND_RATIO) <= 1e-5
        prod = NO.sym6(m["cov6_64"][i])[0] @ NO.sym6(m["icov6_64"][i])[0]
        assert np.max(np.abs(prod - np.eye(3))) <= 1e-12
    # min_points below 3 counts as 3
    tiny = NO.voxel(f32([[0, 0, 0], [0.1, 0, 0]]), (0, 0, 0), min_points=1)
    assert tiny["valid"] == 0
    assert NO.voxel(f32([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]]), (0, 0, 0), min_points=1)["valid"] == 1


def test_hand_pairs_border_and_outside():
    sc = hand_scene()
    m, g = sc["map"], sc["grid"]
    p = sc["target"]
    ok, v, _ = g.addr(p)
    assert ok.tolist() == [True] * 8 + [False] * 5
    assert g.addr(f32([[-0.7, 0.0, 0.0]]))[0][0]   # (Go's truncation: f = -0.2 becomes voxel 0, as in the reference)
    cells = {tuple(g.coords(a)): i for i, a in enumerate(m["addr"]) if m["valid"][i]}
    for nb in (1, 7, 27):
        pi, vj = NO.pairs(m, p, nb)
        got = sorted(zip(pi.tolist(), vj.tolist()))
        want = []
        for i in np.nonzero(ok)[0]:
            for off in NO.offsets(nb):
                c = tuple(int(x) for x in v[i] + np.asarray(off))
                if c in cells:
                    want.append((int(i), cells[c]))
        assert got == sorted(want), nb
    # target 1 sits in voxel (3,0,0), address 3; address 4 is the valid voxel (0,1,0), which is NOT its +x neighbour,
    # and target 2 in (0,1,0) does not see (3,0,0) as its -x neighbour
    pi, vj = NO.pairs(m, p, 7)
    line, plane = _cell(m, g, (3, 0, 0)), _cell(m, g, (0, 1, 0))
    assert sorted(vj[pi == 1].tolist()) == sorted([line, _cell(m, g, (3, 1, 0))])
    assert sorted(vj[pi == 2].tolist()) == [plane]
    s = NO.sums(m, p, None, 7)
    assert s["pairs"] == len(pi) and s["sums"][NO.P_PAIRS] == len(pi)
    assert np.all(np.isfinite(s["sums"]))


def test_constants_and_arguments():
    assert NO.k2_of(0.0, 0.5) is None and NO.k2_of(1.0, 0.5) is None and NO.k2_of(-0.1, 0.5) is None
    assert NO.k2_of(np.nan, 0.5) is None
    assert NO.k2_of(0.55, 1.0) > 0
    with pytest.raises(ValueError):
        NO.offsets(5)


def test_empty_and_zero_targets():
    sc = single_voxel_scene()
    s = NO.sums(sc["map"], np.zeros((0, 3), f32), None, 27)
    assert s["pairs"] == 0 and np.all(s["sums"] == 0)
    with pytest.raises(NO.NotEnoughPairs):
        NO.fit(sc["map"], np.zeros((0, 3), f32))
    empty = NO.build_map(sc["grid"], np.zeros((0, 3), f32))
    assert len(empty["addr"]) == 0
    assert NO.sums(empty, sc["target"], None, 7)["pairs"] == 0


def test_order_sensitivity_is_far_below_the_map_tolerance():
    for name in map_scenes():
        s = order_sensitivity(name)
        print("order sensitivity of %s: %.3g (delta %.3g)" % (name, s, map_delta(name)))
        assert s < 1e-13, name   # measured: 1.5e-15 (prototype); the 64 / ratio * 2^-53 = 7.1e-13 term sets delta
        assert map_delta(name) == 64.0 / scene_params(name)[1] * 2.0 ** -53
