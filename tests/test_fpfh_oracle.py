"""The FPFH oracle (tests/fpfh_oracle.py) itself, on the CPU: pairs worked by hand, the clamps, histograms summed two
ways, and the CONDITION the GPU tests (tests/test_gpu_fpfh.py) rest on -- on their scenes no pair is fragile at the
oracle's bands, so lo == hi everywhere and the count check is an equality."""
import os
import sys

import numpy as np

from pcgol_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_oracle as FO  # noqa: E402
import normals_oracle as NO  # noqa: E402

f32, f64 = np.float32, np.float64
S5, C5 = np.sin(0.5), np.cos(0.5)

# (ps, ns, pt, nt) -> the bins worked by hand, None where the pair is invalid
#   plane:   d = x, n1 = z, v = d x n1 = -y, w = n1 x v = x: f1 = atan2(0, 1) = 0, f2 = 0, f3 = 0: all 5.5 -> 5
#   tilt y:  nt = (0, s, c): a1 = a2 = 0, no swap; f2 = v . nt = -s = -0.479 -> 11 * 0.2603 = 2.86 -> 2; f1 = atan2(0, c) = 0
#   tilt x:  nt = (s, 0, c): a2 = s > a1 = 0: swapped, n1 = nt, d = -x, f3 = -s -> 2; v = d x n1 = (0, c, 0) -> y;
#            w = n1 x v = (-c, 0, s); f2 = v . ns = 0 -> 5; f1 = atan2(w . ns, n1 . ns) = atan2(s, c) = 0.5:
#            11 (0.5 + pi) / 2 pi = 6.375 -> 6
#   f1 = pi: nt = -z: w . nt = +0, n1 . nt = -1: atan2(+0, -1) = pi: 11 -> clamped to 10
HAND = [
    ("plane", (0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 0, 1), (5, 5, 5)),
    ("tilt y", (0, 0, 0), (0, 0, 1), (1, 0, 0), (0, S5, C5), (5, 2, 5)),
    ("tilt x", (0, 0, 0), (0, 0, 1), (1, 0, 0), (S5, 0, C5), (6, 5, 2)),
    ("f1 = pi", (0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 0, -1), (10, 5, 5)),
    ("itself", (1, 2, 3), (0, 0, 1), (1, 2, 3), (0, 0, 1), None),
    ("zero normal", (0, 0, 0), (0, 0, 0), (1, 0, 0), (0, 0, 1), None),
    ("NaN normal", (0, 0, 0), (0, 0, 1), (1, 0, 0), (0, np.nan, 1), None),
    ("inf normal", (0, 0, 0), (np.inf, 0, 1), (1, 0, 0), (0, 0, 1), None),
]


def hand_arrays():
    return tuple(np.array([h[k] for h in HAND], f32) for k in (1, 2, 3, 4))


def test_pairs_worked_by_hand():
    pb = FO.pair_bins(*hand_arrays())
    for k, h in enumerate(HAND):
        if h[5] is None:
            assert not pb["counted"][k] and not pb["sure"][k] and not pb["maybe"][k] and not pb["adm"][k].any(), h[0]
        else:
            assert pb["sure"][k] and pb["counted"][k] and not pb["fragile"][k], h[0]
            assert tuple(pb["bins"][k]) == h[5], (h[0], pb["bins"][k])
            assert np.array_equal(pb["adm"][k], FO._onehot(np.array(h[5]))), h[0]


def test_clamps_and_edges():
    x = np.array([[0.0, 11.0, 5.5], [-1e-3, 11.0 + 1e-3, 10.999], [3.0, 3.0 - 1e-12, 3.0 + 1e-12], [3.0 + 1e-6, 1e-12, 11 - 1e-12]])
    assert FO._bins(x).tolist() == [[0, 10, 5], [0, 10, 10], [3, 2, 3], [3, 0, 10]]
    adm = FO._admit(x)
    assert [sorted(np.nonzero(a)[0].tolist()) for a in adm.reshape(-1, 11)] == \
        [[0], [10], [5], [0], [10], [10], [2, 3], [2, 3], [2, 3], [3], [0], [10]]
    # f3 = +-1 means d parallel to n1: |v| = 0, the pair is invalid, or -- a rounding away -- may count, and then in the
    # clamped bin
    ps = np.zeros((2, 3), f32)
    pt = np.array([[1, 1e-20, 0], [-1, 1e-20, 0]], f32)
    n = np.tile(np.array([1, 0, 0], f32), (2, 1))
    z = np.tile(np.array([0, 0, 1], f32), (2, 1))
    pb = FO.pair_bins(ps, n, pt, z)
    assert pb["maybe"].all() and pb["fragile"].all() and not pb["sure"].any()
    assert np.nonzero(pb["adm"][0, 2])[0].tolist() == [10] and np.nonzero(pb["adm"][1, 2])[0].tolist() == [0]
    assert pb["adm"][:, :2].all()
    exact = FO.pair_bins(ps, n, np.array([[1, 0, 0], [-1, 0, 0]], f32), z)
    assert not exact["counted"].any() and not exact["sure"].any()


def test_fragile_pairs_are_flagged():
    ps = np.zeros((1, 3), f32)
    z = np.array([[0, 0, 1]], f32)
    # an edge: d = (6, 6, 7) has |d| = 11, so a1 = z . d / |d| = 7 / 11 and 11 (a1 + 1) / 2 = 9 to a rounding
    pb = FO.pair_bins(ps, z, np.array([[6, 6, 7]], f32), np.array([[1, 0, 0]], f32))
    assert pb["sure"][0] and pb["fragile"][0]
    assert np.nonzero(pb["adm"][0, 2])[0].tolist() == [8, 9] and pb["adm"][0].sum() == 4
    # (with nt = ns = z instead, a1 == a2 is a swap tie as well, and f3 = -a2 of the swapped triple is admissible too)
    both = FO.pair_bins(ps, z, np.array([[6, 6, 7]], f32), z)
    assert np.nonzero(both["adm"][0, 2])[0].tolist() == [1, 2, 8, 9]
    # a swap tie with a1 = -a2 and unit normals: both role assignments give the same triple (the Darboux frame's
    # symmetry -- spheres, convex shapes), and the pair is not fragile
    pt = np.array([[1, 0, 0]], f32)
    ns = np.array([[S5, 0, C5]], f32)
    nt = np.array([[-S5, C5 * S5, C5 * C5]], f32)
    unit = FO.pair_bins(ps, ns, pt, nt)
    assert unit["sure"][0] and not unit["fragile"][0] and unit["adm"][0].sum() == 3


def _surface(n=500):
    return synth.surface_cloud(n, 0.7, 6)


def test_histograms_summed_two_ways():
    P, N = _surface(500)
    r = 0.1
    offs, ids = NO.brute_force_lists(P, P, r)
    res = FO.fpfh(P, N, np.arange(len(P)), offs, ids)
    assert res["n_valid"] > 10_000
    # pair by pair, in Python
    c2 = np.zeros((len(P), 3, 11), np.int64)
    m2 = np.zeros(len(P), np.int64)
    for q in range(len(P)):
        nb = ids[offs[q]:offs[q + 1]]
        pb = FO.pair_bins(np.tile(P[q], (len(nb), 1)), np.tile(N[q], (len(nb), 1)), P[nb], N[nb])
        for k in np.nonzero(pb["counted"])[0]:
            for f in range(3):
                c2[q, f, pb["bins"][k, f]] += 1
            m2[q] += 1
    assert np.array_equal(res["counts"], c2) and np.array_equal(res["pairs"], m2)
    assert np.array_equal(m2, np.diff(offs) - 1)  # everybody but the point itself
    assert np.all(res["lo"] <= res["counts"]) and np.all(res["counts"] <= res["hi"])
    # FPFH from the definition, query by query
    S = FO.spfh_values(c2, m2)
    for q in range(0, len(P), 7):
        nb = ids[offs[q]:offs[q + 1]]
        nb = nb[nb != q]
        w = 1.0 / NO.dist_sq_f32(P[nb], P[q]).astype(f64)
        W = (w[:, None] * S[nb]).sum(axis=0).reshape(3, 11)
        F = S[q].reshape(3, 11) + 100.0 * W / W.sum(axis=1, keepdims=True)
        assert np.allclose(res["fpfh"][q], F.reshape(-1), rtol=1e-13, atol=0)
        assert np.allclose(F.sum(axis=1), 200.0, rtol=1e-12)


def test_isolated_points_and_zero_normals():
    P, N = _surface(300)
    P = np.concatenate([P, np.array([[50, 50, 50], [60, 60, 60]], f32)])
    N = np.concatenate([N, np.array([[0, 0, 1], [0, 0, 1]], f32)])
    N[:10] = 0
    offs, ids = NO.brute_force_lists(P, P, 0.1)
    res = FO.fpfh(P, N, np.arange(len(P)), offs, ids)
    assert np.all(res["pairs"][-2:] == 0) and np.all(res["fpfh"][-2:] == 0)
    assert np.all(res["pairs"][:10] == 0) and np.all(res["counts"][:10] == 0)
    assert np.all(res["m_lo"] == res["m_hi"])


def scenes():
    """The GPU tests' scenes (tests/test_gpu_fpfh.py): name -> (points, normals, radius)."""
    out = {}
    P, N = synth.surface_cloud(3000, 1.65, 6)
    out["surface"] = (P, N, 0.1)
    rng = np.random.default_rng(41)
    u = rng.standard_normal((3000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    out["sphere"] = (np.ascontiguousarray(0.5 * u, f32), np.ascontiguousarray(u, f32), 0.1)
    v = np.random.default_rng(42).standard_normal((3000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    out["cube"] = (synth.uniform_cloud(3000, 0.5, 3), np.ascontiguousarray(v, f32), 0.06)
    g = np.arange(40, dtype=f64) / 32.0
    L = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    L = np.concatenate([L, np.full((len(L), 1), 0.25)], axis=1)
    out["lattice"] = (np.ascontiguousarray(L, f32), np.tile(np.array([0, 0, 1], f32), (len(L), 1)), 0.1)
    return out


def test_scenes_have_no_fragile_pairs():
    """THE CONDITION: fragile pairs at most 1 in 1e5 valid ones, queries out of the float check at most 1 %.  On these
    scenes there is none at all, so the GPU tests' count checks are equalities."""
    for name, (P, N, r) in scenes().items():
        offs, ids = NO.brute_force_lists(P, P, r)
        res = FO.fpfh(P, N, np.arange(len(P)), offs, ids)
        print(name, "valid pairs", res["n_valid"], "fragile", res["n_fragile"], "per point", res["n_valid"] / len(P))
        assert res["n_valid"] > 20_000, name
        assert res["n_fragile"] <= FO.MAX_FRAGILE_SHARE * res["n_valid"], (name, res["n_fragile"])
        assert (~res["float_ok"]).sum() <= FO.MAX_LEFT_OUT * len(P), name
        assert res["n_fragile"] == 0 and np.array_equal(res["lo"], res["hi"]) and np.array_equal(res["lo"], res["counts"]), name
        if name == "lattice":  # every pair exactly mid-bin
            assert np.all(res["counts"][:, :, 5] == res["pairs"][:, None])
