"""The float64 moving-least-squares oracle (tests/mls_oracle.py) pinned on the noisy surface scene and on cases worked
by hand: it is the contract the GPU kernel (csrc/mls.hip) and the host build of csrc/mls_terms.h are compared with.

Measured with this oracle on the noisy surface (synth.surface_cloud(3000, 2.0, 21) displaced along its analytic
normals by 0.01 N(0, 1), radius = sigma = 0.15, 47.5 neighbours on average): all 3000 points take the polynomial, the
smallest relative eigen-gap is 0.0708, the smallest pivot ratio 0.034 (0.026 with another eigen-solver's u, v: the
pivots depend on the frame), and the RMS distance of the interior points to the true surface falls by a factor 3.79.

The last test bounds what the order of summation moves, on every scene tests/test_gpu_mls.py uses, by a quarter of the
GPU tolerance: the tolerance and the "good" filter fit the inputs before a GPU is asked."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mls_oracle as MO  # noqa: E402
import normals_oracle as NO  # noqa: E402

f32 = np.float32
R = 0.15  # the surface scene's radius and sigma

_CACHE = {}


def surface_scene():
    """(noisy points, queries = 500 inside the box + 50 outside, lists of the own points, lists of the queries)"""
    if "surface" not in _CACHE:
        noisy = MO.noisy_surface()[0]
        q = MO.surface_queries(noisy)
        _CACHE["surface"] = (noisy, q, NO.brute_force_lists(noisy, noisy, R), NO.brute_force_lists(noisy, q, R))
    return _CACHE["surface"]


def surface_own_reference():
    if "own" not in _CACHE:
        noisy, _, own, _ = surface_scene()
        _CACHE["own"] = MO.mls_from_lists(noisy, noisy, *own, R)
    return _CACHE["own"]


def lattice():
    """9 x 9 points on the plane z = 0.5, spacing 1/16: every coordinate exact in float32"""
    k = np.arange(9, dtype=f32) / f32(16)
    x, y = np.meshgrid(k, k, indexing="ij")
    return np.ascontiguousarray(np.column_stack([x.ravel(), y.ravel(), np.full(81, 0.5, f32)]), dtype=f32)


def hand_cases():
    """[dict(name, points, queries, radius, sigma, order, min_neighbors, kinds)]: `kinds` the expected kind of every
    query, or a tuple of admissible kinds.  Shared with tests/test_mls_terms_host.py and tests/test_gpu_mls.py."""
    lat = lattice()
    line_x = np.zeros((41, 3), f32)
    line_x[:, 0] = np.arange(41, dtype=f32) / f32(64)
    line_x += f32([0.25, 0.5, 0.75])
    t = np.linspace(0, 1, 101, dtype=f32)
    line_o = np.ascontiguousarray(t[:, None] * (f32([1, 2, 2]) / f32(3))[None, :], dtype=f32)
    few = f32([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [0.01, 0.01, 0.001], [0.005, 0.002, 0]])
    heap = np.tile(f32([[0.3, 0.2, 0.1]]), (50, 1))
    cases = [
        dict(name="two neighbours", points=few[:2], queries=f32([[0.004, 0.004, 0]]), kinds=[0]),
        dict(name="no neighbour", points=few, queries=f32([[5, 5, 5]]), kinds=[0]),
        dict(name="coincident heap", points=heap, queries=f32([[0.3, 0.2, 0.1], [0.31, 0.2, 0.1]]), kinds=[0, 0]),
        dict(name="three neighbours", points=few[:3], queries=f32([[0.004, 0.004, 0]]), kinds=[1]),
        dict(name="four neighbours", points=few[:4], queries=f32([[0.004, 0.004, 0]]), kinds=[1]),
        dict(name="five neighbours", points=few, queries=f32([[0.004, 0.004, 0]]), kinds=[1]),
        dict(name="five neighbours, six asked for", points=few, queries=f32([[0.004, 0.004, 0]]), min_neighbors=6, kinds=[0]),
        dict(name="coplanar lattice", points=lat, radius=0.2,
             queries=np.concatenate([lat[[40, 0, 8, 44]], f32([[0.26, 0.24, 0.53], [0.3, 0.3, 0.45]])]), kinds=[2] * 6),
        # a line along x: d has exact zeros, so one of u, v is exactly perpendicular to every neighbour, its coordinate
        # exactly 0 and M_11 or M_22 exactly 0: the solve fails whatever the eigen-solver.  (On an oblique line that
        # coordinate is rounding noise, and so is its pivot: either kind, the next case.)
        dict(name="collinear along x, own points", points=line_x, queries=line_x[10:30], radius=0.125, kinds=[1] * 20),
        dict(name="collinear oblique, own points", points=line_o, queries=line_o[40:60], kinds=(1, 2)),
        dict(name="every weight underflows", points=lat, queries=f32([[0.28, 0.28, 0.5], [0.03, 0.22, 0.52]]), radius=0.2,
             sigma=1e-4, kinds=[1, 1]),
        dict(name="order 1 on the lattice", points=lat, queries=lat[[40, 0]], radius=0.2, order=1, kinds=[1, 1]),
    ]
    for c in cases:
        c.setdefault("radius", 0.1)
        c.setdefault("sigma", c["radius"])
        c.setdefault("order", 2)
        c.setdefault("min_neighbors", 3)
    return cases


def case_reference(c, **kw):
    return MO.mls(c["points"], c["queries"], c["radius"], c["sigma"], c["order"], c["min_neighbors"], **kw)


def check_case_kinds(c, kinds):
    if isinstance(c["kinds"], tuple):
        assert np.all(np.isin(kinds, c["kinds"])), (c["name"], kinds)
    else:
        assert kinds.tolist() == c["kinds"], (c["name"], kinds)


def test_noisy_surface_is_smoothed():
    noisy = surface_scene()[0]
    o = surface_own_reference()
    assert abs(o["counts"].mean() - 47.5) < 0.1
    assert np.all(o["kinds"] == MO.POLY)
    print("min gap %.4f, min pivot ratio %.4f" % (o["gap"].min(), o["pivot"].min()))
    assert o["gap"].min() >= 0.05
    assert o["pivot"].min() >= 0.02
    ratio, before, after = MO.rms_ratio(noisy, o["points"])
    print("interior RMS distance to the surface %.6f -> %.6f: ratio %.2f" % (before, after, ratio))
    assert ratio >= 3.0
    assert MO.good(o).all() and not MO.fragile(o, R).any()
    # the polynomial's normals are nearer the analytic ones than the noisy plane fits'
    _, _, nrm = MO.noisy_surface()
    sel = MO.interior(noisy)
    plane = MO.mls_from_lists(noisy, noisy, *surface_scene()[2], R, order=1)
    assert np.all(plane["kinds"] == MO.PLANE)

    def ang(n):
        return np.degrees(np.arccos(np.clip(np.abs(np.sum(n[sel].astype(np.float64) * nrm[sel], axis=1)), 0, 1)))
    assert np.median(ang(o["normals"])) < np.median(ang(plane["normals"])) + 0.5
    assert np.median(ang(o["normals"])) < 3.0


def test_queries_off_the_cloud():
    noisy, q, _, ql = surface_scene()
    o = MO.mls_from_lists(noisy, q, *ql, R)
    inside = MO.good(o)[:500]
    print("good inside queries: %d of 500" % inside.sum())
    assert inside.mean() >= 0.95
    assert np.all(o["kinds"][500:] == MO.UNCHANGED) and np.all(o["counts"][500:] == 0)
    assert np.array_equal(o["points"][500:].view(np.uint32), q[500:].view(np.uint32))
    assert np.all(o["normals"][500:] == 0)
    # the queries, up to 0.05 off the surface, land as near it as the cloud's own points do
    d = MO.surface_distance(o["points"][:500][MO.interior(q[:500])])
    assert np.sqrt(np.mean(d ** 2)) < 0.005


def test_hand_cases():
    for c in hand_cases():
        o = case_reference(c)
        check_case_kinds(c, o["kinds"])
        z = o["kinds"] == 0
        assert np.array_equal(o["points"][z].view(np.uint32), c["queries"][z].view(np.uint32)), c["name"]
        assert np.all(o["normals"][z] == 0), c["name"]
        assert np.allclose(np.linalg.norm(o["normals"][~z].astype(np.float64), axis=1), 1.0, atol=1e-6), c["name"]
        if c["order"] == 1:
            assert o["kinds"].max() <= 1
        if c["name"] == "coplanar lattice":
            assert np.all(np.abs(o["c0"]) <= 1e-12 * c["radius"])
            assert np.array_equal(np.abs(o["normals"]), np.tile(f32([0, 0, 1]), (6, 1)))
            assert np.all(o["normals"][:, 2] == -1)  # (the default viewpoint, the origin, is below z = 0.5)
            assert np.all(o["points"][:, 2] == f32(0.5))  # on the plane, the off-plane queries too
            assert np.array_equal(o["points"][:, :2], c["queries"][:, :2])
        if c["name"].startswith("collinear"):
            assert np.all(o["counts"] >= 6)
            assert np.max(np.abs(o["points"].astype(np.float64) - c["queries"])) <= 1e-6 * c["radius"]
        if c["name"] == "every weight underflows":
            assert np.all(o["pivot"] == 0.0) and np.all(o["points"][:, 2] == f32(0.5))
        if c["name"] == "five neighbours":
            assert o["counts"][0] == 5 and np.isnan(o["pivot"][0])  # (no solve was tried below 6 neighbours)


def test_nan_and_inf_queries_come_back_unchanged():
    lat = lattice()
    q = f32([[np.nan, 0.25, 0.5], [np.inf, 0.25, 0.5], [0.25, 0.25, 0.5]])
    with np.errstate(invalid="ignore"):
        o = MO.mls(lat, q, 0.2)
    assert o["kinds"].tolist() == [0, 0, 2] and o["counts"][:2].tolist() == [0, 0]
    assert np.array_equal(o["points"][:2].view(np.uint32), q[:2].view(np.uint32))


def test_order_one_never_exceeds_the_plane():
    noisy, q, own, ql = surface_scene()
    for pts, lists in ((noisy, own), (q, ql)):
        o = MO.mls_from_lists(noisy, pts, *lists, R, order=1)
        assert o["kinds"].max() == 1 and np.all(np.isnan(o["pivot"]))
    o2 = surface_own_reference()
    assert np.array_equal(o["counts"], MO.mls_from_lists(noisy, q, *ql, R)["counts"])
    assert o2["kinds"].max() == 2


def test_min_neighbors_and_sigma():
    noisy, _, own, _ = surface_scene()
    ref = surface_own_reference()
    mn = int(np.median(ref["counts"]))
    o = MO.mls_from_lists(noisy, noisy, *own, R, min_neighbors=mn)
    low = o["counts"] < mn
    assert low.any() and (~low).any()
    assert np.all(o["kinds"][low] == 0) and np.array_equal(o["points"][low].view(np.uint32), noisy[low].view(np.uint32))
    assert np.array_equal(o["points"][~low], ref["points"][~low])
    half = MO.mls_from_lists(noisy, noisy, *own, R, sigma=R / 2)
    assert np.all(half["kinds"] == 2) and not np.array_equal(half["points"], ref["points"])
    assert MO.rms_ratio(noisy, half["points"])[0] > 1.5  # (a narrower weight averages fewer points: less smoothing)


def _order_independence(points, queries, lists, radius, what, **kw):
    """the oracle with every list as given and in a seeded random order: within a quarter of the GPU tolerance"""
    a = MO.mls_from_lists(points, queries, *lists, radius, **kw)
    b = MO.mls_from_lists(points, queries, *lists, radius, order_rng=np.random.default_rng(77), **kw)
    assert np.array_equal(a["counts"], b["counts"])
    fr = MO.fragile(a, radius) | MO.fragile(b, radius)
    assert np.array_equal(a["kinds"][~fr], b["kinds"][~fr]), what
    g = MO.good(a) & (b["kinds"] == MO.POLY)
    assert np.all(fr[MO.good(a) & ~g]), what
    err = np.abs(a["points64"][g] - b["points64"][g])  # (before the rounding to float32, which would hide it)
    tol = MO.position_tolerance(a, radius)[g]
    worst = float(np.max(err / tol, initial=0.0))
    print("%s: two orders move a position by at most %.3g radius" % (what, float(np.max(err, initial=0.0)) / radius))
    na, nb = a["normals64"][g], b["normals64"][g]
    sin = float(np.max(np.linalg.norm(np.cross(na, nb), axis=1), initial=0.0))
    print("%s: %d good of %d, %d fragile; two orders differ by %.3g of the tolerance, normals by sin %.3g"
          % (what, int(g.sum()), len(queries), int(fr.sum()), worst, sin))
    assert worst <= 0.25 and sin <= 0.25e-6, what
    return a, g, fr


def test_summation_order_stays_within_a_quarter_of_the_gpu_tolerance_on_the_surface():
    noisy, q, own, ql = surface_scene()
    _order_independence(noisy, noisy, own, R, "surface, own points")
    _order_independence(noisy, q, ql, R, "surface, queries")
    _order_independence(noisy, noisy[:129], NO.brute_force_lists(noisy, noisy[:129], R), R, "surface, sigma r/2", sigma=R / 2)
    _order_independence(noisy, noisy[:129], NO.brute_force_lists(noisy, noisy[:129], R), R, "surface, order 1", order=1)


@pytest.mark.parametrize("radius", [0.75, 1.0])
def test_summation_order_stays_within_a_quarter_of_the_gpu_tolerance_on_the_heaps(radius):
    from test_gpu_radius_edges import _heap_queries, _heap_scene
    pts, q = _heap_scene(), _heap_queries(5)
    a, g, fr = _order_independence(pts, q, NO.brute_force_lists(pts, q, radius), radius, "heaps r=%g" % radius)
    fat = g & (a["counts"] >= 4096)
    print("good queries with a fat row: %d; smallest pivot ratio among them %.3g" % (fat.sum(), a["pivot"][fat].min()))
    assert fat.sum() >= 50  # the scene does its job: the wave-shared rows are compared, not filtered away
