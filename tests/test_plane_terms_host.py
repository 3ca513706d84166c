"""csrc/plane_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/plane_terms_host.cpp over the shim
tests/cpp/host_shim): the status, the plane, the refit and the inlier test the kernels of planes.hip compile give the
NumPy oracle's bits (tests/plane_oracle.py) on random triangles, coincident and collinear points, +-0, denormals, NaN and
infinities, normals with tied largest components, and the axis test at equality."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_oracle as PO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("plane_terms") / "libplane_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "plane_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def hypotheses(lib, tri, idx=None, axis=None, cos=0.0):
    tri = np.ascontiguousarray(tri, f32).reshape(-1, 9)
    m = len(tri)
    idx = np.ascontiguousarray(idx if idx is not None else np.tile([0, 1, 2], (m, 1)), np.uint32)
    ax = np.ascontiguousarray(axis, f32) if axis is not None else None
    st, pl = np.full(m, -9, np.int32), np.full((m, 4), 7, f32)
    lib.plane_hypothesis_batch(_p(tri), _p(idx), ctypes.c_int64(m), _p(ax), ctypes.c_float(cos), _p(st), _p(pl))
    return st, pl


def check_hypotheses(lib, tri, idx=None, axis=None, cos=0.0):
    tri = np.ascontiguousarray(tri, f32).reshape(-1, 3, 3)
    st, pl = hypotheses(lib, tri, idx, axis, cos)
    A = PO.Axis(axis, cos) if axis is not None else None
    for k, t in enumerate(tri):
        i = idx[k] if idx is not None else (0, 1, 2)
        with np.errstate(all="ignore"):
            ws, wp = PO.hypothesis(int(i[0]), int(i[1]), int(i[2]), t[0], t[1], t[2], A)
        assert st[k] == ws, (k, t, st[k], ws)
        assert np.array_equal(pl[k].view(np.uint32), wp.view(np.uint32)), (k, t, pl[k], wp)
    return st, pl


def test_status_codes(host):
    out = (ctypes.c_int32 * 5)()
    host.plane_status_codes(out)
    assert list(out) == [PO.NOT_RUN, PO.OK, PO.BAD_SAMPLE, PO.DEGENERATE, PO.AXIS] == [-1, 0, 1, 2, 3]


def test_random_triangles(host):
    rng = np.random.default_rng(5)
    tri = np.concatenate([rng.standard_normal((300, 9)) * s for s in (1e-3, 1.0, 50.0, 1e6)]).astype(f32)
    tri[::7, 3:6] += f32(1e4)  # far from the origin: d is large, the edges are small
    st, pl = check_hypotheses(host, tri)
    assert (st == PO.OK).sum() > 1000
    n = pl[st == PO.OK, :3].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-6)
    lead = np.take_along_axis(n, np.abs(n).argmax(axis=1)[:, None], 1)
    assert np.all(lead > 0)
    for axis, cos in (((0, 0, 1), 0.0), ((0, 0, 1), 0.9), ((1, -2, 0.5), 0.5), ((-3, 0, 0), 0.2)):
        st, pl = check_hypotheses(host, tri[:400], axis=axis, cos=cos)
        assert (st == PO.OK).any() and (cos == 0.0 or (st == PO.AXIS).any())
        assert np.all(pl[st == PO.OK, :3].astype(np.float64) @ np.asarray(axis, np.float64) >= 0)


def test_bad_samples_coincident_and_collinear(host):
    t = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], f32)
    for idx, want in (((4, 4, 9), PO.BAD_SAMPLE), ((4, 9, 4), PO.BAD_SAMPLE), ((9, 4, 4), PO.BAD_SAMPLE), ((1, 2, 3), PO.OK)):
        st, _ = check_hypotheses(host, t, idx=np.array([idx], np.uint32))
        assert st[0] == want
    deg = np.array([[1, 2, 3, 1, 2, 3, 4, 5, 6],           # two coincident points
                    [1, 2, 3, 1, 2, 3, 1, 2, 3],           # three
                    [0, 0, 0, 1, 1, 1, 2, 2, 2],           # collinear
                    [0, 0, 0, 1, 1, 1, 3, 3, 3.000001],    # nearly
                    [0, 0, 0, 1, 0, 0, 2, 1e-6, 0],        # sin^2 at 2.5e-13: below the 1e-12
                    [0, 0, 0, 1, 0, 0, 2, 4e-6, 0]], f32)  # 4e-12: above
    st, _ = check_hypotheses(host, deg)
    assert st.tolist() == [PO.DEGENERATE] * 5 + [PO.OK]


def test_zeros_denormals_and_non_finite(host):
    vals = np.array([0.0, -0.0, 1e-45, -3e-45, 1.1754942e-38, 1.0, -2.5, 3.4028235e38, np.inf, -np.inf, np.nan], f32)
    rng = np.random.default_rng(6)
    tri = vals[rng.integers(0, len(vals), (3000, 9))]
    tri[:500] = np.where(rng.random((500, 9)) < 0.5, tri[:500], rng.standard_normal((500, 9)).astype(f32))
    st, _ = check_hypotheses(host, tri)
    assert (st == PO.OK).any() and (st == PO.DEGENERATE).any()
    st, _ = check_hypotheses(host, tri[:600], axis=(0, 1e-40, -0.0), cos=0.5)
    assert set(st.tolist()) <= {PO.OK, PO.DEGENERATE, PO.AXIS}
    # a denormal triangle is a triangle: float64 holds its cross product
    st, pl = check_hypotheses(host, np.array([[0, 0, 0, 1e-45, 0, 0, 0, 3e-45, 0]], f32))
    assert st[0] == PO.OK and pl[0].tolist() == [0, 0, 1, 0]


def test_tied_components_and_both_sign_rules(host):
    base = []
    for n in itertools.product((-1.0, 0.0, 1.0), repeat=3):
        if not any(n):
            continue
        n = np.array(n)
        u = np.cross(n, [0.3, -0.7, 0.2] if abs(n[0]) + abs(n[1]) else [1, 0, 0])
        v = np.cross(n, u)
        base += [np.concatenate([np.zeros(3), u, v]), np.concatenate([np.zeros(3), v, u])]  # both windings
    tri = np.array(base, f32)
    st, pl = check_hypotheses(host, tri)
    ok = pl[st == PO.OK, :3]
    assert len(ok) >= 40
    for n in ok.astype(np.float64):
        assert n[int(np.abs(n).argmax())] > 0, n  # (argmax: the first of exactly equal ones)
    # exact ties, written down: (1, 1, 0) / sqrt 2 from either winding; (-1, 1, 0): the first of the tied ones decides
    t = np.array([[0, 0, 0, 1, -1, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1, 1, -1, 0], [0, 0, 0, 1, 1, 0, 0, 0, 1]], f32)
    st, pl = check_hypotheses(host, t)
    r = f32(np.sqrt(0.5))
    assert st.tolist() == [0, 0, 0]
    assert pl[0].tolist() == [r, r, 0, 0] and pl[1].tolist() == [r, r, 0, 0] and pl[2].tolist() == [r, -r, 0, 0]
    # with an axis: its side; perpendicular to it (the expression is 0): the rule without an axis
    st, pl = check_hypotheses(host, t, axis=(-1, -1, 0), cos=0.0)
    assert pl[0].tolist() == [-r, -r, 0, 0] and pl[2].tolist() == [r, -r, 0, 0]
    st, pl = check_hypotheses(host, t, axis=(0, 0, 5), cos=0.0)
    assert pl[0].tolist() == [r, r, 0, 0]


def test_axis_test_at_equality(host):
    flat = np.array([[0, 0, 1, 1, 0, 1, 0, 1, 1]], f32)  # n = (0, 0, 1) exactly, d = -1
    st, pl = check_hypotheses(host, flat, axis=(0, 0, 2), cos=1.0)  # |2| >= 1 * 2
    assert st[0] == PO.OK and pl[0].tolist() == [0, 0, 1, -1]
    st, pl = check_hypotheses(host, flat, axis=(0, 0, -2), cos=1.0)
    assert st[0] == PO.OK and pl[0].tolist() == [0, 0, -1, 1]
    st, _ = check_hypotheses(host, flat, axis=(0, 3, 4), cos=0.8)  # 4 against float64(float32(0.8)) * 5: just above 4
    assert st[0] == PO.AXIS
    st, _ = check_hypotheses(host, flat, axis=(0, 3, 4), cos=np.nextafter(f32(0.8), f32(0)))
    assert st[0] == PO.OK
    st, _ = check_hypotheses(host, flat, axis=(0, 3, 4), cos=0.75)  # 0.75 * 5 = 3.75 exactly
    assert st[0] == PO.OK
    st, _ = check_hypotheses(host, flat, axis=(3, 4, 0), cos=0.0)  # perpendicular: 0 >= 0
    assert st[0] == PO.OK
    st, _ = check_hypotheses(host, flat, axis=(3, 4, 0), cos=1e-45)
    assert st[0] == PO.AXIS
    a = np.array([0.3, -0.2, 0.7], f32)
    dot = float(a[2]) / float(PO.Axis(a, 0).norm)
    for c in (np.nextafter(f32(dot), f32(0)), f32(dot), np.nextafter(f32(dot), f32(1))):
        check_hypotheses(host, flat, axis=a, cos=float(c))


def test_refit(host):
    rng = np.random.default_rng(8)
    m = 400
    fr = np.zeros((m, 7))
    fr[:, :3] = rng.standard_normal((m, 3)) * 10
    a = rng.standard_normal((m, 3))
    fr[:, 3:6] = a / np.linalg.norm(a, axis=1)[:, None]
    fr[:, 6] = rng.random(m)
    fr[::9, 6] = 0.0                      # the degenerate frame
    fr[1::9, 3:6] = [[0, 0, 1]]           # identity axes
    fr[2::9, 3:6] = [[-np.sqrt(0.5), np.sqrt(0.5), 0]]
    fr[3, 6] = np.nan
    for axis, cos in ((None, 0.0), ((0, 0, 1), 0.7), ((0, -1, 0), 0.0)):
        ax = np.ascontiguousarray(axis, f32) if axis is not None else None
        ok, pl = np.full(m, -9, np.int32), np.full((m, 4), 7, f32)
        host.plane_refit_batch(_p(fr), ctypes.c_int64(m), _p(ax), ctypes.c_float(cos), _p(ok), _p(pl))
        A = PO.Axis(axis, cos) if axis is not None else None
        for k in range(m):
            wok, wpl = PO.refit(fr[k, :3], fr[k, 3:6], fr[k, 6], A)
            assert bool(ok[k]) == wok and np.array_equal(pl[k].view(np.uint32), wpl.view(np.uint32)), (k, fr[k])
        assert not ok[::9].any() and not ok[3] and ok.any()


def test_inliers_and_live(host):
    rng = np.random.default_rng(9)
    m = 4000
    pl = np.array([0.6, 0.0, 0.8, -0.25], f32)
    pts = (rng.standard_normal((m, 3)) * 0.5).astype(f32)
    pts[:40, 2] = (f32(0.25) - f32(0.6) * pts[:40, 0]) / f32(0.8)  # close to the plane
    special = np.array([0.0, -0.0, 1e-45, np.inf, -np.inf, np.nan, 3.4028235e38], f32)
    pts[40:140] = special[rng.integers(0, len(special), (100, 3))]
    nrm = rng.standard_normal((m, 3)).astype(f32)
    nrm[::5] = pl[:3]
    nrm[140:240] = special[rng.integers(0, len(special), (100, 3))]
    for md, nc, with_n in ((0.02, 0.0, False), (0.02, 0.9, True), (1e-3, 1.0, True), (0.5, 0.0, True)):
        got = np.full(m, -9, np.int32)
        host.plane_inlier_batch(_p(pl), _p(pts), _p(nrm) if with_n else None, ctypes.c_int64(m), ctypes.c_float(md),
                                ctypes.c_float(nc), _p(got))
        want = PO.inlier_mask(pl, pts, md, nrm if with_n else None, nc)
        assert np.array_equal(got.astype(bool), want)
        assert 0 < want.sum() < m
    # the strict <: a layer at exactly max_dist
    z = np.array([[0.25, 0.5, 0.125], [0.25, 0.5, 0.0], [0.25, 0.5, 0.12499999]], f32)
    got = np.zeros(3, np.int32)
    flat = np.array([0, 0, 1, 0], f32)
    host.plane_inlier_batch(_p(flat), _p(z), None, ctypes.c_int64(3), ctypes.c_float(0.125), ctypes.c_float(0), _p(got))
    assert got.tolist() == [0, 1, 1]
    live = np.zeros(m, np.int32)
    host.plane_live_batch(_p(nrm), ctypes.c_int64(m), _p(live))
    assert np.array_equal((live & 1).astype(bool), PO.live_mask(nrm))
    assert np.array_equal((live & 2).astype(bool), PO.live_mask(np.ones((m, 3), f32), nrm))
    assert 0 < (live == 1).sum() and (live == 0).sum() > 0


def test_sample_index(host):
    u = np.array([0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff] * 4, np.uint32)
    mm = np.repeat(np.array([1, 3, 13700, 0x7fffffff], np.uint32), 6)
    out = np.zeros(len(u), np.uint32)
    host.plane_sample_batch(_p(u), _p(mm), ctypes.c_int64(len(u)), _p(out))
    assert out.tolist() == [PO.sample_index(a, b) for a, b in zip(u, mm)]
    assert np.all(out < mm)
