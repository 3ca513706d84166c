"""csrc/fps_terms.h compiled for the host with g++ -ffp-contract=off under -fsanitize=address,undefined, as a program of
its own (tests/cpp/fps_terms_host.cpp over the shim tests/cpp/host_shim): the pick key orders as (d, -id) does, and the
box lemma -- fps_box_lower(s, lo, hi) <= DistSq(p, s) in float32 for every p inside the box -- has no violation over
120 000 triples that hold zero-extent boxes, points on faces and corners, s inside the box, coordinates near 1e6 a few
ulps apart and coordinates near +-3e19 whose squares overflow.  The distances are the NumPy oracle's bits
(tests/fps_oracle.py).  That the program runs to its end with nothing on stderr is the first assertion."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_oracle as FO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
inf = np.inf


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fps_terms") / "fps_terms_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "fps_terms_host.cpp")])
    return exe


def _keys():
    d = f32([0.0, 1e-45, 3e-45, 1e-39, 1e-38, 1.0, 2.5, 3.4e38, inf])  # (every d with every id: equal d, five ids)
    ids = np.array([0, 1, 5, 2 ** 31 - 2, 77], np.int64)
    dd, ii = np.repeat(d, len(ids)), np.tile(ids, len(d))
    return dd, ii


def _triples():
    """(lo, hi, p, s), each (k, 3) float32, lo <= p <= hi"""
    rng = np.random.default_rng(17)
    out = []

    def block(k, centre, extent, ulps=False):
        c = np.broadcast_to(f32(centre), (k, 3)).astype(f32)
        if ulps:  # boxes a few ulps wide: offsets in units of the spacing at the centre
            sp = np.spacing(np.abs(c).astype(f32))
            a = c + rng.integers(-8, 9, (k, 3)).astype(f32) * sp
            b = c + rng.integers(-8, 9, (k, 3)).astype(f32) * sp
            s = c + rng.integers(-40, 41, (k, 3)).astype(f32) * sp
        else:
            a = c + ((rng.random((k, 3)) - 0.5) * extent).astype(f32)
            b = c + ((rng.random((k, 3)) - 0.5) * extent).astype(f32)
            s = c + ((rng.random((k, 3)) - 0.5) * 3 * extent).astype(f32)
        lo, hi = np.minimum(a, b).astype(f32), np.maximum(a, b).astype(f32)
        kind = rng.integers(0, 5, (k, 1))
        zero = rng.random((k, 3)) < 0.2
        hi = np.where((kind == 0) | zero, lo, hi)  # zero-extent boxes (whole, or along some axes)
        t = rng.random((k, 3)).astype(f32)
        p = (lo + (hi - lo) * t).astype(f32)
        p = np.clip(p, lo, hi)
        face = rng.integers(0, 3, (k, 3))  # kind 1: every axis on a face (a corner); kind 2: some axes
        p = np.where((kind == 1) | ((kind == 2) & (face > 0)), np.where(face == 1, lo, hi), p)
        s = np.where(kind == 3, np.clip(s, lo, hi), s)  # s inside the box: the bound is 0
        s = np.where((kind == 4) & (face == 0), p, s)   # s level with p along some axes
        out.append((lo.astype(f32), hi.astype(f32), p.astype(f32), s.astype(f32)))

    for scale in (1e-3, 1.0, 1e3):
        block(20_000, 0.0, scale)
    block(20_000, [1e6, -1e6, 1e6], 0.0, ulps=True)
    block(10_000, [1e6, 1e6, -1e6], 4.0)
    block(15_000, [3e19, -3e19, 3e19], 6e19)   # the squares overflow to +inf
    block(15_000, [-3e19, 3e19, 0.0], 1e19)
    lo, hi, p, s = [np.concatenate(x) for x in zip(*out)]
    assert np.all(lo <= p) and np.all(p <= hi) and np.isfinite(np.stack([lo, hi, p, s])).all()
    return lo, hi, p, s


@pytest.fixture(scope="module")
def output(program):
    dd, ii = _keys()
    lo, hi, p, s = _triples()
    rows = np.concatenate([lo, hi, p, s], axis=1).view(u32)
    lines = ["%d %d" % (len(dd), len(rows))]
    lines += ["%08x %d" % (w, i) for w, i in zip(dd.view(u32), ii)]
    lines += [" ".join("%08x" % w for w in r) for r in rows]
    r = subprocess.run([program], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, "the sanitizer (or the program) stopped: %s" % r.stderr[-2000:]
    assert r.stderr == ""
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(dd) + len(rows) + 4 + 1
    return out


def test_the_key_orders_as_d_then_the_smaller_id(output):
    dd, ii = _keys()
    rows = [r.split() for r in output[:len(dd)]]
    keys = np.array([int(r[0], 16) for r in rows], np.uint64)
    assert np.array_equal(keys, (dd.view(u32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - ii.astype(np.uint64)))
    assert [int(r[1]) for r in rows] == ii.tolist() and [int(r[2], 16) for r in rows] == dd.view(u32).tolist()
    assert np.all(keys != 0) and len(np.unique(keys)) == len(keys)
    # one unsigned maximum = the largest d, then the smallest id: the two orders are the same permutation
    assert np.array_equal(np.argsort(keys, kind="stable"), np.lexsort((-ii, dd.astype(np.float64))))
    assert int(ii[np.argmax(keys)]) == 0 and np.isinf(dd[np.argmax(keys)])


def test_the_box_lemma_has_no_violation(output):
    dd, _ = _keys()
    lo, hi, p, s = _triples()
    k = len(lo)
    assert k >= 100_000
    got = np.array([[int(w, 16) for w in r.split()[:2]] + [int(w) for w in r.split()[2:]] for r in output[len(dd):len(dd) + k]],
                   np.int64)
    lower, dist = got[:, 0].astype(u32).view(f32), got[:, 1].astype(u32).view(f32)
    with np.errstate(over="ignore"):
        want = np.array([FO.dist_sq(p[i:i + 1], s[i]) for i in range(0, k, 997)], f32).reshape(-1)
        assert np.array_equal(dist[::997].view(u32), want.view(u32))  # the program's DistSq is the oracle's
        c = np.clip(s, lo, hi)
        d = c - s
        assert np.array_equal(lower.view(u32), ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).view(u32))
    assert not np.isnan(lower).any() and not np.isnan(dist).any() and np.all(lower >= 0)
    assert got[:, 2].sum() == k, np.nonzero(got[:, 2] == 0)[0][:10]  # zero violations
    assert np.array_equal(got[:, 3], (lower >= dist).astype(np.int64))
    # what the table was made to hold
    assert (lower == 0).sum() > k // 10 and (lower == dist).sum() > k // 10 and (lower < dist).sum() > k // 4
    assert np.isinf(dist).sum() > 10_000 and np.isinf(lower).sum() > 1000 and (np.isinf(dist) & ~np.isinf(lower)).any()
    assert np.all(lo == hi, axis=1).sum() > 10_000
    near = np.abs(s[:, 0]) > 9e5
    assert ((lower[near] > 0) & (lower[near] < 1e-1)).any()


def test_the_constants(output):
    tail = output[-5:-1]
    assert tail[0] == "updates 1 0 1 0"       # strict: an equal distance changes nothing, +inf is not below +inf
    assert tail[1] == "eligible 1 0 0 0"
    assert tail[2] == "skips 1 1 0 0"         # equal: skipped; a NaN bound: touched
    assert tail[3] == "padding -1 bf800000 %d" % (2 ** 31 - 2)
