"""tests/boundary_oracle.py against what can be known without it: the analytic gaps of a unit lattice, a bit-by-bit
loop for the gap of a mask, atan2 for the sector of a direction, and the invariance of the masks under a permutation of
the cloud."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_oracle as BO  # noqa: E402
import boundary_scenes as BS  # noqa: E402

f32, f64, u64 = np.float32, np.float64, np.uint64


def test_tangents_are_the_nearest_doubles():
    """each T[k] is the correctly rounded tan(k pi / 32), from sine and cosine series in 60-digit decimals (math.tan of
    the rounded argument is up to 3 ulp off: no yardstick); T[8] is 1 exactly"""
    import decimal
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        pi = D("3.14159265358979323846264338327950288419716939937510582097494")
        for k in range(1, 16):
            x = pi * k / 32
            sin = cos = D(0)
            term = D(1)
            for j in range(80):  # x^j / j!, x < 1.5
                if j % 2 == 0:
                    cos += term if j % 4 == 0 else -term
                else:
                    sin += term if j % 4 == 1 else -term
                term = term * x / (j + 1)
            assert float(sin / cos) == BO.T[k], k
            # (and math.tan agrees as far as it can: its argument is off by up to an ulp, times d tan = 1 + tan^2)
            arg = k * math.pi / 32
            assert abs(BO.T[k] - math.tan(arg)) <= (1 + BO.T[k] ** 2) * math.ulp(arg) + 2 * math.ulp(BO.T[k]), k
    assert BO.T[8] == 1.0 and len(BO.T) == 16 and np.all(np.diff(BO.T) > 0)


def test_lattice():
    pts, kind = BS.lattice()
    want = np.array([BS.LATTICE_GAPS[k] for k in ("interior", "edge", "corner")])[kind]
    assert np.bincount(kind).tolist() == [25, 20, 4]
    masks = []
    for nz in (1.0, -1.0):
        nrm = np.tile(f32([0, 0, nz]), (len(pts), 1))
        ref = BO.boundary(pts, nrm, BS.LATTICE_RADIUS, 16)
        assert np.array_equal(ref["gaps"], want)
        assert np.array_equal(ref["ids"], np.nonzero(kind > 0)[0]) and len(ref["ids"]) == 24
        assert np.array_equal(BO.boundary(pts, nrm, BS.LATTICE_RADIUS, 32)["ids"], np.nonzero(kind == 2)[0])
        assert np.array_equal(ref["counts"], np.array([9, 6, 4])[kind])
        masks.append(ref["masks"])
    # an interior point's eight neighbours sit on the multiples of 45 degrees: every eighth sector, owned from below
    assert np.all(masks[0][kind == 0] == u64(0x0101010101010101))
    assert not np.array_equal(masks[0], masks[1])  # the flipped normal turns the other way round: other bits, same gaps


def _gap_by_bits(m):
    """the 64 bits written out twice in a row (the cyclic run may pass the end), split at the ones"""
    bits = format(int(m), "064b")
    return min(max(len(run) for run in (bits + bits).split("1")), 64)


def test_gap_against_a_bit_by_bit_loop():
    pat = np.arange(1 << 16, dtype=u64)
    rep = pat | (pat << u64(16)) | (pat << u64(32)) | (pat << u64(48))
    got = BO.gap(rep)
    assert got.tolist() == [_gap_by_bits(m) for m in rep]
    rng = np.random.default_rng(3)
    # masks of every density: the AND of k random words has a bit set with probability 2^-k
    rnd = rng.integers(0, 1 << 63, (100_000, 6), dtype=np.uint64) << u64(1) | rng.integers(0, 2, (100_000, 6), dtype=np.uint64)
    k = rng.integers(1, 7, 100_000)
    m = rnd[:, 0].copy()
    for j in range(1, 6):
        m = np.where(k > j, m & rnd[:, j], m)
    assert BO.gap(m).tolist() == [_gap_by_bits(x) for x in m]
    assert len(np.unique(BO.gap(m))) > 30
    edge = np.array([0, 0xFFFFFFFFFFFFFFFF] + [1 << s for s in range(64)], u64)
    assert BO.gap(edge).tolist() == [64, 0] + [63] * 64
    assert BO.gap(np.array([0x8000000000000001, 0x7FFFFFFFFFFFFFFE, 0xFFFFFFFF00000000], u64)).tolist() == [62, 2, 32]


def test_sector_against_atan2():
    rng = np.random.default_rng(4)
    w = 2.0 * np.pi / 64
    ang = rng.uniform(0, 2 * np.pi, 200_000)
    ang = ang[np.abs(ang / w - np.round(ang / w)) * w > 1e-9]
    rad = np.exp(rng.uniform(-30, 30, len(ang)))
    a, b = rad * np.cos(ang), rad * np.sin(ang)
    want = np.floor(np.mod(np.arctan2(b, a), 2 * np.pi) / w).astype(np.int64)
    assert np.array_equal(BO.sector(a, b), want)
    assert len(np.unique(want)) == 64
    # exactly on the multiples of 45 degrees: a sector owns its lower border
    s = 3.0
    on = BO.sector([s, s, 0, -s, -s, -s, 0, s], [0, s, s, s, 0, -s, -s, -s])
    assert on.tolist() == [0, 8, 16, 24, 32, 40, 48, 56]
    on = BO.sector([s, s, -0.0, -s, -s, -s, 0, s], [-0.0, s, s, s, 0.0, -s, -s, -s])  # (a zero's sign does not enter)
    assert on.tolist() == [0, 8, 16, 24, 32, 40, 48, 56]
    assert BO.sector([0.0, 0.0, -0.0, -0.0], [0.0, -0.0, 0.0, -0.0]).tolist() == [-1] * 4
    # just below a border: the sector before it
    eps = 1e-12
    assert BO.sector([s, s, -eps, eps], [-eps, s * (1 - 1e-15), s, -s]).tolist() == [63, 7, 16, 48]


def test_permuting_the_cloud_permutes_the_masks():
    rng = np.random.default_rng(5)
    pts = rng.random((1500, 3)).astype(f32)
    v = rng.standard_normal((1500, 3))
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    nrm[::50] = 0.0
    ref = BO.boundary(pts, nrm, 0.15, 16, 3)
    perm = rng.permutation(len(pts))
    got = BO.boundary(pts[perm], nrm[perm], 0.15, 16, 3)
    assert np.array_equal(got["masks"], ref["masks"][perm])
    assert np.array_equal(got["gaps"], ref["gaps"][perm]) and np.array_equal(got["counts"], ref["counts"][perm])
    inv = np.argsort(perm)
    assert np.array_equal(got["ids"], np.sort(inv[ref["ids"]]))
    assert 20 < len(ref["ids"]) < 1400 and (ref["gaps"] == -1).sum() >= 30
    gone = rng.choice(len(pts), 150, replace=False)
    d = BO.boundary(pts, nrm, 0.15, 16, 3, deleted=gone)
    assert np.all(d["gaps"][gone] == -1) and not d["counts"][gone].any() and not np.array_equal(d["masks"], ref["masks"])
