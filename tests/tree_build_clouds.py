"""Clouds for tests/test_gpu_tree_build.py: what the device tree build (csrc/kdtree_build_gpu.hip) and the radix sort
under it (csrc/sort.hip) are given there.  Every builder is a pure function of its arguments and checks on the CPU that
the cloud has the property the test relies on; the results are cached, the tests only read them."""
import functools

import numpy as np

f32 = np.float32
u32 = np.uint32

# the ladder of section 1 and what each rung is there for (kUnitMax = 1024 elements to an LDS slice, 2048 elements to
# a sort tile below 2^22 elements, the XCD remap from 64 tiles on, rs_scan_rows_kernel's rounds of 256 tiles)
LADDER = [2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 63, 64, 65,  # one workgroup, every level in LDS; subtrees of 0 and 1
          1023, 1024, 1025,                                      # d0 0 -> 1: the first radix level
          2047, 2048, 2049, 2050,                                # one sort tile -> two; d0 1 -> 2 at 2050
          4095, 4096, 4097, 4099, 4100,                          # two tiles -> three; d0 2 -> 3 at 4100
          32767, 32768, 32769,                                   # the default host / device switch
          129023, 129024, 129025, 131071, 131072, 131073,        # 63 / 64 tiles: the XCD remap, workgroups without a tile
          524288, 524289]                                        # 256 / 257 tiles: a second scan round, 10-bit unit ranks
SWITCH = [32767, 32768, 32769]
NODE_RUNGS = [2, 3, 7, 64, 65, 1025, 2050, 4100, 32769, 131073, 524289]
GRID_RUNGS = [n for n in NODE_RUNGS if n >= 64]


def _frozen(a):
    a = np.ascontiguousarray(a, f32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def distinct_cloud(n, width=10.0, seed=0):
    """n float32 points drawn uniformly from [0, width)^3, no xyz triple twice."""
    rng = np.random.default_rng([n, seed, 11])
    pts = rng.random((n, 3), dtype=f32) * f32(width)
    assert len(np.unique(pts, axis=0)) == n
    return _frozen(pts)


@functools.lru_cache(maxsize=None)
def lattice_cloud(n, seed=0):
    """n points with coordinates from 0..3: 64 sites, so every split coordinate is tied many times over and the order
    of a level's ties is what the sort's stability makes it."""
    rng = np.random.default_rng([n, seed, 12])
    return _frozen(rng.integers(0, 4, size=(n, 3)).astype(f32))


def jittered(pts, m=2000, seed=0):
    """m queries: points of the cloud (drawn with replacement) moved by 0.013 on every axis"""
    rng = np.random.default_rng([len(pts), seed, 13])
    return np.ascontiguousarray(pts[rng.integers(0, len(pts), m)] + f32(0.013), f32)


@functools.lru_cache(maxsize=None)
def flat_cloud(n, seed=0):
    """distinct points with one z: the grid has one layer of cells"""
    pts = distinct_cloud(n, 10.0, seed + 100).copy()
    pts[:, 2] = f32(1.25)
    assert len(np.unique(pts, axis=0)) == n
    return _frozen(pts)


@functools.lru_cache(maxsize=None)
def one_live_byte_cloud(n, digit, seed=0):
    """Every coordinate is a float32 whose bit pattern differs from the others' in byte `digit` only (and in the sign:
    half of the values are negated), so the coordinate sort is decided by ONE of its four 8-bit passes -- above all
    for digit 3, the sign folded into the key.  Digits 0-2: values of [1, 2).  Digit 3: the exponents 0, 2, .., 254
    (finite; exponent 0 is a subnormal) over one mantissa."""
    assert digit in (0, 1, 2, 3)
    rng = np.random.default_rng([n, digit, seed, 14])
    if digit < 3:
        base, byte = 0x3FA5C3E1 & ~(0xFF << (8 * digit)), rng.integers(0, 256, size=(n, 3))
    else:
        base, byte = 0x00345678, rng.integers(0, 128, size=(n, 3))
    bits = (u32(base) | (byte.astype(u32) << u32(8 * digit))).astype(u32)
    assert np.all((bits ^ u32(base)) & ~u32(0xFF << (8 * digit)) == 0)
    for k in range(3):
        assert len(np.unique(bits[:, k])) == (256 if digit < 3 else 128)  # every value of the byte, on every axis
    bits = bits | (rng.integers(0, 2, size=(n, 3)).astype(u32) << u32(31))
    pts = np.ascontiguousarray(bits).view(f32)
    assert np.all(np.isfinite(pts))
    return _frozen(pts)


@functools.lru_cache(maxsize=None)
def sorted_cloud(n, kind, seed=0):
    """"ascending": every axis ascending in id order; "descending4": every axis descending, each value four times;
    "identical": one point n times."""
    rng = np.random.default_rng([n, seed, 15])
    if kind == "ascending":
        pts = np.sort(rng.random((n, 3), dtype=f32) * f32(10), axis=0)
        assert np.all(np.diff(pts, axis=0) >= 0)
    elif kind == "descending4":
        v = -np.sort(-rng.random(((n + 3) // 4, 3), dtype=f32) * f32(10), axis=0)
        pts = np.repeat(v, 4, axis=0)[:n]
        assert np.all(np.diff(pts, axis=0) <= 0) and np.all(pts[0:n - n % 4:4] == pts[3:n:4])
    else:
        assert kind == "identical"
        pts = np.repeat(np.array([[1.5, -2.25, 0.0]], f32), n, axis=0)
    return _frozen(pts)


# -0.0, +0.0, the smallest and the largest subnormal, FLT_MIN, 1, FLT_MAX and inf, of either sign, as bit patterns
_EDGE_FINITE_SMALL = [0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                      0x3F800000, 0xBF800000]
_EDGE_ENDS = [0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000]
assert np.array([1e-45, 1.1754942e-38], f32).view(u32).tolist() == [0x00000001, 0x007FFFFF]
assert np.array([0x00800000, 0x7F7FFFFF], u32).view(f32).tolist() == [np.finfo(f32).tiny, np.finfo(f32).max]


@functools.lru_cache(maxsize=None)
def edge_value_cloud(n, with_ends, seed=0):
    """Every coordinate drawn from {-0.0, +0.0, +-1e-45, +-1.1754942e-38, +-FLT_MIN, +-1} and, with_ends, +-FLT_MAX and
    +-inf.  No NaN.  Every value occurs on every axis."""
    values = np.array(_EDGE_FINITE_SMALL + (_EDGE_ENDS if with_ends else []), u32)
    rng = np.random.default_rng([n, int(with_ends), seed, 16])
    bits = np.ascontiguousarray(values[rng.integers(0, len(values), size=(n, 3))])
    for k in range(3):
        assert np.array_equal(np.unique(bits[:, k]), np.sort(values))
    pts = bits.view(f32)
    assert not np.any(np.isnan(pts))
    return _frozen(pts)


def finite_jittered(pts, m=500, seed=0):
    """m finite queries beside points of a cloud that may hold infinities (an infinite coordinate counts as 0)"""
    rng = np.random.default_rng([len(pts), seed, 17])
    p = pts[rng.integers(0, len(pts), m)]
    q = np.where(np.isfinite(p), p, f32(0)) + f32(0.013)
    assert np.all(np.isfinite(q))
    return np.ascontiguousarray(q, f32)
