"""pcgx_minmax (pc.MinMaxVec3, pc/minmax.go:9-26) against the oracle's sequential loop, vmin and vmax as bit patterns,
at the values and the seams where the two kernels of csrc/sort.hip can go wrong without a random cloud noticing.

The kernels do not run the reference's loop: they reduce with minNum / maxNum over everything and keep, per axis, the
index and sign of the cloud's first zero; point 0 is folded in last (a NaN there sticks).  The packed kernel (stride 12,
offset 0) reads 16-byte words, three per thread and round, re-reads a thread's first word where a round runs past the
end, and leaves the up-to-three floats behind the last whole word to one thread; its workgroup count is 1 mod 3 and
steps at n = 1024, 4096, 7168, ..., 1048576.  The strided kernel takes every other layout, and every cloud under 1024
points.  So: lengths on both sides of each of those steps and of a wave, a workgroup and a round, all four values of
3n mod 4 at the full 1024 workgroups, a ragged second round; five layouts; and, planted one at a time into a cloud
uniform in (-1, 1):

  (a) the strict minimum of one axis and the strict maximum of another in ONE point -- the last, the first, the middle
      one -- for each of the three axis pairs, so that each of the array's last three floats decides a result;
  (b) signed zeros: an axis made positive (negative) but for +0 at i and -0 at j > i, and the signs swapped -- the
      result is the first one's -- for (i, j) across a point, a workgroup, a round and the whole cloud, a lone zero in
      the last point, and a cloud of nothing but zeros of mixed sign;
  (c) NaN: at index 0 (it sticks, with its payload), at 1, n / 2 and n - 1 (skipped), an axis that is NaN everywhere
      but at index 0, a cloud that is all NaN;
  (d) +-inf, and the denormals +-1e-45 as the extreme of an axis (a kernel that flushes them returns a zero).

Every comparison is exact; there is no tolerance."""
import numpy as np
import pytest

import oracle as O
from pcgol_amd import _lib as L
from pcgol_amd import synth

pytestmark = pytest.mark.gpu
f32, u32, u8 = np.float32, np.uint32, np.uint8

LENGTHS = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1366, 1367, 4095, 4096, 4097, 7167, 7168, 100003,
           1048576, 1048577, 1048578, 1048579, 1100001]
LAYOUTS = [(12, 0), (16, 0), (16, 4), (15, 1), (28, 16)]
PAIRS = [(0, "last"), (None, "last"), (1, 2), (255, 256), (2047, 2048), ("mid", "mid+1")]   # (i, j) of the two zeros
NAN = f32(np.nan)
NAN_PAYLOAD = np.array([0xffc12345], u32).view(f32)[0]      # a quiet NaN with a sign and a payload


def _column(kind, base_col):
    """An axis' column: 'pos' > 0 everywhere (>= 2^-20), 'neg' its mirror, NaN all over or everywhere but at index 0,
    zeros of mixed sign with +0 or -0 in front."""
    n = len(base_col)
    if kind == "pos":
        return np.abs(base_col) + f32(2.0 ** -20)
    if kind == "neg":
        return -(np.abs(base_col) + f32(2.0 ** -20))
    if kind == "nan":
        return np.full(n, NAN, f32)
    if kind == "nan_but_0":
        col = np.full(n, NAN, f32)
        col[0] = base_col[0]
        return col
    assert kind in ("zeros+", "zeros-")
    col = np.where(np.random.default_rng(n).random(n) < 0.5, f32(0.0), f32(-0.0)).astype(f32)
    col[0] = f32(0.0) if kind == "zeros+" else f32(-0.0)
    return col


def _plants(n):
    """(label, {axis: column kind}, [(point, axis, value)]) -- every plant on its own, applied to a copy of the cloud"""
    last, mid = n - 1, n // 2
    out = []
    for where, i in (("last", last), ("first", 0), ("middle", mid)):                                     # (a)
        for k in range(3):
            out.append(("a: min of axis %d, max of axis %d in the %s point" % (k, (k + 1) % 3, where), {},
                        [(i, k, f32(-2.0 - k)), (i, (k + 1) % 3, f32(2.0 + k))]))
    named = {"last": last, "mid": mid, "mid+1": mid + 1}
    for side in ("pos", "neg"):                                                                          # (b)
        for p, (i, j) in enumerate(PAIRS):
            i, j = named.get(i, i), named.get(j, j)
            if j >= n or (i is not None and not 0 <= i < j):
                continue
            for first, second in ((f32(0.0), f32(-0.0)), (f32(-0.0), f32(0.0))):
                edits = [(j, p % 3, second)] if i is None else [(i, p % 3, first), (j, p % 3, second)]
                out.append(("b: axis %d %s, zeros %r at %r, %r at %d" % (p % 3, side, first, i, second, j), {p % 3: side}, edits))
    out.append(("b: all zeros of mixed sign, +0 first", {0: "zeros+", 1: "zeros+", 2: "zeros+"}, []))
    out.append(("b: all zeros of mixed sign, -0 first", {0: "zeros-", 1: "zeros-", 2: "zeros-"}, []))
    out.append(("c: NaN at index 0 of axis 1", {}, [(0, 1, NAN)]))                                        # (c)
    out.append(("c: NaN with sign and payload at index 0 of axis 0", {}, [(0, 0, NAN_PAYLOAD)]))
    for i, k in ((1, 0), (mid, 1), (last, 2)):
        if 1 <= i < n:
            out.append(("c: NaN at index %d of axis %d" % (i, k), {}, [(i, k, NAN)]))
    out.append(("c: axis 2 NaN everywhere but at index 0", {2: "nan_but_0"}, []))
    out.append(("c: all NaN", {0: "nan", 1: "nan", 2: "nan"}, []))
    out.append(("d: +inf at index 0 of axis 0", {}, [(0, 0, f32(np.inf))]))                              # (d)
    out.append(("d: +inf in the middle of axis 1", {}, [(mid, 1, f32(np.inf))]))
    out.append(("d: -inf in the last point's axis 2", {}, [(last, 2, f32(-np.inf))]))
    for i in sorted({mid, last}):
        out.append(("d: 1e-45 the min of a positive axis 1, at %d" % i, {1: "pos"}, [(i, 1, f32(1e-45))]))
    for i in sorted({mid, last}):
        out.append(("d: -1e-45 the max of a negative axis 2, at %d" % i, {2: "neg"}, [(i, 2, f32(-1e-45))]))
    return out


def _planted(pts, cols, edits):
    p = pts.copy()
    for k, kind in cols.items():
        p[:, k] = _column(kind, pts[:, k])
    for i, k, v in edits:
        p[i, k] = v
    return p


def _pack(p, filler, off):
    """xyz at `off` of records whose other bytes are `filler`'s"""
    rec = filler.copy()
    rec[:, off:off + 12] = p.view(u8).reshape(len(p), 12)
    return rec


def _minmax_bits(rec, n, stride, off):
    mn, mx = np.zeros(3, f32), np.zeros(3, f32)
    L.check(L.lib().pcgx_minmax(L.ptr(rec), n, stride, off, L.ptr(mn), L.ptr(mx)))
    return np.concatenate([mn, mx]).view(u32)


def _oracle_bits(rec, n, stride, off):
    mn, mx = O.minmax(rec, n, stride, off)
    return np.concatenate([mn, mx]).view(u32)


def _hex(bits):
    return " ".join("%08x" % b for b in bits)


@pytest.mark.parametrize("n", LENGTHS)
def test_minmax_bits_at_planted_values(n):
    pts = synth.uniform_cloud(n, 2.0, 100 + n % 89) - f32(1.0)
    rng = np.random.default_rng(n)
    plants = [("the cloud as it is", {}, [])] + _plants(n)
    layouts = LAYOUTS if n <= 100003 else LAYOUTS[:2]
    problems, decided_by_tail = [], set()
    for stride, off in layouts:
        filler = rng.integers(0, 256, size=(n, stride), dtype=u8)
        for label, cols, edits in plants:
            rec = _pack(_planted(pts, cols, edits), filler, off)
            exp = _oracle_bits(rec, n, stride, off)
            got = _minmax_bits(rec, n, stride, off)
            if not np.array_equal(got, exp):
                problems.append((stride, off, label, _hex(got), _hex(exp)))
            if label.startswith("a:") and "last" in label:     # which of the array's last three floats decided a result
                for i, k, v in edits:
                    assert exp[k] == v.view(u32) or exp[3 + k] == v.view(u32), label
                    decided_by_tail.add(k)
    assert decided_by_tail == {0, 1, 2}
    for p in problems:
        print(p)
    assert not problems, "%d of %d comparisons" % (len(problems), len(plants) * len(layouts))


def test_minmax_of_no_point():
    mn, mx = np.zeros(3, f32), np.zeros(3, f32)
    with pytest.raises(L.ErrNoPoint):
        L.check(L.lib().pcgx_minmax(L.ptr(np.zeros(12, u8)), 0, 12, 0, L.ptr(mn), L.ptr(mx)))
