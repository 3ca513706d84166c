"""pcgx_voxel_filter at non-finite, signed-zero and far-off points (the clouds of tests/voxel_cases.py): one point of a
3000-point cloud replaced by a NaN, an infinity, +-1e30, x = 2e8 (a quotient beyond 2^31 on a grid of more than 2^32
cells) -- the Go code panics, the call ends with PCGX_E_OUT_OF_RANGE and the same words whether the grid and the plan
were made on the device (the bucket path, PCGX_VOXEL_BUCKET_MIN_N=1) or on the host (the radix path) -- or by the
smallest denormal, -0, a point on vMax, 300 copies of one point -- the oracle's bytes on both.  Plain and chunked, one
key and two sorts, packed, padded and unaligned records, the point first, in the middle and last.

Every expectation is the oracle's (voxel_cases.expectations); a "must fail" case is first asserted to raise there.
After every failing call the base cloud goes through the same path and has to give the oracle's bytes: nothing of
the failed call (flags, head words, the min/max ticket) is left behind."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_cases as V  # noqa: E402

import oracle as O  # noqa: E402
from pcgol_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
PLANS = [("device", "1"), ("host", "1000000000")]     # PCGX_VOXEL_BUCKET_MIN_N: who makes the grid and the plan


def _last_error():
    buf = C.create_string_buffer(512)
    L.lib().pcgx_last_error(buf, 512)
    return buf.value


def _raw(rec, stride, off, chunk):
    """(status, its words, the output records)"""
    out = np.empty(V.N * stride, np.uint8)
    m = C.c_int64()
    leafv, chunkv = np.asarray((V.LEAF,) * 3, f32), np.asarray(chunk, np.int32)
    rc = L.lib().pcgx_voxel_filter(L.ptr(rec), V.N, stride, off, L.ptr(leafv), L.ptr(chunkv), L.ptr(out), C.byref(m))
    return rc, (_last_error() if rc else b""), (out[: m.value * stride] if rc == 0 else None)


@pytest.fixture(scope="module")
def expected():
    return V.expectations()


@pytest.fixture(scope="module")
def base_expected():
    return {(chunk, lay): O.voxel_filter(V.records(V.base_cloud(), *lay), V.N, lay[0], lay[1], (V.LEAF,) * 3, chunk)
            for chunk in V.CHUNKS for lay in V.LAYOUTS}


def test_the_oracle_raises_on_every_must_fail_case_and_on_no_other(expected):
    """(so that the comparison below is never a comparison of nothing)"""
    for (name, index, chunk, lay), (kind, what) in expected.items():
        assert (kind == "raise") == (name in V.MUST_FAIL), (name, index, chunk, lay, kind)
        if kind == "raise":
            assert what == V.EXPECTED_CODE[name], (name, index, chunk, lay, what)


@pytest.mark.parametrize("layout", V.LAYOUTS, ids=lambda l: "stride%d_off%d" % l)
@pytest.mark.parametrize("chunk,two_sorts", [(c, False) for c in V.CHUNKS] + [((5, 3, 4), True)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("two_sorts" if v else "one_key"))
def test_special_points_on_both_plans(chunk, two_sorts, layout, expected, base_expected, monkeypatch):
    stride, off = layout
    if two_sorts:
        monkeypatch.setenv("PCGX_VOXEL_TWO_SORTS", "1")
    base = V.records(V.base_cloud(), stride, off)
    problems = []
    for name in list(V.MUST_FAIL) + V.MUST_PASS:
        for index in V.INDICES:
            kind, what = expected[(name, index, chunk, layout)]
            rec = V.records(V.special_cloud(name, index), stride, off)
            seen = []
            for plan, min_n in PLANS:
                monkeypatch.setenv("PCGX_VOXEL_BUCKET_MIN_N", min_n)
                rc, words, out = _raw(rec, stride, off, chunk)
                seen.append((rc, words))
                if kind == "raise":
                    if rc != L.PCGX_E_OUT_OF_RANGE:
                        problems.append((name, index, plan, "status %d %r, %s records; the oracle raises (%d)"
                                         % (rc, words, "no" if out is None else len(out) // stride, what)))
                    if rc != 0:  # no residue: the base cloud through the same path
                        rc2, words2, out2 = _raw(base, stride, off, chunk)
                        if rc2 != 0 or not np.array_equal(out2, base_expected[(chunk, layout)]):
                            problems.append((name, index, plan, "the base cloud after the failed call: status %d %r" % (rc2, words2)))
                elif rc != 0:
                    problems.append((name, index, plan, "status %d %r; the oracle returns %d records" % (rc, words, len(what) // stride)))
                elif not np.array_equal(out, what):
                    problems.append((name, index, plan, "%d records, the oracle's %d%s" % (
                        len(out) // stride, len(what) // stride, "" if len(out) != len(what) else ", bytes differ")))
            if kind == "raise" and seen[0] != seen[1]:
                problems.append((name, index, "both", "the plans disagree: %r" % (seen,)))
    for p in problems:
        print(p)
    assert not problems, "%d of the cases" % len(problems)


def test_device_form_on_a_base_4_bytes_past_alignment(expected, base_expected, monkeypatch):
    """pcgx_voxel_filter_dev on a torch buffer whose base is advanced by 4 bytes: stride 12, but not the packed
    min/max kernel's 16-byte words -- the strided kernel reads the cloud, a NaN at index 0 sticks through it."""
    import torch
    lay = (12, 0)
    leafv = np.asarray((V.LEAF,) * 3, f32)
    problems = []
    for name, index in (("nan_x", 0), ("nan_y", 1500), ("-0.0_xyz", 0), ("1e-45_x", 2999)):
        rec = V.records(V.special_cloud(name, index), *lay)
        d = torch.zeros(V.N * 12 + 16, dtype=torch.uint8, device="cuda")
        assert d.data_ptr() % 16 == 0
        d[4:4 + V.N * 12] = torch.from_numpy(rec.reshape(-1)).cuda()
        o = torch.zeros(V.N * 12, dtype=torch.uint8, device="cuda")
        for chunk in ((0, 0, 0), (5, 3, 4)):
            kind, what = expected[(name, index, chunk, lay)]
            chunkv = np.asarray(chunk, np.int32)
            seen = []
            for plan, min_n in PLANS:
                monkeypatch.setenv("PCGX_VOXEL_BUCKET_MIN_N", min_n)
                m = C.c_int64()
                torch.cuda.synchronize()
                rc = L.lib().pcgx_voxel_filter_dev(C.c_void_p(d.data_ptr() + 4), V.N, 12, 0, L.ptr(leafv), L.ptr(chunkv),
                                                   C.c_void_p(o.data_ptr()), C.byref(m), None)
                words = _last_error() if rc else b""
                torch.cuda.synchronize()
                seen.append((rc, words))
                if kind == "raise":
                    if rc != L.PCGX_E_OUT_OF_RANGE:
                        problems.append((name, index, chunk, plan, "status %d %r; the oracle raises" % (rc, words)))
                elif rc != 0 or not np.array_equal(o[: m.value * 12].cpu().numpy(), what):
                    problems.append((name, index, chunk, plan, "status %d %r, %d records; the oracle's %d"
                                     % (rc, words, m.value, len(what) // 12)))
            if kind == "raise" and seen[0] != seen[1]:
                problems.append((name, index, chunk, "both", "the plans disagree: %r" % (seen,)))
    for p in problems:
        print(p)
    assert not problems
