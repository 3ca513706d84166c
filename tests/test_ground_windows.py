"""segmentation.pmf_windows, the window schedule of the progressive morphological filter, against values worked by hand:
both modes, the cap at MaxDistance and the cut-off at MaxWindowSize.  A pure function: no GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcgol_amd.segmentation import pmf_windows  # noqa: E402
import ground_scenes as GS  # noqa: E402

f32 = np.float32


def _h(values):
    return np.asarray(values, np.float64).astype(f32)


def test_exponential():
    # widths 2 * 2^i + 1 = 3, 5, 9, 17, 33 cells of 0.5 m: 1.5, 2.5, 4.5, 8.5, 16.5 m; 65 cells would be 32.5 m
    half, height = pmf_windows(0.5, 16.5, Slope=0.3, InitialDistance=0.15, MaxDistance=2.5, Base=2, Exponential=True)
    assert half.dtype == np.int32 and height.dtype == f32
    assert list(half) == [1, 2, 4, 8, 16]
    # 0.15, then 0.3 * (2, 4, 8, 16) * 0.5 + 0.15 = 0.45, 0.75, 1.35, 2.55 -> the last is capped at 2.5
    assert np.array_equal(height, _h([0.15, 0.3 * 2 * 0.5 + 0.15, 0.3 * 4 * 0.5 + 0.15, 0.3 * 8 * 0.5 + 0.15, 2.5]))
    assert np.array_equal(half, GS.HILL_HALF) and np.array_equal(height, GS.HILL_HEIGHT)  # the scene's schedule is this one
    half3, _ = pmf_windows(1.0, 60.0, Base=3)
    assert list(half3) == [1, 3, 9, 27]  # widths 3, 7, 19, 55; 163 is too wide


def test_linear():
    # widths 2 (i + 1) 2 + 1 = 5, 9, 13, 17 cells of 1 m; 21 m is too wide for 20
    half, height = pmf_windows(1.0, 20.0, Slope=1.0, InitialDistance=0.5, MaxDistance=3.0, Base=2, Exponential=False)
    assert list(half) == [2, 4, 6, 8]
    assert np.array_equal(height, _h([0.5, 3.0, 3.0, 3.0]))  # 1 * 4 * 1 + 0.5 = 4.5 is above the cap
    half, height = pmf_windows(0.25, 3.0, Slope=0.2, InitialDistance=0.1, MaxDistance=10.0, Base=1, Exponential=False)
    assert list(half) == [1, 2, 3, 4, 5]  # widths 3 .. 11 cells: 0.75 .. 2.75 m
    assert np.array_equal(height, _h([0.1] + [0.2 * 2 * 0.25 + 0.1] * 4))


def test_cut_off_is_inclusive_and_may_leave_nothing():
    assert list(pmf_windows(0.5, 2.5)[0]) == [1, 2]  # 5 cells * 0.5 m == 2.5 m is kept
    assert list(pmf_windows(0.5, 2.4999)[0]) == [1]
    half, height = pmf_windows(1.0, 2.9)
    assert len(half) == 0 and len(height) == 0 and half.dtype == np.int32 and height.dtype == f32


def test_heights_are_float64_rounded_once():
    # 0.1 * 2 * 0.3 + 0.05 in float64 is 0.11000000000000001; rounding every factor to float32 first gives another float32
    _, height = pmf_windows(0.3, 2.0, Slope=0.1, InitialDistance=0.05, MaxDistance=9.0)
    assert height[1] == f32(0.1 * 2 * 0.3 + 0.05)
    _, height = pmf_windows(0.7, 30.0, Slope=1 / 3, InitialDistance=0.1, MaxDistance=100.0)
    want = [0.1] + [1 / 3 * d * 0.7 + 0.1 for d in (2, 4, 8, 16)]
    assert np.array_equal(height, _h(want))


def test_bad_arguments():
    for kw in (dict(CellSize=0.0, MaxWindowSize=1.0), dict(CellSize=-1.0, MaxWindowSize=1.0),
               dict(CellSize=1.0, MaxWindowSize=100.0, Base=1), dict(CellSize=1.0, MaxWindowSize=100.0, Base=0, Exponential=False)):
        with pytest.raises(ValueError):
            pmf_windows(**kw)
