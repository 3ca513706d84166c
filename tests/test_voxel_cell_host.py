"""csrc/voxel_cell.h -- the VoxelGrid filter's grid (voxel_grid_params) and the cell of a point (voxel_key_xyz, and the
general form voxel_key_xyz_any behind it) -- compiled for the host with g++ under
-fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all, as a program of its own
(tests/cpp/voxel_cell_host.cpp), and run on the clouds of tests/voxel_cases.py: NaN, infinities, +-1e30, a quotient
beyond 2^31, the smallest denormal, -0, a point on vMax, a crowded cell; plain and chunked.

What the header's text means on the host is what it means on the device only where the C++ standard defines it:
int64(NaN) and int64(1e30 / leaf) are undefined (x86 gives INT64_MIN; on the MI355X a NaN came out as a valid cell,
DESIGN.md 3.3), and so is an int64 sum that overflows.  The sanitizer ends the program at the first such operation; that it runs to its end is
the first assertion.  Then, case by case, against the oracle: the oracle raises (the Go code panics) exactly where the
grid's status is not 0 or some point's cell is `bad`; where it answers, the number of distinct (chunk, cell) pairs
is the number of records it returns; and the 32-bit lanes agree with the general form on every point."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_cases as V  # noqa: E402

import oracle as O  # noqa: E402

ROOT = V.ROOT
f32 = np.float32
LAYOUT = (12, 0)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("voxel_cell") / "voxel_cell_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "voxel_cell_host.cpp")])
    return exe


def _hex(a):
    return " ".join("%x" % w for w in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32))


@pytest.fixture(scope="module")
def results(program):
    """every case through the program in one run: {(name, index, chunk): (grid words, per-point rows or None)}"""
    keys = [(name, index, chunk) for name in list(V.MUST_FAIL) + V.MUST_PASS for index in V.INDICES for chunk in V.CHUNKS]
    lines = []
    for name, index, chunk in keys:
        pts = V.special_cloud(name, index)
        mn, mx = O.minmax(pts, V.N, 12, 0)      # (the filter's min / max are MinMaxVec3's: a NaN at index 0 sticks)
        lines.append("%s %d %d %d %s %d" % (_hex([V.LEAF] * 3), chunk[0], chunk[1], chunk[2], _hex(np.concatenate([mn, mx])), V.N))
        lines.append(_hex(pts))
    p = subprocess.run([program], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, "the sanitizer (or the program) stopped: %s" % p.stderr[-2000:]
    assert p.stderr == ""
    out = p.stdout.split("\n")
    got, at = {}, 0
    for key in keys:
        head = out[at].split()
        assert head[0] == "grid", out[at]
        grid = [int(w) for w in head[1:]]
        at += 1
        rows = None
        if grid[0] == 0:
            rows = np.array([[int(w) for w in line.split()] for line in out[at:at + V.N]], np.int64)
            assert rows.shape == (V.N, 6)
            at += V.N
        got[key] = (grid, rows)
    assert out[at:] == [""]
    return got


@pytest.fixture(scope="module")
def expected():
    return V.expectations(layouts=[LAYOUT])


def test_the_oracle_raises_on_every_must_fail_case_and_on_no_other(expected):
    for (name, index, chunk, _), (kind, what) in expected.items():
        assert (kind == "raise") == (name in V.MUST_FAIL), (name, index, chunk, kind)
        if kind == "raise":
            assert what == V.EXPECTED_CODE[name], (name, index, chunk, what)


def test_status_and_bad_are_the_oracles_panics(results, expected):
    for (name, index, chunk), (grid, rows) in results.items():
        kind, what = expected[(name, index, chunk, LAYOUT)]
        refused = grid[0] != 0 or bool(rows[:, 0].any())
        assert refused == (kind == "raise"), (name, index, chunk, grid, kind)
        if kind == "bytes":
            assert len(np.unique(rows[:, 1:3], axis=0)) * 12 == len(what), (name, index, chunk)


def test_the_32_bit_lanes_agree_with_the_general_form(results):
    seen_bad = 0
    for key, (_grid, rows) in results.items():
        if rows is not None:
            assert np.array_equal(rows[:, 0:3], rows[:, 3:6]), key
            seen_bad += int(rows[:, 0].sum())
    assert seen_bad > 0     # (NaN, +-1e30 and -inf behind a grid that stands: the general form did run)
