"""The C++ binding of ground segmentation (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::Ground) over the C ABI: compiled with
g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python binding's
results, which tests/test_gpu_ground.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_scenes as GS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ground_mirror.cpp")
TAGS = ["L", "S", "I", "W", "F", "H", "M"]


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "ground_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_ground_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_ground_matches_python(tmp_path):
    from pcgol_amd import kdtree
    exe = _build(tmp_path)
    pts, _ = GS.hill()
    pts = pts[:6000]
    # origin, dims, cell, half, height
    calls = [(GS.HILL_ORIGIN, GS.HILL_DIMS, GS.HILL_CELL, GS.HILL_HALF, GS.HILL_HEIGHT),
             ((4.0, 2.0), (30, 50), 0.75, [2, 9], [0.25, 1.0]), (GS.HILL_ORIGIN, GS.HILL_DIMS, GS.HILL_CELL, [], [])]
    lines = ["P %d" % len(pts)] + ["%r %r %r" % tuple(map(float, p)) for p in pts]
    for origin, dims, cell, half, height in calls:
        lines.append("C %r %r %d %d %r %d" % (float(origin[0]), float(origin[1]), dims[0], dims[1], cell, len(half)))
        lines += ["%d %r" % (int(h), float(ht)) for h, ht in zip(half, height)]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert [w[0] for w in rows] == TAGS * len(calls)
    t = kdtree.New(pts)
    for k, (origin, dims, cell, half, height) in enumerate(calls):
        want = t.Ground(cell, half, height, Origin=origin, Dims=dims)
        got = {w[0]: np.array(w[1:], np.int64) for w in rows[len(TAGS) * k:len(TAGS) * (k + 1)]}
        assert np.array_equal(got["L"], want.labels) and np.array_equal(got["S"], want.sizes), k
        assert np.array_equal(got["I"], want.ids) and np.array_equal(got["W"], want.window), k
        assert np.array_equal(got["F"].astype(np.uint32), want.surface.reshape(-1).view(np.uint32)), k
        assert np.array_equal(got["H"].astype(np.uint32), want.hag.view(np.uint32)), k
        assert np.array_equal(got["M"], want.ids[want.sizes[0]:]), k
        assert want.sizes[0] > 0 and (want.sizes[1] > 0) == (len(half) > 0), k  # the calls do what they are for
