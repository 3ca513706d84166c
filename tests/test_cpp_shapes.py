"""The C++ binding of cylinder and sphere segmentation (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::Shapes) over the C ABI:
compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_shapes.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_scenes as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shapes_mirror.cpp")
TAGS = ["L", "S", "I", "B", "R", "T", "N", "F", "H", "M"]


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "shapes_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_shapes_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_shapes_matches_python(tmp_path):
    from pcgol_amd import kdtree
    exe = _build(tmp_path)
    pts, nrm, _ = SC.yard()
    n_hyp = 96
    smp = SC.samples(n_hyp, 4, 21)
    # kind, max_dist, n_hyp, max_shapes, min_inliers, sample_radius, r_min, r_max, axis, min_axis_cos, min_normal_cos, refine
    calls = [(1, 0.02, n_hyp, 4, 600, 0.3, 0.03, 0.3, None, 0.0, 0.8, 1), (1, 0.02, n_hyp, 4, 600, 0.3, 0.03, 0.3, None, 0.0, 0.8, 0),
             (1, 0.02, n_hyp, 2, 600, 0.3, 0.03, 0.3, (0, 0, 1), 0.95, 0.0, 1), (0, 0.02, n_hyp, 2, 600, 0.4, 0.1, 0.6, None, 0.0, 0.8, 1),
             (0, 0.02, 17, 2, 4000, 0.0, 0.0, 1e30, None, 0.0, 0.0, 1)]
    lines = ["P %d" % len(pts)] + ["%r %r %r %r %r %r" % tuple(map(float, np.concatenate([p, m]))) for p, m in zip(pts, nrm)]
    lines += ["W %d" % smp.size, " ".join(str(int(w)) for w in smp.reshape(-1))]
    for kind, md, nh, mp, mi, sr, r0, r1, axis, cos, ncos, refine in calls:
        a = axis if axis is not None else (0, 0, 0)
        lines.append("C %d %r %d %d %d %r %r %r %d %r %r %r %r %r %d" % (
            kind, md, nh, mp, mi, sr, r0, r1, axis is not None, float(a[0]), float(a[1]), float(a[2]), cos, ncos, refine))
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert [w[0] for w in rows] == TAGS * len(calls)
    t = kdtree.New(pts)
    found = []
    for k, (kind, md, nh, mp, mi, sr, r0, r1, axis, cos, ncos, refine) in enumerate(calls):
        want = t.Shapes(kind, md, nrm, NHyp=nh, MaxShapes=mp, MinInliers=mi, SampleRadius=sr, RMin=r0, RMax=r1, Axis=axis,
                        MinAxisCos=cos, MinNormalCos=ncos, Refine=bool(refine), Samples=smp.reshape(-1)[:2 * nh * mp])
        got = {w[0]: np.array(w[1:], np.int64) for w in rows[len(TAGS) * k:len(TAGS) * (k + 1)]}
        c = want.n_shapes
        assert np.array_equal(got["L"], want.labels) and np.array_equal(got["S"], want.sizes[:c]), k
        assert np.array_equal(got["I"], want.ids) and np.array_equal(got["B"], want.best[:c]), k
        assert np.array_equal(got["R"], want.refined[:c]) and np.array_equal(got["T"], want.status.reshape(-1)), k
        assert np.array_equal(got["N"], want.counts.reshape(-1)), k
        assert np.array_equal(got["F"].astype(np.uint32), want.shapes[:c].reshape(-1).view(np.uint32)), k
        assert np.array_equal(got["H"].astype(np.uint32), want.hyp_shapes.reshape(-1).view(np.uint32)), k
        assert np.array_equal(got["M"], want.ids[len(want.ids) - want.sizes[c - 1]:] if c else want.ids[:0]), k
        found.append(c)
    assert found[0] == 3 and found[1] == 3 and found[2] == 2 and found[3] == 1 and found[4] == 0  # the calls do what they are for
