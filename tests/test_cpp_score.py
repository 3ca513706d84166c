"""The C++ binding of the whole-cloud verification (pcgol_amd/host/pcgx.hpp, pcgx::score_poses and pcgx::pose_select)
over the C ABI: compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box
against the Python binding's results, which tests/test_gpu_score_poses.py compares with the reference and the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_oracle as SO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "score_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "score_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_score_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_score_matches_python(tmp_path):
    from pcgol_amd import alignment, kdtree
    exe = _build(tmp_path)
    s = SO.decoy_scene()
    poses = SO.main_poses()
    P = s["P"].copy()
    P[11, 2] = np.inf  # a point that is never a pair
    status = np.array([0, 0, 1, 0, 0, 0], np.int32)
    counts = np.array([5, 9, 50, 9, 2, 3], np.int64)
    lines = []
    for tag, pts in (("T", s["Q"]), ("P", P)):
        lines.append("%s %d" % (tag, len(pts)))
        lines += [" ".join(repr(float(v)) for v in r) for r in pts]
    lines.append("M %d" % len(poses))
    lines += [" ".join(repr(float(v)) for v in m) for m in poses]
    dists = [0.02, 10.0]
    lines += ["S %r" % d for d in dists]
    lines.append("H %d" % len(status))
    lines += ["%d %d" % (a, b) for a, b in zip(status, counts)]
    ks = [3, 6, 0]
    lines += ["L %d" % k for k in ks]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.split("\n")
    tree = kdtree.New(s["Q"])
    for i, d in enumerate(dists):
        c, sums, best, pose = alignment.ScorePoses(tree, P, poses, d)
        assert out[4 * i].split() == ["S", str(best)]
        assert [int(x) for x in out[4 * i + 1].split()] == c.tolist()
        assert [float(x) for x in out[4 * i + 2].split()] == sums.tolist()  # (a fixed summation order: the same bits)
        assert np.array_equal(np.array([float(x) for x in out[4 * i + 3].split()], np.float32).view(np.uint32),
                              pose.view(np.uint32))
        assert c[0] == 2999
    base = 4 * len(dists)
    for i, k in enumerate(ks):
        ids, _, n_sel = alignment.SelectPoses(status, counts, poses, k)
        assert out[base + 2 * i].split() == ["L", str(n_sel)]
        assert [int(x) for x in out[base + 2 * i + 1].split()] == ids.tolist()
