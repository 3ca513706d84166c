"""The C++ binding of the pose estimation (pcgol_amd/host/pcgx.hpp, pcgx::pose_from_correspondences) over the C ABI:
compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_pose.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pose_oracle import scene_m_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pose_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "pose_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_pose_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_pose_matches_python(tmp_path):
    from pcgol_amd import alignment
    exe = _build(tmp_path)
    s, _ = scene_m_reference()
    P, Q = s["P"].copy(), s["Q"].copy()
    P[s["src"][7], 1] = np.nan  # a point that is never an inlier
    samples = s["samples"][:600]
    lines = []
    for tag, pts in (("P", P), ("Q", Q)):
        lines.append("%s %d" % (tag, len(pts)))
        lines += [" ".join(repr(float(v)) for v in r) for r in pts]
    lines.append("C %d" % len(s["src"]))
    lines += ["%d %d" % (a, b) for a, b in zip(s["src"], s["dst"])]
    lines.append("U %d" % len(samples))
    lines += ["%d %d %d" % tuple(u) for u in samples]
    cases = [(0.01, 0.9, 1), (0.01, 0.0, 0), (0.02, 0.5, 1)]
    lines += ["E %r %r %d" % c for c in cases]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.split("\n")
    pairs = np.stack([s["src"], s["dst"]], axis=1)
    for i, (max_dist, es, refine) in enumerate(cases):
        head = out[3 * i].split()
        assert head[0] == "E"
        found, pose, ids, info = alignment.EstimatePose(P, Q, pairs, 0, max_dist, EdgeSimilarity=es, Refine=bool(refine),
                                                        samples=samples)
        assert [int(x) for x in head[1:]] == [int(found), info["best"], info["best_count"], int(info["refined"]), len(ids)]
        assert np.array_equal(np.array([float(x) for x in out[3 * i + 1].split()], np.float32).view(np.uint32),
                              pose.view(np.uint32))
        assert np.array_equal(np.array([int(x) for x in out[3 * i + 2].split()], np.int64), ids)
        assert found and 7 not in ids and info["refined"] == bool(refine)
