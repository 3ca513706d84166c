"""The C++ binding of the FPFH matching (pcgol_amd/host/pcgx.hpp, pcgx::fpfh_match / pcgx::fpfh_correspondences) over
the C ABI: compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against
the Python binding's results, which tests/test_gpu_match.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_oracle as MO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "match_mirror.cpp")


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "match_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_match_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_match_matches_python(tmp_path):
    from pcgol_amd import features
    exe = _build(tmp_path)
    A, B = MO.scene_r(300, 257, seed=19)
    A[[0, 64, 299]] = 0.0  # unusable queries ...
    B[[1, 128]] = 0.0      # ... and candidates
    B[200, 5] = np.nan
    A[10] = B[20]
    lines = []
    for tag, rows in (("A", A), ("B", B)):
        lines.append("%s %d" % (tag, len(rows)))
        lines += [" ".join(repr(float(v)) for v in r) for r in rows]
    lines += ["M", "C 1.0 1", "C 0.9 0"]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.strip().split("\n")
    m = [w.split() for w in out[:len(A)]]
    assert all(w[0] == "M" and len(w) == 4 for w in m)
    ids, d1, d2 = features.Match(A, B)
    assert np.array_equal(np.array([int(w[1]) for w in m]), ids)
    assert np.array_equal(np.array([float(w[2]) for w in m], np.float32).view(np.uint32), d1.view(np.uint32))
    assert np.array_equal(np.array([float(w[3]) for w in m], np.float32).view(np.uint32), d2.view(np.uint32))
    assert ids[0] == -1 and ids[10] == 20 and d1[10] == 0 and np.isinf(d2[0])
    at = len(A)
    for ratio, mutual in ((1.0, True), (0.9, False)):
        head = out[at].split()
        assert head[0] == "C"
        n = int(head[1])
        got = np.array([[int(x) for x in w.split()] for w in out[at + 1:at + 1 + n]], np.int64).reshape(-1, 2)
        assert np.array_equal(got, features.Correspondences(A, B, ratio, mutual)) and n > 0
        at += 1 + n
    assert at == len(out)
