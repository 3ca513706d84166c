"""The C++ binding of minimum-distance subsampling (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::Thin) over the C ABI:
compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_thin.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "thin_mirror.cpp")
f32 = np.float32


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "thin_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_thin_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]
    sym = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    assert "pcgx_kdtree_thin" in sym  # the mirror's call reaches the ABI


@pytest.mark.gpu
def test_cpp_thin_matches_python(tmp_path):
    from pcgol_amd import kdtree, synth
    exe = _build(tmp_path)
    pts = synth.uniform_cloud(3000, 1.0, 71)
    t = kdtree.New(pts)
    score = np.random.default_rng(72).integers(0, 5, len(pts)).astype(f32)
    score[::97] = np.nan
    blocks = [(None, 0.1, 0), (None, 0.1, 4000000000), (score, 0.15, 0)]
    lines = ["P %d" % len(pts)] + ["%r %r %r" % tuple(map(float, p)) for p in pts]
    for s, r, seed in blocks:
        lines.append("S %d" % (0 if s is None else len(s)))
        if s is not None:
            lines.append(" ".join("nan" if np.isnan(v) else "%r" % float(v) for v in s))
        lines.append("Q %r %d" % (r, seed))
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert [w[0] for w in rows] == ["K", "O"] * len(blocks)
    for k, (s, rad, seed) in enumerate(blocks):
        ids, owner = t.Thin(rad, Seed=seed, Score=s, Owner=True)
        assert np.array_equal(np.array(rows[2 * k][1:], np.int64), ids) and 50 < len(ids) < 2000
        assert np.array_equal(np.array(rows[2 * k + 1][1:], np.int64), owner)
        assert (s is None) or (owner[::97] == -1).all()
