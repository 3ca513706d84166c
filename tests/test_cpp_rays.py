"""The C++ binding of the ray queries (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::RayCast and RayPierce) over the C ABI:
compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on the GPU box against the Python
binding's results, which tests/test_gpu_rays.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rays_mirror.cpp")
TAGS = ["I", "A", "O", "C"]
f32 = np.float32


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "rays_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_rays_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]
    sym = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    assert "pcgx_kdtree_raycast" in sym and "pcgx_kdtree_ray_pierce" in sym  # the mirror's calls reach the ABI


@pytest.mark.gpu
def test_cpp_rays_match_python(tmp_path):
    from pcgol_amd import kdtree, synth
    exe = _build(tmp_path)
    rng = np.random.default_rng(61)
    pts = synth.surface_cloud(3000, 5.0, 62)[0]
    t = kdtree.New(pts)
    vp = f32([2.5, 2.5, 9.0])
    aim = np.concatenate([rng.uniform(-1, 6, (300, 2)), rng.uniform(-0.5, 0.5, (300, 1))], axis=1).astype(f32)
    o, d = np.ascontiguousarray(np.broadcast_to(vp, aim.shape)), aim - vp
    lo, hi = rng.uniform(-0.2, 0.5, 300).astype(f32), rng.uniform(0.9, 1.3, 300).astype(f32)
    blocks = [(None, None, 0.1), (lo, hi, 0.15)]
    lines = ["P %d" % len(pts)] + ["%r %r %r" % tuple(map(float, p)) for p in pts]
    for a, b, rho in blocks:
        lines.append("R %d %d" % (len(o), a is not None))
        for i in range(len(o)):
            row = list(map(float, np.concatenate([o[i], d[i]]))) + ([] if a is None else [float(a[i]), float(b[i])])
            lines.append(" ".join("%r" % v for v in row))
        lines.append("Q %r" % rho)
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert [w[0] for w in rows] == TAGS * len(blocks)
    for k, (a, b, rho) in enumerate(blocks):
        ids, along, off = t.RayCast(o, d, rho, a, b)
        counts = t.RayPierce(o, d, rho, a, b)
        got = rows[4 * k:4 * k + 4]
        assert np.array_equal(np.array(got[0][1:], np.int64), ids) and (ids >= 0).sum() > 50
        assert np.array_equal(np.array([float.fromhex(v) for v in got[1][1:]]), along)
        assert np.array_equal(np.array([float.fromhex(v) for v in got[2][1:]]), off)
        assert np.array_equal(np.array(got[3][1:], np.int32), counts) and counts.any()
