"""The C++ binding of the cylinder statistics and M3C2's finish (pcgol_amd/host/pcgx.hpp, pcgx::KDTree::CylinderStats and
pcgx::M3C2Finish) over the C ABI: compiled with g++ everywhere (CPU check: it builds and links against libpcgx.so), run on
the GPU box against the Python binding's results, which tests/test_gpu_m3c2.py compares with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "m3c2_mirror.cpp")
TAGS = ["N1", "S1", "N2", "S2", "D", "L", "G"]
f32 = np.float32


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "m3c2_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_m3c2_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]
    sym = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    assert "pcgx_kdtree_cylinder_stats" in sym and "pcgx_m3c2_finish" in sym  # the mirror's calls reach the ABI


@pytest.mark.gpu
def test_cpp_m3c2_matches_python(tmp_path):
    from pcgol_amd import change, kdtree, synth
    exe = _build(tmp_path)
    rng = np.random.default_rng(61)
    e1 = synth.surface_cloud(3000, 5.0, 62)[0]
    e2 = synth.surface_cloud(3000, 5.0, 63)[0]
    e2[:, 2] += f32(0.125) * (e2[:, 1] > 2.5)
    t1, t2 = kdtree.New(e1), kdtree.New(e2)
    cores = np.ascontiguousarray(e1[rng.choice(len(e1), 300, replace=False)])
    axes = t1.Normals(0.4, Queries=cores)[0]
    axes[::50] = 0  # unusable ones
    blocks = [(0.2, 0.5, 0.0, 4), (0.3, 1.0, 0.02, 10)]
    lines = []
    for e in (e1, e2):
        lines += ["P %d" % len(e)] + ["%r %r %r" % tuple(map(float, p)) for p in e]
    lines.append("C %d" % len(cores))
    lines += [" ".join("%r" % float(v) for v in np.concatenate([cores[i], axes[i]])) for i in range(len(cores))]
    lines += ["Q %r %r %r %d" % b for b in blocks]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [w.split() for w in r.stdout.rstrip("\n").split("\n")]
    assert [w[0] for w in rows] == TAGS * len(blocks)

    def floats(w):
        return np.array([float.fromhex(v) if "0x" in v else float(v) for v in w[1:]])  # ("nan" is printed as such)
    for k, (rho, half, reg, mc) in enumerate(blocks):
        n1, s1 = t1.CylinderStats(cores, axes, rho, half)
        n2, s2 = t2.CylinderStats(cores, axes, rho, half)
        dist, lod, sig, _, _ = change.M3C2(rho, half, change.WithRegistrationError(reg),
                                           change.WithMinCount(mc)).Compute(t1, t2, cores, axes)
        got = rows[7 * k:7 * k + 7]
        assert np.array_equal(np.array(got[0][1:], np.int32), n1) and np.array_equal(np.array(got[2][1:], np.int32), n2)
        assert np.array_equal(floats(got[1]), s1.reshape(-1)) and np.array_equal(floats(got[3]), s2.reshape(-1))
        assert np.array_equal(floats(got[4]), dist, equal_nan=True) and np.array_equal(floats(got[5]), lod, equal_nan=True)
        assert np.array_equal(np.array(got[6][1:], np.int32).astype(bool), sig)
        assert n1.sum() > 1000 and sig.any() and not sig.all() and np.isnan(dist[::50]).all()
