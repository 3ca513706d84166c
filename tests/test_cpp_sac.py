"""The C++ mirror of pc/sac (pcgol_amd/host/pcgx.hpp, pcgx::sac) over the C ABI: compiled with g++ everywhere (CPU
check: it builds and links against libpcgx.so), run on the GPU box against the reference's tables
(tests/golden/ref_sac.json) and the oracle (tests/sac_oracle.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sac_mirror.cpp")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _build(tmpdir):
    from pcgol_amd import build as B
    B.build()
    exe = os.path.join(str(tmpdir), "sac_mirror")
    libdir = os.path.join(ROOT, "pcgol_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC, "-L" + libdir, "-lpcgx",
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_sac_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpcgx.so" in out and "not found" not in out.split("libpcgx.so")[1].split("\n")[0]


def _grid_lines(res, size, origin, pts):
    lines = ["G %r %d %d %d %r %r %r %d" % (res, *size, *map(float, np.float32(origin)), len(pts))]
    return lines + ["%r %r %r" % tuple(map(float, p)) for p in np.asarray(pts, np.float32)]


@pytest.mark.gpu
def test_cpp_sac_mirror_known_answers(tmp_path, golden):
    import sac_oracle as S
    exe = _build(tmp_path)
    g = golden("ref_sac.json")
    s = g["surface"]
    lines = []
    for c in s["cases"]:
        pts = s["clouds"][c["cloud"]]
        lines += _grid_lines(s["resolution"], s["size"], c["origin"], pts)
        lines.append("F %d %d %d %r" % (*s["fit_ids"], s["inlier_d"]))
        for ids in s["failing_fits"].values():
            lines.append("F %d %d %d %r" % (*ids, s["inlier_d"]))
    t = g["sac"]
    lines += _grid_lines(t["resolution"], t["size"], t["origin"], t["points"])
    for seed in range(5):
        lines.append("S %d %d %r" % (seed, t["n"], t["inlier_d"]))
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.strip().split("\n")
    k = 0
    for c in s["cases"]:
        pts = np.array(s["clouds"][c["cloud"]], np.float32)
        om = S.SurfaceModel(S.Grid(s["resolution"], s["size"], c["origin"], pts), pts)
        oc, _ = om.Fit(s["fit_ids"])
        w = out[k].split()
        k += 1
        assert w[4] == "ok" and int(w[6]) == oc.Evaluate(), (c["name"], out[k - 1])
        inl = [int(x) for x in w[8:w.index("isin")]]
        assert sorted(inl) == s["expected_inliers"], c["name"]
        isin = w[w.index("isin") + 1]
        for i, want in s["is_in"]:
            assert (isin[i] == "1") == want, (c["name"], i)
        assert isin == "".join("1" if oc.IsIn(p, s["inlier_d"]) else "0" for p in pts)
        for _ in s["failing_fits"]:
            assert out[k].endswith("failed"), out[k]
            k += 1
    for seed in range(5):
        w = out[k].split()
        k += 1
        assert w[0] == "sac" and w[1] == "1", out[k - 1]
        assert [int(x) for x in w[5:]] == t["expected_inliers"], (seed, out[k - 1])
