"""The SAC oracle (tests/sac_oracle.py) against the reference's own tables (tests/golden/ref_sac.json), and its
vectorised Evaluate against the per-sample loop of surface.go:202-220.  CPU only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sac_oracle as S  # noqa: E402


def _surface_cases(golden):
    s = golden("ref_sac.json")["surface"]
    for c in s["cases"]:
        yield s, c, np.array(s["clouds"][c["cloud"]], np.float32)


def test_surface_table(golden):
    for s, c, pts in _surface_cases(golden):
        m = S.SurfaceModel(S.Grid(s["resolution"], s["size"], c["origin"], pts), pts)
        co, ok = m.Fit(s["fit_ids"])
        assert ok, c["name"]
        assert sorted(co.Inliers(s["inlier_d"]).tolist()) == s["expected_inliers"], c["name"]
        for i, want in s["is_in"]:
            assert co.IsIn(pts[i], s["inlier_d"]) == want, (c["name"], i)
        for name, ids in s["failing_fits"].items():
            assert m.Fit(ids) == (None, False), (c["name"], name)


def test_sac_table(golden):
    t = golden("ref_sac.json")["sac"]
    pts = np.array(t["points"], np.float32)
    m = S.SurfaceModel(S.Grid(t["resolution"], t["size"], t["origin"], pts), pts)
    for seed in range(8):
        ids = np.random.default_rng(seed).integers(0, len(pts), size=3 * t["n"])
        found, best, _, per = S.compute(m, ids, t["n"])
        assert found
        assert per[best][0].Inliers(t["inlier_d"]).tolist() == t["expected_inliers"], seed
    assert S.compute(m, [], 0)[:3] == (False, -1, 0)


def _random_scene(rng):
    res = float(rng.choice([0.05, 0.1, 0.25]))
    size = rng.integers(3, 12, size=3)
    origin = (rng.random(3) - 0.5).astype(np.float32)
    ext = size * res
    pts = (origin + rng.random((int(rng.integers(20, 200)), 3)) * ext * 1.2 - 0.1 * ext).astype(np.float32)
    return S.Grid(res, size, origin, pts), pts


def test_vectorised_evaluate_is_the_literal_loop():
    rng = np.random.default_rng(7)
    checked = 0
    while checked < 200:
        vg, pts = _random_scene(rng)
        m = S.SurfaceModel(vg, pts)
        for _ in range(20):
            c, ok = m.Fit([int(i) for i in rng.integers(0, len(pts), size=3)])
            if not ok:
                continue
            assert c.Evaluate() == c.evaluate_literal()
            checked += 1


def test_degenerate_fits():
    pts = np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.1, 0.3, 0.1], [0.5, 0.1, 0.1]], np.float32)
    m = S.SurfaceModel(S.Grid(0.1, (8, 8, 8), (0, 0, 0), pts), pts)
    assert m.Fit([0, 0, 1]) == (None, False)        # repeated id
    assert m.Fit([0, 1, 3]) == (None, False)        # collinear
    c, ok = m.Fit([0, 1, 2])                        # z = const: nValid = {false, false, true}
    assert ok and c.norm[0] == 0 and c.norm[1] == 0
    assert c.Evaluate() == len(pts)
    assert m.Fit([0, 1]) == (None, False)           # len(ids) != 3
