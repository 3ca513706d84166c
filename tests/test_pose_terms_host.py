"""csrc/pose_terms.h compiled for the host with g++ -ffp-contract=off into a stand-alone program
(tests/cpp/pose_terms_host.cpp over the shim tests/cpp/host_shim): the statuses the kernels compile are the NumPy
oracle's (tests/pose_oracle.py) on scene M's 4096 hypotheses and on the cases worked by hand, and the rigid solve (Horn's
quaternion by Jacobi) agrees with the oracle's (Kabsch by SVD) within 2^-23 max(1, |.|) per number wherever both
triangles have sin^2 >= 1e-4; the refit over scene M's best inlier set is held to the same bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_oracle as PO  # noqa: E402
from test_pose_oracle import hand_cases, line_scene, lower_refit_scene, scene_m_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, u32 = np.float32, np.float64, np.uint32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_terms")
    exe = str(d / "pose_terms_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "pose_terms_host.cpp")])

    def run(P, Q, src, dst, samples, es, refit_ids=()):
        P, Q = np.ascontiguousarray(P, f32), np.ascontiguousarray(Q, f32)
        samples = np.ascontiguousarray(samples, u32).reshape(-1, 3)
        refit_ids = np.asarray(refit_ids, np.int32)
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([len(P), len(Q), len(src), len(samples), len(refit_ids)], np.int64).tobytes())
            f.write(f32(es).tobytes())
            for a in (P, Q, np.asarray(src, np.int32), np.asarray(dst, np.int32), samples, refit_ids):
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([exe, inp, out])
        raw = open(out, "rb").read()
        n = len(samples)
        status = np.frombuffer(raw, np.int32, n)
        poses = np.frombuffer(raw, f32, 16 * n, 4 * n).reshape(n, 16)
        if not len(refit_ids):
            return status, poses
        at = 4 * n + 64 * n
        allowed = int(np.frombuffer(raw, np.int32, 1, at)[0])
        return status, poses, allowed, np.frombuffer(raw, f32, 16, at + 4), np.frombuffer(raw, f64, 2, at + 68)

    return run


def test_hand_cases(host):
    for name, c in hand_cases().items():
        st, poses = host(c["P"], c["Q"], c["src"], c["dst"], c["samples"], c["es"])
        assert st.tolist() == c["status"], name
        assert not poses[st != 0].any(), name
        if "pose" in c:
            assert PO.pose_close(poses[0], c["pose"])[0], (name, poses[0])
            assert poses[0][[3, 7, 11, 15]].tolist() == [0, 0, 0, 1]
    # a pure translation of a lattice triangle is found exactly: N is diagonal, the quaternion is (1, 0, 0, 0)
    c = hand_cases()["translation"]
    assert np.array_equal(host(c["P"], c["Q"], c["src"], c["dst"], c["samples"], c["es"])[1][0], c["pose"])


def test_scene_m(host):
    for es in (0.9, 0.0):
        s, r = scene_m_reference(es)
        st, poses = host(s["P"], s["Q"], s["src"], s["dst"], s["samples"], es)
        assert np.array_equal(st, r["status"]), es
        assert not poses[st != 0].any()
        assert np.all(poses[st == 0][:, [3, 7, 11, 15]] == np.array([0, 0, 0, 1], f32))
        well = PO.well_conditioned(s["P"], s["Q"], s["src"], s["dst"], r["idx"]) & (st == 0)
        assert well.sum() >= 0.95 * (st == 0).sum()
        ok, worst = PO.pose_close(poses[well], r["own_poses"][well])
        print("edge_similarity %.1f: %d status-0 hypotheses, %d compared; largest pose difference %.3f of the bound "
              "2^-23 max(1, |.|)" % (es, (st == 0).sum(), well.sum(), worst))
        assert ok, worst
        # a proper rotation, never a reflection
        R = poses[st == 0][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3).astype(f64)
        assert np.all(np.linalg.det(R) > 0.999)


def test_refit(host):
    s, r = scene_m_reference()
    ids = r["best_inliers"]
    _, _, allowed, pose, l = host(s["P"], s["Q"], s["src"], s["dst"], s["samples"][:1], 0.9, ids)
    ok, worst = PO.pose_close(pose, r["refit_pose"])
    print("refit over scene M's %d best inliers: largest difference %.3f of the bound; l1 %.6g l2 %.6g" % (len(ids), worst, *l))
    assert allowed == 1 and ok, worst
    # the degeneracy rule: a line is not refitted, two pairs are not, the oracle's (l1, l1 - l2) are the solve's
    s = line_scene()
    assert host(s["P"], s["Q"], s["src"], s["dst"], s["samples"], 0.0, [3, 4, 5, 6, 7])[2] == 0
    assert host(s["P"], s["Q"], s["src"], s["dst"], s["samples"], 0.0, [3, 4])[2] == 0
    _, _, allowed, pose, l = host(s["P"], s["Q"], s["src"], s["dst"], s["samples"], 0.0, [0, 3, 4])
    A, B, _ = PO.pair_points(s["P"], s["Q"], s["src"], s["dst"])
    _, _, S, d = PO.kabsch(A[[0, 3, 4]], B[[0, 3, 4]])
    big = np.abs((A[[0, 3, 4]].astype(f64) - A[[0, 3, 4]].astype(f64).mean(0)).T
                 @ (B[[0, 3, 4]].astype(f64) - B[[0, 3, 4]].astype(f64).mean(0))).max()
    assert allowed == 1 and PO.pose_close(pose, PO.refit(A, B, np.array([0, 3, 4])))[0]
    assert abs(l[0] * big - (S[0] + S[1] + d * S[2])) < 1e-9 * S[0] and abs((l[0] - l[1]) * big - 2 * (S[1] + d * S[2])) < 1e-9 * S[0]
    s = lower_refit_scene()
    want = PO.estimate(s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["max_dist_sq"], s["es"], True)
    _, _, allowed, pose, _ = host(s["P"], s["Q"], s["src"], s["dst"], s["samples"], s["es"], np.arange(7))
    assert allowed == 1 and PO.pose_close(pose, want["refit_pose"])[0]
