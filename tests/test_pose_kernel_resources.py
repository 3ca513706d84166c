"""No kernel of the pose estimation (csrc/pose.hip) may use scratch or spill: pose_count_kernel keeps two hypotheses'
12 + 12 pose numbers in registers under compile-time indices and the pair record in scalar registers; pose_fit_kernel
and pose_finish_kernel hold the 4 x 4 Jacobi solve's two matrices in registers.  hipcc's own resource report, as
tests/test_match_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

POSE_KERNELS = ["pose_gather_kernel", "pose_fit_kernel", "pose_count_kernel", "pose_finish_kernel"]


def test_pose_kernels_use_no_scratch():
    ks = KR.resources("pose.hip")
    assert len(ks) == len(POSE_KERNELS), sorted(ks)  # every kernel of the file is named here
    for want in POSE_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
