"""No kernel of the whole-cloud verification (csrc/pose_score.hip) may use scratch or spill: score_fused_kernel keeps its
pose in scalar registers and the grid search's state, the count and the float64 sum in vector registers; the selection
and the tails are small.  hipcc's own resource report, as tests/test_pose_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

SCORE_KERNELS = ["score_key_kernel", "score_gather_kernel", "score_fused_kernel", "score_walk_add_kernel",
                 "score_transform_kernel", "score_count_kernel", "score_reduce_kernel", "score_finish_kernel",
                 "pose_select_kernel"]


def test_score_kernels_use_no_scratch():
    ks = KR.resources("pose_score.hip")
    assert len(ks) == len(SCORE_KERNELS), sorted(ks)  # every kernel of the file is named here
    for want in SCORE_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
