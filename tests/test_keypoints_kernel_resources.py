"""The suppression kernel of keypoint detection (csrc/keypoints.hip) may use no scratch and spill nothing in any of its
three instantiations (grid, walk, patched walk): two bits, the query and its score are all a lane keeps.  hipcc's own
resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

KEYPOINT_KERNELS = ["local_maxima_kernelILi0E", "local_maxima_kernelILi1E", "local_maxima_kernelILi2E",
                    "keypoints_count_kernel", "keypoints_scan_kernel", "keypoints_write_kernel", "keypoints_tail_kernel"]


def test_keypoint_kernels_use_no_scratch():
    ks = KR.resources("keypoints.hip")
    for want in KEYPOINT_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
