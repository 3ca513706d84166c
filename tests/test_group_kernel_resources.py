"""No kernel of the group geometry (csrc/group_stats.hip) may use scratch or spill: the scans, the slot -> group map, the
three gathers with their segmented reductions, the frames kernel with the Jacobi solve (A and V in registers) and the
oriented boxes.  hipcc's own resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

GROUP_KERNELS = ["gs_tile_sum_kernel", "gs_tile_scan_kernel", "gs_offsets_kernel", "gs_map_kernel", "gs_box_kernel",
                 "gs_moment_kernel", "gs_frame_kernel", "gs_extent_kernel", "gs_obb_kernel"]


def test_group_kernels_use_no_scratch():
    ks = KR.resources("group_stats.hip")
    assert len([n for n in ks if "gs_" in n]) == len(GROUP_KERNELS), sorted(ks)  # every kernel of the file is listed
    for want in GROUP_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
