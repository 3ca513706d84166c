"""No kernel of plane segmentation (csrc/planes.hip) may use scratch or spill, and the count kernel -- hypotheses x points,
two hypotheses a lane -- needs no LDS: hipcc's own resource report, as tests/test_dbscan_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

M = "INS_10PlaneModelE"  # the round machinery's kernels (csrc/consensus_peel.h) as instantiated on planes.hip's model
PLANES_KERNELS = ["peel_gather_kernel", "peel_empty_kernelILi4EE", "planes_fit_kernel", "planes_count_kernelILb0EE",
                  "planes_count_kernelILb1EE", "peel_select_kernel" + M + "EE", "peel_tile_count_kernel" + M + "Li0EE",
                  "peel_tile_count_kernel" + M + "Li1EE", "peel_tile_count_kernel" + M + "Li2EE",
                  "peel_scan_kernel" + M + "Li0EE", "peel_scan_kernel" + M + "Li1EE", "peel_scan_kernel" + M + "Li2EE",
                  "peel_scatter_kernel" + M + "Li0EE", "peel_scatter_kernel" + M + "Li1EE",
                  "peel_scatter_kernel" + M + "Li2EE", "planes_refit_kernel", "peel_round_end_kernel" + M + "EE"]


def test_planes_kernels_use_no_scratch():
    ks = KR.resources("planes.hip")
    for want in PLANES_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert len(hits) == 1, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    assert len([n for n in ks if "_kernel" in n]) == len(PLANES_KERNELS)  # every kernel is listed


def test_count_kernel_needs_no_lds():
    ks = KR.resources("planes.hip")
    hits = {n: r for n, r in ks.items() if "planes_count_kernel" in n}
    assert len(hits) == 2
    for name, r in hits.items():
        assert r.get("LDS Size") == 0, (name, r)
