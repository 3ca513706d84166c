"""No kernel of cylinder and sphere segmentation (csrc/shapes.hip) may use scratch or spill, and the count kernels --
hypotheses x points, two hypotheses a lane -- need no LDS: hipcc's own resource report, as
tests/test_planes_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

M = "INS_10ShapeModelE"  # the round machinery's kernels (csrc/consensus_peel.h) as instantiated on shapes.hip's model
SHAPES_KERNELS = ["peel_gather_kernel", "peel_empty_kernelILi8EE", "shapes_partner_kernelILi0EE", "shapes_partner_kernelILi1EE",
                  "shapes_partner_kernelILi2EE", "shapes_fit_kernel", "shapes_count_kernelILi0ELb0EE",
                  "shapes_count_kernelILi0ELb1EE", "shapes_count_kernelILi1ELb0EE", "shapes_count_kernelILi1ELb1EE",
                  "peel_select_kernel" + M + "EE", "peel_tile_count_kernel" + M + "Li0EE",
                  "peel_tile_count_kernel" + M + "Li1EE", "peel_tile_count_kernel" + M + "Li2EE",
                  "peel_scan_kernel" + M + "Li0EE", "peel_scan_kernel" + M + "Li1EE", "peel_scan_kernel" + M + "Li2EE",
                  "peel_scatter_kernel" + M + "Li0EE", "peel_scatter_kernel" + M + "Li1EE",
                  "peel_scatter_kernel" + M + "Li2EE", "shapes_sums_kernel", "shapes_refit_kernel",
                  "peel_round_end_kernel" + M + "EE"]


def test_shapes_kernels_use_no_scratch():
    ks = KR.resources("shapes.hip")
    for want in SHAPES_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert len(hits) == 1, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    assert len([n for n in ks if "_kernel" in n]) == len(SHAPES_KERNELS)  # every kernel is listed


def test_count_kernels_need_no_lds():
    ks = KR.resources("shapes.hip")
    hits = {n: r for n, r in ks.items() if "shapes_count_kernel" in n}
    assert len(hits) == 4
    for name, r in hits.items():
        assert r.get("LDS Size") == 0, (name, r)
