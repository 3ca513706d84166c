"""No kernel of ground segmentation (csrc/ground.hip) may use scratch or spill, and the morphology kernel holds one grid
row of 8192 words in LDS and no more: hipcc's own resource report, as tests/test_shapes_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

GROUND_KERNELS = ["ground_raster_kernel", "ground_row_kernelILb0EE", "ground_row_kernelILb1EE", "ground_classify_kernel",
                  "ground_finish_kernel", "ground_scan_kernel", "ground_scatter_kernel", "ground_surface_kernel"]


def test_ground_kernels_use_no_scratch():
    ks = KR.resources("ground.hip")
    for want in GROUND_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert len(hits) == 1, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    assert len([n for n in ks if "_kernel" in n]) == len(GROUND_KERNELS)  # every kernel is listed


def test_row_kernels_hold_one_row_in_lds():
    ks = KR.resources("ground.hip")
    hits = {n: r for n, r in ks.items() if "ground_row_kernel" in n}
    assert len(hits) == 2
    for name, r in hits.items():
        assert r.get("LDS Size") == 8192 * 4, (name, r)
