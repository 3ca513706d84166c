"""No kernel of sample consensus (csrc/sac.hip) may use scratch: Fit keeps its twelve crossing points and the edge
lists in registers (every index a compile-time constant), Evaluate its sequences and bits in LDS or global memory.
hipcc's own resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

SAC_KERNELS = ["sac_fit_kernel", "sac_evaluate_kernelILb1E", "sac_evaluate_kernelILb0E", "sac_inliers_count_kernel",
               "sac_inliers_scan_kernel", "sac_inliers_write_kernel", "sac_pack_kernel"]


def test_sac_kernels_use_no_scratch():
    ks = KR.resources("sac.hip")
    for want in SAC_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)


def test_evaluate_fits_a_cu():
    """the LDS build holds two 8192-value sequences and 80 KiB of bits: inside the CU's 160 KiB"""
    ks = KR.resources("sac.hip")
    for name, r in ks.items():
        if "sac_evaluate_kernel" in name:
            assert 0 < r.get("LDS Size", 0) <= 160 * 1024, (name, r)
