"""No kernel of FPFH at chosen points (csrc/fpfh.hip: fpfh_mark_kernel, spfh_kernel<., true>, fpfh_kernel<., true> and
the two flag-count kernels) may use scratch or spill, on any of the three neighbourhood sources: the marking stage keeps
nothing per neighbour, and the other two are spfh_kernel and fpfh_kernel over other queries, whose counters live in
LDS and whose accumulators are indexed by compile-time constants (tests/test_fpfh_kernel_resources.py).  hipcc's own
resource report, as tests/test_normals_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

FPFH_AT_KERNELS = ["fpfh_mark_kernelILi0E", "fpfh_mark_kernelILi1E", "fpfh_mark_kernelILi2E",
                   "spfh_kernelILi0ELb1E", "spfh_kernelILi1ELb1E", "spfh_kernelILi2ELb1E",
                   "fpfh_kernelILi0ELb1E", "fpfh_kernelILi1ELb1E", "fpfh_kernelILi2ELb1E",
                   "fpfh_need_count_kernel", "fpfh_need_scan_kernel"]


def test_fpfh_at_kernels_use_no_scratch():
    ks = KR.resources("fpfh.hip")
    for want in FPFH_AT_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
