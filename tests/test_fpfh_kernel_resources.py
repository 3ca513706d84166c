"""No kernel of the FPFH descriptors (csrc/fpfh.hip) may use scratch: spfh_kernel's counters are indexed by a bin known
only at run time and live in an LDS table for that reason, fpfh_kernel's 33 float64 accumulators and the nine uint4 of
a record are indexed by compile-time constants and stay in registers.  hipcc's own resource report, as
tests/test_normals_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

FPFH_KERNELS = ["spfh_kernelILi0ELb0E", "spfh_kernelILi1ELb0E", "spfh_kernelILi2ELb0E",
                "fpfh_kernelILi0ELb0E", "fpfh_kernelILi1ELb0E", "fpfh_kernelILi2ELb0E"]


def test_fpfh_kernels_use_no_scratch():
    ks = KR.resources("fpfh.hip")
    for want in FPFH_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
