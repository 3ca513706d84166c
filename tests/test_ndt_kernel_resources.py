"""No kernel of NDT registration (csrc/ndt.hip) may use scratch or spill: the nine moments, the Jacobi solve and the
clamped reconstruction of the map kernel, and the pose, the 30 float64 accumulators and one pair's terms of every
instantiation of the sums kernel (1, 7 and 27 candidate voxels) stay in registers.  hipcc's own resource report, as
tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

NDT_KERNELS = ["ndt_sums_kernelILi%dE" % nb for nb in (1, 7, 27)] + [
    "ndt_map_kernel", "ndt_final_reduce_kernel", "ndt_valid_count_kernel", "ndt_valid_scan_kernel",
    "ndt_valid_write_kernel"]


def test_ndt_kernels_use_no_scratch():
    ks = KR.resources("ndt.hip")
    for want in NDT_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
