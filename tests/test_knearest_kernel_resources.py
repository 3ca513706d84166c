"""No kernel of k nearest neighbours (csrc/knearest.hip) or of statistical outlier removal (csrc/sor.hip) may use
scratch: each lane's best k live in LDS laid out [slot][lane], never in a runtime-indexed register array.  Nor may the
kernel that gathers the tree's own points for q == NULL without a grid (csrc/range.hip, query_source).  hipcc's own
resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

KNEAREST_KERNELS = ["knearest_kernelILi0ELb0E", "knearest_kernelILi1ELb0E", "knearest_kernelILi2ELb0E",
                    "knearest_kernelILi0ELb1E", "knearest_kernelILi1ELb1E", "knearest_kernelILi2ELb1E"]
SOR_KERNELS = ["sor_finite_count_kernel", "sor_scan_kernel", "sor_finite_write_kernel", "sor_nan_kernel",
               "sor_place_kernel", "sor_partial_kernelILi0E", "sor_partial_kernelILi1E", "sor_final_kernelILi0E",
               "sor_final_kernelILi1E", "sor_keep_count_kernel", "sor_keep_write_kernel"]


def _check(src, names):
    ks = KR.resources(src)
    for want in names:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)


def test_knearest_kernels_use_no_scratch():
    _check("knearest.hip", KNEAREST_KERNELS)
    _check("range.hip", ["own_points_kernel"])


def test_sor_kernels_use_no_scratch():
    _check("sor.hip", SOR_KERNELS)
