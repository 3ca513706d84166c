"""No kernel of the FPFH matching (csrc/fpfh_match.hip) may use scratch or spill: fpfh_match_kernel keeps two queries'
33 + 33 floats in registers under compile-time indices, and the candidate row in scalar registers.  hipcc's own
resource report, as tests/test_fpfh_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

MATCH_KERNELS = ["fpfh_usable_kernel", "fpfh_match_kernel", "fpfh_merge_kernel", "fpfh_corr_kernel"]


def test_match_kernels_use_no_scratch():
    ks = KR.resources("fpfh_match.hip")
    assert len(ks) == len(MATCH_KERNELS), sorted(ks)  # every kernel of the file is named here
    for want in MATCH_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
