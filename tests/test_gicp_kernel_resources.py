"""No kernel the Generalized ICP extension adds (csrc/icp.hip) may use scratch or spill: icp_gicp_sums_kernel keeps its
30 float64 sums and one pair's terms (gicp_terms.h, every index a compile-time constant) in registers; the set-up
kernels pack covariances; and the correspondence kernels' new instantiations that leave pairs and ids but form no sums
(icp_grid_kernel<true, false, false>, icp_corr_kernel<false, true, ., false>, icp_corr_xkernel<false, true, false>)
stay what their summing twins are (the walk kernel's instantiations, old and new, park scalar registers in vector
lanes -- "SGPRs Spill", no memory behind it -- so only the kernels written for this extension are held to zero there).
hipcc's own resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

NEW_KERNELS = ["icp_gicp_sums_kernel", "pack_base_cov_kernel", "gather_target_cov_kernel"]
GICP_KERNELS = NEW_KERNELS + ["icp_grid_kernelILb1ELb0ELb0E", "icp_corr_kernelILb0ELb1ELb1ELb0E", "icp_corr_kernelILb0ELb1ELb0ELb0E",
                "icp_corr_xkernelILb0ELb1ELb0E"]


def test_gicp_kernels_use_no_scratch():
    ks = KR.resources("icp.hip")
    for want in GICP_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            print(name, r)
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0, (name, r)
            if want in NEW_KERNELS:
                assert r.get("SGPRs Spill") == 0, (name, r)
