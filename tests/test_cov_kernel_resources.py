"""No kernel of k-NN covariances (csrc/knearest.hip, knearest_kernel<kSrc, false, true>) may use scratch or spill: the
list stays in LDS laid out [slot][lane], the moments and the 3 x 3 Jacobi solve (cov3.h, every index a compile-time
constant) in registers.  Nor may the kernel that makes the id -> node map the covariances fetch through
(csrc/range.hip, range_inverse_map).  hipcc's own resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

COV_KERNELS = {"knearest.hip": ["knearest_kernelILi0ELb0ELb1E", "knearest_kernelILi1ELb0ELb1E",
                                "knearest_kernelILi2ELb0ELb1E"],
               "range.hip": ["range_invert_nodes_kernel"]}


def test_covariance_kernels_use_no_scratch():
    for source, names in COV_KERNELS.items():
        ks = KR.resources(source)
        for want in names:
            hits = {n: r for n, r in ks.items() if want in n}
            assert hits, (want, sorted(ks))
            for name, r in hits.items():
                assert r.get("ScratchSize") == 0, (name, r)
                assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
