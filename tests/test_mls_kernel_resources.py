"""No kernel of moving-least-squares smoothing (csrc/mls.hip) may use scratch: the nine moments and the box of pass 1,
the frame (14 float64), the 28 float64 sums of the normal equations, a second set of them while the wave shares a fat
row, and the 6 x 6 Cholesky (every index a compile-time constant after unrolling) stay in registers.  hipcc's own
resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

# mls_kernel<kSrc, kOrder>: grid, walk, xwalk x order 1, 2
MLS_KERNELS = ["mls_kernelILi%dELi%dE" % (src, order) for src in (0, 1, 2) for order in (1, 2)]


def test_mls_kernels_use_no_scratch():
    ks = KR.resources("mls.hip")
    for want in MLS_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
