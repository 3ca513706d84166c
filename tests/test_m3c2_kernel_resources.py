"""The kernels of the cylinder statistics and M3C2's finish (csrc/m3c2.hip) may use no scratch and spill nothing, in
every instantiation: source (grid, walk, patched walk) x lanes per cylinder (8, 16, 64), the scan over all points and
the finish.  hipcc's own resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

# cyl_kernel<kSrc, W>: grid (0), walk (1), patched walk (2)
M3C2_KERNELS = ["cyl_kernelILi%dELi%dE" % (s, w) for s in (0, 1, 2) for w in (8, 16, 64)] + \
               ["cyl_scan_kernel", "m3c2_finish_kernel"]


def test_m3c2_kernels_use_no_scratch():
    ks = KR.resources("m3c2.hip")
    for want in M3C2_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert len(hits) == 1, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    assert len([n for n in ks if "_kernel" in n]) == len(M3C2_KERNELS)  # every kernel is listed
