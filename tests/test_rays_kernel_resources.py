"""The kernels of the ray queries (csrc/rays.hip) may use no scratch and spill nothing: in the grid instantiation of both
modes -- a ray, its clipped range, the best hit and a ball's centre are all a lane keeps, the ray being the wave's -- and
in the others too.  hipcc's own resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

# ray_kernel<kSrc, kPierce>: grid (0), walk (1), patched walk (2), first hit (b0) and pierce (b1); and the scan over all
# points that serves a tree with non-finite coordinates
RAY_KERNELS = ["ray_kernelILi%dELb%dE" % (s, m) for s in (0, 1, 2) for m in (0, 1)] + \
              ["ray_scan_kernelILb0E", "ray_scan_kernelILb1E"]


def test_ray_kernels_use_no_scratch():
    ks = KR.resources("rays.hip")
    for want in RAY_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert len(hits) == 1, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    assert len([n for n in ks if "_kernel" in n]) == len(RAY_KERNELS)  # every kernel is listed
