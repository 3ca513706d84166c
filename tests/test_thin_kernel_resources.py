"""The kernels of minimum-distance subsampling (csrc/thin.hip) may use no scratch and spill nothing: the round kernel in
its three sources and both priority modes -- a lane keeps its point, its priority and three bits --, the owner kernel in
its three sources, and the commit / scan / write kernels of the list compaction.  hipcc's own resource report, as
tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

# thin_round_kernel<kSrc, kScore>: grid (0), walk (1), patched walk (2), hash (b0) and score (b1) mode
THIN_KERNELS = ["thin_round_kernelILi%dELb%dE" % (s, m) for s in (0, 1, 2) for m in (0, 1)] + \
               ["thin_owner_kernelILi%dE" % s for s in (0, 1, 2)] + \
               ["thin_prep_kernel", "thin_commit_kernel", "thin_scan_kernel", "thin_write_kernel"]


def test_thin_kernels_use_no_scratch():
    ks = KR.resources("thin.hip")
    for want in THIN_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert len(hits) == 1, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    assert len([n for n in ks if "_kernel" in n]) == len(THIN_KERNELS)  # every kernel is listed
