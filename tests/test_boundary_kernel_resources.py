"""The kernel of boundary detection (csrc/boundary.hip) may use no scratch and spill nothing in any of its three
instantiations (grid, walk, patched walk): a 64-bit mask, a count, one bit, the query and its frame are all a lane keeps,
and the tangents are literals, not a table.  hipcc's own resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

BOUNDARY_KERNELS = ["boundary_kernelILi0E", "boundary_kernelILi1E", "boundary_kernelILi2E"]


def test_boundary_kernels_use_no_scratch():
    ks = KR.resources("boundary.hip")
    for want in BOUNDARY_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert len(hits) == 1, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    assert len([n for n in ks if "_kernel" in n]) == len(BOUNDARY_KERNELS)  # every kernel is listed
