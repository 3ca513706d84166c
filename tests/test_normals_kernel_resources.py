"""No kernel of normal estimation (csrc/normals.hip) may use scratch: the nine float64 moments, the neighbours' box and
the 3 x 3 Jacobi solve (every index a compile-time constant) stay in registers.  Nor may the kernel that gathers a
tree's own points for normals and k nearest neighbours (csrc/range.hip, query_source).  hipcc's own resource report, as
tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

NORMALS_KERNELS = {"normals.hip": ["normals_kernelILi0E", "normals_kernelILi1E", "normals_kernelILi2E"],
                   "range.hip": ["own_points_kernel"]}


def test_normals_kernels_use_no_scratch():
    for source, names in NORMALS_KERNELS.items():
        ks = KR.resources(source)
        for want in names:
            hits = {n: r for n, r in ks.items() if want in n}
            assert hits, (want, sorted(ks))
            for name, r in hits.items():
                assert r.get("ScratchSize") == 0, (name, r)
                assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
