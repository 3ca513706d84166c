"""No kernel of cluster extraction (csrc/cluster.hip) may use scratch or spill: the staging gathers, every instantiation
of the grid passes and of the walk's union (no read, flags, normals), the per-root counts, the naming, the ranking and
the grouping stay in registers -- and so do the pointer jumping (csrc/uf.h) and the component passes
(csrc/radius_graph.h) the file shares with region growing, in both files.  hipcc's own resource report, as
tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

CLUSTER_KERNELS = ["rgraph_grid_kernelILb%dENS_11ClusterEdgeILi%dE" % (h, c) for h in (0, 1) for c in (0, 1, 2)] + [
    "rgraph_walk_kernelINS_11ClusterEdgeILi1E", "rgraph_walk_kernelINS_11ClusterEdgeILi2E", "cl_init_kernel",
    "cl_stage_grid_kernel", "cl_stage_tree_kernel", "cl_root_stats_kernel", "cl_name_kernel", "cl_rank_kernel",
    "cl_label_kernel", "cl_ids_kernel", "uf_jump_kernel"]


def _no_scratch(source, wanted):
    ks = KR.resources(source)
    for want in wanted:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)


def test_cluster_kernels_use_no_scratch():
    _no_scratch("cluster.hip", CLUSTER_KERNELS)


def test_shared_union_find_in_region_growing_uses_no_scratch():
    _no_scratch("segment.hip", ["uf_jump_kernel", "rgraph_grid_kernelILb0ENS_10RegionEdgeE",
                                "rgraph_grid_kernelILb1ENS_10RegionEdgeE", "rgraph_walk_kernelINS_10RegionEdgeE"])
