"""No kernel of density clustering (csrc/dbscan.hip) or of radius outlier removal (csrc/sor.hip) may use scratch or spill:
both instantiations of the grid's flag pass (with and without the early stop), the walk's flag pass, the two border
passes and the kind scatter stay in registers, and so do the flag forms of the outlier filter's keep kernels.  hipcc's
own resource report, as tests/test_cluster_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

DBSCAN_KERNELS = ["db_flag_grid_kernelILb0EE", "db_flag_grid_kernelILb1EE", "db_flag_walk_kernel", "db_border_grid_kernel",
                  "db_border_walk_kernel", "db_kind_kernel",
                  "uf_jump_kernel"]  # (csrc/radius_graph.h brings csrc/uf.h's per-file copy along; not launched here)
ROR_KERNELS = ["ror_place_kernel", "ror_keep_count_kernel", "ror_keep_write_kernel"]


def _no_scratch(source, wanted):
    ks = KR.resources(source)
    for want in wanted:
        hits = {n: r for n, r in ks.items() if want in n}
        assert hits, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)


def test_dbscan_kernels_use_no_scratch():
    _no_scratch("dbscan.hip", DBSCAN_KERNELS)
    assert len([n for n in KR.resources("dbscan.hip") if "_kernel" in n]) == len(DBSCAN_KERNELS)  # every kernel is listed


def test_ror_kernels_use_no_scratch():
    _no_scratch("sor.hip", ROR_KERNELS)
