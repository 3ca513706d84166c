"""The kernels of consistent normal orientation (csrc/orient.hip) may use no scratch and spill nothing: the edge kernel
in its three sources -- a lane keeps its point, its normal, its root and one edge of two 64-bit words --, the tie, hook and
jump kernels of a round, the three kernels of the list compaction, and the kernels behind the rounds.  hipcc's own
resource report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

# orient_edge_kernel<kSrc>: grid (0), walk (1), patched walk (2); orient_member_kernel<kMode>: anchor (1), votes (2);
# orient_offer_kernel<kStep>: weights (0), pair words (1), the better stays (2)
ORIENT_KERNELS = ["orient_edge_kernelILi%dE" % s for s in (0, 1, 2)] + \
                 ["orient_member_kernelILi%dE" % m for m in (1, 2)] + \
                 ["orient_offer_kernelILi%dE" % k for k in (0, 1, 2)] + \
                 ["orient_prep_kernel", "orient_tie_kernel", "orient_count_kernel", "orient_scan_kernel",
                  "orient_write_kernel", "orient_hook_kernel", "orient_jump_kernel", "orient_minid_kernel",
                  "orient_sign_kernel", "orient_out_kernel",
                  "uf_jump_kernel"]  # (uf.h's, which radius_graph.h brings along with wave_root_flush; not launched here)


def test_orient_kernels_use_no_scratch():
    ks = KR.resources("orient.hip")
    for want in ORIENT_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert len(hits) == 1, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    assert len([n for n in ks if "_kernel" in n]) == len(ORIENT_KERNELS)  # every kernel is listed
