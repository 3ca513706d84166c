"""The kernels of the group footprints (csrc/group_hull.hip), by hipcc's own resource report as
tests/test_kernel_resources.py reads it: every gh_ kernel is listed here, and the kernels that touch every slot of the
list or every entry of the sort (offsets, extremes, filter, sort keys, heads, the three compaction kernels) use no
scratch and do not spill.  The figures of the others (reduce, bounds, chain, write, rect) are printed and stand in
DESIGN 3.20; at the time of writing none of them uses scratch either, and the reduce's stacks take 36 KB of LDS."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

EVERY_SLOT = ["gh_offsets_kernel", "gh_extreme_kernel", "gh_filter_kernel", "gh_key_kernel", "gh_head_kernel",
              "gh_flag_count_kernel", "gh_flag_scan_kernel", "gh_flag_write_kernel"]
SURVIVORS = ["gh_reduce_kernel", "gh_bounds_kernel", "gh_chain_kernel", "gh_write_kernel", "gh_rect_kernel"]


def test_hull_kernels_are_listed_and_the_slot_kernels_use_no_scratch():
    ks = KR.resources("group_hull.hip")
    names = [n for n in ks if "gh_" in n]
    assert len(names) == len(EVERY_SLOT) + len(SURVIVORS) + 1, sorted(ks)  # (gh_offsets_kernel is compiled twice)
    for want in EVERY_SLOT + SURVIVORS:
        assert any(want in n for n in names), (want, sorted(ks))
    assert all(any(w in n for w in EVERY_SLOT + SURVIVORS) for n in names), sorted(ks)
    assert not any("gs_" in n for n in ks), sorted(ks)  # the shared kernels stay in group_stats.hip
    for want in EVERY_SLOT:
        for name, r in ks.items():
            if want in name:
                assert r.get("ScratchSize") == 0, (name, r)
                assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    for want in SURVIVORS:
        for name, r in ks.items():
            if want in name:
                print(want, {k: r.get(k) for k in ("VGPRs", "SGPRs", "ScratchSize", "LDS Size", "Occupancy")})
