"""The kernels of farthest-point sampling (csrc/fps.hip) may use no scratch and spill nothing: the gather out of the
tree's slots, the prep kernel (a wave per tile: box and key), the pick kernel (a lane keeps a tile's key and box, a
touched tile is four points a lane), the finish kernel, and the two kernels of the filter form.  hipcc's own resource
report, as tests/test_kernel_resources.py reads it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

FPS_KERNELS = ["fps_gather_kernel", "fps_prep_kernel", "fps_pick_kernel", "fps_finish_kernel", "fps_filter_xyz_kernel",
               "fps_filter_copy_kernel"]


def test_fps_kernels_use_no_scratch():
    ks = KR.resources("fps.hip")
    for want in FPS_KERNELS:
        hits = {n: r for n, r in ks.items() if want in n}
        assert len(hits) == 1, (want, sorted(ks))
        for name, r in hits.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    assert len([n for n in ks if "_kernel" in n]) == len(FPS_KERNELS)  # every kernel is listed
