// Host stand-in for <hip/hip_runtime.h>: just enough for csrc/cov3.h (tests/test_cov3_host.py) and csrc/voxel_cell.h
// (tests/test_voxel_cell_host.py) to compile with g++.
// The qualifiers go away; __shfl_xor is declared only: NormAcc::wave_sum needs a wave and is never called on the host.
#pragma once
#define __device__
#define __host__
#define __forceinline__ inline
template <class T>
T __shfl_xor(T v, int lane_mask);
