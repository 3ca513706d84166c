// Host stand-in for <hip/hip_runtime.h>: just enough for csrc/cov3.h to compile with g++ (tests/test_cov3_host.py).
// The qualifiers go away; __shfl_xor is declared only: NormAcc::wave_sum needs a wave and is never called on the host.
#pragma once
#define __device__
#define __host__
#define __forceinline__ inline
template <class T>
T __shfl_xor(T v, int lane_mask);
