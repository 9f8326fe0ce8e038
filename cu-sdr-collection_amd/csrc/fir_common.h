// fir_common.h — what the two FIR units that write a second record (ddc.hip: gc_downconvert, resample.hip: gc_resample) share on the
// device: the read of a sample from the staged span and the wave reduction of a count.  Both are inlined into their kernels; the six
// ddc_kernel instantiations compile to the instructions they had with this text in ddc.hip.  The per-output finish is NOT here: as a
// function it gave ddc_kernel the same instructions in another order, so each unit writes it out.
#pragma once
#include "record_fmt.h"

namespace gcorr {

// sample at byte offset `off` of the staged span as (re, im): record_sample (record_fmt.h) at a byte pointer.  Not folded into it: an
// int16 pair is one 32-bit LDS read here and two 16-bit global loads there, and one form for both would change the kernels of one
template <int MODE>
__device__ __forceinline__ void staged_sample(const uint8_t* lds, int off, double& re, double& im) {
  using F = Fmt<MODE>;
  int v0, v1 = 0;
  if constexpr (F::values == 2 && F::value_bytes == 1) {
    const unsigned int w = *(const unsigned short*)(lds + off);
    v0 = (int)(signed char)(w & 0xffu);
    v1 = (int)(signed char)(w >> 8);
  } else if constexpr (F::values == 2) {
    const unsigned int w = *(const unsigned int*)(lds + off);
    v0 = (int)(short)(w & 0xffffu);
    v1 = (int)(short)(w >> 16);
  } else if constexpr (F::value_bytes == 1) {
    v0 = (int)*(const signed char*)(lds + off);
  } else {
    v0 = (int)*(const short*)(lds + off);
  }
  re = (double)(F::swap ? v1 : v0);
  im = (double)(F::swap ? v0 : v1);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

}  // namespace gcorr
