// fir_common.h — what the three units that write a second record through a float64 complex FIR (ddc.hip: gc_downconvert,
// resample.hip: gc_resample, array.hip: gc_array_combine, and gc_array_covariance for the staging) share on the device and in their
// drivers: the staging of a span into LDS, the read of a staged sample, the per-output finish, the hand-over of the two counters
// from a workgroup to one of kFirStatSlots slots, and the host's handling of those slots.  All device functions are inlined into their
// kernels; DESIGN.md 4.15 has what that is held to (registers, the tap loop's text, the time) and the figures.
#pragma once
#include "fir_plan.h"
#include "record_fmt.h"

namespace gcorr {

constexpr int kFirStatSlots = 64;  // pairs {clipped, sum_sq} the workgroups of a call add into: workgroup b takes slot b mod kFirStatSlots, the host adds the slots

// `nvec` 16-byte vectors of the record from byte offset base16 (fir_stage_base, fir_stage_vecs) into `vecs`, by the WG threads of the
// workgroup, each a RecVec load (record_fmt.h: one 16-byte global load where the vector lies inside the record, byte by byte and zero
// outside for the record's partial last vector and for the padding in front of sample 0 and behind the last sample)
template <int MODE, int WG>
__device__ __forceinline__ void stage_span(const uint8_t* rec, long long rec_bytes, long long base16, int nvec, uint4* vecs) {
  for (int i = (int)threadIdx.x; i < nvec; i += WG) {
    RecVec<MODE> q;
    q.load(rec, base16 + 16LL * i, rec_bytes);
    vecs[i] = q.words();
  }
}

// sample at byte offset `off` of the staged span as integers (re, im): record_sample (record_fmt.h) at a byte pointer.  Not folded
// into it: an int16 pair is one 32-bit LDS read here and two 16-bit global loads there, and one form for both would change the kernels of one
template <int MODE>
__device__ __forceinline__ void staged_ints(const uint8_t* lds, int off, int& re, int& im) {
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
  re = F::swap ? v1 : v0;
  im = F::swap ? v0 : v1;
}
template <int MODE>
__device__ __forceinline__ void staged_sample(const uint8_t* lds, int off, double& re, double& im) {
  int r, i;
  staged_ints<MODE>(lds, off, r, i);
  re = (double)r;
  im = (double)i;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// The finish of one output: the sums (ar, ai) rotated by the NCO's phase word `ph` (NCO; one float64 sincos of an angle in [-pi, pi]),
// rint, clamp, the two counters and one store as sample s of dst's record in the format `dmode` (gcorr::Mode, a wave-uniform
// run-time branch).  Scalars, not a struct of the format: DESIGN.md 4.15.
template <bool NCO>
__device__ __forceinline__ void fir_finish(double ar, double ai, unsigned long long ph, int dmode, uint8_t* dst, long long s, unsigned long long& clipped,
                                           unsigned long long& sum_sq) {
  const bool d16 = dmode == I16_IQ || dmode == I16_QI || dmode == I16_REAL, dreal = dmode == I8_REAL || dmode == I16_REAL;
  const bool dswap = dmode == I8_QI || dmode == I16_QI;
  const double lo = d16 ? -32768.0 : -128.0, hi = d16 ? 32767.0 : 127.0;
  double yr = ar, yi = ai;
  if constexpr (NCO) {
    const double ang = (double)(long long)ph * (kFirTwoPi * 0x1p-64);  // the product of the constants is exact
    double sn, cs;
    sincos(ang, &sn, &cs);
    yr = cs * ar + sn * ai;
    yi = cs * ai - sn * ar;
  }
  const double rr = rint(yr), ri = rint(yi);
  const long long o_re = (long long)fmin(fmax(rr, lo), hi), o_im = (long long)fmin(fmax(ri, lo), hi);
  clipped += (rr < lo || rr > hi) ? 1ull : 0ull;
  sum_sq += (unsigned long long)(o_re * o_re);
  if (!dreal) {
    clipped += (ri < lo || ri > hi) ? 1ull : 0ull;
    sum_sq += (unsigned long long)(o_im * o_im);
  }
  const int o0 = (int)(dswap ? o_im : o_re), o1 = (int)(dswap ? o_re : o_im);
  if (dreal) {
    if (d16) reinterpret_cast<short*>(dst)[s] = (short)o0;
    else reinterpret_cast<signed char*>(dst)[s] = (signed char)o0;
  } else if (d16) {
    reinterpret_cast<uint32_t*>(dst)[s] = ((uint32_t)o0 & 0xffffu) | ((uint32_t)o1 << 16);
  } else {
    reinterpret_cast<unsigned short*>(dst)[s] = (unsigned short)(((uint32_t)o0 & 0xffu) | (((uint32_t)o1 & 0xffu) << 8));
  }
}

// The hand-over of a workgroup of WAVES waves: the threads' counters through a wave reduction by shuffles, the waves joined in LDS
// (16 WAVES bytes of static LDS), one pair of integer atomics per workgroup into its slot of `stats` - adds to one address queue up
template <int WAVES>
__device__ __forceinline__ void fir_hand_over(unsigned long long clipped, unsigned long long sum_sq, unsigned long long* stats) {
  __shared__ unsigned long long wave_part[WAVES][2];
  const int tid = (int)threadIdx.x;
  clipped = wave_sum(clipped);
  sum_sq = wave_sum(sum_sq);
  if ((tid & 63) == 0) {
    wave_part[tid >> 6][0] = clipped;
    wave_part[tid >> 6][1] = sum_sq;
  }
  __syncthreads();
  if (tid == 0) {
    clipped = sum_sq = 0ull;
    for (int w = 0; w < WAVES; ++w) clipped += wave_part[w][0], sum_sq += wave_part[w][1];
    unsigned long long* const slot = stats + 2 * (blockIdx.x % kFirStatSlots);
    if (clipped) atomicAdd(&slot[0], clipped);
    if (sum_sq) atomicAdd(&slot[1], sum_sq);
  }
}

// The slots on the host: room for them in the unit's buffer, zeroed on the call's stream before the launch ...
inline int fir_stats_begin(const char* fn, GcBuf& stats, hipStream_t stream) {
  if (gc_buf_reserve(stats, sizeof(unsigned long long[kFirStatSlots][2]), false) != hipSuccess) return gc_nomem(fn);
  GC_HIP(hipMemsetAsync(stats.p, 0, sizeof(unsigned long long[kFirStatSlots][2]), stream));
  return GC_OK;
}
// ... and copied back behind it: returns once the stream is idle, sums = {clipped, sum_sq} over the slots
inline int fir_stats_end(const GcBuf& stats, hipStream_t stream, unsigned long long (&sums)[2]) {
  unsigned long long slots[kFirStatSlots][2];
  GC_HIP(hipMemcpyAsync(slots, stats.p, sizeof slots, hipMemcpyDeviceToHost, stream));
  GC_HIP(hipStreamSynchronize(stream));
  sums[0] = sums[1] = 0ull;
  for (int i = 0; i < kFirStatSlots; ++i) sums[0] += slots[i][0], sums[1] += slots[i][1];
  return GC_OK;
}

}  // namespace gcorr
