// bank_common.h — what gc_correlate_bank (corr_bank.hip) and gc_correlate_ddm (corr_ddm.hip) share: the chunk geometry, a
// sample's load and conversion, the reference's ramp element, the table boundary of an entry and the host's validation.  The
// DDM is defined as the bank at a shifted carrier, bit for bit (include/gnsscorr.h): both kernels take these pieces from here
// so that neither has arithmetic of its own to drift from the other's.
#pragma once
#include <algorithm>
#include <cmath>

#include "corr_common.h"

namespace gcorr {

constexpr int kBankChunk = 1024;  // S: samples per work item
constexpr int kBankWG = 256;      // threads per workgroup: kBankChunk / kBankWG consecutive samples per thread in the prefix sums
constexpr int kBankSPT = kBankChunk / kBankWG;
constexpr int kBankWaves = kBankWG / 64;
constexpr long long kBankPartialBytes = 256LL << 20;  // partial sums of one sub-batch of blocks at most

template <int MODE>
__device__ __forceinline__ void bank_load_sample(const uint8_t* __restrict__ base, long long idx, float& a, float& b) {
  float x0, x1;
  if constexpr (MODE == I8_IQ || MODE == I8_QI) {
    const unsigned int w = *(const unsigned short*)(base + 2 * idx);  // one 16-bit load per sample
    x0 = (float)(signed char)(w & 0xffu);
    x1 = (float)(signed char)(w >> 8);
  } else if constexpr (MODE == I16_IQ || MODE == I16_QI) {
    const short* s = (const short*)base + 2 * idx;
    x0 = (float)s[0];
    x1 = (float)s[1];
  } else if constexpr (MODE == I8_REAL) {
    x0 = (float)((const signed char*)base)[idx];
    x1 = 0.0f;
  } else {
    x0 = (float)((const short*)base)[idx];
    x1 = 0.0f;
  }
  a = Fmt<MODE>::swap ? x1 : x0;
  b = Fmt<MODE>::swap ? x0 : x1;
}

// One (arm, tap) ramp of a block: the reference's colon element i and its table index.
struct BankRamp {
  double a, b, sp, m;
  int N;
  __device__ __forceinline__ int index(int i) const {
    const int back = N - 1 - i;
    double t;
    if (i < back)
      t = __dadd_rn(a, __dmul_rn((double)i, sp));
    else if (i > back)
      t = __dadd_rn(b, -__dmul_rn((double)back, sp));
    else
      t = __dadd_rn(a, b) / 2.0;
    return (int)ceil(__dmul_rn(t, m));
  }
  // e(k): the smallest sample of the chunk [i0, i_last] whose index is >= k, for index(i0) < k <= index(i_last) - it lies in
  // (i0, i_last].  A candidate from a float64 division, corrected with the element rule itself: down while sample e - 1 already
  // has index >= k, up while sample e has index < k.
  __device__ __forceinline__ int boundary(int k, int i0, int i_last) const {
    const double x = ((double)(k - 1) / m - a) / sp;
    int e = (int)fmin(fmax(floor(x) + 1.0, (double)(i0 + 1)), (double)i_last);
    while (e > i0 + 1 && index(e - 1) >= k) --e;
    while (e < i_last && index(e) < k) ++e;
    return e;
  }
};

inline int bank_record_mode(const gc_context* ctx) {
  if (ctx->if_dtype == GC_I8) return ctx->if_layout == GC_IQ ? I8_IQ : ctx->if_layout == GC_QI ? I8_QI : I8_REAL;
  return ctx->if_layout == GC_IQ ? I16_IQ : ctx->if_layout == GC_QI ? I16_QI : I16_REAL;
}

// What gc_correlate_bank accepts (include/gnsscorr.h), for it and for the functions defined through it (`fn`: the name in the
// error texts); *arms = the most arms a channel of the list has.
inline int bank_validate(const char* fn, const gc_context* ctx, int nblocks, const gc_block* b, int ntaps, const double* off, int* arms) {
  if (ntaps < 1 || ntaps > GC_BANK_MAX_TAPS) {
    gc_set_error("%s: %d taps (1 .. %d)", fn, ntaps, GC_BANK_MAX_TAPS);
    return GC_E_INVALID;
  }
  double omax = 0.0;
  for (int j = 0; j < ntaps; ++j) {
    if (!std::isfinite(off[j])) {
      gc_set_error("%s: tap offset %d is not finite", fn, j);
      return GC_E_INVALID;
    }
    omax = std::max(omax, std::fabs(off[j]));
  }
  if (nblocks == 0) return GC_OK;  // an empty list is no call sequence error, as in gc_correlate
  if (ctx->precision != GC_PREC_F32) {
    gc_set_error("%s: float32 kernels only (gc_set_precision GC_PREC_F32)", fn);
    return GC_E_UNSUPPORTED;
  }
  if (!ctx->d_if) {
    gc_set_error("no IF buffer loaded");
    return GC_E_STATE;
  }
  if (!(ctx->fs > 0)) {
    gc_set_error("sampling frequency not set (gc_set_sampling_freq)");
    return GC_E_STATE;
  }
  *arms = 1;
  bool seen[GC_MAX_CHANNELS] = {false};
  for (int i = 0; i < nblocks; ++i) {
    const gc_block& k = b[i];
    if (k.channel < 0 || k.channel >= GC_MAX_CHANNELS || !ctx->ch[k.channel].configured) {
      gc_set_error("block %d: channel %d not configured", i, k.channel);
      return GC_E_STATE;
    }
    const HostChannel& c = ctx->ch[k.channel];
    double max_mult = 1.0;
    for (int a = 0; a < c.arms; ++a) {
      if (!c.d_tab[a]) {
        gc_set_error("block %d: channel %d arm %d has no code table", i, k.channel, a);
        return GC_E_STATE;
      }
      if (k.table_offset[a] != 0) {
        gc_set_error("block %d: %s reads whole tables periodically (table_offset must be 0)", i, fn);
        return GC_E_INVALID;
      }
      max_mult = std::max(max_mult, c.mult[a]);
    }
    if (!seen[k.channel]) {  // per channel: no window, pads that are the period, every offset within one period
      seen[k.channel] = true;
      *arms = std::max(*arms, c.arms);
      for (int a = 0; a < c.arms; ++a) {
        if (c.window[a] > 0) {
          gc_set_error("channel %d arm %d: %s does not take a code window (gc_set_code_window)", k.channel, a, fn);
          return GC_E_UNSUPPORTED;
        }
        const std::vector<int8_t>& t = c.h_tab[a];
        const int n = c.nent[a];
        if ((int)t.size() != n || n < 3 || t[0] != t[n - 2] || t[n - 1] != t[1]) {
          gc_set_error("channel %d arm %d: the table's pads are not its period ([c(end) c c(1)])", k.channel, a);
          return GC_E_INVALID;
        }
        if (!(omax * c.index_scale * c.mult[a] < (double)(n - 2))) {
          gc_set_error("channel %d arm %d: a tap offset of %g chips reaches a code period (%d entries) or more", k.channel, a, omax, n - 2);
          return GC_E_INVALID;
        }
      }
    }
    if (k.blksize <= 0 || k.first_sample < 0 || !(k.code_phase_step > 0) || !(k.rem_code_phase > -1.0) ||
        !std::isfinite(k.rem_code_phase) || !std::isfinite(k.carr_freq) || !std::isfinite(k.rem_carr_phase)) {
      gc_set_error("block %d: invalid descriptor", i);
      return GC_E_INVALID;
    }
    const double rate = k.code_phase_step * c.index_scale * max_mult;  // table entries per sample of the fastest arm
    if (rate > 1.0) {
      gc_set_error("block %d: %g table entries per sample (%s takes at most one)", i, rate, fn);
      return GC_E_UNSUPPORTED;
    }
    if (!(rate >= 1.0 / 65536.0)) {
      gc_set_error("block %d: %g table entries per sample (below 2^-16)", i, rate);
      return GC_E_INVALID;
    }
    if (!(((double)k.blksize * k.code_phase_step + std::fabs(k.rem_code_phase) + omax) * c.index_scale * max_mult < 2147483000.0)) {
      gc_set_error("block %d: the ramps' table indices leave int32", i);
      return GC_E_INVALID;
    }
    if ((uint64_t)k.first_sample + (uint64_t)k.blksize > ctx->if_nsamples) {
      gc_set_error("block %d: samples [%lld, %lld) exceed the IF buffer (%llu samples)", i, (long long)k.first_sample,
                   (long long)(k.first_sample + k.blksize), (unsigned long long)ctx->if_nsamples);
      return GC_E_RANGE;  // tracking.m:241-245
    }
  }
  return GC_OK;
}

}  // namespace gcorr
