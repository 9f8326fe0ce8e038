// fir_plan.h — what the host plans of the three units that write a second record through a float64 complex FIR share (ddc_plan.h:
// gc_downconvert, resample_plan.h: gc_resample, array_plan.h: gc_array_combine and, for the staging, gc_array_covariance): the NCO's
// two integers, the tile of consecutive outputs with the input span under it, the staging of a span in whole 16-byte vectors, and
// the checks of a source and a destination that may differ in format and length.  Nothing here calls HIP; the tile and the staging
// functions are the kernels' own arithmetic (__host__ __device__), and the CPU shims under tests/ run all of it without a device.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "record_check.h"

constexpr int kFirMaxBps = 4;               // bytes per sample of the widest format (int16 pairs): a tile is sized for it, whatever the records hold
// A span is staged in whole 16-byte vectors of the record from the vector that holds its first byte: up to 15 bytes in front and
// 15 behind
constexpr long long kFirStageSlack = 32;
constexpr double kFirTwoPi = 6.283185307179586;

inline bool fir_finite(double v) { return v - v == 0.0; }

// phase_step of the definition at the rate the NCO counts at; false where the ratio does not round into [-2^63, 2^63)
inline bool fir_phase_step(double carr_freq, double rate, uint64_t* step) {
  const double X = std::ldexp(carr_freq / rate, 64);
  if (!(X >= -9223372036854775808.0 && X < 9223372036854775808.0)) return false;
  *step = (uint64_t)(int64_t)std::llrint(X);
  return true;
}
inline uint64_t fir_phase0(double carr_phase) {
  const double q = carr_phase / kFirTwoPi;
  const double r = q - std::rint(q);
  const double X = std::ldexp(r, 64);
  if (X >= 9223372036854775808.0 || X <= -9223372036854775808.0) return 1ull << 63;
  return (uint64_t)(int64_t)std::llrint(X);
}
inline double fir_nco_freq(uint64_t step, double rate) { return std::ldexp((double)(int64_t)step, -64) * rate; }

// Tile t of a walk in tiles of `tile` outputs: outputs [m0, m0 + n), output m at record sample first + m decim, input samples
// [n_lo, n_hi] (n_lo may be negative, n_hi may lie beyond the record: zeros).  The kernels stage what these three functions say:
// base = the byte offset in the record, a multiple of 16 and possibly negative, of the vector that holds n_lo's first byte;
// vecs = the 16-byte vectors from there to the one that holds n_hi's last byte.
struct FirTile {
  long long m0 = 0, n = 0, n_lo = 0, n_hi = 0;
};
__host__ __device__ inline FirTile fir_tile(long long tile, long long t, long long first, long long n, int decim, int ntaps) {
  FirTile r;
  r.m0 = t * tile;
  r.n = tile < n - r.m0 ? tile : n - r.m0;
  r.n_lo = first + r.m0 * decim - (ntaps - 1);
  r.n_hi = first + (r.m0 + r.n - 1) * decim;
  return r;
}
__host__ __device__ inline long long fir_stage_base(long long n_lo, int bps) {
  const long long b = n_lo * bps;
  return (b >= 0 ? b / 16 : -((-b + 15) / 16)) * 16;
}
__host__ __device__ inline long long fir_stage_vecs(long long n_lo, long long n_hi, int bps) {
  return ((n_hi + 1) * bps - fir_stage_base(n_lo, bps) + 15) / 16;
}

// What gc_downconvert and gc_resample (`fn`) ask of their two records after their own argument checks, in the order of
// include/gnsscorr.h: a record on both sides and a sampling frequency - GC_E_STATE; |carr_freq| below fs / 2 and a phase step at
// `nco_rate` (fs, or fs * interp), one device, a destination that neither is the source nor overlaps it (not check_record_pair: dst
// may differ in format and length) - GC_E_INVALID; [dst_first, dst_first + noutputs) inside dst - GC_E_RANGE.
inline int fir_check_records(const char* fn, const gc_context* src, const gc_context* dst, double carr_freq, double nco_rate, long long dst_first,
                             long long noutputs, uint64_t* step) {
  if (!src->d_if || !dst->d_if) {
    gc_set_error("%s: no IF record loaded", fn);
    return GC_E_STATE;
  }
  if (!(src->fs > 0.0)) {
    gc_set_error("%s: the source's sampling frequency is not set", fn);
    return GC_E_STATE;
  }
  if (!(std::fabs(carr_freq) < src->fs / 2.0) || !fir_phase_step(carr_freq, nco_rate, step)) {
    gc_set_error("%s: |carr_freq| %g is not below half the sampling frequency %g", fn, carr_freq, src->fs);
    return GC_E_INVALID;
  }
  if (dst->device != src->device) {
    gc_set_error("%s: the destination is on another device", fn);
    return GC_E_INVALID;
  }
  if (gc_records_overlap(dst, src)) {
    gc_set_error("%s: the destination record is the source's or overlaps it", fn);
    return GC_E_INVALID;
  }
  char who[64];
  std::snprintf(who, sizeof who, "%s (destination)", fn);
  return check_record_range(who, dst, dst_first, noutputs);
}
