// ddc_plan.h — what the driver of the down-converter (ddc.hip: gc_downconvert) decides on the host: the argument checks, the NCO's
// two integers, the tile of consecutive outputs a workgroup takes with the input span and the LDS bytes that go with it, and the walk
// of the tiles over noutputs.  Nothing here calls HIP, allocates on the device or launches; tests/ddc_plan_shim.hip runs all of it
// without a device.  From the two contexts the checks read d_if, device, if_nsamples, if_dtype, if_layout and (src) fs.
#pragma once
#include <cmath>
#include <cstdint>

#include "record_check.h"

constexpr int kDdcWG = 256;                 // threads of a workgroup
constexpr int kDdcChains = 4;               // outputs a thread carries at most: independent float64 add chains that share every tap read
constexpr int kDdcMaxTile = kDdcWG * kDdcChains;
// What a workgroup's LDS may take: the taps as (re, im) doubles and the tile's input span as the record's own bytes.  60 KB: below
// the 64 KB a launch gets without asking for more, two workgroups per CU of 160 KB, and room for the largest accepted (D, T).
constexpr long long kDdcLdsBudget = 60 * 1024;
constexpr long long kDdcStaticLds = kDdcWG / 64 * 16;  // next to it, outside the budget: the waves' two result counters
static_assert(kDdcLdsBudget + kDdcStaticLds <= 64 * 1024, "a launch gets 64 KB of LDS without asking for more");
constexpr int kDdcMaxBps = 4;               // bytes per sample of the widest format (int16 pairs): the tile is sized for it, whatever src holds
// The span is staged in whole 16-byte vectors of the record from the vector that holds its first byte: up to 15 bytes in front and
// 15 behind
constexpr long long kDdcStageSlack = 32;
constexpr double kDdcTwoPi = 6.283185307179586;

inline long long ddc_taps_bytes(int ntaps) { return 16LL * ntaps; }
// input samples under `outs` consecutive outputs: the first output's oldest to the last output's newest
inline long long ddc_span(long long outs, int decim, int ntaps) { return (outs - 1) * decim + ntaps; }
// LDS bytes of a tile of `outs` outputs of a record of `bps` bytes per sample: taps, then the staged vectors
inline long long ddc_lds_bytes(long long outs, int decim, int ntaps, int bps) {
  return ddc_taps_bytes(ntaps) + (ddc_span(outs, decim, ntaps) * bps + kDdcStageSlack + 15) / 16 * 16;
}
// outputs per workgroup: as many as fit the budget at the widest format, at most kDdcMaxTile; 0 for a (D, T) that is not accepted
inline long long ddc_tile_outputs(int decim, int ntaps) {
  if (decim < 1 || decim > GC_DDC_MAX_DECIM || ntaps < 1 || ntaps > GC_DDC_MAX_TAPS) return 0;
  const long long span_max = (kDdcLdsBudget - ddc_taps_bytes(ntaps) - kDdcStageSlack - 15) / kDdcMaxBps;
  long long outs = (span_max - ntaps) / decim + 1;
  if (outs > kDdcMaxTile) outs = kDdcMaxTile;
  return outs;
}
static_assert((kDdcLdsBudget - 16LL * GC_DDC_MAX_TAPS - kDdcStageSlack - 15) / kDdcMaxBps >= GC_DDC_MAX_TAPS, "one output of the longest filter fits");

// phase_step of the definition; false where the ratio does not round into [-2^63, 2^63)
inline bool ddc_phase_step(double carr_freq, double fs, uint64_t* step) {
  const double X = std::ldexp(carr_freq / fs, 64);
  if (!(X >= -9223372036854775808.0 && X < 9223372036854775808.0)) return false;
  *step = (uint64_t)(int64_t)std::llrint(X);
  return true;
}
inline uint64_t ddc_phase0(double carr_phase) {
  const double q = carr_phase / kDdcTwoPi;
  const double r = q - std::rint(q);
  const double X = std::ldexp(r, 64);
  if (X >= 9223372036854775808.0 || X <= -9223372036854775808.0) return 1ull << 63;
  return (uint64_t)(int64_t)std::llrint(X);
}
inline double ddc_nco_freq(uint64_t step, double fs) { return std::ldexp((double)(int64_t)step, -64) * fs; }

struct DdcPlan {
  uint64_t phase_step = 0, phase0 = 0;
  double carr_freq = 0.0;   // the frequency the NCO runs at
  long long tile = 0;       // outputs per workgroup
  long long ntiles = 0;
  long long span = 0;       // input samples a full tile stages
  long long lds_bytes = 0;  // of a full tile at src's format
  long long lds_budget = 0; // what the tile was sized against (the widest format)
  int src_bps = 0, dst_bps = 0;
};

// Tile t of the walk: outputs [m0, m0 + n), input samples [n_lo, n_hi] (n_lo may be negative, n_hi may lie beyond the record: zeros)
// The kernel stages what these three functions say (they are the kernel's own arithmetic: ddc.hip calls them on the device):
// base = the byte offset in the record, a multiple of 16 and possibly negative, of the vector that holds n_lo's first byte;
// vecs = the 16-byte vectors from there to the one that holds n_hi's last byte.
struct DdcTile {
  long long m0 = 0, n = 0, n_lo = 0, n_hi = 0;
};
__host__ __device__ inline DdcTile ddc_tile(long long tile, long long t, long long first_sample, long long noutputs, int decim, int ntaps) {
  DdcTile r;
  r.m0 = t * tile;
  r.n = tile < noutputs - r.m0 ? tile : noutputs - r.m0;
  r.n_lo = first_sample + r.m0 * decim - (ntaps - 1);
  r.n_hi = first_sample + (r.m0 + r.n - 1) * decim;
  return r;
}
__host__ __device__ inline long long ddc_stage_base(long long n_lo, int bps) {
  const long long b = n_lo * bps;
  return (b >= 0 ? b / 16 : -((-b + 15) / 16)) * 16;
}
__host__ __device__ inline long long ddc_stage_vecs(long long n_lo, long long n_hi, int bps) {
  return ((n_hi + 1) * bps - ddc_stage_base(n_lo, bps) + 15) / 16;
}
inline bool ddc_tile_at(const DdcPlan& pl, long long first_sample, long long noutputs, int decim, int ntaps, long long t, DdcTile* out) {
  if (t < 0 || t >= pl.ntiles) return false;
  *out = ddc_tile(pl.tile, t, first_sample, noutputs, decim, ntaps);
  return true;
}

inline bool ddc_finite(double v) { return v - v == 0.0; }

// gc_downconvert's checks (include/gnsscorr.h): arguments, then state, then what needs both, then range; then the plan.  *pl is
// written only where the call is accepted.
inline int ddc_check(const gc_context* src, const gc_context* dst, const gc_ddc_params* p, const double* taps, DdcPlan* pl) {
  if (!src || !dst || !p || !taps) {
    gc_set_error("gc_downconvert: null argument");
    return GC_E_INVALID;
  }
  if (p->first_sample < 0 || p->dst_first < 0 || p->noutputs < 1 || p->decim < 1 || p->decim > GC_DDC_MAX_DECIM || p->ntaps < 1 ||
      p->ntaps > GC_DDC_MAX_TAPS || !ddc_finite(p->carr_freq) || !ddc_finite(p->carr_phase)) {
    gc_set_error("gc_downconvert: bad arguments (first_sample %lld, noutputs %lld, dst_first %lld, decim %d, ntaps %d, carr_freq %g, carr_phase %g)",
                 (long long)p->first_sample, (long long)p->noutputs, (long long)p->dst_first, p->decim, p->ntaps, p->carr_freq, p->carr_phase);
    return GC_E_INVALID;
  }
  for (int k = 0; k < 2 * p->ntaps; ++k)
    if (!ddc_finite(taps[k])) {
      gc_set_error("gc_downconvert: tap %d is not finite", k / 2);
      return GC_E_INVALID;
    }
  if (!src->d_if || !dst->d_if) {
    gc_set_error("gc_downconvert: no IF record loaded");
    return GC_E_STATE;
  }
  if (!(src->fs > 0.0)) {
    gc_set_error("gc_downconvert: the source's sampling frequency is not set");
    return GC_E_STATE;
  }
  uint64_t step = 0;
  if (!(std::fabs(p->carr_freq) < src->fs / 2.0) || !ddc_phase_step(p->carr_freq, src->fs, &step)) {
    gc_set_error("gc_downconvert: |carr_freq| %g is not below half the sampling frequency %g", p->carr_freq, src->fs);
    return GC_E_INVALID;
  }
  if (dst->device != src->device) {
    gc_set_error("gc_downconvert: the destination is on another device");
    return GC_E_INVALID;
  }
  // not check_record_pair: dst may differ in format and length, and may not be the source
  const int sb = gc_record_bps(src), db = gc_record_bps(dst);
  const uint64_t sbytes = src->if_nsamples * (uint64_t)sb, dbytes = dst->if_nsamples * (uint64_t)db;
  if (dst->d_if == src->d_if || (dst->d_if < src->d_if + sbytes && src->d_if < dst->d_if + dbytes)) {
    gc_set_error("gc_downconvert: the destination record is the source's or overlaps it");
    return GC_E_INVALID;
  }
  const int rc = check_record_range("gc_downconvert (destination)", dst, (long long)p->dst_first, (long long)p->noutputs);
  if (rc) return rc;
  // the last output's oldest sample: first_sample + (noutputs - 1) D - (T - 1), in 128 bits (noutputs is bounded by dst's record only)
  const __int128 oldest = (__int128)p->first_sample + (__int128)(p->noutputs - 1) * p->decim - (p->ntaps - 1);
  if (oldest >= (__int128)src->if_nsamples) {
    gc_set_error("gc_downconvert: the last output has no record sample under it (%llu samples)", (unsigned long long)src->if_nsamples);
    return GC_E_RANGE;
  }
  DdcPlan q;
  q.phase_step = step;
  q.phase0 = ddc_phase0(p->carr_phase);
  q.carr_freq = ddc_nco_freq(step, src->fs);
  q.tile = ddc_tile_outputs(p->decim, p->ntaps);
  q.ntiles = ((long long)p->noutputs + q.tile - 1) / q.tile;
  q.span = ddc_span(q.tile, p->decim, p->ntaps);
  q.src_bps = sb;
  q.dst_bps = db;
  q.lds_bytes = ddc_lds_bytes(q.tile, p->decim, p->ntaps, sb);
  q.lds_budget = kDdcLdsBudget;
  *pl = q;
  return GC_OK;
}
