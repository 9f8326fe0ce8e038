// ddc_plan.h — what the driver of the down-converter (ddc.hip: gc_downconvert) decides on the host: the argument checks, the tile of
// consecutive outputs a workgroup takes with the LDS bytes that go with it, and the walk of the tiles over noutputs.  The NCO's two
// integers, the tile's input span, its staging and the checks of the two records are fir_plan.h's, shared with the resampler and the
// array unit.  Nothing here calls HIP, allocates on the device or launches; tests/ddc_plan_shim.hip runs all of it without a
// device.  From the two contexts the checks read d_if, device, if_nsamples, if_dtype, if_layout and (src) fs.
#pragma once
#include "fir_plan.h"

constexpr int kDdcWG = 256;                 // threads of a workgroup
constexpr int kDdcChains = 4;               // outputs a thread carries at most: independent float64 add chains that share every tap read
constexpr int kDdcMaxTile = kDdcWG * kDdcChains;
// What a workgroup's LDS may take: the taps as (re, im) doubles and the tile's input span as the record's own bytes.  60 KB: below
// the 64 KB a launch gets without asking for more, two workgroups per CU of 160 KB, and room for the largest accepted (D, T).
constexpr long long kDdcLdsBudget = 60 * 1024;
constexpr long long kDdcStaticLds = kDdcWG / 64 * 16;  // next to it, outside the budget: the waves' two result counters
static_assert(kDdcLdsBudget + kDdcStaticLds <= 64 * 1024, "a launch gets 64 KB of LDS without asking for more");

inline long long ddc_taps_bytes(int ntaps) { return 16LL * ntaps; }
// input samples under `outs` consecutive outputs: the first output's oldest to the last output's newest
inline long long ddc_span(long long outs, int decim, int ntaps) { return (outs - 1) * decim + ntaps; }
// LDS bytes of a tile of `outs` outputs of a record of `bps` bytes per sample: taps, then the staged vectors
inline long long ddc_lds_bytes(long long outs, int decim, int ntaps, int bps) {
  return ddc_taps_bytes(ntaps) + (ddc_span(outs, decim, ntaps) * bps + kFirStageSlack + 15) / 16 * 16;
}
// outputs per workgroup: as many as fit the budget at the widest format, at most kDdcMaxTile; 0 for a (D, T) that is not accepted
inline long long ddc_tile_outputs(int decim, int ntaps) {
  if (decim < 1 || decim > GC_DDC_MAX_DECIM || ntaps < 1 || ntaps > GC_DDC_MAX_TAPS) return 0;
  const long long span_max = (kDdcLdsBudget - ddc_taps_bytes(ntaps) - kFirStageSlack - 15) / kFirMaxBps;
  long long outs = (span_max - ntaps) / decim + 1;
  if (outs > kDdcMaxTile) outs = kDdcMaxTile;
  return outs;
}
static_assert((kDdcLdsBudget - 16LL * GC_DDC_MAX_TAPS - kFirStageSlack - 15) / kFirMaxBps >= GC_DDC_MAX_TAPS, "one output of the longest filter fits");

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

// The names that fir_plan.h's NCO, tile and staging went by while they stood here.  Nothing in csrc/ uses them; they stay because
// tests/ddc_plan_shim.hip and tests/resample_plan_shim.hip call the plan by them, and those shims run unedited.
using DdcTile = FirTile;
constexpr long long kDdcStageSlack = kFirStageSlack;
inline bool ddc_phase_step(double carr_freq, double fs, uint64_t* step) { return fir_phase_step(carr_freq, fs, step); }
inline uint64_t ddc_phase0(double carr_phase) { return fir_phase0(carr_phase); }
inline double ddc_nco_freq(uint64_t step, double fs) { return fir_nco_freq(step, fs); }
inline long long ddc_stage_base(long long n_lo, int bps) { return fir_stage_base(n_lo, bps); }
inline long long ddc_stage_vecs(long long n_lo, long long n_hi, int bps) { return fir_stage_vecs(n_lo, n_hi, bps); }

// tile t of the walk (fir_plan.h: fir_tile, which ddc.hip calls on the device)
inline bool ddc_tile_at(const DdcPlan& pl, long long first_sample, long long noutputs, int decim, int ntaps, long long t, FirTile* out) {
  if (t < 0 || t >= pl.ntiles) return false;
  *out = fir_tile(pl.tile, t, first_sample, noutputs, decim, ntaps);
  return true;
}

// gc_downconvert's checks (include/gnsscorr.h): arguments, then state, then what needs both, then range; then the plan.  *pl is
// written only where the call is accepted.
inline int ddc_check(const gc_context* src, const gc_context* dst, const gc_ddc_params* p, const double* taps, DdcPlan* pl) {
  if (!src || !dst || !p || !taps) {
    gc_set_error("gc_downconvert: null argument");
    return GC_E_INVALID;
  }
  if (p->first_sample < 0 || p->dst_first < 0 || p->noutputs < 1 || p->decim < 1 || p->decim > GC_DDC_MAX_DECIM || p->ntaps < 1 ||
      p->ntaps > GC_DDC_MAX_TAPS || !fir_finite(p->carr_freq) || !fir_finite(p->carr_phase)) {
    gc_set_error("gc_downconvert: bad arguments (first_sample %lld, noutputs %lld, dst_first %lld, decim %d, ntaps %d, carr_freq %g, carr_phase %g)",
                 (long long)p->first_sample, (long long)p->noutputs, (long long)p->dst_first, p->decim, p->ntaps, p->carr_freq, p->carr_phase);
    return GC_E_INVALID;
  }
  for (int k = 0; k < 2 * p->ntaps; ++k)
    if (!fir_finite(taps[k])) {
      gc_set_error("gc_downconvert: tap %d is not finite", k / 2);
      return GC_E_INVALID;
    }
  uint64_t step = 0;
  const int rc = fir_check_records("gc_downconvert", src, dst, p->carr_freq, src->fs, (long long)p->dst_first, (long long)p->noutputs, &step);
  if (rc) return rc;
  // the last output's oldest sample: first_sample + (noutputs - 1) D - (T - 1), in 128 bits (noutputs is bounded by dst's record only)
  const __int128 oldest = (__int128)p->first_sample + (__int128)(p->noutputs - 1) * p->decim - (p->ntaps - 1);
  if (oldest >= (__int128)src->if_nsamples) {
    gc_set_error("gc_downconvert: the last output has no record sample under it (%llu samples)", (unsigned long long)src->if_nsamples);
    return GC_E_RANGE;
  }
  DdcPlan q;
  q.phase_step = step;
  q.phase0 = fir_phase0(p->carr_phase);
  q.carr_freq = fir_nco_freq(step, src->fs);
  q.tile = ddc_tile_outputs(p->decim, p->ntaps);
  q.ntiles = ((long long)p->noutputs + q.tile - 1) / q.tile;
  q.span = ddc_span(q.tile, p->decim, p->ntaps);
  q.src_bps = gc_record_bps(src);
  q.dst_bps = gc_record_bps(dst);
  q.lds_bytes = ddc_lds_bytes(q.tile, p->decim, p->ntaps, q.src_bps);
  q.lds_budget = kDdcLdsBudget;
  *pl = q;
  return GC_OK;
}
