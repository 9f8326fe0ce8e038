// excise_plan.h — what the drivers of the excision (excise.hip: gc_excise_pulses, gc_excise_bins, gc_excise_sweep) decide on the host, from integers:
// the argument checks; how the blanker's range is laid over the hot-sample bitmap and cut into the tiles its kernels take one workgroup
// each; the segment count of the spectral excision and the samples a tile of its segment list finishes (the budget of a tile and
// the walk over the list are seg_fft.h's, shared with the probe); the mask rows of the swept excision.  Nothing
// here calls HIP, allocates on the device or launches; tests/excise_plan_shim.hip runs all of it without a device.  From the two
// contexts the checks read d_if, device, if_nsamples, if_dtype and if_layout (record_check.h: the pair of records, the range).  The one refusal that is not decided here is the
// transform planner's (make_plan, acq_fft.hip: GC_E_UNSUPPORTED).
#pragma once
#include <cstdint>

#include "record_check.h"
#include "seg_fft.h"

constexpr int kExciseTile = 16384;                          // samples of the bitmap per workgroup of the mark and the blank kernel
constexpr int kExciseTileWords = kExciseTile / 64;          // 64 samples per bitmap word
constexpr int kExciseHalo = GC_EXCISE_MAX_GUARD / 64;       // zero words in front of the first tile and behind the last: the longest guard
static_assert(GC_EXCISE_MAX_GUARD % 64 == 0 && kExciseTile % 64 == 0, "whole bitmap words");

// Bit b of the bitmap is record sample base + b; base is a multiple of 64 at or below first_sample, so every 16 bytes of the record
// (4, 8 or 16 samples) lie in one word and a tile begins on a 16-byte boundary of the record.  Bits of samples outside the range, and
// beyond the record, are zero: only the samples of the range are examined.
struct ExcisePulsePlan {
  long long base = 0;    // record sample of bit 0
  long long ntiles = 0;  // tiles that cover [base, first_sample + nsamples)
  long long words = 0;   // of the bitmap: kExciseHalo + ntiles * kExciseTileWords + kExciseHalo + 1 (the blank kernel's last prefix count reads one word past the halo)
  int bps = 0;           // bytes per sample
};

inline ExcisePulsePlan excise_pulse_plan(long long first_sample, long long nsamples, int bps) {
  ExcisePulsePlan pl;
  const long long end = first_sample + nsamples;
  pl.bps = bps;
  pl.base = first_sample / 64 * 64;
  pl.ntiles = (end - pl.base + kExciseTile - 1) / kExciseTile;
  pl.words = pl.ntiles * kExciseTileWords + 2 * kExciseHalo + 1;
  return pl;
}

// gc_excise_pulses' checks (include/gnsscorr.h), arguments before state before range; then the plan
inline int excise_check_pulses(const gc_context* src, const gc_context* dst, const gc_excise_pulse_params* p, ExcisePulsePlan* pl) {
  if (!src || !dst || !p) {
    gc_set_error("gc_excise_pulses: null argument");
    return GC_E_INVALID;
  }
  if (p->first_sample < 0 || p->nsamples < 1 || p->threshold2 < 0 || p->before < 0 || p->before > GC_EXCISE_MAX_GUARD || p->after < 0 ||
      p->after > GC_EXCISE_MAX_GUARD) {
    gc_set_error("gc_excise_pulses: bad arguments (first_sample %lld, nsamples %lld, threshold2 %lld, before %d, after %d)", (long long)p->first_sample,
                 (long long)p->nsamples, (long long)p->threshold2, p->before, p->after);
    return GC_E_INVALID;
  }
  int rc = check_record_pair("gc_excise_pulses", src, dst);
  if (rc) return rc;
  rc = check_record_range("gc_excise_pulses", src, (long long)p->first_sample, (long long)p->nsamples);
  if (rc) return rc;
  *pl = excise_pulse_plan((long long)p->first_sample, (long long)p->nsamples, gc_record_bps(src));
  return GC_OK;
}

// ---- gc_excise_bins: segments of nfft samples that overlap by half, cut into tiles whose rows fit a byte budget ------------------------
// (seg_fft.h under the excision's names; the library always passes the default budget and has no switch for it)
using ExciseBudget = SegBudget;
inline long long excise_tile_segments(int nfft, const SegBudget& b) { return seg_tile_segments(nfft, b); }
struct ExciseBinsPlan {
  long long H = 0;     // nfft / 2: the hop, and the samples a segment pair finishes
  long long K = 0;     // segments: ceil(nsamples / H) + 1; segment k covers the range-relative samples [(k - 1) H, (k + 1) H)
  long long tile = 0;  // segments per tile at most
  long long nsamples = 0;
};

// A tile [g0, g0 + n) of the segment list finishes the range samples [m0, m1): those whose two segments it holds, counting the
// second half of segment g0 - 1 that the tile before it left behind (carried: g0 > 0).  The tile's last segment is the next carry.
struct ExciseTile : SegTile {
  long long carried = -1;     // the segment whose second half the tile reads from the carry buffer (-1: none)
  long long m0 = 0, m1 = 0;   // range samples the tile writes (empty: m0 >= m1)
};

inline long long excise_segments(long long nsamples, int nfft) {
  const long long H = nfft / 2;
  return (nsamples + H - 1) / H + 1;
}

// the tile walk: for (ExciseTile t; excise_next_tile(pl, t);) - seg_next_tile and what the tile it names finishes
inline bool excise_next_tile(const ExciseBinsPlan& pl, ExciseTile& t) {
  if (!seg_next_tile(pl.tile, pl.K, t)) return false;
  t.carried = t.g0 > 0 ? t.g0 - 1 : -1;
  t.m0 = (t.g0 > 0 ? t.g0 - 1 : 0) * pl.H;
  t.m1 = (t.g0 + t.n - 1) * pl.H;
  if (t.m1 > pl.nsamples) t.m1 = pl.nsamples;
  return true;
}

// gc_excise_bins' arguments (include/gnsscorr.h): GC_E_INVALID.  The transform planner's refusal (make_plan: GC_E_UNSUPPORTED) is
// asked by the driver between this and excise_check_bins_state.
inline int excise_check_bins(const gc_context* src, const gc_context* dst, const gc_excise_bins_params* p, const float* gain) {
  if (!src || !dst || !p || !gain) {
    gc_set_error("gc_excise_bins: null argument");
    return GC_E_INVALID;
  }
  if (p->first_sample < 0 || p->nsamples < 1 || p->nfft < 4 || (p->nfft & 1) || p->reserved != 0) {
    gc_set_error("gc_excise_bins: bad arguments (first_sample %lld, nsamples %lld, nfft %d, reserved %d)", (long long)p->first_sample,
                 (long long)p->nsamples, p->nfft, p->reserved);
    return GC_E_INVALID;
  }
  for (int b = 0; b < p->nfft; ++b)
    if (!(gain[b] - gain[b] == 0.0f)) {  // neither NaN nor an infinity
      gc_set_error("gc_excise_bins: gain[%d] is not finite", b);
      return GC_E_INVALID;
    }
  return GC_OK;
}

// ... and what the contexts must hold for them: GC_E_STATE, GC_E_INVALID (a destination that does not match), GC_E_RANGE; then the plan
inline int excise_check_segments(const char* who, const gc_context* src, const gc_context* dst, long long first_sample, long long nsamples, int nfft,
                                 const SegBudget& b, ExciseBinsPlan* pl) {
  int rc = check_record_pair(who, src, dst);
  if (rc) return rc;
  rc = check_record_range(who, src, first_sample, nsamples);
  if (rc) return rc;
  pl->H = nfft / 2;
  pl->K = excise_segments(nsamples, nfft);
  pl->tile = excise_tile_segments(nfft, b);
  pl->nsamples = nsamples;
  return GC_OK;
}

inline int excise_check_bins_state(const gc_context* src, const gc_context* dst, const gc_excise_bins_params* p, const SegBudget& b, ExciseBinsPlan* pl) {
  return excise_check_segments("gc_excise_bins", src, dst, (long long)p->first_sample, (long long)p->nsamples, p->nfft, b, pl);
}

// ---- gc_excise_sweep: gc_excise_bins' segments and tiles, and one mask bit per cell (segment, bin) ---------------------------------------
// A segment's mask row is W = ceil(nfft / 64) words; bin b is bit b & 63 of word b >> 6, the bits from nfft on are zero.  The [K]
// arrays of the caller (hot, cut: W words per row; power: nfft floats per row) are filled tile by tile: the rows of the tile
// [g0, g0 + n) begin at row g0, which is excise_mask_offset words into a mask and excise_power_offset floats into the power.
struct ExciseSweepPlan {
  ExciseBinsPlan seg;
  long long W = 0;  // mask words per segment
};

inline long long excise_mask_words(int nfft) { return ((long long)nfft + 63) / 64; }
inline long long excise_tile_rows(const ExciseSweepPlan& pl) { return pl.seg.tile < pl.seg.K ? pl.seg.tile : pl.seg.K; }  // rows the tile buffers hold
inline long long excise_mask_offset(const ExciseSweepPlan& pl, const ExciseTile& t) { return t.g0 * pl.W; }
inline long long excise_power_offset(const ExciseSweepPlan& pl, const ExciseTile& t) { return t.g0 * 2 * pl.seg.H; }

// gc_excise_sweep's arguments (include/gnsscorr.h): GC_E_INVALID.  The planner's refusal comes between this and the state, as for the bins.
inline int excise_check_sweep(const gc_context* src, const gc_context* dst, const gc_excise_sweep_params* p, const float* limit, const float* gain) {
  if (!src || !dst || !p || !limit) {
    gc_set_error("gc_excise_sweep: null argument");
    return GC_E_INVALID;
  }
  if (p->first_sample < 0 || p->nsamples < 1 || p->nfft < 4 || (p->nfft & 1) || p->widen < 0 || p->widen > GC_EXCISE_MAX_WIDEN) {
    gc_set_error("gc_excise_sweep: bad arguments (first_sample %lld, nsamples %lld, nfft %d, widen %d)", (long long)p->first_sample,
                 (long long)p->nsamples, p->nfft, p->widen);
    return GC_E_INVALID;
  }
  for (int b = 0; b < p->nfft; ++b) {
    if (!(limit[b] >= 0.0f)) {  // a NaN or a negative value; +INF protects the bin
      gc_set_error("gc_excise_sweep: limit[%d] is NaN or negative", b);
      return GC_E_INVALID;
    }
    if (gain && !(gain[b] - gain[b] == 0.0f)) {
      gc_set_error("gc_excise_sweep: gain[%d] is not finite", b);
      return GC_E_INVALID;
    }
  }
  return GC_OK;
}

inline int excise_check_sweep_state(const gc_context* src, const gc_context* dst, const gc_excise_sweep_params* p, const SegBudget& b, ExciseSweepPlan* pl) {
  ExciseBinsPlan seg;
  const int rc = excise_check_segments("gc_excise_sweep", src, dst, (long long)p->first_sample, (long long)p->nsamples, p->nfft, b, &seg);
  if (rc) return rc;
  pl->seg = seg;
  pl->W = excise_mask_words(p->nfft);
  return GC_OK;
}
