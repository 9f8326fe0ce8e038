// probe_plan.h — what the drivers of the record probe (probe.hip: gc_probe_psd, gc_probe_histogram) decide on the host, from integers:
// the argument checks, the segment count of a span, and what of a span a tile of the (span, segment) list holds (the budget of a
// tile and the walk over the list are seg_fft.h's, shared with the excision).
// Nothing here calls HIP, allocates on the device or launches; tests/probe_plan_shim.hip runs all of it without a device.  From the
// context the checks read d_if, fs and if_nsamples.  The one refusal that is not decided here is the transform planner's (make_plan,
// acq_fft.hip: GC_E_UNSUPPORTED for a prime factor of 7 or more or a row longer than 2048) - the driver asks it between
// probe_check_args and probe_check_state.
// Reference: probeData.m:76,104,128-131 (every package's include/probeData.m) and MATLAB's pwelch: segments of nfft samples that
// overlap by noverlap, what is left over dropped, no detrending.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "record_check.h"
#include "seg_fft.h"

// The probe's names for the shared budget and walk (seg_fft.h).  The library always passes ProbeBudget() and has no switch for it.
#ifndef GC_PROBE_TILE_MB
#define GC_PROBE_TILE_MB 128  // build macro for A/B libraries only (docs/KNOBS.md, scripts/variants.sh probe "T64:-DGC_PROBE_TILE_MB=64")
#endif
struct ProbeBudget : SegBudget { ProbeBudget() : SegBudget{(long long)GC_PROBE_TILE_MB << 20} {} };
using ProbeTile = SegTile;
inline long long probe_tile_segments(int nfft, const SegBudget& b) { return seg_tile_segments(nfft, b); }

struct ProbePlan {
  long long step = 0;   // nfft - noverlap
  long long K = 0;      // segments per span
  long long total = 0;  // nspans * K: the list the tiles cut, global segment g = span * K + k
  long long tile = 0;   // segments per tile at most
};
// the tile walk: for (ProbeTile t; probe_next_tile(pl, t);) - a tile may end one span and begin the next
inline bool probe_next_tile(const ProbePlan& pl, ProbeTile& t) { return seg_next_tile(pl.tile, pl.total, t); }

// K = floor((nsamples - noverlap) / step) (pwelch; >= 1 for every nsamples >= nfft)
inline long long probe_segments(long long nsamples, int nfft, int noverlap) { return (nsamples - noverlap) / (long long)(nfft - noverlap); }

// What of span `span` a tile [g0, g0 + n) of the segment list holds: its segments [*k0, *k1) (empty: k0 >= k1).  The span's
// accumulator is carried (read before it is added to) when *k0 > 0, and the span is finished by this tile when *k1 == K.  The
// power kernel and the shim both go through this function.
GC_FFT_HD inline void probe_span_range(long long g0, long long n, long long K, long long span, long long* k0, long long* k1) {
  const long long lo = span * K, hi = lo + K;
  const long long a = g0 > lo ? g0 : lo, b = g0 + n < hi ? g0 + n : hi;
  *k0 = a - lo;
  *k1 = b - lo;
}

// gc_probe_psd's arguments (include/gnsscorr.h): GC_E_INVALID
inline int probe_check_args(const gc_context* ctx, const gc_probe_psd_params* p, const double* psd) {
  if (!ctx || !p || !psd) {
    gc_set_error("gc_probe_psd: null argument");
    return GC_E_INVALID;
  }
  if (p->first_sample < 0 || p->nsamples < 1 || p->nspans < 1 || p->nfft < 2 || p->noverlap < 0 || p->noverlap >= p->nfft || p->nsamples < p->nfft ||
      (p->window != GC_WIN_RECT && p->window != GC_WIN_HAMMING)) {
    gc_set_error("gc_probe_psd: bad arguments (first_sample %lld, nsamples %lld, nfft %d, noverlap %d, window %d, nspans %d)", (long long)p->first_sample,
                 (long long)p->nsamples, p->nfft, p->noverlap, p->window, p->nspans);
    return GC_E_INVALID;
  }
  return GC_OK;
}

// ... and what the context must hold for them: GC_E_STATE, GC_E_RANGE; then the plan
inline int probe_check_state(const gc_context* ctx, const gc_probe_psd_params* p, const SegBudget& b, ProbePlan* pl) {
  if (!ctx->d_if) {
    gc_set_error("gc_probe_psd: no IF record loaded");
    return GC_E_STATE;
  }
  if (!(ctx->fs > 0)) {
    gc_set_error("gc_probe_psd: sampling frequency not set (gc_set_sampling_freq)");
    return GC_E_STATE;
  }
  // first_sample + nspans * nsamples <= if_nsamples, without forming a product that may leave int64
  const unsigned long long have = ctx->if_nsamples, first = (unsigned long long)p->first_sample;
  if (first > have || (have - first) / (unsigned long long)p->nsamples < (unsigned long long)p->nspans) {
    gc_set_error("gc_probe_psd: %d span(s) of %lld samples from %lld end beyond the record (%llu samples)", p->nspans, (long long)p->nsamples,
                 (long long)p->first_sample, have);
    return GC_E_RANGE;
  }
  pl->step = p->nfft - p->noverlap;
  pl->K = probe_segments(p->nsamples, p->nfft, p->noverlap);
  pl->total = pl->K * (long long)p->nspans;
  pl->tile = probe_tile_segments(p->nfft, b);
  return GC_OK;
}

// gc_probe_histogram's checks: GC_E_INVALID, GC_E_STATE, GC_E_RANGE
inline int probe_check_histogram(const gc_context* ctx, long long first_sample, long long nsamples, const uint64_t* counts) {
  if (!ctx || !counts || first_sample < 0 || nsamples < 1) {
    gc_set_error("gc_probe_histogram: bad arguments");
    return GC_E_INVALID;
  }
  if (!ctx->d_if) {
    gc_set_error("gc_probe_histogram: no IF record loaded");
    return GC_E_STATE;
  }
  return check_record_range("gc_probe_histogram", ctx, first_sample, nsamples);
}

// workgroups of the histogram kernel and samples each takes: whole multiples of the workgroup's 256 threads, at most 2048 workgroups
// (the combine kernel walks their partial rows) up to 2^42 samples; beyond that more workgroups, never more than 2^31 samples each
// (a workgroup's partial counts are 32-bit)
struct ProbeHistGrid {
  long long per_wg = 0;
  long long grid = 0;
};
inline ProbeHistGrid probe_hist_grid(long long nsamples) {
  const long long threads = 256, min_per = 16 * threads, max_wg = 2048;
  long long per = std::max(min_per, (nsamples + max_wg - 1) / max_wg);
  per = std::min((per + threads - 1) / threads * threads, 1LL << 31);
  ProbeHistGrid g;
  g.per_wg = per;
  g.grid = (nsamples + per - 1) / per;
  return g;
}
