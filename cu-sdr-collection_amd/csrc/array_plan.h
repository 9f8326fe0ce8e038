// array_plan.h — what the driver of the antenna-array unit (array.hip: gc_array_covariance, gc_array_combine) decides on the host: the
// argument checks of both calls, the tile of consecutive samples a workgroup takes with each record's staged span and the LDS bytes
// that go with it, the walk of the tiles over a range, and the constants that bound the covariance kernel's narrow accumulators.  The
// tile's span and its staging are fir_plan.h's, shared with the down-converter and the resampler.
// Nothing here calls HIP, allocates on the device or launches; tests/array_plan_shim.hip runs all of it without a device.  From the
// contexts the checks read d_if, device, if_nsamples, if_dtype and if_layout.
#pragma once
#include "fir_plan.h"

constexpr int kArrWG = 256;                 // threads of a workgroup
constexpr int kArrChains = 4;               // samples a thread carries at most: the combine's independent float64 add chains, the covariance's samples per pass
constexpr int kArrMaxTile = kArrWG * kArrChains;
// What a workgroup's LDS may take: the K spans as the records' own bytes and (combine) the K T weights as (re, im) doubles.  56 KB,
// with the covariance's wave sums next to it: below the 64 KB a launch gets without asking for more, two workgroups per CU of 160 KB.
constexpr long long kArrLdsBudget = 56 * 1024;
// next to it, outside the budget: per wave the 2 K sums of K passes as 8-byte integers (covariance); the waves' two counters (combine)
constexpr long long kArrStaticLds = (long long)(kArrWG / 64) * GC_ARRAY_MAX_RECORDS * 2 * GC_ARRAY_MAX_RECORDS * 8;
static_assert(kArrLdsBudget + kArrStaticLds <= 64 * 1024, "a launch gets 64 KB of LDS without asking for more");
// The covariance of int8 records adds in int32 up to the wave's sum of a pass: a pass of the whole workgroup adds at most kArrMaxTile
// samples, each two products of at most 128^2 = 2^14 in magnitude.  int16 records add in int64 throughout (a product pair reaches
// 2^31).
constexpr long long kArrCovI32Cap = kArrMaxTile;
static_assert(kArrCovI32Cap * 2 * 128 * 128 < (1LL << 31), "an int8 pass stays inside int32");
constexpr long long kArrCovMaxSamples = 1LL << 31;  // 2^31 samples * 2 products * 2^30 = 2^62: every int16 sum stays inside 63 bits
constexpr int kArrCovSlots = 64;            // copies of the covariance the workgroups add into; the host adds them (the combine's two counters: fir_common.h)

inline long long arr_weights_bytes(int nrecords, int ntaps) { return 16LL * nrecords * ntaps; }
// LDS bytes of one record's span under `tile` consecutive samples with T - 1 samples of lead-in, at `bps` bytes per sample
inline long long arr_rec_bytes(long long tile, int ntaps, int bps) { return ((tile + ntaps - 1) * bps + kFirStageSlack + 15) / 16 * 16; }
// LDS bytes of a tile: (combine) the weights, then the K spans
inline long long arr_lds_bytes(long long tile, int nrecords, int ntaps, int bps, bool weights) {
  return (weights ? arr_weights_bytes(nrecords, ntaps) : 0) + nrecords * arr_rec_bytes(tile, ntaps, bps);
}
// samples per workgroup: as many as fit the budget at the widest format with the weights, at most kArrMaxTile; 0 for a (K, T) that is
// not accepted.  One function for both calls (T = ntaps or nlags): the covariance leaves the weights' room unused.  (A workgroup of
// the covariance that took four tiles as one, in up to 152 KB of LDS, was measured and was no faster: DESIGN.md 4.16.)
inline long long arr_tile_outputs(int nrecords, int ntaps) {
  if (nrecords < 1 || nrecords > GC_ARRAY_MAX_RECORDS || ntaps < 1 || ntaps > GC_ARRAY_MAX_TAPS) return 0;
  const long long per_rec = (kArrLdsBudget - arr_weights_bytes(nrecords, ntaps)) / nrecords / 16 * 16;
  long long tile = (per_rec - kFirStageSlack - 15) / kFirMaxBps - (ntaps - 1);
  if (tile > kArrMaxTile) tile = kArrMaxTile;
  return tile;
}
static_assert(((kArrLdsBudget - 16LL * GC_ARRAY_MAX_RECORDS * GC_ARRAY_MAX_TAPS) / GC_ARRAY_MAX_RECORDS / 16 * 16 - kFirStageSlack - 15) / kFirMaxBps -
                      (GC_ARRAY_MAX_TAPS - 1) >= kArrMaxTile,
              "the largest (K, T) takes a full tile");

struct ArrPlan {
  long long tile = 0;       // samples per workgroup
  long long ntiles = 0;
  long long span = 0;       // samples of one record a full tile stages
  long long rec_bytes = 0;  // LDS bytes of one record's span at the sources' format
  long long lds_bytes = 0;  // of a full tile at the sources' format
  long long lds_budget = 0; // what the tile was sized against (the widest format)
  int src_bps = 0, dst_bps = 0;  // dst_bps: 0 for the covariance
};

// Tile t of the walk: samples [m0, m0 + n) of the range, record samples [n_lo, n_hi] (n_lo may be negative: zeros) - fir_plan.h's
// tile at a decimation of 1, which array.hip calls on the device and stages with fir_stage_base and fir_stage_vecs
inline bool arr_tile_at(const ArrPlan& pl, long long first_sample, long long nsamples, int ntaps, long long t, FirTile* out) {
  if (t < 0 || t >= pl.ntiles) return false;
  *out = fir_tile(pl.tile, t, first_sample, nsamples, 1, ntaps);
  return true;
}

// What both calls ask of their records, in the order of include/gnsscorr.h: one device, one source format, (dst) no overlap with a
// source - GC_E_INVALID; a record everywhere - GC_E_STATE; [first, first + n) inside every source and [dst_first, dst_first + n)
// inside dst - GC_E_RANGE.  srcs and its K entries are not null (the callers' argument checks); dst is null for the covariance.
inline int arr_check_records(const char* fn, gc_context* const* srcs, int K, const gc_context* dst, long long first, long long n, long long dst_first) {
  const gc_context* s0 = srcs[0];
  for (int a = 1; a < K; ++a)
    if (srcs[a]->device != s0->device) {
      gc_set_error("%s: source %d is on another device", fn, a);
      return GC_E_INVALID;
    }
  if (dst && dst->device != s0->device) {
    gc_set_error("%s: the destination is on another device", fn);
    return GC_E_INVALID;
  }
  for (int a = 1; a < K; ++a)
    if (srcs[a]->if_dtype != s0->if_dtype || srcs[a]->if_layout != s0->if_layout) {
      gc_set_error("%s: source %d differs from source 0 in dtype or layout", fn, a);
      return GC_E_INVALID;
    }
  if (dst && dst->d_if)
    for (int a = 0; a < K; ++a)
      if (srcs[a]->d_if && gc_records_overlap(dst, srcs[a])) {
        gc_set_error("%s: the destination record is source %d's or overlaps it", fn, a);
        return GC_E_INVALID;
      }
  for (int a = 0; a < K; ++a)
    if (!srcs[a]->d_if) {
      gc_set_error("%s: source %d has no IF record loaded", fn, a);
      return GC_E_STATE;
    }
  if (dst && !dst->d_if) {
    gc_set_error("%s: the destination has no IF record loaded", fn);
    return GC_E_STATE;
  }
  for (int a = 0; a < K; ++a) {
    const int rc = check_record_range(fn, srcs[a], first, n);
    if (rc) return rc;
  }
  if (dst) {
    const int rc = check_record_range(fn, dst, dst_first, n);
    if (rc) return rc;
  }
  return GC_OK;
}

inline bool arr_null_entry(gc_context* const* srcs, int K) {
  for (int a = 0; a < K; ++a)
    if (!srcs[a]) return true;
  return false;
}

inline ArrPlan arr_plan(int K, int T, long long n, int src_bps, int dst_bps, bool weights) {
  ArrPlan q;
  q.tile = arr_tile_outputs(K, T);
  q.ntiles = (n + q.tile - 1) / q.tile;
  q.span = q.tile + T - 1;
  q.src_bps = src_bps;
  q.dst_bps = dst_bps;
  q.rec_bytes = arr_rec_bytes(q.tile, T, src_bps);
  q.lds_bytes = arr_lds_bytes(q.tile, K, T, src_bps, weights);
  q.lds_budget = kArrLdsBudget;
  return q;
}

// gc_array_covariance's checks (include/gnsscorr.h), then the plan.  *pl is written only where the call is accepted.
inline int arr_cov_check(gc_context* const* srcs, const gc_array_cov_params* p, const int64_t* cov, ArrPlan* pl) {
  if (!srcs || !p || !cov) {
    gc_set_error("gc_array_covariance: null argument");
    return GC_E_INVALID;
  }
  if (p->nrecords < 1 || p->nrecords > GC_ARRAY_MAX_RECORDS || p->nlags < 1 || p->nlags > GC_ARRAY_MAX_TAPS || p->first_sample < 0 || p->nsamples < 1 ||
      p->nsamples > kArrCovMaxSamples) {
    gc_set_error("gc_array_covariance: bad arguments (first_sample %lld, nsamples %lld, nrecords %d, nlags %d)", (long long)p->first_sample,
                 (long long)p->nsamples, p->nrecords, p->nlags);
    return GC_E_INVALID;
  }
  if (arr_null_entry(srcs, p->nrecords)) {
    gc_set_error("gc_array_covariance: null source");
    return GC_E_INVALID;
  }
  const int rc = arr_check_records("gc_array_covariance", srcs, p->nrecords, nullptr, (long long)p->first_sample, (long long)p->nsamples, 0);
  if (rc) return rc;
  *pl = arr_plan(p->nrecords, p->nlags, (long long)p->nsamples, gc_record_bps(srcs[0]), 0, false);
  return GC_OK;
}

// gc_array_combine's checks, then the plan.  *pl is written only where the call is accepted.
inline int arr_combine_check(gc_context* const* srcs, const gc_context* dst, const gc_array_combine_params* p, const double* weights, ArrPlan* pl) {
  if (!srcs || !dst || !p || !weights) {
    gc_set_error("gc_array_combine: null argument");
    return GC_E_INVALID;
  }
  if (p->nrecords < 1 || p->nrecords > GC_ARRAY_MAX_RECORDS || p->ntaps < 1 || p->ntaps > GC_ARRAY_MAX_TAPS || p->first_sample < 0 || p->dst_first < 0 ||
      p->noutputs < 1) {
    gc_set_error("gc_array_combine: bad arguments (first_sample %lld, noutputs %lld, dst_first %lld, nrecords %d, ntaps %d)", (long long)p->first_sample,
                 (long long)p->noutputs, (long long)p->dst_first, p->nrecords, p->ntaps);
    return GC_E_INVALID;
  }
  if (arr_null_entry(srcs, p->nrecords)) {
    gc_set_error("gc_array_combine: null source");
    return GC_E_INVALID;
  }
  for (int k = 0; k < 2 * p->nrecords * p->ntaps; ++k)
    if (!fir_finite(weights[k])) {
      gc_set_error("gc_array_combine: weight %d of record %d is not finite", k / 2 % p->ntaps, k / 2 / p->ntaps);
      return GC_E_INVALID;
    }
  const int rc = arr_check_records("gc_array_combine", srcs, p->nrecords, dst, (long long)p->first_sample, (long long)p->noutputs, (long long)p->dst_first);
  if (rc) return rc;
  *pl = arr_plan(p->nrecords, p->ntaps, (long long)p->noutputs, gc_record_bps(srcs[0]), gc_record_bps(dst), true);
  return GC_OK;
}
