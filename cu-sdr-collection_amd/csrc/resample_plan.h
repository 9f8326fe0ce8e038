// resample_plan.h — what the driver of the resampler (resample.hip: gc_resample) decides on the host: the argument checks, the NCO's
// two integers, the branches J of the polyphase filter, the tile of consecutive outputs a workgroup takes with the input span and the
// LDS bytes that go with it, and the walk of the tiles over noutputs.  Nothing here calls HIP, allocates on the device or launches;
// tests/resample_plan_shim.hip runs all of it without a device.  The NCO's integers, the finiteness test, the checks of the two records
// and the staging of a span in whole 16-byte vectors are fir_plan.h's; the workgroup's shape and the LDS budget are the
// down-converter's (ddc_plan.h), and with L = 1 the tile is ddc_tile_outputs(M, T).
#pragma once
#include "ddc_plan.h"

constexpr int kRsWG = kDdcWG;
constexpr int kRsChains = kDdcChains;       // outputs a thread carries at most; they share the phase, and with it every tap read
constexpr int kRsMaxTile = 1024;
constexpr long long kRsLdsBudget = kDdcLdsBudget;
static_assert(kRsMaxTile == kRsWG * kRsChains, "a thread carries kRsChains outputs of the largest tile");
static_assert(GC_RS_MAX_INTERP <= kRsWG, "one lane per phase at least");

__host__ __device__ inline int rs_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}
// Lp: the period of the phase p_m in m
__host__ __device__ inline int rs_phase_period(int interp, int decim) { return interp / rs_gcd(interp, decim); }
// Lanes of a workgroup that take outputs, and the distance in outputs between the chains of one lane: the largest multiple of Lp in
// kRsWG, so that every chain of a lane has the lane's phase and every output below kRsChains * stride has a lane.  (The next multiple
// ABOVE kRsWG would leave the outputs kRsWG .. stride - 1 of each round without a lane.)  Lp <= 64: at least 208 of 256 lanes work.
__host__ __device__ inline int rs_stride(int interp, int decim) {
  const int lp = rs_phase_period(interp, decim);
  return kRsWG / lp * lp;
}
// J: the taps of the longest branch, ceil(T / L)
__host__ __device__ inline int rs_branches(int interp, int ntaps) { return (ntaps + interp - 1) / interp; }
// (re, im) doubles of a staged tap row taps[p][0 .. J-1]: J, made odd where there is more than one row, so that the rows of
// neighbouring phases start 16 bytes * an odd number apart and a gather over the phases spreads over the LDS banks
__host__ __device__ inline int rs_row(int interp, int ntaps) {
  const int J = rs_branches(interp, ntaps);
  return interp == 1 ? J : (J | 1);
}
__host__ __device__ inline long long rs_taps_bytes(int interp, int ntaps) { return 16LL * interp * rs_row(interp, ntaps); }
// input samples under `outs` consecutive outputs at most (the first output on phase L - 1): the first output's oldest to the last's newest
inline long long rs_span(long long outs, int interp, int decim, int ntaps) {
  return ((outs - 1) * decim + (interp - 1)) / interp + rs_branches(interp, ntaps);
}
inline long long rs_lds_bytes(long long outs, int interp, int decim, int ntaps, int bps) {
  return rs_taps_bytes(interp, ntaps) + (rs_span(outs, interp, decim, ntaps) * bps + kFirStageSlack + 15) / 16 * 16;
}
inline bool rs_accepts(int interp, int decim, int ntaps) {
  return interp >= 1 && interp <= GC_RS_MAX_INTERP && decim >= 1 && decim <= GC_DDC_MAX_DECIM * interp && ntaps >= 1 && ntaps <= GC_RS_MAX_TAPS;
}
// outputs per workgroup: as many as fit the budget at the widest format, at most kRsChains per working lane; 0 for an (L, M, T) that
// is not accepted
inline long long rs_tile_outputs(int interp, int decim, int ntaps) {
  if (!rs_accepts(interp, decim, ntaps)) return 0;
  const long long span_max = (kRsLdsBudget - rs_taps_bytes(interp, ntaps) - kFirStageSlack - 15) / kFirMaxBps;
  long long outs = (span_max - rs_branches(interp, ntaps)) * interp / decim + 1;
  const long long most = (long long)kRsChains * rs_stride(interp, decim);
  return outs > most ? most : outs;
}
// one output fits whatever is accepted: the rows hold fewer than T + 2 L taps (J L < T + L, and one tap per row of padding), a branch
// at most T samples
static_assert((kRsLdsBudget - 16LL * (GC_RS_MAX_TAPS + 2 * GC_RS_MAX_INTERP) - kFirStageSlack - 15) / kFirMaxBps >= GC_RS_MAX_TAPS, "one output of the longest filter fits");
static_assert((kRsLdsBudget - 16LL * GC_RS_MAX_INTERP * ((GC_RS_MAX_TAPS / GC_RS_MAX_INTERP) | 1) - kFirStageSlack - 15) / kFirMaxBps >= GC_RS_MAX_TAPS / GC_RS_MAX_INTERP,
              "one output fits at the corner L = 64, T = 2048");

struct RsPlan {
  uint64_t phase_step = 0, phase0 = 0;
  double carr_freq = 0.0;   // the frequency the NCO runs at
  double out_rate = 0.0;    // (fs L) / M
  long long tile = 0;       // outputs per workgroup
  long long ntiles = 0;
  long long span = 0;       // input samples a full tile stages at most
  long long lds_bytes = 0;  // of a full tile at src's format
  long long lds_budget = 0;
  int src_bps = 0, dst_bps = 0;
  int branches = 0;         // J
  int row = 0;              // (re, im) doubles of a staged tap row
  int stride = 0;           // working lanes of a workgroup
};

// Tile t of the walk: outputs [m0, m0 + n), the first one at tick u0 = n0 L + p0, input samples [n_lo, n_hi] (n_lo may be negative,
// n_hi may lie beyond the record: zeros).  The kernel calls rs_tile and rs_output on the device, and stages with fir_stage_base and
// fir_stage_vecs.
struct RsTile {
  long long m0 = 0, n = 0, u0 = 0, n0 = 0, n_lo = 0, n_hi = 0;
  int p0 = 0;
};
__host__ __device__ inline RsTile rs_tile(long long tile, long long t, long long first_tick, long long noutputs, int interp, int decim, int ntaps) {
  RsTile r;
  r.m0 = t * tile;
  r.n = tile < noutputs - r.m0 ? tile : noutputs - r.m0;
  r.u0 = first_tick + r.m0 * decim;
  r.n0 = r.u0 / interp;
  r.p0 = (int)(r.u0 - r.n0 * interp);
  r.n_lo = r.n0 - (rs_branches(interp, ntaps) - 1);
  r.n_hi = r.n0 + (r.p0 + (r.n - 1) * decim) / interp;
  return r;
}
// output q of a tile whose first output has the phase p0 (q < kRsMaxTile, so p0 + q M < 2^23): its newest sample is n0 + *dn, its phase *p
__host__ __device__ inline void rs_output(int p0, int q, int interp, int decim, int* dn, int* p) {
  const int v = p0 + q * decim;
  *dn = v / interp;
  *p = v - *dn * interp;
}
inline bool rs_tile_at(const RsPlan& pl, const gc_rs_params* p, long long t, RsTile* out) {
  if (t < 0 || t >= pl.ntiles) return false;
  *out = rs_tile(pl.tile, t, (long long)p->first_tick, (long long)p->noutputs, p->interp, p->decim, p->ntaps);
  return true;
}

// gc_resample's checks (include/gnsscorr.h), in gc_downconvert's order: arguments, then state, then what needs both, then range; then
// the plan.  *pl is written only where the call is accepted.
inline int rs_check(const gc_context* src, const gc_context* dst, const gc_rs_params* p, const double* taps, RsPlan* pl) {
  if (!src || !dst || !p || !taps) {
    gc_set_error("gc_resample: null argument");
    return GC_E_INVALID;
  }
  if (p->first_tick < 0 || p->dst_first < 0 || p->noutputs < 1 || !rs_accepts(p->interp, p->decim, p->ntaps) || p->reserved != 0 ||
      !fir_finite(p->carr_freq) || !fir_finite(p->carr_phase)) {
    gc_set_error("gc_resample: bad arguments (first_tick %lld, noutputs %lld, dst_first %lld, interp %d, decim %d, ntaps %d, reserved %d, carr_freq %g, carr_phase %g)",
                 (long long)p->first_tick, (long long)p->noutputs, (long long)p->dst_first, p->interp, p->decim, p->ntaps, p->reserved, p->carr_freq, p->carr_phase);
    return GC_E_INVALID;
  }
  for (int k = 0; k < 2 * p->ntaps; ++k)
    if (!fir_finite(taps[k])) {
      gc_set_error("gc_resample: tap %d is not finite", k / 2);
      return GC_E_INVALID;
    }
  const double tick_rate = src->fs * (double)p->interp;
  uint64_t step = 0;
  const int rc = fir_check_records("gc_resample", src, dst, p->carr_freq, tick_rate, (long long)p->dst_first, (long long)p->noutputs, &step);
  if (rc) return rc;
  // here, where dst's record bounds noutputs, not among the arguments: up to here every status is gc_downconvert's for the same call
  const __int128 last_tick = (__int128)p->first_tick + (__int128)(p->noutputs - 1) * p->decim;
  if (last_tick > (__int128)INT64_MAX) {
    gc_set_error("gc_resample: the last output's tick does not fit in 63 bits");
    return GC_E_INVALID;
  }
  const int J = rs_branches(p->interp, p->ntaps);
  const long long oldest = (long long)(last_tick / p->interp) - (J - 1);  // the last output's oldest sample
  if (oldest >= 0 && (unsigned long long)oldest >= src->if_nsamples) {
    gc_set_error("gc_resample: the last output has no record sample under it (%llu samples)", (unsigned long long)src->if_nsamples);
    return GC_E_RANGE;
  }
  RsPlan q;
  q.phase_step = step;
  q.phase0 = fir_phase0(p->carr_phase);
  q.carr_freq = fir_nco_freq(step, tick_rate);
  q.out_rate = tick_rate / (double)p->decim;
  q.tile = rs_tile_outputs(p->interp, p->decim, p->ntaps);
  q.ntiles = ((long long)p->noutputs + q.tile - 1) / q.tile;
  q.span = rs_span(q.tile, p->interp, p->decim, p->ntaps);
  q.src_bps = gc_record_bps(src);
  q.dst_bps = gc_record_bps(dst);
  q.lds_bytes = rs_lds_bytes(q.tile, p->interp, p->decim, p->ntaps, q.src_bps);
  q.lds_budget = kRsLdsBudget;
  q.branches = J;
  q.row = rs_row(p->interp, p->ntaps);
  q.stride = rs_stride(p->interp, p->decim);
  *pl = q;
  return GC_OK;
}
