// The host plan of the resampler (csrc/resample_plan.h) on the CPU: two contexts that hold record FACTS only (an address that is
// never read, the device, the length, the format, the sampling frequency - no device memory) for gc_resample's argument checks, the
// NCO's two integers, the tile and its LDS bytes, and the tile walk, written out as plain integers.  Built by
// tests/test_resample_plan_cpu.py with the flags of resample.hip; no GPU is touched.
#include <cstdarg>

#include "../cu-sdr-collection_amd/csrc/resample_plan.h"

void gc_set_error(const char*, ...) {}

extern "C" {

// `address` 0: no record; otherwise an address that is never read, so that two contexts can share, overlap or miss each other
void* rs_shim_create(long long address, int device, unsigned long long if_nsamples, int dtype, int layout, double fs) {
  gc_context* ctx = new gc_context();
  ctx->d_if = address ? reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(address)) : nullptr;
  ctx->device = device;
  ctx->if_nsamples = if_nsamples;
  ctx->if_dtype = dtype;
  ctx->if_layout = layout;
  ctx->fs = fs;
  return ctx;
}

void rs_shim_destroy(void* ctx) { delete static_cast<gc_context*>(ctx); }

// gc_resample up to its first HIP call; where the call is accepted
// out = {phase_step, phase0, tile, ntiles, span, lds_bytes, lds_budget, src_bps, dst_bps, branches, row, stride},
// dbl = {the NCO's frequency, out_rate}
int rs_shim_check(void* src, void* dst, const gc_rs_params* p, const double* taps, unsigned long long* out, double* dbl) {
  RsPlan pl;
  const int rc = rs_check(static_cast<const gc_context*>(src), static_cast<const gc_context*>(dst), p, taps, &pl);
  if (rc) return rc;
  out[0] = pl.phase_step;
  out[1] = pl.phase0;
  out[2] = (unsigned long long)pl.tile;
  out[3] = (unsigned long long)pl.ntiles;
  out[4] = (unsigned long long)pl.span;
  out[5] = (unsigned long long)pl.lds_bytes;
  out[6] = (unsigned long long)pl.lds_budget;
  out[7] = (unsigned long long)pl.src_bps;
  out[8] = (unsigned long long)pl.dst_bps;
  out[9] = (unsigned long long)pl.branches;
  out[10] = (unsigned long long)pl.row;
  out[11] = (unsigned long long)pl.stride;
  dbl[0] = pl.carr_freq;
  dbl[1] = pl.out_rate;
  return GC_OK;
}

long long rs_shim_tile_outputs(int interp, int decim, int ntaps) { return rs_tile_outputs(interp, decim, ntaps); }

long long rs_shim_ddc_tile_outputs(int decim, int ntaps) { return ddc_tile_outputs(decim, ntaps); }

long long rs_shim_lds_bytes(long long outs, int interp, int decim, int ntaps, int bps) { return rs_lds_bytes(outs, interp, decim, ntaps, bps); }

// out = {Lp, stride, J, row, bytes of the staged taps}
void rs_shim_geometry(int interp, int decim, int ntaps, long long* out) {
  out[0] = rs_phase_period(interp, decim);
  out[1] = rs_stride(interp, decim);
  out[2] = rs_branches(interp, ntaps);
  out[3] = rs_row(interp, ntaps);
  out[4] = rs_taps_bytes(interp, ntaps);
}

// the walk over noutputs in tiles of rs_tile_outputs: per tile {m0, n, u0, n0, p0, n_lo, n_hi}.  Returns the integers written (or needed).
long long rs_shim_walk(long long first_tick, long long noutputs, int interp, int decim, int ntaps, long long* out, long long cap) {
  RsPlan pl;
  pl.tile = rs_tile_outputs(interp, decim, ntaps);
  if (pl.tile < 1) return 0;
  pl.ntiles = (noutputs + pl.tile - 1) / pl.tile;
  gc_rs_params p = {};
  p.first_tick = first_tick;
  p.noutputs = noutputs;
  p.interp = interp;
  p.decim = decim;
  p.ntaps = ntaps;
  long long n = 0;
  RsTile t;
  for (long long i = 0; rs_tile_at(pl, &p, i, &t); ++i)
    for (long long v : {t.m0, t.n, t.u0, t.n0, (long long)t.p0, t.n_lo, t.n_hi}) {
      if (n < cap) out[n] = v;
      ++n;
    }
  return n;
}

// output q of a tile whose first output has the phase p0: out = {samples past the tile's n0, phase}
void rs_shim_output(int p0, int q, int interp, int decim, long long* out) {
  int dn, p;
  rs_output(p0, q, interp, decim, &dn, &p);
  out[0] = dn;
  out[1] = p;
}

// what the kernel stages for the input samples [n_lo, n_hi]: out = {byte offset of the first vector, vectors}
void rs_shim_stage(long long n_lo, long long n_hi, int bps, long long* out) {
  out[0] = ddc_stage_base(n_lo, bps);
  out[1] = ddc_stage_vecs(n_lo, n_hi, bps);
}

void rs_shim_constants(long long* out) {
  out[0] = kRsWG;
  out[1] = kRsChains;
  out[2] = kRsMaxTile;
  out[3] = kRsLdsBudget;
  out[4] = GC_RS_MAX_TAPS;
  out[5] = GC_RS_MAX_INTERP;
  out[6] = kDdcStageSlack;
  out[7] = GC_DDC_MAX_DECIM;
}

}  // extern "C"
