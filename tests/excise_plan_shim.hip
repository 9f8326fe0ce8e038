// The host plan of the excision (csrc/excise_plan.h) on the CPU: two contexts that hold record FACTS only (an address that is never
// read, the device, the length, the format - no device memory) for the argument checks of gc_excise_pulses and gc_excise_bins, the
// layout of the blanker's range over its bitmap and tiles, and the spectral excision's segment count and tile walk under budgets
// the caller chooses, written out as plain integers.  Built by tests/test_excise_plan_cpu.py with the flags of excise.hip; no GPU
// is touched.
#include <cstdarg>

#include "../cu-sdr-collection_amd/csrc/excise_plan.h"

void gc_set_error(const char*, ...) {}

extern "C" {

// `address` 0: no record; otherwise an address inside one static array, so that two contexts can share, overlap or miss each other
void* excise_shim_create(long long address, int device, unsigned long long if_nsamples, int dtype, int layout) {
  gc_context* ctx = new gc_context();
  ctx->d_if = address ? reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(address)) : nullptr;  // never read
  ctx->device = device;
  ctx->if_nsamples = if_nsamples;
  ctx->if_dtype = dtype;
  ctx->if_layout = layout;
  return ctx;
}

void excise_shim_destroy(void* ctx) { delete static_cast<gc_context*>(ctx); }

// gc_excise_pulses up to its first HIP call; out = {base, ntiles, words, bps} where the call is accepted
int excise_shim_check_pulses(void* src, void* dst, const gc_excise_pulse_params* p, long long* out) {
  ExcisePulsePlan pl;
  const int rc = excise_check_pulses(static_cast<const gc_context*>(src), static_cast<const gc_context*>(dst), p, &pl);
  if (rc) return rc;
  out[0] = pl.base;
  out[1] = pl.ntiles;
  out[2] = pl.words;
  out[3] = pl.bps;
  return GC_OK;
}

// gc_excise_bins up to the transform planner's question: excise_check_bins, then excise_check_bins_state under tile_bytes (0: the
// library's); out = {H, K, tile} where the call is accepted
int excise_shim_check_bins(void* src, void* dst, const gc_excise_bins_params* p, const float* gain, long long tile_bytes, long long* out) {
  int rc = excise_check_bins(static_cast<const gc_context*>(src), static_cast<const gc_context*>(dst), p, gain);
  if (rc) return rc;
  ExciseBudget b;
  if (tile_bytes > 0) b.tile_bytes = tile_bytes;
  ExciseBinsPlan pl;
  rc = excise_check_bins_state(static_cast<const gc_context*>(src), static_cast<const gc_context*>(dst), p, b, &pl);
  if (rc) return rc;
  out[0] = pl.H;
  out[1] = pl.K;
  out[2] = pl.tile;
  return GC_OK;
}

long long excise_shim_segments(long long nsamples, int nfft) { return excise_segments(nsamples, nfft); }

long long excise_shim_tile_segments(int nfft, long long tile_bytes) {
  ExciseBudget b;
  if (tile_bytes > 0) b.tile_bytes = tile_bytes;
  return excise_tile_segments(nfft, b);
}

// gc_excise_bins' walk over K segments of hop H in tiles of `tile`: per tile {g0, n, carried, m0, m1}.  Returns the integers written
// (or needed).
long long excise_shim_walk(long long nsamples, long long H, long long K, long long tile, long long* out, long long cap) {
  long long n = 0;
  ExciseBinsPlan pl;
  pl.H = H;
  pl.K = K;
  pl.tile = tile;
  pl.nsamples = nsamples;
  for (ExciseTile t; excise_next_tile(pl, t);)
    for (long long v : {t.g0, t.n, t.carried, t.m0, t.m1}) {
      if (n < cap) out[n] = v;
      ++n;
    }
  return n;
}

void excise_shim_constants(long long* out) {
  out[0] = kExciseTile;
  out[1] = kExciseTileWords;
  out[2] = kExciseHalo;
  out[3] = GC_EXCISE_MAX_GUARD;
}

}  // extern "C"
