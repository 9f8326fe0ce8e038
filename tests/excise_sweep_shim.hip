// The host plan of the swept excision (csrc/excise_plan.h) on the CPU: two contexts that hold record FACTS only (an address that is
// never read, the device, the length, the format - no device memory) for the argument checks of gc_excise_sweep, the words of a mask
// row, and the rows the tile walk names in the caller's [K] arrays under budgets the caller chooses, written out as plain integers.
// Built by tests/test_excise_sweep_plan_cpu.py with the flags of excise.hip; no GPU is touched.
#include <cstdarg>

#include "../cu-sdr-collection_amd/csrc/excise_plan.h"

void gc_set_error(const char*, ...) {}

extern "C" {

void* sweep_shim_create(long long address, int device, unsigned long long if_nsamples, int dtype, int layout) {
  gc_context* ctx = new gc_context();
  ctx->d_if = address ? reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(address)) : nullptr;  // never read
  ctx->device = device;
  ctx->if_nsamples = if_nsamples;
  ctx->if_dtype = dtype;
  ctx->if_layout = layout;
  return ctx;
}

void sweep_shim_destroy(void* ctx) { delete static_cast<gc_context*>(ctx); }

// gc_excise_sweep up to the transform planner's question, then the state under tile_bytes (0: the library's);
// out = {H, K, tile, W, rows of the tile buffers} where the call is accepted
int sweep_shim_check(void* src, void* dst, const gc_excise_sweep_params* p, const float* limit, const float* gain, long long tile_bytes, long long* out) {
  int rc = excise_check_sweep(static_cast<const gc_context*>(src), static_cast<const gc_context*>(dst), p, limit, gain);
  if (rc) return rc;
  ExciseBudget b;
  if (tile_bytes > 0) b.tile_bytes = tile_bytes;
  ExciseSweepPlan pl;
  rc = excise_check_sweep_state(static_cast<const gc_context*>(src), static_cast<const gc_context*>(dst), p, b, &pl);
  if (rc) return rc;
  out[0] = pl.seg.H;
  out[1] = pl.seg.K;
  out[2] = pl.seg.tile;
  out[3] = pl.W;
  out[4] = excise_tile_rows(pl);
  return GC_OK;
}

long long sweep_shim_mask_words(int nfft) { return excise_mask_words(nfft); }

// the walk over K segments of an nfft-point sweep in tiles of `tile`: per tile {g0, n, mask offset in words, power offset in floats}.
// Returns the integers written (or needed).
long long sweep_shim_walk(long long nsamples, int nfft, long long tile, long long* out, long long cap) {
  long long n = 0;
  ExciseSweepPlan pl;
  pl.seg.H = nfft / 2;
  pl.seg.K = excise_segments(nsamples, nfft);
  pl.seg.tile = tile;
  pl.seg.nsamples = nsamples;
  pl.W = excise_mask_words(nfft);
  for (ExciseTile t; excise_next_tile(pl.seg, t);)
    for (long long v : {t.g0, t.n, excise_mask_offset(pl, t), excise_power_offset(pl, t)}) {
      if (n < cap) out[n] = v;
      ++n;
    }
  return n;
}

int sweep_shim_max_widen() { return GC_EXCISE_MAX_WIDEN; }

}  // extern "C"
