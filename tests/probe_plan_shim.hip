// The host plan of the record probe (csrc/probe_plan.h) on the CPU: a context that holds record FACTS only (whether there is one, its
// length, the sampling frequency - no device memory) for the argument checks, the segment count, and the tile walk over the (span,
// segment) list under budgets the caller chooses, written out as plain integers.  Built by tests/test_probe_plan_cpu.py with the
// flags of probe.hip; no GPU is touched.
#include <cstdarg>

#include "../cu-sdr-collection_amd/csrc/probe_plan.h"

void gc_set_error(const char*, ...) {}

extern "C" {

void* probe_shim_create(int have_record, unsigned long long if_nsamples, double fs) {
  static uint8_t no_record;
  gc_context* ctx = new gc_context();
  ctx->d_if = have_record ? &no_record : nullptr;  // never read
  ctx->if_nsamples = if_nsamples;
  ctx->fs = fs;
  return ctx;
}

void probe_shim_destroy(void* ctx) { delete static_cast<gc_context*>(ctx); }

// gc_probe_psd up to the transform planner's question: probe_check_args, then probe_check_state under tile_bytes (0: the library's);
// out = {step, K, total, tile} where the call is accepted
int probe_shim_check(void* ctx, const gc_probe_psd_params* p, int have_psd, long long tile_bytes, long long* out) {
  static double some_output;
  int rc = probe_check_args(static_cast<const gc_context*>(ctx), p, have_psd ? &some_output : nullptr);
  if (rc) return rc;
  ProbeBudget b;
  if (tile_bytes > 0) b.tile_bytes = tile_bytes;
  ProbePlan pl;
  rc = probe_check_state(static_cast<const gc_context*>(ctx), p, b, &pl);
  if (rc) return rc;
  out[0] = pl.step;
  out[1] = pl.K;
  out[2] = pl.total;
  out[3] = pl.tile;
  return GC_OK;
}

int probe_shim_check_histogram(void* ctx, long long first_sample, long long nsamples, int have_counts) {
  static uint64_t some_output;
  return probe_check_histogram(static_cast<const gc_context*>(ctx), first_sample, nsamples, have_counts ? &some_output : nullptr);
}

long long probe_shim_segments(long long nsamples, int nfft, int noverlap) { return probe_segments(nsamples, nfft, noverlap); }

long long probe_shim_tile_segments(int nfft, long long tile_bytes) {
  ProbeBudget b;
  if (tile_bytes > 0) b.tile_bytes = tile_bytes;
  return probe_tile_segments(nfft, b);
}

// gc_probe_psd's walk over nspans spans of K segments in tiles of `tile`: per tile {g0, n, first span, last span}, then per span of
// the tile {span, k0, k1} as probe_span_range gives them to the power kernel.  Returns the integers written (or needed).
long long probe_shim_walk(long long K, int nspans, long long tile, long long* out, long long cap) {
  long long n = 0;
  auto put = [&](long long v) {
    if (n < cap) out[n] = v;
    ++n;
  };
  ProbePlan pl;
  pl.K = K;
  pl.total = K * nspans;
  pl.tile = tile;
  for (ProbeTile t; probe_next_tile(pl, t);) {
    const long long span0 = t.g0 / K, span1 = (t.g0 + t.n - 1) / K;
    for (long long v : {t.g0, t.n, span0, span1}) put(v);
    for (long long s = span0; s <= span1; ++s) {
      long long k0, k1;
      probe_span_range(t.g0, t.n, K, s, &k0, &k1);
      for (long long v : {s, k0, k1}) put(v);
    }
  }
  return n;
}

void probe_shim_hist_grid(long long nsamples, long long* out) {
  const ProbeHistGrid g = probe_hist_grid(nsamples);
  out[0] = g.per_wg;
  out[1] = g.grid;
}

}  // extern "C"
