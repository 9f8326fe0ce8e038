// seg_fft.h — the segment transform of the record units (probe.hip: gc_probe_psd; excise.hip: gc_excise_bins, gc_excise_sweep): a
// stretch of the record cut into windowed segments that are transformed tile by tile on the acquisition's pass kernels (seg_fft.hip).
// Shared: the byte budget of a tile and the walk over the segment list (host integers, no HIP call: the plan headers and their CPU shims use
// them), the gather and the transform of a tile's rows, their per-context state.  A unit writes its checks, its window and the kernel that finishes a segment.
#pragma once
#include <algorithm>

#include "fft_plan.h"

// What one tile's rows may take: two buffers of float2 rows (the transform's passes go from one to the other and back), so that a
// tile that is gathered, transformed and finished stays inside the 256 MB last-level cache.  The CPU tests pass budgets of a few segments.
struct SegBudget { long long tile_bytes = 128LL << 20; };

// segments of an nfft-point transform per tile under `b`: two float2 rows each, at least one
inline long long seg_tile_segments(int nfft, const SegBudget& b) {
  const long long row = 2LL * (long long)nfft * (long long)sizeof(float2);
  return std::max<long long>(1, b.tile_bytes / row);
}

struct SegTile {
  long long g0 = 0, n = 0;  // first segment of the list, segments (0: before the first tile)
};

// the tile walk: for (SegTile t; seg_next_tile(tile, total, t);) - consecutive runs of at most `tile` segments of a list of `total`
inline bool seg_next_tile(long long tile, long long total, SegTile& t) {
  t.g0 += t.n;
  t.n = std::min(tile, total - t.g0);
  return t.n > 0;
}

namespace gcacq {

// The rows a segment transform takes, from the context's record in file order (c1 = 0 for a real record): the samples from `first` are
// cut into spans of `nsamples`, a span into K segments `step` apart, the first one `lead` samples in front of the span.  Row t of
// rows[nrows][nfft] is segment g = g0 + t (span = g / K, k = g - span K): value n is win[n] * x of span sample m = k step - lead + n,
// and zero where m lies outside [0, nsamples).
struct RowGather {
  long long first, nsamples, step, K, lead;
};
int gather_rows(gc_context* ctx, const RowGather& r, long long g0, long long nrows, int nfft, const float* win, float2* rows);

// What a unit keeps per context for its transforms (grow-only; seg_fft_free releases it)
struct SegFft {
  int n = 0;  // transform length of plan and tw (0: none)
  Plan plan;
  GcBuf tw, rows_a, rows_b;
};
// The two row buffers for tiles of `tile_rows` segments of pl.n points, and - where pl.n is not the length the state holds - the plan
// and its twiddle table on the context's stream, which is then waited for.  GC_E_NOMEM in the name of `who`.
int seg_fft_prepare(gc_context* ctx, SegFft* s, const Plan& pl, long long tile_rows, const char* who);
void seg_fft_free(SegFft* s);
// Transform of `nbatch` rows of a (natural order, pl.n values each) in place, b the intermediate, with the twiddle table tw of pl.n
// entries; the result in storage order (fft_plan.h).  inverse = 1 is the unnormalised inverse.  (acq_fft.hip's two_pass without a
// pre-operation; gc_debug_fft is this between an upload and a download.)
int transform_rows(gc_context* ctx, const Plan& pl, const float2* tw, float2* a_rows, float2* b_rows, long long nbatch, int inverse);

#if defined(__HIPCC__)
// blockIdx.x -> (row, element), blocks_per_row workgroups of THREADS per row (element may lie past the row's end): const auto [row, el] = row_element<..>(..)
struct RowElement {
  long long row;
  int el;
};
template <int THREADS>
__device__ __forceinline__ RowElement row_element(int blocks_per_row) {
  const long long row = blockIdx.x / (unsigned)blocks_per_row;
  return {row, (int)(blockIdx.x - (unsigned)(row * blocks_per_row)) * THREADS + (int)threadIdx.x};
}
#endif

}  // namespace gcacq
