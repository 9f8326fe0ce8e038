// seg_fft.hip — the segment transform of the record units (seg_fft.h): a tile's rows gathered from the record, their transform on the
// acquisition's pass kernels, the per-context state.  The one record-side unit that includes acq_internal.h (PassArgs, two_pass).
#include "seg_fft.h"
#include "acq_internal.h"
#include "record_fmt.h"

using namespace gcacq;

namespace {
// One workgroup per kFftThreads consecutive values of one row (gather_rows); row 0 is segment k0 of span span0.  The division is
// taken only by the rows behind a span's end (wave-uniform), and the record is read without a branch - outside the span a sample
// of the span that is not used - so that it and the window's value are in flight together.
template <int MODE>
__global__ __launch_bounds__(kFftThreads) void gather_rows_kernel(const uint8_t* __restrict__ rec, const RowGather r, long long span0, long long k0, int nfft,
                                                                   int blocks_per_row, const float* __restrict__ win, float2* __restrict__ rows) {
  const auto [t, n] = row_element<kFftThreads>(blocks_per_row);
  if (n >= nfft) return;
  long long span = span0, k = k0 + t;
  if (k >= r.K) {
    const long long q = k / r.K;
    span += q;
    k -= q * r.K;
  }
  const long long m = k * r.step - r.lead + n;
  const bool inside = m >= 0 && m < r.nsamples;
  int c0, c1;
  gcorr::file_sample<MODE>(rec, r.first + span * r.nsamples + (inside ? m : 0), c0, c1);
  const float w = win[n];
  rows[t * nfft + n] = make_float2(w * (float)(inside ? c0 : 0), w * (float)(inside ? c1 : 0));  // a real record: w * 0 = +0, the windows are not negative
}
}  // namespace

namespace gcacq {

int gather_rows(gc_context* ctx, const RowGather& r, long long g0, long long nrows, int nfft, const float* win, float2* rows) {
  const int bpr = (nfft + kFftThreads - 1) / kFftThreads;
  const long long span0 = g0 / r.K, k0 = g0 - span0 * r.K;
  gcorr::gc_with_file_mode(gcorr::gc_record_mode(ctx), [&](auto m) {
    hipLaunchKernelGGL(gather_rows_kernel<decltype(m)::value>, dim3((unsigned int)(nrows * bpr)), dim3(kFftThreads), 0, ctx->stream, ctx->d_if, r, span0, k0, nfft,
                       bpr, win, rows);
  });
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int transform_rows(gc_context* ctx, const Plan& pl, const float2* tw, float2* a_rows, float2* b_rows, long long nbatch, int inverse) {
  PassArgs a;
  std::memset(&a, 0, sizeof a);
  a.in = a_rows;
  a.in_batch_stride = pl.n;
  return two_pass(ctx, pl, tw, a, PRE_NONE, inverse, b_rows, a_rows, nbatch);
}

int seg_fft_prepare(gc_context* ctx, SegFft* s, const Plan& pl, long long tile_rows, const char* who) {
  const size_t rows_bytes = (size_t)tile_rows * (size_t)pl.n * sizeof(float2);
  if (gc_buf_reserve(s->rows_a, rows_bytes, false) != hipSuccess || gc_buf_reserve(s->rows_b, rows_bytes, false) != hipSuccess) return gc_nomem(who);
  if (s->n == pl.n) return GC_OK;
  s->n = 0;
  if (gc_buf_reserve(s->tw, (size_t)pl.n * sizeof(float2), false) != hipSuccess) return gc_nomem(who);
  const int rc = upload_twiddles(ctx, pl.n, (float2*)s->tw.p);
  if (rc) return rc;
  s->plan = pl;
  s->n = pl.n;
  return GC_OK;
}

void seg_fft_free(SegFft* s) {
  for (GcBuf* b : {&s->tw, &s->rows_a, &s->rows_b}) gc_buf_free(*b);
}

}  // namespace gcacq
