// probe.hip - gc_probe_psd, gc_probe_histogram: what every package's include/probeData.m looks at before acquisition is tried
// (probeData.m:76 the stretch of record, :104 z = first + i * second value of each pair, :128-131 pwelch(data, 32768, 2048, 32768, fs),
// :146-163 hist(., -128:128) and dmax), computed where the record lives.  DESIGN.md 4.10.
//
// Spectrum: the (span, segment) list is cut into tiles (seg_fft.h, shared with the excision); per tile
//   gather_rows           converts and windows the tile's segments into float2 rows (seg_fft.hip, next to the transform it feeds),
//   transform_rows        runs the acquisition's two pass kernels over the rows (seg_fft.hip),
//   probe_power_kernel    adds |X|^2 of the tile's segments, in segment order, into the float64 accumulator of (span, bin).
// Histogram: probe_hist_kernel counts into per-wave LDS histograms and writes one partial row per workgroup,
//   probe_hist_combine_kernel adds the rows in 64-bit, one workgroup per bin.
// The probe's plan, twiddle table and rows (SegFft), window and accumulators are its own (ProbeState, kept in gc_context::probe): nothing of the
// acquisition's scratch, the conditioned signal or the bank's buffers is read, written or reallocated.
// A sample's components in file order are record_fmt.h's (file_sample, gc_with_file_mode); the range check is record_check.h's.
#include "probe_plan.h"
#include "record_fmt.h"

using namespace gcacq;

namespace {

constexpr int kProbeThreads = 256;
constexpr int kHistWaves = kProbeThreads / 64;
constexpr int kHistRow = 2 * GC_PROBE_HIST_BINS;  // a workgroup's partial row: both components

struct ProbeState {
  SegFft fft;
  int win_n = 0, win_kind = -1;  // what `win` holds
  double sumw2 = 0.0;
  GcBuf win, acc, hist_part, hist_max, hist_out;
};

// One thread per (span of the tile, storage position): |X|^2 of the span's segments in this tile, in segment order, added in float64 to
// what the span's earlier tiles left (probe_span_range: carried when the span began before this tile), written to the natural bin
// of the storage position (fft_plan.h).
__global__ __launch_bounds__(kProbeThreads) void probe_power_kernel(const float2* __restrict__ rows, long long g0, long long nseg, long long K,
                                                                     long long span0, int nfft, int n1, int n2, int blocks_per_row,
                                                                     double* __restrict__ acc) {
  const auto [j, pos] = row_element<kProbeThreads>(blocks_per_row);
  if (pos >= nfft) return;
  const long long span = span0 + j;
  long long k0, k1;
  probe_span_range(g0, nseg, K, span, &k0, &k1);
  if (k0 >= k1) return;
  double* const dst = acc + span * nfft + fft_bin_at(pos, n1, n2);
  double sum = k0 > 0 ? *dst : 0.0;
  const float2* __restrict__ src = rows + (span * K + k0 - g0) * nfft + pos;
  for (long long k = k0; k < k1; ++k, src += nfft) {
    const float2 v = *src;
    sum += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
  }
  *dst = sum;
}

// Counts of samples [s0, s0 + per_wg) of the range (cut at nsamples) in a private histogram per wave - a noise-like record hits a few
// dozen bins, and four waves on one LDS row would queue on them - then the workgroup's partial row and its largest c0^2 + c1^2.
template <int MODE>
__global__ __launch_bounds__(kProbeThreads) void probe_hist_kernel(const uint8_t* __restrict__ rec, long long first_sample, long long nsamples,
                                                                    long long per_wg, unsigned int* __restrict__ part,
                                                                    long long* __restrict__ part_max) {
  __shared__ unsigned int h[kHistWaves][kHistRow];
  __shared__ long long wmax[kHistWaves];
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int i = tid; i < kHistWaves * kHistRow; i += kProbeThreads) (&h[0][0])[i] = 0u;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * per_wg, hi = lo + per_wg < nsamples ? lo + per_wg : nsamples;
  long long m = 0;
  for (long long i = lo + tid; i < hi; i += kProbeThreads) {
    int c0, c1;
    gcorr::file_sample<MODE>(rec, first_sample + i, c0, c1);
    atomicAdd(&h[wave][min(max(c0, -128), 128) + 128], 1u);
    long long n2 = (long long)c0 * c0;
    if constexpr (gcorr::Fmt<MODE>::values == 2) {
      atomicAdd(&h[wave][GC_PROBE_HIST_BINS + min(max(c1, -128), 128) + 128], 1u);
      n2 += (long long)c1 * c1;
    }
    m = n2 > m ? n2 : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_xor(m, off, 64);
    m = o > m ? o : m;
  }
  if ((tid & 63) == 0) wmax[wave] = m;
  __syncthreads();
  for (int i = tid; i < kHistRow; i += kProbeThreads) {
    unsigned int c = 0;
    for (int w = 0; w < kHistWaves; ++w) c += h[w][i];
    part[(size_t)blockIdx.x * kHistRow + i] = c;
  }
  if (tid == 0) {
    for (int w = 1; w < kHistWaves; ++w) m = wmax[w] > m ? wmax[w] : m;
    part_max[blockIdx.x] = m;
  }
}

// One workgroup per output: out[i] = sum over the workgroups' partial rows, i < kHistRow, in 64-bit; out[kHistRow] = the largest partial
// maximum.  (Integer sums: the order does not matter.  One thread per output walking all 2 048 rows - dependent loads - took 0.6 ms: seven
// eighths of the call at one second of record)
__global__ __launch_bounds__(kProbeThreads) void probe_hist_combine_kernel(const unsigned int* __restrict__ part, const long long* __restrict__ part_max,
                                                                            long long nwg, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh[kHistWaves];
  const int i = blockIdx.x, tid = threadIdx.x;
  const bool is_max = i == kHistRow;
  unsigned long long v = 0;
  for (long long g = tid; g < nwg; g += kProbeThreads) {
    const unsigned long long x = is_max ? (unsigned long long)part_max[g] : (unsigned long long)part[g * kHistRow + i];
    v = is_max ? (x > v ? x : v) : v + x;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = is_max ? (o > v ? o : v) : v + o;
  }
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kHistWaves; ++w) v = is_max ? (sh[w] > v ? sh[w] : v) : v + sh[w];
    out[i] = v;
  }
}

// the n-point window of `kind`
int probe_window(gc_context* ctx, ProbeState* s, int n, int kind) {
  if (s->win_n == n && s->win_kind == kind) return GC_OK;
  s->win_n = 0;
  if (gc_buf_reserve(s->win, (size_t)n * sizeof(float), false) != hipSuccess) return gc_nomem("gc_probe_psd");
  std::vector<float> w((size_t)n);
  double sum2 = 0.0;
  for (int k = 0; k < n; ++k) {
    const double v = kind == GC_WIN_HAMMING ? 0.54 - 0.46 * std::cos(2.0 * 3.14159265358979323846 * (double)k / (double)(n - 1)) : 1.0;
    sum2 += v * v;
    w[(size_t)k] = (float)v;
  }
  GC_HIP(hipMemcpyAsync(s->win.p, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  GC_HIP(hipStreamSynchronize(ctx->stream));
  s->sumw2 = sum2;
  s->win_n = n;
  s->win_kind = kind;
  return GC_OK;
}

}  // namespace

void gc_probe_free(gc_context* ctx) {
  ProbeState* s = static_cast<ProbeState*>(ctx->probe);
  if (!s) return;
  seg_fft_free(&s->fft);
  for (GcBuf* b : {&s->win, &s->acc, &s->hist_part, &s->hist_max, &s->hist_out}) gc_buf_free(*b);
  delete s;
  ctx->probe = nullptr;
}

extern "C" long long gc_debug_probe_tile_segments(int nfft) { return nfft < 2 ? 0 : probe_tile_segments(nfft, ProbeBudget()); }

extern "C" int gc_probe_psd(gc_context* ctx, const gc_probe_psd_params* p, double* psd, int64_t* nsegments) {
  int rc = probe_check_args(ctx, p, psd);
  if (rc) return rc;
  Plan plan;
  rc = plan_or_refuse(p->nfft, &plan);
  if (rc) return rc;
  ProbePlan pl;
  rc = probe_check_state(ctx, p, ProbeBudget(), &pl);
  if (rc) return rc;
  GC_HIP(hipSetDevice(ctx->device));
  ProbeState* s = gc_unit_state<ProbeState>(ctx->probe);
  if (!s) return gc_nomem("gc_probe_psd");
  const int nfft = p->nfft;
  const size_t cells = (size_t)p->nspans * (size_t)nfft;
  if (gc_buf_reserve(s->acc, cells * sizeof(double), false) != hipSuccess) return gc_nomem("gc_probe_psd");
  rc = seg_fft_prepare(ctx, &s->fft, plan, std::min(pl.tile, pl.total), "gc_probe_psd");
  if (rc) return rc;
  rc = probe_window(ctx, s, nfft, p->window);
  if (rc) return rc;
  float2 *const rows_a = (float2*)s->fft.rows_a.p, *const rows_b = (float2*)s->fft.rows_b.p;
  const int bpr = (nfft + kProbeThreads - 1) / kProbeThreads;
  const RowGather segs = {(long long)p->first_sample, (long long)p->nsamples, pl.step, pl.K, 0};
  for (ProbeTile t; probe_next_tile(pl, t);) {
    rc = gather_rows(ctx, segs, t.g0, t.n, nfft, (const float*)s->win.p, rows_a);
    if (rc) return rc;
    rc = transform_rows(ctx, s->fft.plan, (const float2*)s->fft.tw.p, rows_a, rows_b, t.n, 0);
    if (rc) return rc;
    const long long span0 = t.g0 / pl.K, span1 = (t.g0 + t.n - 1) / pl.K;
    hipLaunchKernelGGL(probe_power_kernel, dim3((unsigned int)((span1 - span0 + 1) * bpr)), dim3(kProbeThreads), 0, ctx->stream,
                       (const float2*)rows_a, t.g0, t.n, pl.K, span0, nfft, plan.n1, plan.n2, bpr, (double*)s->acc.p);
    GC_HIP(hipGetLastError());
  }
  std::vector<double> host(cells);
  GC_HIP(hipMemcpyAsync(host.data(), s->acc.p, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GC_HIP(hipStreamSynchronize(ctx->stream));
  const double den = (double)pl.K * ctx->fs * s->sumw2;
  for (size_t i = 0; i < cells; ++i) psd[i] = host[i] / den;
  if (nsegments) *nsegments = pl.K;
  return GC_OK;
}

extern "C" int gc_probe_histogram(gc_context* ctx, int64_t first_sample, int64_t nsamples, uint64_t* counts, int64_t* max_norm2) {
  int rc = probe_check_histogram(ctx, (long long)first_sample, (long long)nsamples, counts);
  if (rc) return rc;
  GC_HIP(hipSetDevice(ctx->device));
  ProbeState* s = gc_unit_state<ProbeState>(ctx->probe);
  if (!s) return gc_nomem("gc_probe_histogram");
  const ProbeHistGrid g = probe_hist_grid((long long)nsamples);
  if (gc_buf_reserve(s->hist_part, (size_t)g.grid * kHistRow * sizeof(unsigned int), false) != hipSuccess ||
      gc_buf_reserve(s->hist_max, (size_t)g.grid * sizeof(long long), false) != hipSuccess ||
      gc_buf_reserve(s->hist_out, (size_t)(kHistRow + 1) * sizeof(unsigned long long), false) != hipSuccess)
    return gc_nomem("gc_probe_histogram");
  gcorr::gc_with_file_mode(gcorr::gc_record_mode(ctx), [&](auto m) {
    hipLaunchKernelGGL(probe_hist_kernel<decltype(m)::value>, dim3((unsigned int)g.grid), dim3(kProbeThreads), 0, ctx->stream, ctx->d_if,
                       (long long)first_sample, (long long)nsamples, g.per_wg, (unsigned int*)s->hist_part.p, (long long*)s->hist_max.p);
  });
  GC_HIP(hipGetLastError());
  hipLaunchKernelGGL(probe_hist_combine_kernel, dim3(kHistRow + 1), dim3(kProbeThreads), 0, ctx->stream,
                     (const unsigned int*)s->hist_part.p, (const long long*)s->hist_max.p, g.grid, (unsigned long long*)s->hist_out.p);
  GC_HIP(hipGetLastError());
  unsigned long long host[kHistRow + 1];
  GC_HIP(hipMemcpyAsync(host, s->hist_out.p, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
  GC_HIP(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < kHistRow; ++i) counts[i] = host[i];
  if (max_norm2) *max_norm2 = (int64_t)host[kHistRow];
  return GC_OK;
}
