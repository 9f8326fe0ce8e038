// excise.hip — gc_excise_pulses: the samples of a range that stand over a level, and a guard of samples around each, written as zero
// (include/gnsscorr.h has the definition).  Exact integers throughout; samples in file order, as the probe takes them.
//
// The range is laid over a bitmap of one bit per sample (excise_plan.h: bit 0 a multiple of 64 at or below the range's first sample,
// kExciseHalo zero words on either side) and cut into tiles of kExciseTile samples, one workgroup each:
//   excise_mark_kernel     one thread per 16 bytes of record: c0^2 + c1^2 > threshold2 of its samples in 64 bits, the lanes of a
//                          bitmap word joined by shuffles, one store per word.  Samples outside the range give zero bits.
//   excise_blank_kernel    the tile's words and a halo of the longest guard on either side into LDS, an exclusive prefix count of hot
//                          bits over them; sample n is blanked iff the count over [n - after, n + before] is not zero: two prefix
//                          reads and two masked popcounts.  A thread's 16 bytes are loaded, blanked and stored as a RecVec
//                          (record_fmt.h); in place, 16 bytes without a blanked sample are neither read nor written.  The tile's
//                          blanked bits are kept in LDS and folded into its summary: ones at its head, ones at its tail, longest run,
//                          runs, blanked and hot samples.
//   excise_combine_kernel  folds the tiles' summaries in tile order - a run that crosses a tile boundary is the tail of one joined to
//                          the head of the next - into the four statistics.
// No atomics; integer sums; a sample's output depends on its own bytes and the hot bits within the guards of it.
//
// gc_excise_bins: a gain per frequency bin, by weighted overlap-add (sine window, half-overlapping segments) on the acquisition's
// float32 transform.  The segment list is cut into tiles (excise_plan.h); per tile
//   gather_rows            converts and windows the tile's segments into float2 rows, zero outside the range (acq_fft.hip),
//   transform_rows         forward: the pass pair the probe runs (acq_fft.hip),
//   excise_gain_kernel     multiplies by the gain and moves storage position [k1][k2] to natural bin k1 + n1 k2, where the inverse
//                          pair expects it,
//   transform_rows         inverse = 1,
//   excise_add_kernel      one thread per 16 bytes of record: y = s v of the earlier segment's second half + s v of the later
//                          segment's first half, quantised into a RecVec; y itself to a float2 buffer of the range when the caller
//                          asks for it,
//   excise_carry_kernel    keeps s v of the second half of the tile's last segment for the next tile: its samples are not gathered
//                          again after they were overwritten (in place), and a sample's value is the same sum wherever the cut falls.
// Out of place the record is copied first and the add kernel works on the copy.
// The unit's buffers are its own (ExciseState, kept in gc_context::excise, grow-only, released by gc_destroy).
#include <algorithm>
#include <cmath>

#include "acq_internal.h"
#include "excise_plan.h"
#include "record_fmt.h"

using namespace gcorr;

namespace {

constexpr int kExciseWG = 256;
constexpr int kExciseLdsWords = kExciseTileWords + 2 * kExciseHalo + 1;  // the tile, its halos, and the word the last prefix count names
static_assert(kExciseLdsWords <= 2 * kExciseWG, "the prefix count takes two words per thread");
static_assert(kExciseTileWords == kExciseWG, "one thread per word of the tile's blanked bits");

struct ExciseState {  // grow-only device buffers of the context (released by gc_destroy)
  GcBuf bitmap, tiles, stats;  // gc_excise_pulses
  int n = 0;                   // gc_excise_bins: transform length of plan, tw and win (0: none)
  gcacq::Plan plan;
  GcBuf tw, win, gain, rows_a, rows_b, carry, values;  // win: w[nfft] then s[nfft]
};

// A stretch of samples as the run statistics see it: `pre` blanked samples at its head, `suf` at its tail (both `len` when all are),
// the longest run inside, the runs, and two plain sums
struct Runs {
  long long len, pre, suf, best, runs, blanked, hot;
};

__host__ __device__ inline Runs join(const Runs& a, const Runs& b) {
  Runs r;
  r.len = a.len + b.len;
  r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
  r.suf = b.suf == b.len ? b.len + a.suf : b.suf;
  const long long mid = a.suf + b.pre;
  r.best = a.best > b.best ? a.best : b.best;
  r.best = mid > r.best ? mid : r.best;
  r.runs = a.runs + b.runs - ((a.suf > 0 && b.pre > 0) ? 1 : 0);
  r.blanked = a.blanked + b.blanked;
  r.hot = a.hot + b.hot;
  return r;
}

struct TileRuns {  // a tile's summary (len = kExciseTile)
  int32_t pre, suf, best, runs, blanked, hot;
};

struct ExciseArgs {
  const uint8_t* src;
  uint8_t* dst;
  unsigned long long* bitmap;  // word kExciseHalo + w holds the samples base + 64 w ..
  TileRuns* tiles;
  long long base, first, end;  // record samples: bit 0 of the bitmap, the range
  long long rec_bytes;         // of the record
  long long threshold2;
  int before, after;
  int in_place;
};

// the bits of the lanes that share a bitmap word (64 / per16 consecutive lanes), in every one of them
template <int PER16>
__device__ __forceinline__ unsigned long long join_word(unsigned int mask, int lane) {
  constexpr int lanes = 64 / PER16;
  unsigned long long x = (unsigned long long)mask << ((lane & (lanes - 1)) * PER16);
#pragma unroll
  for (int o = 1; o < lanes; o <<= 1) x |= __shfl_xor(x, o, 64);
  return x;
}

template <int MODE>
__global__ __launch_bounds__(kExciseWG) void excise_mark_kernel(const ExciseArgs p) {
  using F = Fmt<MODE>;
  constexpr int P = F::per16, kVecs = kExciseTile / P / kExciseWG;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const long long tile0 = p.base + (long long)blockIdx.x * kExciseTile;  // the tile's first sample
  unsigned long long* const words = p.bitmap + kExciseHalo + (long long)blockIdx.x * kExciseTileWords;
#pragma unroll 1
  for (int k = 0; k < kVecs; ++k) {
    const int q = k * kExciseWG + tid;
    const long long n0 = tile0 + (long long)q * P;
    unsigned int mask = 0u;
    if (n0 + P > p.first && n0 < p.end) {  // p.end is inside the record: at least one sample of it
      RecVec<MODE> d;
      d.load(p.src, n0 * F::bps, p.rec_bytes);
#pragma unroll
      for (int s = 0; s < P; ++s) {
        int c0, c1;
        d.get(s, c0, c1);
        const long long n = n0 + s;
        if (n >= p.first && n < p.end && (long long)c0 * c0 + (long long)c1 * c1 > p.threshold2) mask |= 1u << s;
      }
    }
    const unsigned long long word = join_word<P>(mask, lane);
    if ((lane & (64 / P - 1)) == 0) words[(q * P) >> 6] = word;
  }
}

// hot bits below LDS bit x
__device__ __forceinline__ int hot_below(const unsigned long long* w, const int* pre, int x) {
  const int j = x >> 6;
  return pre[j] + __popcll(w[j] & ((1ull << (x & 63)) - 1ull));
}

template <int MODE>
__global__ __launch_bounds__(kExciseWG) void excise_blank_kernel(const ExciseArgs p) {
  using F = Fmt<MODE>;
  constexpr int P = F::per16, kVecs = kExciseTile / P / kExciseWG;
  __shared__ unsigned long long w[kExciseLdsWords];  // LDS bit x is tile sample x - GC_EXCISE_MAX_GUARD
  __shared__ int pre[kExciseLdsWords];               // hot bits in the words in front of each
  __shared__ unsigned long long bl[kExciseTileWords];  // the tile's blanked bits
  __shared__ int wave_sum[kExciseWG / 64];
  __shared__ Runs wave_runs[kExciseWG / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long* const g = p.bitmap + (long long)blockIdx.x * kExciseTileWords;  // the tile's front halo begins here
  for (int j = tid; j < kExciseLdsWords; j += kExciseWG) w[j] = g[j];
  __syncthreads();
  {  // exclusive prefix count: two words per thread, the lanes by shuffles, the waves in index order
    const int j0 = 2 * tid;
    const int c0 = j0 < kExciseLdsWords ? __popcll(w[j0]) : 0, c1 = j0 + 1 < kExciseLdsWords ? __popcll(w[j0 + 1]) : 0;
    int incl = c0 + c1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int off = 0;
    for (int i = 0; i < wave; ++i) off += wave_sum[i];
    const int excl = off + incl - c0 - c1;
    if (j0 < kExciseLdsWords) pre[j0] = excl;
    if (j0 + 1 < kExciseLdsWords) pre[j0 + 1] = excl + c0;
  }
  __syncthreads();
  const long long tile0 = p.base + (long long)blockIdx.x * kExciseTile;
#pragma unroll 1
  for (int k = 0; k < kVecs; ++k) {
    const int q = k * kExciseWG + tid;
    const long long n0 = tile0 + (long long)q * P;
    unsigned int mask = 0u;
    const bool mine = n0 + P > p.first && n0 < p.end;  // the vector holds a sample of the range
    if (mine) {
#pragma unroll
      for (int s = 0; s < P; ++s) {
        const long long n = n0 + s;
        const int x = GC_EXCISE_MAX_GUARD + q * P + s;
        if (n >= p.first && n < p.end && hot_below(w, pre, x + p.before + 1) - hot_below(w, pre, x - p.after) > 0) mask |= 1u << s;
      }
    }
    if (mine && (mask != 0u || !p.in_place)) {
      RecVec<MODE> d;
      d.load(p.src, n0 * F::bps, p.rec_bytes);
#pragma unroll
      for (int s = 0; s < P; ++s)
        if (mask >> s & 1u) d.zero(s);
      d.store(p.dst, n0 * F::bps, p.rec_bytes);
    }
    const unsigned long long word = join_word<P>(mask, lane);
    if ((lane & (64 / P - 1)) == 0) bl[(q * P) >> 6] = word;
  }
  __syncthreads();
  // the tile's summary: one word per thread, the lanes joined in order by shuffles, the waves by thread 0
  Runs r;
  {
    const unsigned long long x = bl[tid];
    r.len = 64;
    r.pre = ~x ? __ffsll((long long)~x) - 1 : 64;
    r.suf = ~x ? __clzll((long long)~x) : 64;
    int best = 0;
    for (unsigned long long y = x; y; y &= y << 1) ++best;
    r.best = best;
    r.runs = __popcll(x & ~(x << 1));
    r.blanked = __popcll(x);
    r.hot = __popcll(w[kExciseHalo + tid]);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    Runs b;
    b.len = __shfl_down(r.len, o, 64);
    b.pre = __shfl_down(r.pre, o, 64);
    b.suf = __shfl_down(r.suf, o, 64);
    b.best = __shfl_down(r.best, o, 64);
    b.runs = __shfl_down(r.runs, o, 64);
    b.blanked = __shfl_down(r.blanked, o, 64);
    b.hot = __shfl_down(r.hot, o, 64);
    r = join(r, b);  // lane 0 after the step: lanes 0 .. 2 o - 1 in order (the other lanes' values are not used)
  }
  if (lane == 0) wave_runs[wave] = r;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < kExciseWG / 64; ++i) r = join(r, wave_runs[i]);
    TileRuns t;
    t.pre = (int32_t)r.pre, t.suf = (int32_t)r.suf, t.best = (int32_t)r.best, t.runs = (int32_t)r.runs, t.blanked = (int32_t)r.blanked, t.hot = (int32_t)r.hot;
    p.tiles[blockIdx.x] = t;
  }
}

// The tiles' summaries in tile order: every thread joins a stretch of consecutive tiles, thread 0 the threads' results.
// out = {hot, blanked, runs, longest}
__global__ __launch_bounds__(kExciseWG) void excise_combine_kernel(const TileRuns* __restrict__ tiles, long long ntiles, long long* __restrict__ out) {
  __shared__ Runs part[kExciseWG];
  const int tid = (int)threadIdx.x;
  const long long per = (ntiles + kExciseWG - 1) / kExciseWG, lo = min(ntiles, tid * per), hi = min(ntiles, lo + per);
  Runs r = {0, 0, 0, 0, 0, 0, 0};  // no samples: join's identity
  for (long long t = lo; t < hi; ++t) {
    const TileRuns x = tiles[t];
    const Runs b = {kExciseTile, x.pre, x.suf, x.best, x.runs, x.blanked, x.hot};
    r = join(r, b);
  }
  part[tid] = r;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < kExciseWG; ++i) r = join(r, part[i]);
    out[0] = r.hot, out[1] = r.blanked, out[2] = r.runs, out[3] = r.best;
  }
}

// ---- gc_excise_bins ------------------------------------------------------------------------------------------------------------------

// out[t][b] = gain[b] * in[t][storage position of bin b], b = k1 + n1 k2 at position k1 n2 + k2
__global__ __launch_bounds__(kExciseWG) void excise_gain_kernel(const float2* __restrict__ in, float2* __restrict__ out, const float* __restrict__ gain,
                                                                 int nfft, int n1, int n2, int blocks_per_row) {
  const long long t = blockIdx.x / (unsigned)blocks_per_row;
  const int b = (int)(blockIdx.x - (unsigned)(t * blocks_per_row)) * kExciseWG + (int)threadIdx.x;
  if (b >= nfft) return;
  const int k2 = b / n1, k1 = b - k2 * n1;
  const float2 x = in[t * nfft + k1 * n2 + k2];
  const float g = gain[b];
  out[t * nfft + b] = make_float2(g * x.x, g * x.y);
}

struct AddArgs {
  const float2* rows;   // the tile's inverse transforms, storage order: value n of a row at (n mod n1) n2 + n / n1
  const float2* carry;  // s v of the second half of segment g0 - 1 (g0 > 0)
  const float* scale;   // s[nfft]
  uint8_t* rec;         // the destination record (out of place: a copy of the source)
  float2* values;       // [nsamples] or null
  long long first, m0, m1;  // the range's first record sample; the range samples this tile finishes
  long long rec_bytes;      // of the record
  long long g0;
  int nfft, n1, n2;
};

__device__ __forceinline__ float2 scaled(const AddArgs& p, long long row, int n) {
  const int k2 = n / p.n1, k1 = n - k2 * p.n1;
  const float2 v = p.rows[row * p.nfft + k1 * p.n2 + k2];
  const float s = p.scale[n];
  return make_float2(s * v.x, s * v.y);
}

template <int MODE>
__global__ __launch_bounds__(kExciseWG) void excise_add_kernel(const AddArgs p, long long v0, long long nvec) {
  using F = Fmt<MODE>;
  constexpr int P = F::per16;
  const long long i = (long long)blockIdx.x * kExciseWG + threadIdx.x;
  if (i >= nvec) return;
  const long long n0 = (v0 + i) * P;
  RecVec<MODE> d;
  d.load(p.rec, n0 * F::bps, p.rec_bytes);
  const int H = p.nfft / 2;
#pragma unroll
  for (int s = 0; s < P; ++s) {
    const long long m = n0 + s - p.first;
    if (m < p.m0 || m >= p.m1) continue;  // another tile's, or outside the range: the bytes stay
    const long long k0 = m / H;
    const int r = (int)(m - k0 * H);
    const float2 lo = k0 >= p.g0 ? scaled(p, k0 - p.g0, H + r) : p.carry[r];
    const float2 hi = scaled(p, k0 + 1 - p.g0, r);
    const float y_re = lo.x + hi.x, y_im = lo.y + hi.y;
    if (p.values) p.values[m] = make_float2(y_re, y_im);
    d.put(s, quantise<MODE>(y_re), quantise<MODE>(y_im));
  }
  d.store(p.rec, n0 * F::bps, p.rec_bytes);
}

// carry[r] = s[H + r] * v[H + r] of row `row`
__global__ __launch_bounds__(kExciseWG) void excise_carry_kernel(const AddArgs p, long long row, float2* __restrict__ carry) {
  const int H = p.nfft / 2, r = (int)(blockIdx.x * kExciseWG + threadIdx.x);
  if (r < H) carry[r] = scaled(p, row, H + r);
}

}  // namespace

void gc_excise_free(gc_context* ctx) {
  ExciseState* s = static_cast<ExciseState*>(ctx->excise);
  if (!s) return;
  for (GcBuf* b : {&s->bitmap, &s->tiles, &s->stats, &s->tw, &s->win, &s->gain, &s->rows_a, &s->rows_b, &s->carry, &s->values}) gc_buf_free(*b);
  delete s;
  ctx->excise = nullptr;
}

extern "C" int gc_excise_pulses(gc_context* src, gc_context* dst, const gc_excise_pulse_params* p, gc_excise_pulse_stats* stats) {
  ExcisePulsePlan pl;
  const int rc = excise_check_pulses(src, dst, p, &pl);
  if (rc) return rc;
  if (pl.ntiles > 0x7fffffffLL) {
    gc_set_error("gc_excise_pulses: %lld tiles in one call", pl.ntiles);
    return GC_E_INVALID;
  }
  // nothing has been written up to here
  GC_HIP(hipSetDevice(src->device));
  if (dst != src) GC_HIP(hipStreamSynchronize(dst->stream));  // the destination's own pending work comes first
  ExciseState* s = gc_unit_state<ExciseState>(src->excise);
  if (!s) return gc_nomem("gc_excise_pulses");
  if (gc_buf_reserve(s->bitmap, (size_t)pl.words * sizeof(unsigned long long), false) != hipSuccess ||
      gc_buf_reserve(s->tiles, (size_t)pl.ntiles * sizeof(TileRuns), false) != hipSuccess ||
      gc_buf_reserve(s->stats, 4 * sizeof(long long), false) != hipSuccess)
    return gc_nomem("gc_excise_pulses");
  const long long first = (long long)p->first_sample, end = first + (long long)p->nsamples;
  unsigned long long* const bitmap = (unsigned long long*)s->bitmap.p;
  const size_t back = (size_t)kExciseHalo + (size_t)pl.ntiles * kExciseTileWords;  // the mark kernel writes every word in between
  GC_HIP(hipMemsetAsync(bitmap, 0, (size_t)kExciseHalo * sizeof(unsigned long long), src->stream));
  GC_HIP(hipMemsetAsync(bitmap + back, 0, (size_t)(kExciseHalo + 1) * sizeof(unsigned long long), src->stream));
  const bool in_place = dst->d_if == src->d_if;
  if (!in_place) {  // the record outside the range is copied; the blank kernel writes every 16 bytes that hold a sample of the range
    const size_t head = (size_t)first * (size_t)pl.bps, tail0 = (size_t)end * (size_t)pl.bps, bytes = (size_t)src->if_nsamples * (size_t)pl.bps;
    if (head) GC_HIP(hipMemcpyAsync(dst->d_if, src->d_if, head, hipMemcpyDeviceToDevice, src->stream));
    if (bytes > tail0) GC_HIP(hipMemcpyAsync(dst->d_if + tail0, src->d_if + tail0, bytes - tail0, hipMemcpyDeviceToDevice, src->stream));
  }
  ExciseArgs a;
  a.src = src->d_if;
  a.dst = dst->d_if;
  a.bitmap = bitmap;
  a.tiles = (TileRuns*)s->tiles.p;
  a.base = pl.base;
  a.first = first;
  a.end = end;
  a.rec_bytes = (long long)src->if_nsamples * pl.bps;
  a.threshold2 = (long long)p->threshold2;
  a.before = p->before;
  a.after = p->after;
  a.in_place = in_place ? 1 : 0;
  gc_with_mode(gc_record_mode(src), [&](auto m) {
    hipLaunchKernelGGL(excise_mark_kernel<decltype(m)::value>, dim3((unsigned int)pl.ntiles), dim3(kExciseWG), 0, src->stream, a);
    hipLaunchKernelGGL(excise_blank_kernel<decltype(m)::value>, dim3((unsigned int)pl.ntiles), dim3(kExciseWG), 0, src->stream, a);
  });
  GC_HIP(hipGetLastError());
  hipLaunchKernelGGL(excise_combine_kernel, dim3(1), dim3(kExciseWG), 0, src->stream, (const TileRuns*)s->tiles.p, pl.ntiles, (long long*)s->stats.p);
  GC_HIP(hipGetLastError());
  long long host[4];
  GC_HIP(hipMemcpyAsync(host, s->stats.p, sizeof host, hipMemcpyDeviceToHost, src->stream));
  GC_HIP(hipStreamSynchronize(src->stream));
  if (stats) {
    stats->hot = host[0];
    stats->blanked = host[1];
    stats->runs = host[2];
    stats->longest = host[3];
  }
  return GC_OK;
}

extern "C" long long gc_debug_excise_tile_segments(int nfft) { return nfft < 4 ? 0 : excise_tile_segments(nfft, ExciseBudget()); }

extern "C" int gc_excise_bins(gc_context* src, gc_context* dst, const gc_excise_bins_params* p, const float* gain, float* values) {
  int rc = excise_check_bins(src, dst, p, gain);
  if (rc) return rc;
  gcacq::Plan plan;
  rc = gcacq::plan_or_refuse(p->nfft, &plan);
  if (rc) return rc;
  ExciseBinsPlan pl;
  rc = excise_check_bins_state(src, dst, p, ExciseBudget(), &pl);
  if (rc) return rc;
  const int nfft = p->nfft, H = nfft / 2;
  const long long first = (long long)p->first_sample, nsamples = (long long)p->nsamples;
  // nothing has been written up to here
  GC_HIP(hipSetDevice(src->device));
  if (dst != src) GC_HIP(hipStreamSynchronize(dst->stream));  // the destination's own pending work comes first
  ExciseState* s = gc_unit_state<ExciseState>(src->excise);
  if (!s) return gc_nomem("gc_excise_bins");
  const size_t rows_bytes = (size_t)std::min(pl.tile, pl.K) * (size_t)nfft * sizeof(float2);
  if (gc_buf_reserve(s->rows_a, rows_bytes, false) != hipSuccess || gc_buf_reserve(s->rows_b, rows_bytes, false) != hipSuccess ||
      gc_buf_reserve(s->gain, (size_t)nfft * sizeof(float), false) != hipSuccess || gc_buf_reserve(s->carry, (size_t)H * sizeof(float2), false) != hipSuccess ||
      (values && gc_buf_reserve(s->values, (size_t)nsamples * sizeof(float2), false) != hipSuccess))
    return gc_nomem("gc_excise_bins");
  if (s->n != nfft) {  // the plan, the twiddle table, the window w and the scale s of an nfft-point excision
    s->n = 0;
    if (gc_buf_reserve(s->tw, (size_t)nfft * sizeof(float2), false) != hipSuccess || gc_buf_reserve(s->win, 2 * (size_t)nfft * sizeof(float), false) != hipSuccess)
      return gc_nomem("gc_excise_bins");
    const double pi = 3.14159265358979323846;
    std::vector<float> win(2 * (size_t)nfft);
    for (int k = 0; k < nfft; ++k) {
      const float w = (float)std::sin(pi * ((double)k + 0.5) / (double)nfft);
      win[(size_t)k] = w;
      win[(size_t)nfft + (size_t)k] = (float)((double)w / (double)nfft);
    }
    GC_HIP(hipMemcpyAsync(s->win.p, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice, src->stream));
    rc = gcacq::upload_twiddles(src, nfft, (float2*)s->tw.p);  // waits for the stream: win is gone below
    if (rc) return rc;
    s->plan = plan;
    s->n = nfft;
  }
  GC_HIP(hipMemcpyAsync(s->gain.p, gain, (size_t)nfft * sizeof(float), hipMemcpyHostToDevice, src->stream));
  const int bps = gc_record_bps(src);
  if (dst->d_if != src->d_if)  // out of place: the add kernel works on a copy
    GC_HIP(hipMemcpyAsync(dst->d_if, src->d_if, (size_t)src->if_nsamples * (size_t)bps, hipMemcpyDeviceToDevice, src->stream));
  const int bpr = (nfft + kExciseWG - 1) / kExciseWG, per16 = 16 / bps;
  float2 *const rows_a = (float2*)s->rows_a.p, *const rows_b = (float2*)s->rows_b.p;
  const float* const win = (const float*)s->win.p;
  AddArgs a;
  a.rows = rows_b;
  a.carry = (const float2*)s->carry.p;
  a.scale = win + nfft;
  a.rec = dst->d_if;
  a.values = values ? (float2*)s->values.p : nullptr;
  a.first = first;
  a.rec_bytes = (long long)src->if_nsamples * bps;
  a.nfft = nfft;
  a.n1 = plan.n1;
  a.n2 = plan.n2;
  const gcacq::RowGather segs = {first, nsamples, H, pl.K, H};  // segment k covers the range samples [(k - 1) H, (k + 1) H): one span of K segments
  for (ExciseTile t; excise_next_tile(pl, t);) {
    const dim3 grid((unsigned int)(t.n * bpr)), wg(kExciseWG);
    // the gather reads the SOURCE: in place its samples are this tile's and later ones', which no add kernel has written yet
    rc = gcacq::gather_rows(src, segs, t.g0, t.n, nfft, win, rows_a);
    if (rc) return rc;
    rc = gcacq::transform_rows(src, s->plan, (const float2*)s->tw.p, rows_a, rows_b, t.n, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(excise_gain_kernel, grid, wg, 0, src->stream, (const float2*)rows_a, rows_b, (const float*)s->gain.p, nfft, plan.n1, plan.n2, bpr);
    GC_HIP(hipGetLastError());
    rc = gcacq::transform_rows(src, s->plan, (const float2*)s->tw.p, rows_b, rows_a, t.n, 1);
    if (rc) return rc;
    a.g0 = t.g0;
    a.m0 = t.m0;
    a.m1 = t.m1;
    if (t.m0 < t.m1) {
      const long long v0 = (first + t.m0) / per16, v1 = (first + t.m1 + per16 - 1) / per16;
      const unsigned int wgs = (unsigned int)((v1 - v0 + kExciseWG - 1) / kExciseWG);
      gc_with_mode(gc_record_mode(src), [&](auto m) {
        hipLaunchKernelGGL(excise_add_kernel<decltype(m)::value>, dim3(wgs), wg, 0, src->stream, a, v0, v1 - v0);
      });
      GC_HIP(hipGetLastError());
    }
    if (t.g0 + t.n < pl.K) {
      hipLaunchKernelGGL(excise_carry_kernel, dim3((unsigned int)((H + kExciseWG - 1) / kExciseWG)), wg, 0, src->stream, a, t.n - 1, (float2*)s->carry.p);
      GC_HIP(hipGetLastError());
    }
  }
  if (values) GC_HIP(hipMemcpyAsync(values, s->values.p, (size_t)nsamples * sizeof(float2), hipMemcpyDeviceToHost, src->stream));
  GC_HIP(hipStreamSynchronize(src->stream));
  return GC_OK;
}
