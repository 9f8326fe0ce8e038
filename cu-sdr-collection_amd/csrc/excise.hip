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
// float32 transform.  The segment list is cut into tiles (seg_fft.h, shared with the probe: budget, walk, rows and transform state;
// excise_plan.h: the samples a tile finishes); per tile
//   gather_rows            converts and windows the tile's segments into float2 rows, zero outside the range (seg_fft.hip),
//   transform_rows         forward: the pass pair the probe runs (seg_fft.hip),
//   excise_gain_kernel     multiplies by the gain and moves every value from its storage position to its natural bin (fft_plan.h),
//                          where the inverse pair expects it,
//   transform_rows         inverse = 1,
//   excise_add_kernel      one thread per 16 bytes of record: y = s v of the earlier segment's second half + s v of the later
//                          segment's first half, quantised into a RecVec; y itself to a float2 buffer of the range when the caller
//                          asks for it,
//   excise_carry_kernel    keeps s v of the second half of the tile's last segment for the next tile: its samples are not gathered
//                          again after they were overwritten (in place), and a sample's value is the same sum wherever the cut falls.
// Out of place the record is copied first and the add kernel works on the copy.
//
// gc_excise_sweep: the same overlap-add (one driver, excise_overlap_add) with a decision per cell (segment, bin) in the gain kernel's place:
//   excise_sweep_mark_kernel      one lane per bin in natural order: P = re^2 + im^2 of X, P > limit[b]; a wave's ballot is one word of
//                                 the segment's hot row, written by one lane; P itself to the tile's power rows when asked for,
//   excise_sweep_apply_kernel     one lane per bin: cut iff a hot bit lies within `widen` bins around the circle (at most three words of
//                                 the hot row); the ballot is a word of the cut row; Y = 0 where cut, else gain * X, in natural order,
//   excise_sweep_segments_kernel  one thread per segment: the popcounts of its two rows; hot cells, cut cells, segments with a cut cell
//                                 and the most cut cells of one segment by 64-bit integer atomics,
//   excise_sweep_bins_kernel      bin_cut: a wave walks a stretch of one word column of the cut rows, lane b counting bit b.
// The tile's mask rows and power go to the caller's [K] arrays at row g0 after each tile.  No float atomics: the counts are exact.
// The unit's buffers are its own (ExciseState, kept in gc_context::excise, grow-only, released by gc_destroy).
#include <algorithm>
#include <cmath>

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
  gcacq::SegFft fft;           // gc_excise_bins: fft.n is also the length that win holds
  GcBuf win, gain, carry, values;  // win: w[nfft] then s[nfft]
  GcBuf limit, hot, cut, power, counts;                // gc_excise_sweep: a tile's mask rows and power; the four sums, then bin_cut
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

// out[t][b] = gain[b] * in[t][storage position of bin b]
__global__ __launch_bounds__(kExciseWG) void excise_gain_kernel(const float2* __restrict__ in, float2* __restrict__ out, const float* __restrict__ gain,
                                                                 int nfft, int n1, int n2, int blocks_per_row) {
  const auto [t, b] = gcacq::row_element<kExciseWG>(blocks_per_row);
  if (b >= nfft) return;
  const float2 x = in[t * nfft + gcacq::fft_pos_of(b, n1, n2)];
  const float g = gain[b];
  out[t * nfft + b] = make_float2(g * x.x, g * x.y);
}

// ---- gc_excise_sweep: the gain kernel's place taken by a decision per cell ----------------------------------------------------------------

constexpr int kSweepRows = 128;  // mask rows a wave of excise_sweep_bins_kernel walks

struct SweepArgs {
  const float2* x;                // the tile's forward transforms, storage order
  float2* y;                      // what the inverse pair reads: natural bin order
  const float* limit;             // [nfft]
  const float* gain;              // [nfft] or null: a gain of ones
  unsigned long long *hot, *cut;  // the tile's mask rows, [rows][W]
  float* power;                   // the tile's [rows][nfft] or null
  int nfft, n1, n2, blocks_per_row, W, widen;
};

// One lane per bin, in natural order: P and the comparison; a wave's ballot is one word of the segment's hot row.  The lanes from
// nfft on vote 0, so the last word's upper bits are 0.
__global__ __launch_bounds__(kExciseWG) void excise_sweep_mark_kernel(const SweepArgs p) {
  const auto [t, b] = gcacq::row_element<kExciseWG>(p.blocks_per_row);
  bool hot = false;
  if (b < p.nfft) {
    const float2 x = p.x[t * p.nfft + gcacq::fft_pos_of(b, p.n1, p.n2)];
    const float pw = __fadd_rn(__fmul_rn(x.x, x.x), __fmul_rn(x.y, x.y));  // two products and a sum, each rounded by itself
    hot = pw > p.limit[b];
    if (p.power) p.power[t * p.nfft + b] = pw;
  }
  const unsigned long long word = __ballot(hot);
  if ((threadIdx.x & 63) == 0 && (b >> 6) < p.W) p.hot[t * p.W + (b >> 6)] = word;
}

// a hot bit among the bins lo .. hi of a row, 0 <= lo <= hi < nfft: at most three words where hi - lo <= 2 GC_EXCISE_MAX_WIDEN
__device__ __forceinline__ bool any_hot(const unsigned long long* __restrict__ row, int lo, int hi) {
  unsigned long long any = 0ull;
  for (int j = lo >> 6; j <= hi >> 6; ++j) {
    unsigned long long m = ~0ull;
    if (j == lo >> 6) m &= ~0ull << (lo & 63);
    if (j == hi >> 6) m &= ~0ull >> (63 - (hi & 63));
    any |= row[j] & m;
  }
  return any != 0ull;
}

// One lane per bin: cut iff a hot bin lies within `widen` of it around the circle of nfft bins (the bits are addressed by bin number,
// so an nfft that is no multiple of 64 wraps where it should); Y = 0 where cut, else gain * X, moved as excise_gain_kernel moves it.
__global__ __launch_bounds__(kExciseWG) void excise_sweep_apply_kernel(const SweepArgs p) {
  const auto [t, b] = gcacq::row_element<kExciseWG>(p.blocks_per_row);
  bool cut = false;
  if (b < p.nfft) {
    const unsigned long long* const row = p.hot + t * p.W;
    const int lo = b - p.widen, hi = b + p.widen, last = p.nfft - 1;
    if (2 * p.widen + 1 >= p.nfft) cut = any_hot(row, 0, last);  // every bin is within widen of every other
    else if (lo < 0) cut = any_hot(row, lo + p.nfft, last) || any_hot(row, 0, hi);
    else if (hi > last) cut = any_hot(row, lo, last) || any_hot(row, 0, hi - p.nfft);
    else cut = any_hot(row, lo, hi);
    float2 y = make_float2(0.0f, 0.0f);
    if (!cut) {
      y = p.x[t * p.nfft + gcacq::fft_pos_of(b, p.n1, p.n2)];
      if (p.gain) {
        const float g = p.gain[b];
        y = make_float2(g * y.x, g * y.y);
      }
    }
    p.y[t * p.nfft + b] = y;
  }
  const unsigned long long word = __ballot(cut);
  if ((threadIdx.x & 63) == 0 && (b >> 6) < p.W) p.cut[t * p.W + (b >> 6)] = word;
}

// The counts, integers throughout.  acc = {hot cells, cut cells, segments with a cut cell, most cut cells of one segment}, then
// bin_cut[nfft].  One thread per segment of the tile: the popcounts of its two rows, the waves' sums and maximum by integer atomics.
__global__ __launch_bounds__(kExciseWG) void excise_sweep_segments_kernel(const unsigned long long* __restrict__ hot, const unsigned long long* __restrict__ cut,
                                                                           long long rows, int W, unsigned long long* __restrict__ acc) {
  const long long k = (long long)blockIdx.x * kExciseWG + threadIdx.x;
  int h = 0, c = 0;
  if (k < rows)
    for (int j = 0; j < W; ++j) {
      h += __popcll(hot[k * W + j]);
      c += __popcll(cut[k * W + j]);
    }
  long long hs = h, cs = c;
  int any = c > 0 ? 1 : 0, most = c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hs += __shfl_down(hs, o, 64);
    cs += __shfl_down(cs, o, 64);
    any += __shfl_down(any, o, 64);
    most = max(most, __shfl_down(most, o, 64));
  }
  if ((threadIdx.x & 63) == 0 && cs > 0) {  // no cut cell: no hot one either
    atomicAdd(acc + 0, (unsigned long long)hs);
    atomicAdd(acc + 1, (unsigned long long)cs);
    atomicAdd(acc + 2, (unsigned long long)any);
    atomicMax(acc + 3, (unsigned long long)most);
  }
}

// bin_cut: workgroup (stretch, word) walks 4 kSweepRows rows of one word column, lane b adding bit b; one atomic per bin and workgroup
__global__ __launch_bounds__(kExciseWG) void excise_sweep_bins_kernel(const unsigned long long* __restrict__ cut, long long rows, int W, int nfft,
                                                                       unsigned long long* __restrict__ bin_cut) {
  __shared__ unsigned int part[kExciseWG / 64][64];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const long long stretch = blockIdx.x / (unsigned)W;
  const int w = (int)(blockIdx.x - (unsigned)(stretch * W));
  const long long k0 = (stretch * (kExciseWG / 64) + wave) * kSweepRows, k1 = min(rows, k0 + kSweepRows);
  unsigned int n = 0u;
  for (long long k = k0; k < k1; ++k) n += (unsigned int)(cut[k * W + w] >> lane) & 1u;
  part[wave][lane] = n;
  __syncthreads();
  if (wave == 0) {
    for (int i = 1; i < kExciseWG / 64; ++i) n += part[i][lane];
    const int b = w * 64 + lane;
    if (b < nfft && n > 0u) atomicAdd(bin_cut + b, (unsigned long long)n);
  }
}

struct AddArgs {
  const float2* rows;   // the tile's inverse transforms, storage order (fft_plan.h)
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
  const float2 v = p.rows[row * p.nfft + gcacq::fft_pos_of(n, p.n1, p.n2)];
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
  gcacq::seg_fft_free(&s->fft);
  for (GcBuf* b : {&s->bitmap, &s->tiles, &s->stats, &s->win, &s->gain, &s->carry, &s->values, &s->limit, &s->hot, &s->cut, &s->power, &s->counts})
    gc_buf_free(*b);
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

namespace {

struct Sweep {  // what gc_excise_sweep puts where gc_excise_bins has its gain kernel
  const float* limit;
  int widen;
  const gc_excise_sweep_out* out;  // never null (its members may be)
  gc_excise_sweep_stats* stats;    // may be null
  ExciseSweepPlan pl;
};

// The overlap-add of both calls, after their checks: nothing has been written when it begins.  gain: [nfft] on the host, or null
// (gc_excise_sweep's gain of ones); sw: null for gc_excise_bins.
int excise_overlap_add(const char* who, gc_context* src, gc_context* dst, long long first, long long nsamples, int nfft, const gcacq::Plan& plan,
                       const ExciseBinsPlan& pl, const float* gain, float* values, const Sweep* sw) {
  const int H = nfft / 2;
  int rc;
  GC_HIP(hipSetDevice(src->device));
  if (dst != src) GC_HIP(hipStreamSynchronize(dst->stream));  // the destination's own pending work comes first
  ExciseState* s = gc_unit_state<ExciseState>(src->excise);
  if (!s) return gc_nomem(who);
  const size_t tile_rows = (size_t)std::min(pl.tile, pl.K);
  if (gc_buf_reserve(s->gain, (size_t)nfft * sizeof(float), false) != hipSuccess || gc_buf_reserve(s->carry, (size_t)H * sizeof(float2), false) != hipSuccess ||
      (values && gc_buf_reserve(s->values, (size_t)nsamples * sizeof(float2), false) != hipSuccess))
    return gc_nomem(who);
  const size_t counts_bytes = (4 + (size_t)nfft) * sizeof(unsigned long long);  // the four sums, then bin_cut
  if (sw) {
    const size_t mask_bytes = tile_rows * (size_t)sw->pl.W * sizeof(unsigned long long);
    if (gc_buf_reserve(s->limit, (size_t)nfft * sizeof(float), false) != hipSuccess || gc_buf_reserve(s->hot, mask_bytes, false) != hipSuccess ||
        gc_buf_reserve(s->cut, mask_bytes, false) != hipSuccess || gc_buf_reserve(s->counts, counts_bytes, false) != hipSuccess ||
        (sw->out->power && gc_buf_reserve(s->power, tile_rows * (size_t)nfft * sizeof(float), false) != hipSuccess))
      return gc_nomem(who);
  }
  std::vector<float> host_win;
  if (s->fft.n != nfft) {  // the window w and the scale s of an nfft-point excision, queued in front of the plan's twiddle table
    s->fft.n = 0;
    if (gc_buf_reserve(s->win, 2 * (size_t)nfft * sizeof(float), false) != hipSuccess) return gc_nomem(who);
    const double pi = 3.14159265358979323846;
    host_win.resize(2 * (size_t)nfft);
    for (int k = 0; k < nfft; ++k) {
      const float w = (float)std::sin(pi * ((double)k + 0.5) / (double)nfft);
      host_win[(size_t)k] = w;
      host_win[(size_t)nfft + (size_t)k] = (float)((double)w / (double)nfft);
    }
    GC_HIP(hipMemcpyAsync(s->win.p, host_win.data(), host_win.size() * sizeof(float), hipMemcpyHostToDevice, src->stream));
  }
  rc = gcacq::seg_fft_prepare(src, &s->fft, plan, (long long)tile_rows, who);  // a new length: waits for the stream, host_win may go
  if (rc && !host_win.empty()) (void)hipStreamSynchronize(src->stream);
  if (rc) return rc;
  if (gain) GC_HIP(hipMemcpyAsync(s->gain.p, gain, (size_t)nfft * sizeof(float), hipMemcpyHostToDevice, src->stream));
  if (sw) {
    GC_HIP(hipMemcpyAsync(s->limit.p, sw->limit, (size_t)nfft * sizeof(float), hipMemcpyHostToDevice, src->stream));
    GC_HIP(hipMemsetAsync(s->counts.p, 0, counts_bytes, src->stream));
  }
  const int bps = gc_record_bps(src);
  if (dst->d_if != src->d_if)  // out of place: the add kernel works on a copy
    GC_HIP(hipMemcpyAsync(dst->d_if, src->d_if, (size_t)src->if_nsamples * (size_t)bps, hipMemcpyDeviceToDevice, src->stream));
  const int bpr = (nfft + kExciseWG - 1) / kExciseWG, per16 = 16 / bps;
  float2 *const rows_a = (float2*)s->fft.rows_a.p, *const rows_b = (float2*)s->fft.rows_b.p;
  const float2* const tw = (const float2*)s->fft.tw.p;
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
  SweepArgs m = {};
  if (sw) {
    m.x = rows_a;
    m.y = rows_b;
    m.limit = (const float*)s->limit.p;
    m.gain = gain ? (const float*)s->gain.p : nullptr;
    m.hot = (unsigned long long*)s->hot.p;
    m.cut = (unsigned long long*)s->cut.p;
    m.power = sw->out->power ? (float*)s->power.p : nullptr;
    m.nfft = nfft, m.n1 = plan.n1, m.n2 = plan.n2, m.blocks_per_row = bpr, m.W = (int)sw->pl.W, m.widen = sw->widen;
  }
  unsigned long long* const counts = (unsigned long long*)s->counts.p;
  const gcacq::RowGather segs = {first, nsamples, H, pl.K, H};  // segment k covers the range samples [(k - 1) H, (k + 1) H): one span of K segments
  for (ExciseTile t; excise_next_tile(pl, t);) {
    const dim3 grid((unsigned int)(t.n * bpr)), wg(kExciseWG);
    // the gather reads the SOURCE: in place its samples are this tile's and later ones', which no add kernel has written yet
    rc = gcacq::gather_rows(src, segs, t.g0, t.n, nfft, win, rows_a);
    if (rc) return rc;
    rc = gcacq::transform_rows(src, s->fft.plan, tw, rows_a, rows_b, t.n, 0);
    if (rc) return rc;
    if (!sw) {
      hipLaunchKernelGGL(excise_gain_kernel, grid, wg, 0, src->stream, (const float2*)rows_a, rows_b, (const float*)s->gain.p, nfft, plan.n1, plan.n2, bpr);
      GC_HIP(hipGetLastError());
    } else {
      hipLaunchKernelGGL(excise_sweep_mark_kernel, grid, wg, 0, src->stream, m);
      hipLaunchKernelGGL(excise_sweep_apply_kernel, grid, wg, 0, src->stream, m);
      GC_HIP(hipGetLastError());
      const long long stretches = (t.n + (kExciseWG / 64) * kSweepRows - 1) / ((kExciseWG / 64) * kSweepRows);
      hipLaunchKernelGGL(excise_sweep_segments_kernel, dim3((unsigned int)((t.n + kExciseWG - 1) / kExciseWG)), wg, 0, src->stream,
                         (const unsigned long long*)m.hot, (const unsigned long long*)m.cut, t.n, m.W, counts);
      hipLaunchKernelGGL(excise_sweep_bins_kernel, dim3((unsigned int)(stretches * m.W)), wg, 0, src->stream, (const unsigned long long*)m.cut, t.n, m.W,
                         nfft, counts + 4);
      GC_HIP(hipGetLastError());
      // the tile's rows of the [K] arrays: row g0 on (excise_plan.h); the next tile's kernels follow the copies on the stream
      const size_t mask_bytes = (size_t)t.n * (size_t)m.W * sizeof(unsigned long long);
      if (sw->out->hot) GC_HIP(hipMemcpyAsync(sw->out->hot + excise_mask_offset(sw->pl, t), m.hot, mask_bytes, hipMemcpyDeviceToHost, src->stream));
      if (sw->out->cut) GC_HIP(hipMemcpyAsync(sw->out->cut + excise_mask_offset(sw->pl, t), m.cut, mask_bytes, hipMemcpyDeviceToHost, src->stream));
      if (m.power)
        GC_HIP(hipMemcpyAsync(sw->out->power + excise_power_offset(sw->pl, t), m.power, (size_t)t.n * (size_t)nfft * sizeof(float), hipMemcpyDeviceToHost, src->stream));
    }
    rc = gcacq::transform_rows(src, s->fft.plan, tw, rows_b, rows_a, t.n, 1);
    if (rc) return rc;
    a.g0 = t.g0;
    a.m0 = t.m0;
    a.m1 = t.m1;
    if (t.m0 < t.m1) {
      const long long v0 = (first + t.m0) / per16, v1 = (first + t.m1 + per16 - 1) / per16;
      const unsigned int wgs = (unsigned int)((v1 - v0 + kExciseWG - 1) / kExciseWG);
      gc_with_mode(gc_record_mode(src), [&](auto mode) {
        hipLaunchKernelGGL(excise_add_kernel<decltype(mode)::value>, dim3(wgs), wg, 0, src->stream, a, v0, v1 - v0);
      });
      GC_HIP(hipGetLastError());
    }
    if (t.g0 + t.n < pl.K) {
      hipLaunchKernelGGL(excise_carry_kernel, dim3((unsigned int)((H + kExciseWG - 1) / kExciseWG)), wg, 0, src->stream, a, t.n - 1, (float2*)s->carry.p);
      GC_HIP(hipGetLastError());
    }
  }
  if (values) GC_HIP(hipMemcpyAsync(values, s->values.p, (size_t)nsamples * sizeof(float2), hipMemcpyDeviceToHost, src->stream));
  std::vector<unsigned long long> host;
  if (sw) {
    host.resize(4 + (size_t)nfft);
    GC_HIP(hipMemcpyAsync(host.data(), counts, counts_bytes, hipMemcpyDeviceToHost, src->stream));
  }
  GC_HIP(hipStreamSynchronize(src->stream));
  if (sw) {
    if (sw->stats) {
      sw->stats->segments = (int64_t)pl.K;
      sw->stats->hot = (int64_t)host[0];
      sw->stats->cut = (int64_t)host[1];
      sw->stats->segments_cut = (int64_t)host[2];
      sw->stats->most_cut = (int64_t)host[3];
    }
    if (sw->out->bin_cut)
      for (int b = 0; b < nfft; ++b) sw->out->bin_cut[b] = (int64_t)host[4 + (size_t)b];
  }
  return GC_OK;
}

}  // namespace

extern "C" int gc_excise_bins(gc_context* src, gc_context* dst, const gc_excise_bins_params* p, const float* gain, float* values) {
  int rc = excise_check_bins(src, dst, p, gain);
  if (rc) return rc;
  gcacq::Plan plan;
  rc = gcacq::plan_or_refuse(p->nfft, &plan);
  if (rc) return rc;
  ExciseBinsPlan pl;
  rc = excise_check_bins_state(src, dst, p, ExciseBudget(), &pl);
  if (rc) return rc;
  // nothing has been written up to here
  return excise_overlap_add("gc_excise_bins", src, dst, (long long)p->first_sample, (long long)p->nsamples, p->nfft, plan, pl, gain, values, nullptr);
}

extern "C" int gc_excise_sweep(gc_context* src, gc_context* dst, const gc_excise_sweep_params* p, const float* limit, const float* gain,
                               const gc_excise_sweep_out* out, gc_excise_sweep_stats* stats) {
  int rc = excise_check_sweep(src, dst, p, limit, gain);
  if (rc) return rc;
  gcacq::Plan plan;
  rc = gcacq::plan_or_refuse(p->nfft, &plan);
  if (rc) return rc;
  const gc_excise_sweep_out none = {nullptr, nullptr, nullptr, nullptr, nullptr};
  Sweep sw = {limit, p->widen, out ? out : &none, stats, ExciseSweepPlan()};
  rc = excise_check_sweep_state(src, dst, p, ExciseBudget(), &sw.pl);
  if (rc) return rc;
  // nothing has been written up to here
  return excise_overlap_add("gc_excise_sweep", src, dst, (long long)p->first_sample, (long long)p->nsamples, p->nfft, plan, sw.pl.seg, gain,
                            sw.out->values, &sw);
}

