// array.hip — gc_array_covariance, gc_array_combine: the two halves of antenna-array null steering that run over every sample
// (include/gnsscorr.h has the definitions).  The covariance is exact in integers; the combine is float64, every operation rounded by
// itself (the unit is compiled with -ffp-contract=off).
//
// Both kernels cut the range into tiles of consecutive samples (array_plan.h), one workgroup each, and stage the tile's span of all K
// records, with T - 1 (L - 1) samples of lead-in, as the records' own bytes into LDS: whole 16-byte vectors of each record from the
// vector that holds the span's first byte, each a RecVec load (record_fmt.h: zero in front of sample 0, byte by byte at a record's
// partial last vector).  Record a's span starts a * rec_bytes behind record 0's; a sample has the same offset in every span.
//
// array_cov_kernel    lanes own samples: a thread carries up to kArrChains of them, kArrWG apart.  One pass per (l, a): the thread
//                     reads x_a[n] once and x_b[n - l] for every b, and keeps the 2 K sums of the pass in registers (int32 for int8
//                     records - array_plan.h bounds it -, int64 for int16).  The 16 sums are then reduced over the wave by a
//                     butterfly that halves the values a lane holds with every step (17 shuffles, not 96), the waves' sums of the K
//                     passes of a lag meet in LDS, and one 64-bit integer atomic per output and workgroup adds them into one of
//                     kArrCovSlots copies, which the host adds.  Integer sums: the order changes nothing.
// array_combine_kernel  ddc_kernel's shape at D = 1 (ddc.hip): the K T weights as double2 in LDS, kArrChains independent add chains
//                     that share every broadcast weight read, a ascending and k ascending within it, then fir_common.h's per-output
//                     finish without the NCO and its hand-over of the two counters.
// The staging of a span and the read of a staged sample are fir_common.h's too; the tile and its span are fir_plan.h's at D = 1.
// The unit's buffers are its own (ArrState, kept in gc_context::arr of srcs[0], grow-only, released by gc_destroy).
#include "array_plan.h"
#include "fir_common.h"
#include "record_fmt.h"

using namespace gcorr;

namespace {

constexpr int kArrK = GC_ARRAY_MAX_RECORDS;

struct ArrState {  // grow-only device buffers of the context (released by gc_destroy)
  GcBuf weights, stats, cov;
};

struct ArrArgs {
  const uint8_t* src[kArrK];
  long long src_bytes[kArrK];    // of each record: samples * bytes per sample
  uint8_t* dst;                  // combine
  const double* weights;         // combine: [K][T][2]
  unsigned long long* out;       // covariance: [kArrCovSlots][L][K][K][2], workgroup b adds to copy b mod kArrCovSlots; combine: [kFirStatSlots]{clipped, sum_sq} (fir_common.h)
  long long first, n, dst_first;
  int nrecords, ntaps, tile;     // ntaps: T, or L
  int rec_bytes;                 // LDS bytes of one record's span
  int dst_mode;                  // gcorr::Mode of dst
};

// the K spans of the tile into `vecs`; returns the byte offset in the record of the first staged vector
template <int MODE>
__device__ __forceinline__ long long stage_spans(const ArrArgs& p, const FirTile& tile, uint4* vecs) {
  using F = Fmt<MODE>;
  const long long base16 = fir_stage_base(tile.n_lo, F::bps);
  const int nvec = (int)fir_stage_vecs(tile.n_lo, tile.n_hi, F::bps);  // <= (span * bps + 15 + 15 + 15) / 16: inside rec_bytes
  const int rec_vecs = p.rec_bytes / 16;
  for (int a = 0; a < p.nrecords; ++a) {
    const uint8_t* const rec = p.src[a];
    const long long nbytes = p.src_bytes[a];
    stage_span<MODE, kArrWG>(rec, nbytes, base16, nvec, vecs + a * rec_vecs);
  }
  return base16;
}

// The sums over the wave of v[0 .. 2 W): a step at lane distance d adds the pairs of lanes d apart, the lower lane going on with
// the lower half of the values and the upper lane with the upper half.  After the four halving steps (W = 8) a lane holds one value,
// after two more whole steps its sum over the wave: value ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 +
// ((lane >> 2) & 1), the same in the four lanes that differ in their low two bits.
template <typename Acc, int N>
__device__ __forceinline__ void halve(Acc (&v)[2 * kArrK], int lane, int dist) {
  const bool up = (lane & dist) != 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const Acc keep = up ? v[i + N] : v[i], send = up ? v[i] : v[i + N];
    v[i] = keep + __shfl_xor(send, dist, 64);
  }
}
template <typename Acc>
__device__ __forceinline__ Acc wave_sum16(Acc (&v)[2 * kArrK], int lane) {
  static_assert(kArrK == 8, "four halving steps take 16 values to one");
  halve<Acc, 8>(v, lane, 32);
  halve<Acc, 4>(v, lane, 16);
  halve<Acc, 2>(v, lane, 8);
  halve<Acc, 1>(v, lane, 4);
  Acc s = v[0];
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 1, 64);
  return s;
}
__device__ __forceinline__ int wave_sum16_index(int lane) { return ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1); }

template <int MODE>
__global__ __launch_bounds__(kArrWG) void array_cov_kernel(const ArrArgs p) {
  using F = Fmt<MODE>;
  using Acc = std::conditional_t<F::value_bytes == 1, int, long long>;  // array_plan.h: kArrCovI32Cap
  extern __shared__ uint4 arr_lds[];
  __shared__ long long wave_part[kArrWG / 64][kArrK][2 * kArrK];  // [wave][a][2 b + {re, im}] of one lag
  static_assert(sizeof(wave_part) == kArrStaticLds, "array_plan.h counts these bytes");
  const int tid = (int)threadIdx.x, lane = tid & 63, K = p.nrecords, L = p.ntaps;
  const uint8_t* const bytes = reinterpret_cast<const uint8_t*>(arr_lds);

  const FirTile tile = fir_tile(p.tile, (long long)blockIdx.x, p.first, p.n, 1, L);
  const int cnt = (int)tile.n;  // >= 1: the grid is ceil(n / tile)
  const long long base16 = stage_spans<MODE>(p, tile, arr_lds);
  __syncthreads();

  // sample j of this thread is tile sample tid + j kArrWG
  int off[kArrChains];
#pragma unroll
  for (int j = 0; j < kArrChains; ++j) off[j] = (int)((p.first + tile.m0 + tid + j * kArrWG) * F::bps - base16);
  unsigned long long* const slot = p.out + (size_t)(blockIdx.x % kArrCovSlots) * L * K * K * 2;

#pragma unroll 1
  for (int l = 0; l < L; ++l) {
#pragma unroll 1
    for (int a = 0; a < K; ++a) {
      Acc acc[2 * kArrK];
#pragma unroll
      for (int i = 0; i < 2 * kArrK; ++i) acc[i] = 0;
      const uint8_t* const span_a = bytes + a * p.rec_bytes;
#pragma unroll
      for (int j = 0; j < kArrChains; ++j) {
        if (tid + j * kArrWG >= cnt) continue;
        int ar, ai;
        staged_ints<MODE>(span_a, off[j], ar, ai);
        const int lagged = off[j] - l * F::bps;  // >= 0: the span starts L - 1 samples in front of the tile
#pragma unroll
        for (int b = 0; b < kArrK; ++b)
          if (b < K) {
            int br, bi;
            staged_ints<MODE>(bytes + b * p.rec_bytes, lagged, br, bi);
            acc[2 * b] += (Acc)ar * br + (Acc)ai * bi;
            acc[2 * b + 1] += (Acc)ai * br - (Acc)ar * bi;
          }
      }
      const Acc s = wave_sum16<Acc>(acc, lane);
      if ((lane & 3) == 0) wave_part[tid >> 6][a][wave_sum16_index(lane)] = (long long)s;
    }
    __syncthreads();
    for (int i = tid; i < K * 2 * K; i += kArrWG) {  // one integer atomic per output and workgroup, spread over kArrCovSlots copies
      const int a = i / (2 * K), c = i - a * 2 * K;
      long long s = 0;
#pragma unroll
      for (int w = 0; w < kArrWG / 64; ++w) s += wave_part[w][a][c];
      if (s) atomicAdd(&slot[((size_t)l * K + a) * K * 2 + c], (unsigned long long)s);
    }
    __syncthreads();
  }
}

template <int MODE>
__global__ __launch_bounds__(kArrWG) void array_combine_kernel(const ArrArgs p) {
  using F = Fmt<MODE>;
  extern __shared__ uint4 arr_lds[];
  const int tid = (int)threadIdx.x, K = p.nrecords, T = p.ntaps;
  double2* const wts = reinterpret_cast<double2*>(arr_lds);  // 16 K T bytes
  uint4* const vecs = arr_lds + K * T;
  const uint8_t* const bytes = reinterpret_cast<const uint8_t*>(vecs);

  const FirTile tile = fir_tile(p.tile, (long long)blockIdx.x, p.first, p.n, 1, T);
  const long long m0 = tile.m0;
  const int cnt = (int)tile.n;  // >= 1: the grid is ceil(noutputs / tile)
  const long long base16 = stage_spans<MODE>(p, tile, vecs);
  for (int k = tid; k < K * T; k += kArrWG) wts[k] = make_double2(p.weights[2 * k], p.weights[2 * k + 1]);
  __syncthreads();

  // output j of this thread is tile output tid + j kArrWG; one that the tile does not have computes output 0 again and stores nothing
  int off[kArrChains];
  double ar[kArrChains], ai[kArrChains];
#pragma unroll
  for (int j = 0; j < kArrChains; ++j) {
    const int q = tid + j * kArrWG;
    off[j] = (int)((p.first + m0 + (q < cnt ? q : 0)) * F::bps - base16);
    ar[j] = 0.0;
    ai[j] = 0.0;
  }
  const int chains = (cnt + kArrWG - 1) / kArrWG;  // uniform over the workgroup: the chains that hold an output at all
#pragma unroll 1
  for (int a = 0; a < K; ++a) {
    const uint8_t* const span = bytes + a * p.rec_bytes;
    const double2* const wa = wts + a * T;
#pragma unroll 1
    for (int k = 0; k < T; ++k) {
      const double2 g = wa[k];
#pragma unroll
      for (int j = 0; j < kArrChains; ++j)
        if (j < chains) {
          double xr, xi;
          staged_sample<MODE>(span, off[j] - k * F::bps, xr, xi);
          const double pr = g.x * xr - g.y * xi;
          const double pi = g.x * xi + g.y * xr;
          ar[j] = ar[j] + pr;
          ai[j] = ai[j] + pi;
        }
    }
  }

  unsigned long long clipped = 0ull, sum_sq = 0ull;
#pragma unroll
  for (int j = 0; j < kArrChains; ++j) {
    const int q = tid + j * kArrWG;
    if (q >= cnt) continue;
    fir_finish<false>(ar[j], ai[j], 0ull, p.dst_mode, p.dst, p.dst_first + m0 + q, clipped, sum_sq);
  }
  fir_hand_over<kArrWG / 64>(clipped, sum_sq, p.out);
}

// what both drivers do after an accepted check: the device, the other streams' pending work, the records into the arguments
int arr_begin(gc_context* const* srcs, gc_context* dst, int K, const ArrPlan& pl, ArrArgs* a) {
  gc_context* const s0 = srcs[0];
  GC_HIP(hipSetDevice(s0->device));
  for (int i = 1; i < K; ++i)
    if (srcs[i]->stream != s0->stream) GC_HIP(hipStreamSynchronize(srcs[i]->stream));
  if (dst && dst->stream != s0->stream) GC_HIP(hipStreamSynchronize(dst->stream));
  for (int i = 0; i < kArrK; ++i) {
    a->src[i] = i < K ? srcs[i]->d_if : nullptr;
    a->src_bytes[i] = i < K ? (long long)srcs[i]->if_nsamples * pl.src_bps : 0;
  }
  a->dst = dst ? dst->d_if : nullptr;
  a->weights = nullptr;
  a->nrecords = K;
  a->tile = (int)pl.tile;
  a->rec_bytes = (int)pl.rec_bytes;
  a->dst_mode = dst ? gc_record_mode(dst) : 0;
  return GC_OK;
}

}  // namespace

void gc_array_free(gc_context* ctx) {
  ArrState* s = static_cast<ArrState*>(ctx->arr);
  if (!s) return;
  gc_buf_free(s->weights);
  gc_buf_free(s->stats);
  gc_buf_free(s->cov);
  delete s;
  ctx->arr = nullptr;
}

extern "C" long long gc_debug_array_tile_outputs(int nrecords, int ntaps) { return arr_tile_outputs(nrecords, ntaps); }

extern "C" int gc_array_covariance(gc_context* const* srcs, const gc_array_cov_params* p, int64_t* cov) {
  ArrPlan pl;
  int rc = arr_cov_check(srcs, p, cov, &pl);
  if (rc) return rc;
  // nothing has been written up to here
  gc_context* const s0 = srcs[0];
  const int K = p->nrecords, L = p->nlags;
  ArrArgs a;
  rc = arr_begin(srcs, nullptr, K, pl, &a);
  if (rc) return rc;
  ArrState* s = gc_unit_state<ArrState>(s0->arr);
  if (!s) return gc_nomem("gc_array_covariance");
  const size_t nout = (size_t)L * K * K * 2, bytes = nout * kArrCovSlots * sizeof(unsigned long long);
  if (gc_buf_reserve(s->cov, bytes, false) != hipSuccess) return gc_nomem("gc_array_covariance");
  std::vector<unsigned long long> slots;
  try {
    slots.resize(nout * kArrCovSlots);
  } catch (const std::bad_alloc&) {
    return gc_nomem("gc_array_covariance");
  }
  GC_HIP(hipMemsetAsync(s->cov.p, 0, bytes, s0->stream));
  a.out = (unsigned long long*)s->cov.p;
  a.first = (long long)p->first_sample;
  a.n = (long long)p->nsamples;
  a.dst_first = 0;
  a.ntaps = L;
  gc_with_mode(gc_record_mode(s0), [&](auto m) {
    hipLaunchKernelGGL(array_cov_kernel<decltype(m)::value>, dim3((unsigned int)pl.ntiles), dim3(kArrWG), (size_t)pl.lds_bytes, s0->stream, a);
  });
  GC_HIP(hipGetLastError());
  GC_HIP(hipMemcpyAsync(slots.data(), s->cov.p, bytes, hipMemcpyDeviceToHost, s0->stream));
  GC_HIP(hipStreamSynchronize(s0->stream));
  for (size_t i = 0; i < nout; ++i) {
    unsigned long long v = 0ull;
    for (int k = 0; k < kArrCovSlots; ++k) v += slots[(size_t)k * nout + i];
    cov[i] = (int64_t)v;
  }
  return GC_OK;
}

extern "C" int gc_array_combine(gc_context* const* srcs, gc_context* dst, const gc_array_combine_params* p, const double* weights,
                                gc_array_combine_result* res) {
  ArrPlan pl;
  int rc = arr_combine_check(srcs, dst, p, weights, &pl);
  if (rc) return rc;
  if (pl.ntiles > 0x7fffffffLL) {
    gc_set_error("gc_array_combine: %lld tiles in one call", pl.ntiles);
    return GC_E_INVALID;
  }
  // nothing has been written up to here
  gc_context* const s0 = srcs[0];
  const int K = p->nrecords, T = p->ntaps;
  ArrArgs a;
  rc = arr_begin(srcs, dst, K, pl, &a);
  if (rc) return rc;
  ArrState* s = gc_unit_state<ArrState>(s0->arr);
  if (!s) return gc_nomem("gc_array_combine");
  const size_t w_bytes = (size_t)K * T * 2 * sizeof(double);
  if (gc_buf_reserve(s->weights, w_bytes, false) != hipSuccess) return gc_nomem("gc_array_combine");
  rc = fir_stats_begin("gc_array_combine", s->stats, s0->stream);
  if (rc) return rc;
  GC_HIP(hipMemcpyAsync(s->weights.p, weights, w_bytes, hipMemcpyHostToDevice, s0->stream));
  a.weights = (const double*)s->weights.p;
  a.out = (unsigned long long*)s->stats.p;
  a.first = (long long)p->first_sample;
  a.n = (long long)p->noutputs;
  a.dst_first = (long long)p->dst_first;
  a.ntaps = T;
  gc_with_mode(gc_record_mode(s0), [&](auto m) {
    hipLaunchKernelGGL(array_combine_kernel<decltype(m)::value>, dim3((unsigned int)pl.ntiles), dim3(kArrWG), (size_t)pl.lds_bytes, s0->stream, a);
  });
  GC_HIP(hipGetLastError());
  unsigned long long host[2];
  rc = fir_stats_end(s->stats, s0->stream, host);
  if (rc) return rc;
  if (res) {
    res->clipped = (int64_t)host[0];
    res->sum_sq = host[1];
  }
  return GC_OK;
}
