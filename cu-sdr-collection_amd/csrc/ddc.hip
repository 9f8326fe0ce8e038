// ddc.hip — gc_downconvert: a band of a record as a second record at a lower rate (include/gnsscorr.h has the definition): complex
// FIR, integer decimation, a 64-bit phase-accumulator NCO, requantisation into any of the six formats.  Float64, every operation
// rounded by itself (the unit is compiled with -ffp-contract=off).
//
// The outputs are cut into tiles of consecutive outputs (ddc_plan.h), one workgroup each:
//   stage    the tile's input span [n_lo, n_hi] as the record's own bytes into LDS, in whole 16-byte vectors of the record from the
//            vector that holds n_lo's first byte, each a RecVec load (record_fmt.h: one 16-byte global load where the vector lies
//            inside the record, byte by byte and zero outside for the record's partial last vector and for the padding in front of
//            sample 0 and behind the last sample).  The samples stay integers in LDS - as doubles the span of the longest filter
//            at the largest decimation would not fit - and are converted where they are used.  The taps go next to them as
//            (re, im) doubles.
//   filter   a thread carries up to kDdcChains outputs, kDdcWG apart: that many independent add chains, which share every tap read
//            (the tap's address is the same in all lanes: one broadcast read).  k ascending, products and sums as the definition
//            writes them.
//   finish   per OUTPUT: the NCO's phase from the absolute record index in 64-bit integers, one float64 sincos of an angle in
//            [-pi, pi], the rotation, rint, clamp and one store of the sample in dst's format (a wave-uniform run-time branch).
//   result   clipped components and the sum of squares as integers: a wave reduction by shuffles, the waves joined in LDS, one pair
//            of integer atomics per workgroup into one of 64 slots, which the host adds.
// An output depends on its T samples and on n_m only; the tile decides nothing but who computes it.
// The staging, the read of a staged sample, the finish and the hand-over of the result are fir_common.h's, shared with resample.hip
// and array.hip; the tile and its span are fir_plan.h's.
// The unit's buffers are its own (DdcState, kept in gc_context::ddc, grow-only, released by gc_destroy).
#include "ddc_plan.h"
#include "fir_common.h"
#include "record_fmt.h"

using namespace gcorr;

namespace {

struct DdcState {  // grow-only device buffers of the context (released by gc_destroy)
  GcBuf taps, stats;
};

struct DdcArgs {
  const uint8_t* src;
  uint8_t* dst;
  const double* taps;          // [T][2]
  unsigned long long* stats;   // [kFirStatSlots]{clipped, sum_sq} (fir_common.h)
  long long first, nout, dst_first;
  long long src_bytes;         // of the record: samples * bytes per sample
  unsigned long long phase_step, phase0;
  int decim, ntaps, tile;
  int dst_mode;                // gcorr::Mode of dst
};

template <int MODE>
__global__ __launch_bounds__(kDdcWG) void ddc_kernel(const DdcArgs p) {
  using F = Fmt<MODE>;
  extern __shared__ uint4 ddc_lds[];
  const int tid = (int)threadIdx.x, T = p.ntaps, D = p.decim;
  double2* const taps = reinterpret_cast<double2*>(ddc_lds);  // 16 T bytes
  uint4* const vecs = ddc_lds + T;
  const uint8_t* const bytes = reinterpret_cast<const uint8_t*>(vecs);

  const FirTile tile = fir_tile(p.tile, (long long)blockIdx.x, p.first, p.nout, D, T);
  const long long m0 = tile.m0;
  const int cnt = (int)tile.n;  // >= 1: the grid is ceil(nout / tile)
  const long long base16 = fir_stage_base(tile.n_lo, F::bps);
  const int nvec = (int)fir_stage_vecs(tile.n_lo, tile.n_hi, F::bps);  // <= (span * bps + 15 + 15) / 16: inside ddc_lds_bytes

  stage_span<MODE, kDdcWG>(p.src, p.src_bytes, base16, nvec, vecs);
  for (int k = tid; k < T; k += kDdcWG) taps[k] = make_double2(p.taps[2 * k], p.taps[2 * k + 1]);
  __syncthreads();

  // output j of this thread is tile output tid + j kDdcWG; one that the tile does not have computes output 0 again and stores nothing
  int off[kDdcChains];
  double ar[kDdcChains], ai[kDdcChains];
#pragma unroll
  for (int j = 0; j < kDdcChains; ++j) {
    const int q = tid + j * kDdcWG;
    const long long n = p.first + (m0 + (q < cnt ? q : 0)) * (long long)D;
    off[j] = (int)(n * F::bps - base16);
    ar[j] = 0.0;
    ai[j] = 0.0;
  }
  const int chains = (cnt + kDdcWG - 1) / kDdcWG;  // uniform over the workgroup: the chains that hold an output at all
#pragma unroll 1
  for (int k = 0; k < T; ++k) {
    const double2 g = taps[k];
#pragma unroll
    for (int j = 0; j < kDdcChains; ++j)
      if (j < chains) {
        double xr, xi;
        staged_sample<MODE>(bytes, off[j] - k * F::bps, xr, xi);
        const double pr = g.x * xr - g.y * xi;
        const double pi = g.x * xi + g.y * xr;
        ar[j] = ar[j] + pr;
        ai[j] = ai[j] + pi;
      }
  }

  unsigned long long clipped = 0ull, sum_sq = 0ull;
#pragma unroll
  for (int j = 0; j < kDdcChains; ++j) {
    const int q = tid + j * kDdcWG;
    if (q >= cnt) continue;
    const long long m = m0 + q;
    const unsigned long long n = (unsigned long long)(p.first + m * D);
    fir_finish<true>(ar[j], ai[j], p.phase0 + p.phase_step * n, p.dst_mode, p.dst, p.dst_first + m, clipped, sum_sq);
  }
  fir_hand_over<kDdcWG / 64>(clipped, sum_sq, p.stats);
}

}  // namespace

void gc_ddc_free(gc_context* ctx) {
  DdcState* s = static_cast<DdcState*>(ctx->ddc);
  if (!s) return;
  gc_buf_free(s->taps);
  gc_buf_free(s->stats);
  delete s;
  ctx->ddc = nullptr;
}

extern "C" long long gc_debug_ddc_tile_outputs(int decim, int ntaps) { return ddc_tile_outputs(decim, ntaps); }

extern "C" int gc_downconvert(gc_context* src, gc_context* dst, const gc_ddc_params* p, const double* taps, gc_ddc_result* res) {
  DdcPlan pl;
  int rc = ddc_check(src, dst, p, taps, &pl);
  if (rc) return rc;
  if (pl.ntiles > 0x7fffffffLL) {
    gc_set_error("gc_downconvert: %lld tiles in one call", pl.ntiles);
    return GC_E_INVALID;
  }
  // nothing has been written up to here
  GC_HIP(hipSetDevice(src->device));
  GC_HIP(hipStreamSynchronize(dst->stream));  // the destination's own pending work comes first
  DdcState* s = gc_unit_state<DdcState>(src->ddc);
  if (!s) return gc_nomem("gc_downconvert");
  const size_t taps_bytes = (size_t)p->ntaps * 2 * sizeof(double);
  if (gc_buf_reserve(s->taps, taps_bytes, false) != hipSuccess) return gc_nomem("gc_downconvert");
  rc = fir_stats_begin("gc_downconvert", s->stats, src->stream);
  if (rc) return rc;
  GC_HIP(hipMemcpyAsync(s->taps.p, taps, taps_bytes, hipMemcpyHostToDevice, src->stream));
  DdcArgs a;
  a.src = src->d_if;
  a.dst = dst->d_if;
  a.taps = (const double*)s->taps.p;
  a.stats = (unsigned long long*)s->stats.p;
  a.first = (long long)p->first_sample;
  a.nout = (long long)p->noutputs;
  a.dst_first = (long long)p->dst_first;
  a.src_bytes = (long long)src->if_nsamples * pl.src_bps;
  a.phase_step = pl.phase_step;
  a.phase0 = pl.phase0;
  a.decim = p->decim;
  a.ntaps = p->ntaps;
  a.tile = (int)pl.tile;
  a.dst_mode = gc_record_mode(dst);
  gc_with_mode(gc_record_mode(src), [&](auto m) {
    hipLaunchKernelGGL(ddc_kernel<decltype(m)::value>, dim3((unsigned int)pl.ntiles), dim3(kDdcWG), (size_t)pl.lds_bytes, src->stream, a);
  });
  GC_HIP(hipGetLastError());
  unsigned long long host[2];
  rc = fir_stats_end(s->stats, src->stream, host);
  if (rc) return rc;
  if (res) {
    res->phase_step = pl.phase_step;
    res->phase0 = pl.phase0;
    res->clipped = (int64_t)host[0];
    res->sum_sq = host[1];
    res->carr_freq = pl.carr_freq;
  }
  return GC_OK;
}
