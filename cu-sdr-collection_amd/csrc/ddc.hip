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
// The unit's buffers are its own (DdcState, kept in gc_context::ddc, grow-only, released by gc_destroy).
#include "ddc_plan.h"
#include "fir_common.h"
#include "record_fmt.h"

using namespace gcorr;

namespace {

constexpr int kDdcStatSlots = 64;

struct DdcState {  // grow-only device buffers of the context (released by gc_destroy)
  GcBuf taps, stats;
};

struct DdcArgs {
  const uint8_t* src;
  uint8_t* dst;
  const double* taps;          // [T][2]
  unsigned long long* stats;   // [kDdcStatSlots]{clipped, sum_sq}: workgroup b adds to slot b mod kDdcStatSlots, the host adds the slots
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
  __shared__ unsigned long long wave_part[kDdcWG / 64][2];
  const int tid = (int)threadIdx.x, T = p.ntaps, D = p.decim;
  double2* const taps = reinterpret_cast<double2*>(ddc_lds);  // 16 T bytes
  uint4* const vecs = ddc_lds + T;
  const uint8_t* const bytes = reinterpret_cast<const uint8_t*>(vecs);

  const DdcTile tile = ddc_tile(p.tile, (long long)blockIdx.x, p.first, p.nout, D, T);
  const long long m0 = tile.m0;
  const int cnt = (int)tile.n;  // >= 1: the grid is ceil(nout / tile)
  const long long base16 = ddc_stage_base(tile.n_lo, F::bps);
  const int nvec = (int)ddc_stage_vecs(tile.n_lo, tile.n_hi, F::bps);  // <= (span * bps + 15 + 15) / 16: inside ddc_lds_bytes

  for (int i = tid; i < nvec; i += kDdcWG) {
    RecVec<MODE> q;
    q.load(p.src, base16 + 16LL * i, p.src_bytes);
    vecs[i] = q.words();
  }
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
  const int dmode = p.dst_mode;
  const bool d16 = dmode == I16_IQ || dmode == I16_QI || dmode == I16_REAL, dreal = dmode == I8_REAL || dmode == I16_REAL;
  const bool dswap = dmode == I8_QI || dmode == I16_QI;
  const double lo = d16 ? -32768.0 : -128.0, hi = d16 ? 32767.0 : 127.0;
#pragma unroll
  for (int j = 0; j < kDdcChains; ++j) {
    const int q = tid + j * kDdcWG;
    if (q >= cnt) continue;
    const long long m = m0 + q;
    const unsigned long long n = (unsigned long long)(p.first + m * D);
    const unsigned long long ph = p.phase0 + p.phase_step * n;
    const double ang = (double)(long long)ph * (kDdcTwoPi * 0x1p-64);  // the product of the constants is exact
    double sn, cs;
    sincos(ang, &sn, &cs);
    const double yr = cs * ar[j] + sn * ai[j];
    const double yi = cs * ai[j] - sn * ar[j];
    const double rr = rint(yr), ri = rint(yi);
    const long long o_re = (long long)fmin(fmax(rr, lo), hi), o_im = (long long)fmin(fmax(ri, lo), hi);
    clipped += (rr < lo || rr > hi) ? 1ull : 0ull;
    sum_sq += (unsigned long long)(o_re * o_re);
    if (!dreal) {
      clipped += (ri < lo || ri > hi) ? 1ull : 0ull;
      sum_sq += (unsigned long long)(o_im * o_im);
    }
    const long long s = p.dst_first + m;
    const int o0 = (int)(dswap ? o_im : o_re), o1 = (int)(dswap ? o_re : o_im);
    if (dreal) {
      if (d16) reinterpret_cast<short*>(p.dst)[s] = (short)o0;
      else reinterpret_cast<signed char*>(p.dst)[s] = (signed char)o0;
    } else if (d16) {
      reinterpret_cast<uint32_t*>(p.dst)[s] = ((uint32_t)o0 & 0xffffu) | ((uint32_t)o1 << 16);
    } else {
      reinterpret_cast<unsigned short*>(p.dst)[s] = (unsigned short)(((uint32_t)o0 & 0xffu) | (((uint32_t)o1 & 0xffu) << 8));
    }
  }
  clipped = wave_sum(clipped);
  sum_sq = wave_sum(sum_sq);
  if ((tid & 63) == 0) {
    wave_part[tid >> 6][0] = clipped;
    wave_part[tid >> 6][1] = sum_sq;
  }
  __syncthreads();
  if (tid == 0) {  // one pair of integer atomics per workgroup, spread over kDdcStatSlots addresses: adds to one address queue up
    clipped = sum_sq = 0ull;
    for (int w = 0; w < kDdcWG / 64; ++w) clipped += wave_part[w][0], sum_sq += wave_part[w][1];
    unsigned long long* const slot = p.stats + 2 * (blockIdx.x % kDdcStatSlots);
    if (clipped) atomicAdd(&slot[0], clipped);
    if (sum_sq) atomicAdd(&slot[1], sum_sq);
  }
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
  const int rc = ddc_check(src, dst, p, taps, &pl);
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
  if (gc_buf_reserve(s->taps, taps_bytes, false) != hipSuccess || gc_buf_reserve(s->stats, sizeof(unsigned long long[kDdcStatSlots][2]), false) != hipSuccess)
    return gc_nomem("gc_downconvert");
  GC_HIP(hipMemcpyAsync(s->taps.p, taps, taps_bytes, hipMemcpyHostToDevice, src->stream));
  GC_HIP(hipMemsetAsync(s->stats.p, 0, sizeof(unsigned long long[kDdcStatSlots][2]), src->stream));
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
  unsigned long long slots[kDdcStatSlots][2], host[2] = {0ull, 0ull};
  GC_HIP(hipMemcpyAsync(slots, s->stats.p, sizeof slots, hipMemcpyDeviceToHost, src->stream));
  GC_HIP(hipStreamSynchronize(src->stream));
  for (int i = 0; i < kDdcStatSlots; ++i) host[0] += slots[i][0], host[1] += slots[i][1];
  if (res) {
    res->phase_step = pl.phase_step;
    res->phase0 = pl.phase0;
    res->clipped = (int64_t)host[0];
    res->sum_sq = host[1];
    res->carr_freq = pl.carr_freq;
  }
  return GC_OK;
}
