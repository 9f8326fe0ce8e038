// resample.hip — gc_resample: a record at the rate L / M of its own as a second record (include/gnsscorr.h has the definition): the
// polyphase form of gc_downconvert (ddc.hip).  Complex FIR given at the rate fs L, of which output m meets the taps j L + p_m only,
// a 64-bit phase-accumulator NCO addressed by the tick, requantisation into any of the six formats.  Float64, every operation rounded
// by itself (the unit is compiled with -ffp-contract=off).
//
// The outputs are cut into tiles of consecutive outputs (resample_plan.h), one workgroup each:
//   stage    the tile's input span [n_lo, n_hi] as the record's own bytes into LDS in whole 16-byte vectors, as ddc.hip does.  In
//            front of them the taps PHASE-MAJOR, taps[p][j] = g[j L + p], zero where j L + p >= T, a row of rs_row() (re, im)
//            doubles per phase: the host lays them out so (once per call) and the workgroup copies them.
//   filter   lane q < stride takes the tile's outputs q, q + stride, .. (at most kRsChains), stride = the largest multiple of
//            Lp = L / gcd(L, M) in the workgroup: all chains of a lane have one phase, so one tap read per j feeds them all.  Lanes
//            next to each other take outputs next to each other (coalesced stores, sample reads M / L samples apart) and read the
//            rows of up to Lp phases: a gather, spread over the banks by the odd row length.  For Lp = 1 all lanes
//            read one address: ddc.hip's broadcast.  j ascending over all J of a row, products and sums as the definition writes
//            them; the zero taps at the end of a short row add +-0.
//   finish   per output, and the result: ddc.hip's, with the tick in place of the sample index.
// An output depends on its samples and on u_m only; the tile decides nothing but who computes it.
// staged_sample and wave_sum are ddc.hip's (fir_common.h); the finish is written out in both units, because as a shared function it
// changed the order of ddc_kernel's instructions.
// The unit's buffers are its own (RsState, kept in gc_context::rs, grow-only, released by gc_destroy).
#include <new>
#include <vector>

#include "fir_common.h"
#include "record_fmt.h"
#include "resample_plan.h"

using namespace gcorr;

namespace {

constexpr int kRsStatSlots = 64;

struct RsState {  // grow-only device buffers of the context (released by gc_destroy)
  GcBuf taps, stats;
};

struct RsArgs {
  const uint8_t* src;
  uint8_t* dst;
  const double2* taps;         // [L][row]: phase-major, zero-padded
  unsigned long long* stats;   // [kRsStatSlots]{clipped, sum_sq}: workgroup b adds to slot b mod kRsStatSlots, the host adds the slots
  long long first_tick, nout, dst_first;
  long long src_bytes;         // of the record: samples * bytes per sample
  unsigned long long phase_step, phase0;
  int interp, decim, ntaps, tile;
  int stride, row, branches;   // rs_stride, rs_row, rs_branches of (interp, decim, ntaps)
  int dst_mode;                // gcorr::Mode of dst
};

template <int MODE>
__global__ __launch_bounds__(kRsWG) void rs_kernel(const RsArgs p) {
  using F = Fmt<MODE>;
  extern __shared__ uint4 rs_lds[];
  __shared__ unsigned long long wave_part[kRsWG / 64][2];
  const int tid = (int)threadIdx.x, L = p.interp, M = p.decim, J = p.branches;
  const int ntap = L * p.row;                                  // staged (re, im) pairs: 16 bytes each
  double2* const taps = reinterpret_cast<double2*>(rs_lds);
  uint4* const vecs = rs_lds + ntap;
  const uint8_t* const bytes = reinterpret_cast<const uint8_t*>(vecs);

  const RsTile tile = rs_tile(p.tile, (long long)blockIdx.x, p.first_tick, p.nout, L, M, p.ntaps);
  const int cnt = (int)tile.n;  // >= 1: the grid is ceil(nout / tile)
  const long long base16 = ddc_stage_base(tile.n_lo, F::bps);
  const int nvec = (int)ddc_stage_vecs(tile.n_lo, tile.n_hi, F::bps);  // <= (span * bps + 15 + 15) / 16: inside rs_lds_bytes

  for (int i = tid; i < nvec; i += kRsWG) {
    RecVec<MODE> q;
    q.load(p.src, base16 + 16LL * i, p.src_bytes);
    vecs[i] = q.words();
  }
  for (int k = tid; k < ntap; k += kRsWG) taps[k] = p.taps[k];
  __syncthreads();

  // chain c of this lane is tile output tid + c stride.  A lane without an output (tid >= stride, tid >= cnt) runs output 0's
  // addresses; a chain the tile does not have runs its lane's first output again; neither stores
  const int stride = p.stride;
  const bool lane_on = tid < stride && tid < cnt;
  int dn, ph;
  rs_output(tile.p0, lane_on ? tid : 0, L, M, &dn, &ph);
  const double2* const row = taps + ph * p.row;
  int off[kRsChains];
  double ar[kRsChains], ai[kRsChains];
#pragma unroll
  for (int c = 0; c < kRsChains; ++c) {
    const int q = tid + c * stride;
    int dq, pq;
    rs_output(tile.p0, (lane_on && q < cnt) ? q : (lane_on ? tid : 0), L, M, &dq, &pq);  // pq == ph: stride M is a multiple of L
    off[c] = (int)((tile.n0 + dq) * F::bps - base16);
    ar[c] = 0.0;
    ai[c] = 0.0;
  }
  const int chains = (cnt + stride - 1) / stride;  // uniform over the workgroup: the chains that hold an output at all
#pragma unroll 1
  for (int j = 0; j < J; ++j) {
    const double2 g = row[j];
#pragma unroll
    for (int c = 0; c < kRsChains; ++c)
      if (c < chains) {
        double xr, xi;
        staged_sample<MODE>(bytes, off[c] - j * F::bps, xr, xi);
        const double pr = g.x * xr - g.y * xi;
        const double pi = g.x * xi + g.y * xr;
        ar[c] = ar[c] + pr;
        ai[c] = ai[c] + pi;
      }
  }

  unsigned long long clipped = 0ull, sum_sq = 0ull;
  const int dmode = p.dst_mode;
  const bool d16 = dmode == I16_IQ || dmode == I16_QI || dmode == I16_REAL, dreal = dmode == I8_REAL || dmode == I16_REAL;
  const bool dswap = dmode == I8_QI || dmode == I16_QI;
  const double lo = d16 ? -32768.0 : -128.0, hi = d16 ? 32767.0 : 127.0;
#pragma unroll
  for (int c = 0; c < kRsChains; ++c) {
    const int q = tid + c * stride;
    if (tid >= stride || q >= cnt) continue;
    const unsigned long long u = (unsigned long long)(tile.u0 + (long long)q * M);
    const unsigned long long phs = p.phase0 + p.phase_step * u;
    const double ang = (double)(long long)phs * (kDdcTwoPi * 0x1p-64);  // the product of the constants is exact
    double sn, cs;
    sincos(ang, &sn, &cs);
    const double yr = cs * ar[c] + sn * ai[c];
    const double yi = cs * ai[c] - sn * ar[c];
    const double rr = rint(yr), ri = rint(yi);
    const long long o_re = (long long)fmin(fmax(rr, lo), hi), o_im = (long long)fmin(fmax(ri, lo), hi);
    clipped += (rr < lo || rr > hi) ? 1ull : 0ull;
    sum_sq += (unsigned long long)(o_re * o_re);
    if (!dreal) {
      clipped += (ri < lo || ri > hi) ? 1ull : 0ull;
      sum_sq += (unsigned long long)(o_im * o_im);
    }
    const long long s = p.dst_first + tile.m0 + q;
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
  if (tid == 0) {  // one pair of integer atomics per workgroup, spread over kRsStatSlots addresses
    clipped = sum_sq = 0ull;
    for (int w = 0; w < kRsWG / 64; ++w) clipped += wave_part[w][0], sum_sq += wave_part[w][1];
    unsigned long long* const slot = p.stats + 2 * (blockIdx.x % kRsStatSlots);
    if (clipped) atomicAdd(&slot[0], clipped);
    if (sum_sq) atomicAdd(&slot[1], sum_sq);
  }
}

}  // namespace

void gc_rs_free(gc_context* ctx) {
  RsState* s = static_cast<RsState*>(ctx->rs);
  if (!s) return;
  gc_buf_free(s->taps);
  gc_buf_free(s->stats);
  delete s;
  ctx->rs = nullptr;
}

extern "C" long long gc_debug_rs_tile_outputs(int interp, int decim, int ntaps) { return rs_tile_outputs(interp, decim, ntaps); }

extern "C" int gc_resample(gc_context* src, gc_context* dst, const gc_rs_params* p, const double* taps, gc_rs_result* res) {
  RsPlan pl;
  const int rc = rs_check(src, dst, p, taps, &pl);
  if (rc) return rc;
  if (pl.ntiles > 0x7fffffffLL) {
    gc_set_error("gc_resample: %lld tiles in one call", pl.ntiles);
    return GC_E_INVALID;
  }
  // the taps phase-major: row p holds g[p], g[L + p], .. and zeros up to the row's length
  const int L = p->interp, T = p->ntaps;
  std::vector<double> rows;
  try {
    rows.assign((size_t)L * pl.row * 2, 0.0);
  } catch (const std::bad_alloc&) {
    gc_set_error("gc_resample: out of host memory");
    return GC_E_NOMEM;
  }
  for (int k = 0; k < T; ++k) {
    const size_t at = ((size_t)(k % L) * pl.row + (size_t)(k / L)) * 2;
    rows[at] = taps[2 * k];
    rows[at + 1] = taps[2 * k + 1];
  }
  // nothing has been written up to here
  GC_HIP(hipSetDevice(src->device));
  GC_HIP(hipStreamSynchronize(dst->stream));  // the destination's own pending work comes first
  RsState* s = gc_unit_state<RsState>(src->rs);
  if (!s) return gc_nomem("gc_resample");
  const size_t taps_bytes = rows.size() * sizeof(double);
  if (gc_buf_reserve(s->taps, taps_bytes, false) != hipSuccess || gc_buf_reserve(s->stats, sizeof(unsigned long long[kRsStatSlots][2]), false) != hipSuccess)
    return gc_nomem("gc_resample");
  GC_HIP(hipMemcpyAsync(s->taps.p, rows.data(), taps_bytes, hipMemcpyHostToDevice, src->stream));
  GC_HIP(hipMemsetAsync(s->stats.p, 0, sizeof(unsigned long long[kRsStatSlots][2]), src->stream));
  RsArgs a;
  a.src = src->d_if;
  a.dst = dst->d_if;
  a.taps = (const double2*)s->taps.p;
  a.stats = (unsigned long long*)s->stats.p;
  a.first_tick = (long long)p->first_tick;
  a.nout = (long long)p->noutputs;
  a.dst_first = (long long)p->dst_first;
  a.src_bytes = (long long)src->if_nsamples * pl.src_bps;
  a.phase_step = pl.phase_step;
  a.phase0 = pl.phase0;
  a.interp = L;
  a.decim = p->decim;
  a.ntaps = T;
  a.tile = (int)pl.tile;
  a.stride = pl.stride;
  a.row = pl.row;
  a.branches = pl.branches;
  a.dst_mode = gc_record_mode(dst);
  gc_with_mode(gc_record_mode(src), [&](auto m) {
    hipLaunchKernelGGL(rs_kernel<decltype(m)::value>, dim3((unsigned int)pl.ntiles), dim3(kRsWG), (size_t)pl.lds_bytes, src->stream, a);
  });
  GC_HIP(hipGetLastError());
  unsigned long long slots[kRsStatSlots][2], host[2] = {0ull, 0ull};
  GC_HIP(hipMemcpyAsync(slots, s->stats.p, sizeof slots, hipMemcpyDeviceToHost, src->stream));
  GC_HIP(hipStreamSynchronize(src->stream));  // also: `rows` is read by the copy above until here
  for (int i = 0; i < kRsStatSlots; ++i) host[0] += slots[i][0], host[1] += slots[i][1];
  if (res) {
    res->phase_step = pl.phase_step;
    res->phase0 = pl.phase0;
    res->clipped = (int64_t)host[0];
    res->sum_sq = host[1];
    res->carr_freq = pl.carr_freq;
    res->out_rate = pl.out_rate;
  }
  return GC_OK;
}
