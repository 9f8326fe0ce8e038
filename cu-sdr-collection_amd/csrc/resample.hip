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
// The staging, the read of a staged sample, the finish and the hand-over of the result are fir_common.h's, shared with ddc.hip and
// array.hip.
// The unit's buffers are its own (RsState, kept in gc_context::rs, grow-only, released by gc_destroy).
#include <new>
#include <vector>

#include "fir_common.h"
#include "record_fmt.h"
#include "resample_plan.h"

using namespace gcorr;

namespace {

struct RsState {  // grow-only device buffers of the context (released by gc_destroy)
  GcBuf taps, stats;
};

struct RsArgs {
  const uint8_t* src;
  uint8_t* dst;
  const double2* taps;         // [L][row]: phase-major, zero-padded
  unsigned long long* stats;   // [kFirStatSlots]{clipped, sum_sq} (fir_common.h)
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
  const int tid = (int)threadIdx.x, L = p.interp, M = p.decim, J = p.branches;
  const int ntap = L * p.row;                                  // staged (re, im) pairs: 16 bytes each
  double2* const taps = reinterpret_cast<double2*>(rs_lds);
  uint4* const vecs = rs_lds + ntap;
  const uint8_t* const bytes = reinterpret_cast<const uint8_t*>(vecs);

  const RsTile tile = rs_tile(p.tile, (long long)blockIdx.x, p.first_tick, p.nout, L, M, p.ntaps);
  const int cnt = (int)tile.n;  // >= 1: the grid is ceil(nout / tile)
  const long long base16 = fir_stage_base(tile.n_lo, F::bps);
  const int nvec = (int)fir_stage_vecs(tile.n_lo, tile.n_hi, F::bps);  // <= (span * bps + 15 + 15) / 16: inside rs_lds_bytes

  stage_span<MODE, kRsWG>(p.src, p.src_bytes, base16, nvec, vecs);
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
#pragma unroll
  for (int c = 0; c < kRsChains; ++c) {
    const int q = tid + c * stride;
    if (tid >= stride || q >= cnt) continue;
    const unsigned long long u = (unsigned long long)(tile.u0 + (long long)q * M);
    fir_finish<true>(ar[c], ai[c], p.phase0 + p.phase_step * u, p.dst_mode, p.dst, p.dst_first + tile.m0 + q, clipped, sum_sq);
  }
  fir_hand_over<kRsWG / 64>(clipped, sum_sq, p.stats);
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
  int rc = rs_check(src, dst, p, taps, &pl);
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
  if (gc_buf_reserve(s->taps, taps_bytes, false) != hipSuccess) return gc_nomem("gc_resample");
  rc = fir_stats_begin("gc_resample", s->stats, src->stream);
  if (rc) return rc;
  GC_HIP(hipMemcpyAsync(s->taps.p, rows.data(), taps_bytes, hipMemcpyHostToDevice, src->stream));
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
  unsigned long long host[2];
  rc = fir_stats_end(s->stats, src->stream, host);  // synchronises; `rows` is read by the copy above until then
  if (rc) return rc;
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
