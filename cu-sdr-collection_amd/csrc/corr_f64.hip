// corr_f64.hip — the float64 correlator (gc_set_precision GC_PREC_F64): tracking.m:247-300 restated operation by operation in
// float64, for every channel kind and record format, and its persistent device-loop instantiation.
//
// Per sample (one thread per sample, grid-stride), every rule from replica_f64.h:
//   code index  the reference's float64 colon element, then ceil(t * arm_mult) + table_offset, clamped to the table; tables are
//               read from HBM through L2 (the GPS L2C CL table has 1.5 M entries)
//   carrier     trig = (carrFreq * 2 * pi) * (i / fs) + remCarrPhase, then float64 cos / sin of trig itself
//   baseband    real / imag(exp(-1i * trig) .* raw)
//   sums        float64, 6 per arm
// Reduction in a fixed order - lanes by fixed shuffles, waves in index order, splits in index order (combine_partials_kernel or the
// host loop) - so a result is bitwise the same from run to run.
//
// The argument of cos / sin reaches ~1e5 - 1e6 rad (a 10-ms block of a 20 MHz carrier: 1.3e6); ocml's float64 sincos takes its
// small-argument (Cody-Waite, three-part pi/2) reduction for |x| < 2^30 (the compare against 0x41d00000 00000000 in the ISA) and
// branches to the Payne-Hanek path (v_trig_preop_f64) above - present in the code object, never taken for these arguments.
//
// Two instantiations:
//   corr_f64_kernel          one launch per epoch (gc_correlate, gc_track's host-closed loop): workgroups of kF64WG threads,
//                            `splits` workgroups per block
//   corr_f64_devloop_kernel  gc_track_device: ONE workgroup of 16 waves per channel runs every epoch - correlate, reduce in LDS,
//                            thread 0 closes the loop with devloop.h (the float64 statements of tracking.m:302-335 the host loop
//                            runs) and writes the next block to LDS, barrier.  No inter-workgroup message, no poll.
#include "corr_common.h"
#include "devloop.h"
#include "replica_f64.h"

using namespace gcorr;

namespace {

constexpr int kF64WG = 256;       // per-epoch launch
constexpr int kF64LoopWG = 1024;  // device loop: 16 waves per channel

struct F64Args {
  const uint8_t* if_base;
  const gc_block* blocks;
  const DevChannel* chans;
  double* out;      // [nblocks][GC_OUT_STRIDE] when splits == 1
  double* partial;  // [nblocks][splits][GC_OUT_STRIDE] when splits > 1
  double fs;
  int splits;
};

// Sums of samples i_beg + tid, i_beg + tid + nthr, ... < i_end of block `blk` into acc (zeroed by the caller).
template <int MODE>
__device__ __forceinline__ void f64_accumulate(const uint8_t* __restrict__ if_base, const DevChannel* __restrict__ chn, const gc_block& blk,
                                               double fs, int i_beg, int i_end, int tid, int nthr, double (&acc)[GC_OUT_STRIDE]) {
  const int arms = chn->arms;
  const double R = chn->index_scale, rem = blk.rem_code_phase, step = blk.code_phase_step, d = blk.el_spacing;
  const int N = blk.blksize;
  const Ramp64 ramp[3] = {ramp64(rem, -d, step, R, N), ramp64(rem, 0.0, step, R, N), ramp64(rem, d, step, R, N)};  // early, prompt, late
  const Carrier64 carr = carrier64(blk.carr_freq, blk.rem_carr_phase);
  const int8_t* tab[GC_MAX_ARMS];
  double mult[GC_MAX_ARMS];
  int off[GC_MAX_ARMS], last[GC_MAX_ARMS];
#pragma unroll
  for (int ar = 0; ar < GC_MAX_ARMS; ++ar) {
    tab[ar] = chn->tab[ar];
    mult[ar] = chn->mult[ar];
    off[ar] = blk.table_offset[ar];
    last[ar] = chn->nent[ar] - 1;
  }
  const uint8_t* base = if_base;
  for (int i = i_beg + tid; i < i_end; i += nthr) {
    double re, im, sn, cs, ib, qb;
    record_sample<MODE>(base, blk.first_sample + i, re, im);
    carr.at(i, fs, sn, cs);
    wipe_off(sn, cs, re, im, ib, qb);
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      // The taps share step and length, so they are named once: the compiler then forms the three elements with selects and
      // shares i*sp and (N-1-i)*sp among them.  With each ramp's own copies (ramp[x].at(i)) it keeps a branch per tap, and the
      // 192-channel device loop measured 1.5 % slower.
      const double t = colon_at(ramp[x].a, ramp[x].b, ramp[1].sp, N, i);
#pragma unroll
      for (int ar = 0; ar < GC_MAX_ARMS; ++ar) {
        if (ar < arms) {
          const double c = (double)tab[ar][code_index(t, mult[ar], off[ar], last[ar])];
          acc[ar * 6 + 2 * x] += c * ib;
          acc[ar * 6 + 2 * x + 1] += c * qb;
        }
      }
    }
  }
}

// Lanes by fixed shuffles, then the waves in index order (thread v < GC_OUT_STRIDE holds output v on return).
template <int WAVES>
__device__ __forceinline__ double f64_block_reduce(double (&acc)[GC_OUT_STRIDE], double (*red)[GC_OUT_STRIDE], int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int v = 0; v < GC_OUT_STRIDE; ++v) {
    double x = acc[v];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if (lane == 0) red[wave][v] = x;
  }
  __syncthreads();
  double s = 0.0;
  if (tid < GC_OUT_STRIDE)
    for (int w = 0; w < WAVES; ++w) s += red[w][tid];
  return s;
}

template <int MODE>
__global__ __launch_bounds__(kF64WG) void corr_f64_kernel(const F64Args p) {
  __shared__ double red[kF64WG / 64][GC_OUT_STRIDE];
  const long long lb = blockIdx.x / p.splits;
  const int split = (int)(blockIdx.x - lb * p.splits);
  const gc_block blk = p.blocks[lb];
  const DevChannel* __restrict__ chn = p.chans + blk.channel;
  const int N = blk.blksize;
  const int per = (N + p.splits - 1) / p.splits;
  const int i_beg = split * per, i_end = min(N, i_beg + per);
  double acc[GC_OUT_STRIDE];
#pragma unroll
  for (int v = 0; v < GC_OUT_STRIDE; ++v) acc[v] = 0.0;
  f64_accumulate<MODE>(p.if_base, chn, blk, p.fs, i_beg, i_end, (int)threadIdx.x, kF64WG, acc);
  const double s = f64_block_reduce<kF64WG / 64>(acc, red, (int)threadIdx.x);
  if (threadIdx.x < GC_OUT_STRIDE) {
    if (p.splits == 1)
      p.out[lb * GC_OUT_STRIDE + threadIdx.x] = s;
    else
      p.partial[(lb * p.splits + split) * GC_OUT_STRIDE + threadIdx.x] = s;
  }
}

// tracking.m:273-335 for the epoch's sums (devloop.h, as the lane kernel's closer runs it), the records and the state to device memory,
// the next block and the status to LDS.  Out of line: its registers are not the correlation loop's.
__device__ __noinline__ void f64_close(const DevLoopArgs* __restrict__ dl, DevLoopChan& st, gc_block& sblk, int& sstatus, const double* ssum, int c,
                                       int e, int arms, double R) {
  double sums[GC_OUT_STRIDE];
#pragma unroll
  for (int v = 0; v < GC_OUT_STRIDE; ++v) sums[v] = ssum[v];
  gc_block b = sblk;
  const DevLoopPre pre = devloop_pre(dl, st, b, R);
  double rv[GC_TRK_NFIELDS];
  const int status = devloop_post<GC_MAX_ARMS>(dl, st, b, e, sums, arms, R, pre, [&](int f, double v) { rv[f] = v; });
  devloop_commit(dl, dl->chan + c, st, c, e, rv, arms, 0);
  sblk = b;
  sstatus = status;
}

// Device loop: workgroup c runs channel slot c from the state gc_track_device put in dl->chan[c] until its status is not 0
// (all its epochs done, record exhausted, NCO diverged, paused at the end of a window).  Records and the final state go to device memory (devloop_commit).
template <int MODE>
__global__ __launch_bounds__(kF64LoopWG) void corr_f64_devloop_kernel(const DevLoopArgs* __restrict__ dl, const F64Args p) {
  __shared__ double red[kF64LoopWG / 64][GC_OUT_STRIDE];
  __shared__ double ssum[GC_OUT_STRIDE];
  __shared__ gc_block sblk;
  __shared__ int sstatus;
  __shared__ DevLoopChan st;  // the loop state, thread 0's (in LDS: no registers held across the correlation)
  const int c = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (tid == 0) {
    st = dl->chan[c];
    sblk = st.blk;
    sstatus = st.status;
  }
  __syncthreads();
  const DevChannel* __restrict__ chn = p.chans + sblk.channel;
  const double R = chn->index_scale;
  const int arms = chn->arms;
  for (int e = 0; sstatus == 0; ++e) {
    const gc_block blk = sblk;
    double acc[GC_OUT_STRIDE];
#pragma unroll
    for (int v = 0; v < GC_OUT_STRIDE; ++v) acc[v] = 0.0;
    f64_accumulate<MODE>(p.if_base, chn, blk, p.fs, 0, blk.blksize, tid, kF64LoopWG, acc);
    const double s = f64_block_reduce<kF64LoopWG / 64>(acc, red, tid);
    if (tid < GC_OUT_STRIDE) ssum[tid] = s;
    __syncthreads();
    if (tid == 0) f64_close(dl, st, sblk, sstatus, ssum, c, e, arms, R);
    __syncthreads();
  }
}

F64Args make_args(const gc_context* ctx) {
  F64Args a;
  a.if_base = ctx->d_if;
  a.blocks = nullptr;
  a.chans = ctx->d_channels;
  a.out = nullptr;
  a.partial = nullptr;
  a.fs = ctx->fs;
  a.splits = 1;
  return a;
}

template <int MODE>
int launch_devloop_mode(gc_context* ctx, const DevLoopArgs* dl, F64Args& a, int nch) {
  void* args[2] = {(void*)&dl, (void*)&a};
  // no workgroup waits for another, but the grid enters the persistent-kernel ledger all the same (gc_track_multi's admission)
  GC_PERSIST(gc_launch_persistent(ctx, (const void*)corr_f64_devloop_kernel<MODE>, dim3((unsigned int)nch), dim3(kF64LoopWG), args, 0u));
  return GC_OK;
}

}  // namespace

int gc_launch_correlator_f64(gc_context* ctx, const gc_block* d_blocks, int64_t nblocks, int splits, double* d_out, double* d_partial) {
  const long long total = (long long)nblocks * splits;
  if (splits < 1 || total > 0x7fffffffLL) {
    gc_set_error("float64 correlator: bad launch (%lld blocks x %d splits)", (long long)nblocks, splits);
    return GC_E_INVALID;
  }
  F64Args a = make_args(ctx);
  a.blocks = d_blocks;
  a.out = d_out;
  a.partial = d_partial;
  a.splits = splits;
  const dim3 grid((unsigned int)total), block(kF64WG);
  gc_with_mode(gc_record_mode(ctx), [&](auto m) {
    hipLaunchKernelGGL(corr_f64_kernel<decltype(m)::value>, grid, block, 0, ctx->stream, a);
  });
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gc_launch_devloop_f64(gc_context* ctx, const DevLoopArgs* dl, int nch) {
  F64Args a = make_args(ctx);
  return gc_with_mode(gc_record_mode(ctx), [&](auto m) {
    return launch_devloop_mode<decltype(m)::value>(ctx, dl, a, nch);
  });
}
