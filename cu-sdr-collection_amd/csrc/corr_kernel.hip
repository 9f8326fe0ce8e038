// corr_kernel.hip — the correlator launch (plan from launch_plan.h, kernel arguments, dispatch), the exact per-sample kernel
// for channels with mixed ramp multipliers, and the partial-sum combiner.  The two production kernels live in
// corr_fast.hip (low chipping rates: at most one table transition per lane-chunk) and corr_lane.hip (any rate).
#include "launch_plan.h"
#include "replica_f64.h"

using namespace gcorr;

namespace {

// ---- exact reference kernel for channels whose arms use DIFFERENT ramp multipliers ---------------------
// (BDS B1C wide-band: data BOC(1,1), pilot BOC(1,1) and pilot BOC(6,1) read through ceil(6*t),
// BDS/B1C/include/WB_tracking.m:285-317; the 122 762-entry BOC(6,1) table does not fit LDS next to the
// other two).  One thread per sample (grid-stride), every index from the reference's float64 colon element
// rule, tables read through L2: simple and exact rather than fast — this is one signal of twelve.
template <int MODE>
__global__ __launch_bounds__(kWG) void corr_epl_mixed_kernel(const KArgs p) {
  __shared__ double red[kWG / 64][GC_OUT_STRIDE];
  const long long lb = blockIdx.x / p.splits;
  const int split = (int)(blockIdx.x - lb * p.splits);
  const gc_block blk = p.blocks[lb];
  const DevChannel* __restrict__ chn = p.chans + blk.channel;
  const int arms = chn->arms;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double R = chn->index_scale, rem = blk.rem_code_phase, step = blk.code_phase_step, d = blk.el_spacing;
  const int N = blk.blksize;
  const Ramp64 ramp[3] = {ramp64(rem, -d, step, R, N), ramp64(rem, 0.0, step, R, N), ramp64(rem, d, step, R, N)};  // early, prompt, late
  const double tau = blk.carr_freq / p.fs;
  const double ph0 = blk.rem_carr_phase * 0.15915494309189535;
  const int per = (N + p.splits - 1) / p.splits;
  const int i_beg = split * per, i_end = min(N, i_beg + per);
  float acc[GC_OUT_STRIDE];
#pragma unroll
  for (int v = 0; v < GC_OUT_STRIDE; ++v) acc[v] = 0.f;
  for (int i = i_beg + tid; i < i_end; i += kWG) {
    float a, b;
    record_sample<MODE>(p.if_base, blk.first_sample + i, a, b);
    const double ph = ph0 + (double)i * tau;
    float sn, cs;
    sincospif(2.0f * (float)(ph - floor(ph)), &sn, &cs);
    const float xr = a * cs + b * sn, xi = b * cs - a * sn;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const double t = ramp[x].at(i);
      for (int ar = 0; ar < arms; ++ar) {
        const float c = (float)chn->tab[ar][code_index(t, chn->mult[ar], blk.table_offset[ar], chn->nent[ar] - 1)];
        acc[ar * 6 + 2 * x] = fmaf(c, xr, acc[ar * 6 + 2 * x]);
        acc[ar * 6 + 2 * x + 1] = fmaf(c, xi, acc[ar * 6 + 2 * x + 1]);
      }
    }
  }
#pragma unroll
  for (int v = 0; v < GC_OUT_STRIDE; ++v) {
    float x = acc[v];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) red[wave][v] = (double)x;
  }
  __syncthreads();
  if (tid < GC_OUT_STRIDE) {
    double sum = 0.0;
    for (int w = 0; w < kWG / 64; ++w) sum += red[w][tid];
    if (p.splits == 1)
      p.out[lb * GC_OUT_STRIDE + tid] = sum;
    else
      p.partial[(lb * p.splits + split) * GC_OUT_STRIDE + tid] = sum;
  }
}

__global__ void combine_partials_kernel(const double* __restrict__ partial, double* __restrict__ out,
                                        long long nblocks, int splits) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nblocks * GC_OUT_STRIDE) return;
  const long long lb = i / GC_OUT_STRIDE;
  const int v = (int)(i - lb * GC_OUT_STRIDE);
  double s = 0.0;
  for (int k = 0; k < splits; ++k) s += partial[(lb * splits + k) * GC_OUT_STRIDE + v];
  out[i] = s;
}

}  // namespace

int gc_launch_correlator(gc_context* ctx, const LaunchScope& s, const gc_block* d_blocks, int64_t nblocks, int splits,
                         double* d_out, double* d_partial, unsigned int notify_tag) {
  if (nblocks <= 0) return GC_OK;
  LaunchPlan plan;
  int rc = gc_plan_launch(ctx, s, nblocks, splits, notify_tag != 0, &plan);
  if (rc != GC_OK) return rc;
  ctx->last_kernel = plan.kernel;
  KArgs a;
  a.if_base = ctx->d_if;
  a.blocks = d_blocks;
  a.chans = ctx->d_channels;
  a.out = d_out;
  a.partial = d_partial;
  a.fs = ctx->fs;
  a.inv_fs = 1.0 / ctx->fs;
  a.nblocks = nblocks;
  a.splits = splits;
  a.xcd_swizzle = plan.xcd_swizzle;
  a.red_off = s.lds_bytes;
  a.bpw = plan.bpw;
  a.stride = plan.stride;
  InlineBlocks ib;
  a.tagged = nullptr;
  a.notify_tag = 0;
  a.use_inline = 0;
  a.devloop = nullptr;
  a.wide = plan.wide;
  a.total_wg = plan.total_wg;
  a.share_el = plan.share_el ? 1 : 0;
  a.derived = plan.derived ? 1 : 0;
  if (s.fast >= 0 && notify_tag != 0 && ctx->h_tagged_pinned) {
    // closed loop: d_blocks is the host-mapped descriptor buffer (readable by the host right here)
    a.tagged = reinterpret_cast<TaggedSlot*>(ctx->h_tagged_pinned);
    a.notify_tag = notify_tag;
    if (nblocks <= kInlineBlocks) {
      a.use_inline = 1;
      for (int64_t i = 0; i < nblocks; ++i) ib.b[i] = d_blocks[i];
    }
  }
  switch (plan.kernel) {
    case 6: rc = gc_launch_correlator_f64(ctx, d_blocks, nblocks, splits, d_out, d_partial); break;  // no tagged records: the caller reads d_out / d_partial after a synchronise
    case 5: return gc_launch_correlator_cboc(ctx, a, s, plan);
    case 4: return gc_launch_correlator_multi(ctx, a, s, plan);
    case 0: rc = gc_launch_correlator_lane(ctx, a, ib, s, plan); break;
    case -1: {  // mixed ramp multipliers: exact per-sample kernel
      const dim3 grid(plan.grid);
      gc_with_mode(gc_record_mode(ctx), [&](auto m) {
        hipLaunchKernelGGL((corr_epl_mixed_kernel<decltype(m)::value>), grid, dim3(kWG), 0, ctx->stream, a);
      });
      rc = (hipGetLastError() == hipSuccess) ? GC_OK : GC_E_HIP;
      break;
    }
    default: rc = gc_launch_correlator_fast(ctx, a, ib, s, plan); break;  // 1, 2, 3: single-wave, WIDE, float-table WIDE
  }
  if (rc != GC_OK) return rc;
  if (splits > 1 && d_out != nullptr) {
    const long long n = nblocks * GC_OUT_STRIDE;
    hipLaunchKernelGGL(combine_partials_kernel, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0,
                       ctx->stream, d_partial, d_out, (long long)nblocks, splits);
    GC_HIP(hipGetLastError());
  }
  return GC_OK;
}
