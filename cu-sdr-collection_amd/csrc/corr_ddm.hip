// corr_ddm.hip — gc_correlate_ddm: a block's correlation at up to GC_BANK_MAX_TAPS code offsets and up to GC_DDM_MAX_FREQS
// carrier offsets (a delay-Doppler map).
//
// Defined as an identity: bin m of a block is what gc_correlate_bank (corr_bank.hip) returns for the block with carr_freq
// replaced by the float64 sum carr_freq + freq_offsets[m], bit for bit.  So every expression below is the bank's, in the bank's
// order (bank_common.h holds what the two files share); what differs is what is computed ONCE for several bins:
//
//   work item   (block, chunk of kBankChunk samples, group of kDdmGroup consecutive bins), one workgroup of kBankWG threads.
//               The chunk is the bank's: its prefix sums restart there, so the chunk size is part of the identity.
//   phase A     a thread's kBankSPT consecutive samples are loaded and converted once and stay in registers.  Per bin of the
//               group: phase ph0 + i * tau_m reduced in float64 (tau_m = (carr_freq + f_m) / fs), float32 sincospi, the two
//               products, the thread's running sums, the wave's shuffle scan - the values and the order of the bank's scan,
//               which reads the mixed samples back from LDS where this one has them in registers.  No rotation recurrence across
//               samples or bins: either would make a bin depend on its neighbours.  P_g[0 .. n] per bin in LDS.
//   phase B     a wavefront per (arm, tap) pair, a lane per table entry, as in the bank.  The entry's two table values, their
//               comparison and the boundary e(k) - the float64 search that is the expensive part of a tap - do not depend on
//               the carrier: computed once, then one read of P_g[e - i0] and two fmaf per bin.  The bank's shuffle tree and
//               closing fmaf(c_end, P_g[n], acc) per bin.
//   sums        float64 partials [chunk][arm][bin][tap][2], added over a block's chunks in index order by ddm_combine_kernel.
//               No atomics.
#include "bank_common.h"

using namespace gcorr;

// Bins per work item: kDdmGroup * (kBankChunk + 1) float2 of LDS (4: 32.9 KB, four workgroups per CU).  Measured at 4, 8 and 16
// (DESIGN.md 4.7): the smallest group won - phase A, per bin whatever the group, wants the waves the LDS leaves room for more than
// phase B wants its boundaries shared further.  A throw-away build sets another value (scripts/ddm_timing.py).
#ifndef GC_DDM_GROUP
#define GC_DDM_GROUP 4
#endif

namespace {

constexpr int kDdmGroup = GC_DDM_GROUP;
static_assert(kDdmGroup >= 1 && kDdmGroup * (kBankChunk + 1) * 8 + kDdmGroup * kBankWaves * 8 <= 160 * 1024, "a workgroup's LDS");

struct DdmArgs {
  const uint8_t* if_base;
  const gc_block* blocks;
  const DevChannel* chans;
  const int32_t* chunk_base;  // [nblocks + 1]: chunks before block b
  const double* offsets;      // [ntaps] chips
  const double* freqs;        // [nfreq] Hz
  double* partial;            // [total chunks][arms][nfreq][ntaps][2]
  double* out;                // [nblocks][arms][nfreq][ntaps][2]
  double fs;
  int nblocks;
  int ntaps;
  int nfreq;
  int arms;  // arms of the partial / out layout: the most a channel of the call has
};

template <int MODE>
__global__ __launch_bounds__(kBankWG) void ddm_chunk_kernel(const DdmArgs p) {
  __shared__ float2 P[kDdmGroup][kBankChunk + 1];
  __shared__ float2 wsum[kDdmGroup][kBankWaves];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the block this chunk belongs to: the last b with chunk_base[b] <= blockIdx.x (uniform)
  const int item = (int)blockIdx.x;
  int lo = 0, hi = p.nblocks;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.chunk_base[mid] <= item) lo = mid;
    else hi = mid;
  }
  const gc_block blk = p.blocks[lo];
  const DevChannel* __restrict__ chn = p.chans + blk.channel;
  const int N = blk.blksize;
  const int i0 = (item - p.chunk_base[lo]) * kBankChunk;
  const int n = min(kBankChunk, N - i0);  // 1 .. kBankChunk samples in this chunk
  const int m0 = (int)blockIdx.y * kDdmGroup;
  const int gn = min(kDdmGroup, p.nfreq - m0);  // 1 .. kDdmGroup bins in this group (uniform)

  // ---- phase A: the thread's samples once, then per bin mix and prefix sums -------------------------------------------------
  float xa[kBankSPT], xb[kBankSPT];
#pragma unroll
  for (int q = 0; q < kBankSPT; ++q) {
    const int li = kBankSPT * tid + q;
    xa[q] = 0.0f;
    xb[q] = 0.0f;
    if (li < n) bank_load_sample<MODE>(p.if_base, blk.first_sample + i0 + li, xa[q], xb[q]);
  }
  const double ph0 = blk.rem_carr_phase * 0.15915494309189535;
  float2 s[kDdmGroup][kBankSPT];
  float2 before[kDdmGroup];
#pragma unroll
  for (int g = 0; g < kDdmGroup; ++g) {
    if (g < gn) {
      const double tau = __dadd_rn(blk.carr_freq, p.freqs[m0 + g]) / p.fs;
#pragma unroll
      for (int q = 0; q < kBankSPT; ++q) {
        const int li = kBankSPT * tid + q;
        float2 x = make_float2(0.0f, 0.0f);
        if (li < n) {
          const float a = xa[q], b = xb[q];
          const double ph = ph0 + (double)(i0 + li) * tau;
          float sn, cs;
          sincospif(2.0f * (float)(ph - floor(ph)), &sn, &cs);
          x = make_float2(a * cs + b * sn, b * cs - a * sn);
        }
        s[g][q] = q == 0 ? x : make_float2(s[g][q - 1].x + x.x, s[g][q - 1].y + x.y);
      }
      float2 incl = s[g][kBankSPT - 1];  // inclusive scan of the threads' totals over the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float ux = __shfl_up(incl.x, o, 64), uy = __shfl_up(incl.y, o, 64);
        if (lane >= o) {
          incl.x += ux;
          incl.y += uy;
        }
      }
      if (lane == 63) wsum[g][wave] = incl;
      // what precedes this thread's samples in its wave: the inclusive value of the lane below
      const float ex = __shfl_up(incl.x, 1, 64), ey = __shfl_up(incl.y, 1, 64);
      before[g] = lane == 0 ? make_float2(0.0f, 0.0f) : make_float2(ex, ey);
    }
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < kDdmGroup; ++g) {
    if (g < gn) {
      float2 wbase = make_float2(0.0f, 0.0f);  // the waves before, in index order
      for (int w = 0; w < wave; ++w) {
        wbase.x += wsum[g][w].x;
        wbase.y += wsum[g][w].y;
      }
      float2 bf = before[g];
      bf.x += wbase.x;
      bf.y += wbase.y;
#pragma unroll
      for (int q = 0; q < kBankSPT; ++q) P[g][kBankSPT * tid + q + 1] = make_float2(bf.x + s[g][q].x, bf.y + s[g][q].y);
      if (tid == 0) P[g][0] = make_float2(0.0f, 0.0f);
    }
  }
  __syncthreads();

  // ---- phase B: a wavefront per (arm, tap) pair, a lane per table entry the chunk crosses; every boundary once for the group ----
  const int arms = chn->arms;
  const double R = chn->index_scale, rem = blk.rem_code_phase, step = blk.code_phase_step;
  const double nm1s = __dmul_rn((double)(N - 1), step);
  const int i_last = i0 + n - 1;
  double* __restrict__ prow = p.partial + (long long)item * p.arms * p.nfreq * p.ntaps * 2;
  for (int pair = wave; pair < arms * p.ntaps; pair += kBankWaves) {
    const int arm = pair / p.ntaps, j = pair - arm * p.ntaps;
    const double o = p.offsets[j];
    BankRamp rp;
    rp.a = __dmul_rn(__dadd_rn(rem, o), R);
    rp.b = __dmul_rn(__dadd_rn(__dadd_rn(nm1s, rem), o), R);
    rp.sp = __dmul_rn(step, R);
    rp.m = chn->mult[arm];
    rp.N = N;
    const int8_t* __restrict__ tab = chn->tab[arm];
    const int L = chn->nent[arm] - 2;  // the code's period in entries
    const int k_lo = rp.index(i0), k_hi = rp.index(i_last);
    float2 acc[kDdmGroup];
#pragma unroll
    for (int g = 0; g < kDdmGroup; ++g) acc[g] = make_float2(0.0f, 0.0f);
    for (int k = k_lo + 1 + lane; k <= k_hi; k += 64) {
      int r = (k - 1) % L;
      if (r < 0) r += L;
      const int c_prev = tab[r], c_k = tab[r + 1];  // entries 1 + mod(k - 2, L) (= entry r: the pad is the period) and 1 + mod(k - 1, L)
      if (c_prev == c_k) continue;
      const int e = rp.boundary(k, i0, i_last);
      const float d = (float)(c_prev - c_k);
#pragma unroll
      for (int g = 0; g < kDdmGroup; ++g) {
        if (g < gn) {
          const float2 v = P[g][e - i0];
          acc[g].x = fmaf(d, v.x, acc[g].x);
          acc[g].y = fmaf(d, v.y, acc[g].y);
        }
      }
    }
    int r = (k_hi - 1) % L;
    if (r < 0) r += L;
    const float c_end = (float)tab[r + 1];
#pragma unroll
    for (int g = 0; g < kDdmGroup; ++g) {
      if (g < gn) {
        float2 a = acc[g];
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) {
          a.x += __shfl_down(a.x, sh, 64);
          a.y += __shfl_down(a.y, sh, 64);
        }
        if (lane == 0) {
          double* dst = prow + 2 * (((long long)arm * p.nfreq + m0 + g) * p.ntaps + j);
          dst[0] = (double)fmaf(c_end, P[g][n].x, a.x);
          dst[1] = (double)fmaf(c_end, P[g][n].y, a.y);
        }
      }
    }
  }
}

// out[b][arm][bin][tap][c] = the block's chunk partials in chunk order; arms the block's channel does not have are zero.
__global__ void ddm_combine_kernel(const DdmArgs p) {
  const long long row = (long long)p.arms * p.nfreq * p.ntaps * 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)p.nblocks * row) return;
  const int b = (int)(i / row);
  const int v = (int)(i - (long long)b * row);
  const int arm = v / (2 * p.nfreq * p.ntaps);
  double s = 0.0;
  if (arm < p.chans[p.blocks[b].channel].arms)
    for (int q = p.chunk_base[b]; q < p.chunk_base[b + 1]; ++q) s += p.partial[(long long)q * row + v];
  p.out[i] = s;
}

int ddm_launch(gc_context* ctx, const DdmArgs& a, int total_chunks) {
  const dim3 grid((unsigned int)total_chunks, (unsigned int)((a.nfreq + kDdmGroup - 1) / kDdmGroup)), block(kBankWG);
  switch (bank_record_mode(ctx)) {
    case I8_IQ: hipLaunchKernelGGL(ddm_chunk_kernel<I8_IQ>, grid, block, 0, ctx->stream, a); break;
    case I8_QI: hipLaunchKernelGGL(ddm_chunk_kernel<I8_QI>, grid, block, 0, ctx->stream, a); break;
    case I16_IQ: hipLaunchKernelGGL(ddm_chunk_kernel<I16_IQ>, grid, block, 0, ctx->stream, a); break;
    case I16_QI: hipLaunchKernelGGL(ddm_chunk_kernel<I16_QI>, grid, block, 0, ctx->stream, a); break;
    case I8_REAL: hipLaunchKernelGGL(ddm_chunk_kernel<I8_REAL>, grid, block, 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL(ddm_chunk_kernel<I16_REAL>, grid, block, 0, ctx->stream, a); break;
  }
  GC_HIP(hipGetLastError());
  const long long nout = (long long)a.nblocks * a.arms * a.nfreq * a.ntaps * 2;
  hipLaunchKernelGGL(ddm_combine_kernel, dim3((unsigned int)((nout + 255) / 256)), dim3(256), 0, ctx->stream, a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

}  // namespace

extern "C" int gc_correlate_ddm(gc_context* ctx, int nblocks, const gc_block* blocks, int ntaps, const double* tap_offsets, int nfreq,
                                const double* freq_offsets, double* out) {
  if (!ctx || nblocks < 0 || !tap_offsets || !freq_offsets || (nblocks > 0 && (!blocks || !out))) {
    gc_set_error("gc_correlate_ddm: bad arguments");
    return GC_E_INVALID;
  }
  if (nfreq < 1 || nfreq > GC_DDM_MAX_FREQS) {
    gc_set_error("gc_correlate_ddm: %d frequency bins (1 .. %d)", nfreq, GC_DDM_MAX_FREQS);
    return GC_E_INVALID;
  }
  for (int m = 0; m < nfreq; ++m)
    if (!std::isfinite(freq_offsets[m])) {
      gc_set_error("gc_correlate_ddm: frequency offset %d is not finite", m);
      return GC_E_INVALID;
    }
  int arms = 1;
  int rc = bank_validate("gc_correlate_ddm", ctx, nblocks, blocks, ntaps, tap_offsets, &arms);
  if (rc) return rc;
  if (nblocks == 0) return GC_OK;
  for (int i = 0; i < nblocks; ++i)
    for (int m = 0; m < nfreq; ++m)
      if (!std::isfinite(blocks[i].carr_freq + freq_offsets[m])) {  // what the bank answers to that carr_freq
        gc_set_error("block %d: invalid descriptor (carr_freq + frequency offset %d is not finite)", i, m);
        return GC_E_INVALID;
      }
  GC_HIP(hipSetDevice(ctx->device));
  if ((rc = gc_sync_channels(ctx))) return rc;
  const long long row = (long long)arms * nfreq * ntaps * 2;  // doubles per chunk (partials) and per block (results)
  const long long full = (long long)GC_MAX_ARMS * nfreq * ntaps * 2;
  const long long max_chunks = std::max<long long>(1, std::min<long long>(kBankPartialBytes / (row * 8), 0x40000000LL));
  // the bank's scratch: the two calls never overlap on a context
  GcBuf& bblk = ctx->bank[gc_context::BANK_BLOCKS];
  GcBuf& btap = ctx->bank[gc_context::BANK_TAPS];
  GcBuf& bfrq = ctx->bank[gc_context::BANK_FREQS];
  GcBuf& bchk = ctx->bank[gc_context::BANK_CHUNKS];
  GcBuf& bpar = ctx->bank[gc_context::BANK_PARTIAL];
  GcBuf& bout = ctx->bank[gc_context::BANK_OUT];
  if (gc_buf_reserve(btap, sizeof(double) * GC_BANK_MAX_TAPS, false) != hipSuccess ||
      gc_buf_reserve(bfrq, sizeof(double) * GC_DDM_MAX_FREQS, false) != hipSuccess) {
    gc_set_error("gc_correlate_ddm: device allocation failed");
    return GC_E_NOMEM;
  }
  GC_HIP(hipMemcpyAsync(btap.p, tap_offsets, sizeof(double) * (size_t)ntaps, hipMemcpyHostToDevice, ctx->stream));
  GC_HIP(hipMemcpyAsync(bfrq.p, freq_offsets, sizeof(double) * (size_t)nfreq, hipMemcpyHostToDevice, ctx->stream));
  std::vector<int32_t> base;
  std::vector<double> compact;
  for (int first = 0; first < nblocks;) {
    // the sub-batch: blocks from `first` while their chunks' partial sums fit (one block at least)
    base.assign(1, 0);
    int nb = 0;
    while (first + nb < nblocks) {
      const long long c = ((long long)blocks[first + nb].blksize + kBankChunk - 1) / kBankChunk;
      if (nb > 0 && base.back() + c > max_chunks) break;
      base.push_back((int32_t)(base.back() + c));
      ++nb;
    }
    const long long chunks = base.back();
    if (gc_buf_reserve(bblk, sizeof(gc_block) * (size_t)nb, false) != hipSuccess ||
        gc_buf_reserve(bchk, sizeof(int32_t) * (size_t)(nb + 1), false) != hipSuccess ||
        gc_buf_reserve(bpar, sizeof(double) * (size_t)(chunks * row), false) != hipSuccess ||
        gc_buf_reserve(bout, sizeof(double) * (size_t)(nb * row), false) != hipSuccess) {
      gc_set_error("gc_correlate_ddm: device allocation failed (%d blocks, %lld chunks, %d taps, %d bins)", nb, chunks, ntaps, nfreq);
      return GC_E_NOMEM;
    }
    GC_HIP(hipMemcpyAsync(bblk.p, blocks + first, sizeof(gc_block) * (size_t)nb, hipMemcpyHostToDevice, ctx->stream));
    GC_HIP(hipMemcpyAsync(bchk.p, base.data(), sizeof(int32_t) * (size_t)(nb + 1), hipMemcpyHostToDevice, ctx->stream));
    DdmArgs a;
    a.if_base = ctx->d_if;
    a.blocks = (const gc_block*)bblk.p;
    a.chans = ctx->d_channels;
    a.chunk_base = (const int32_t*)bchk.p;
    a.offsets = (const double*)btap.p;
    a.freqs = (const double*)bfrq.p;
    a.partial = (double*)bpar.p;
    a.out = (double*)bout.p;
    a.fs = ctx->fs;
    a.nblocks = nb;
    a.ntaps = ntaps;
    a.nfreq = nfreq;
    a.arms = arms;
    if ((rc = ddm_launch(ctx, a, (int)chunks))) return rc;
    double* dst = out + (size_t)first * full;
    if (arms == GC_MAX_ARMS) {
      GC_HIP(hipMemcpyAsync(dst, bout.p, sizeof(double) * (size_t)(nb * row), hipMemcpyDeviceToHost, ctx->stream));
      GC_HIP(hipStreamSynchronize(ctx->stream));
    } else {  // the device rows hold the call's arms only: the others are zero on the host's side
      compact.resize((size_t)(nb * row));
      GC_HIP(hipMemcpyAsync(compact.data(), bout.p, sizeof(double) * compact.size(), hipMemcpyDeviceToHost, ctx->stream));
      GC_HIP(hipStreamSynchronize(ctx->stream));
      for (int b = 0; b < nb; ++b) {
        double* o = dst + (size_t)b * full;
        std::memcpy(o, compact.data() + (size_t)b * row, sizeof(double) * (size_t)row);
        std::memset(o + row, 0, sizeof(double) * (size_t)(full - row));
      }
    }
    first += nb;
  }
  return GC_OK;
}
