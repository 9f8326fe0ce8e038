// corr_bank.hip — gc_correlate_bank: the correlation function of a block at up to GC_BANK_MAX_TAPS code offsets.
//
// The E/P/L kernels pay per sample and tap.  Here the samples of a block are read, converted and carrier-mixed ONCE, and every
// tap then costs work per table entry its ramp crosses, not per sample (GPS L1 C/A at 18 Msps: 1 023 entries against 18 000
// samples):
//
//   work item   (block, chunk of kBankChunk consecutive samples), one workgroup of kBankWG threads each
//   phase A     the chunk's samples mixed with the carrier - phase ph0 + i * carrFreq / fs reduced in float64, float32 sincospi,
//               as the float32 correlators do - and their inclusive prefix sums P[0 .. n] left in LDS as float pairs.  The sums
//               restart at every chunk: |P| stays below the chunk's sum |x|, which keeps float32 cancellation at the 1e-8 level.
//   phase B     per (arm, tap) the replica index p(i) = ceil(fl(t_i * m_a)) is non-decreasing in i (t_i strictly increasing for
//               2^-16 <= step * R * m_a <= 1), so with k_lo = p(first), k_hi = p(last) and e(k) = the smallest sample whose
//               index is >= k
//                   sum_i c[p(i)] x_i = c[k_hi] * P[n] + sum_{k = k_lo + 1 .. k_hi} (c[k - 1] - c[k]) * P[e(k)]
//               (the transition form: one boundary per entry, none where neighbouring entries are equal).  A wavefront takes
//               an (arm, tap) pair at a time, its lanes the pair's entries.  e(k) is a candidate from a float64 division,
//               corrected with the element rule itself - down while sample e - 1 already has index >= k, up while sample e has
//               index < k - so it IS the per-sample definition's boundary, ties included.  t_i is the reference's float64 colon
//               element (corr_f64.hip, corr_kernel.hip: forwards from the start in the first half, backwards from the end in
//               the second, the mean in the middle).  Tables are read as int8 from device memory, periodically: index p reads
//               entry 1 + mod(p - 1, n - 2), and since the pads are the period (checked on the host) c[k - 1] is the entry before.
//   sums        float32 per chunk and (arm, tap) - lanes by fixed shuffles -, written as float64 partials and added over a
//               block's chunks in index order by bank_combine_kernel.  No atomics: the same input gives the same bits.
#include "bank_common.h"

using namespace gcorr;

namespace {

struct BankArgs {
  const uint8_t* if_base;
  const gc_block* blocks;
  const DevChannel* chans;
  const int32_t* chunk_base;  // [nblocks + 1]: chunks before block b
  const double* offsets;      // [ntaps] chips
  double* partial;            // [total chunks][arms][ntaps][2]
  double* out;                // [nblocks][arms][ntaps][2]
  double fs;
  int nblocks;
  int ntaps;
  int arms;  // arms of the partial / out layout: the most a channel of the call has
};

template <int MODE>
__global__ __launch_bounds__(kBankWG) void bank_chunk_kernel(const BankArgs p) {
  __shared__ float2 P[kBankChunk + 1];
  __shared__ float2 wsum[kBankWaves];
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

  // ---- phase A: mix, prefix sums --------------------------------------------------------------------------------------------
  const double tau = blk.carr_freq / p.fs;
  const double ph0 = blk.rem_carr_phase * 0.15915494309189535;
#pragma unroll
  for (int r = 0; r < kBankSPT; ++r) {
    const int li = r * kBankWG + tid;
    float2 x = make_float2(0.0f, 0.0f);
    if (li < n) {
      float a, b;
      bank_load_sample<MODE>(p.if_base, blk.first_sample + i0 + li, a, b);
      const double ph = ph0 + (double)(i0 + li) * tau;
      float sn, cs;
      sincospif(2.0f * (float)(ph - floor(ph)), &sn, &cs);
      x = make_float2(a * cs + b * sn, b * cs - a * sn);
    }
    P[li] = x;
  }
  __syncthreads();
  float2 s[kBankSPT];
#pragma unroll
  for (int q = 0; q < kBankSPT; ++q) {
    const float2 v = P[kBankSPT * tid + q];
    s[q] = q == 0 ? v : make_float2(s[q - 1].x + v.x, s[q - 1].y + v.y);
  }
  float2 incl = s[kBankSPT - 1];  // inclusive scan of the threads' totals over the wave, then the waves before in index order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ux = __shfl_up(incl.x, o, 64), uy = __shfl_up(incl.y, o, 64);
    if (lane >= o) {
      incl.x += ux;
      incl.y += uy;
    }
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();  // every thread has read its samples: P is rewritten in place, shifted by one
  // what precedes this thread's samples: the inclusive value of the lane below (no subtraction, no second rounding) and the waves before
  const float ex = __shfl_up(incl.x, 1, 64), ey = __shfl_up(incl.y, 1, 64);
  float2 before = lane == 0 ? make_float2(0.0f, 0.0f) : make_float2(ex, ey);
  float2 wbase = make_float2(0.0f, 0.0f);
  for (int w = 0; w < wave; ++w) {
    wbase.x += wsum[w].x;
    wbase.y += wsum[w].y;
  }
  before.x += wbase.x;
  before.y += wbase.y;
#pragma unroll
  for (int q = 0; q < kBankSPT; ++q) P[kBankSPT * tid + q + 1] = make_float2(before.x + s[q].x, before.y + s[q].y);
  if (tid == 0) P[0] = make_float2(0.0f, 0.0f);
  __syncthreads();

  // ---- phase B: a wavefront per (arm, tap) pair, a lane per table entry the chunk crosses --------------------------------------
  const int arms = chn->arms;
  const double R = chn->index_scale, rem = blk.rem_code_phase, step = blk.code_phase_step;
  const double nm1s = __dmul_rn((double)(N - 1), step);
  const int i_last = i0 + n - 1;
  double* __restrict__ prow = p.partial + (long long)item * p.arms * p.ntaps * 2;
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
    float2 acc = make_float2(0.0f, 0.0f);
    for (int k = k_lo + 1 + lane; k <= k_hi; k += 64) {
      int r = (k - 1) % L;
      if (r < 0) r += L;
      const int c_prev = tab[r], c_k = tab[r + 1];  // entries 1 + mod(k - 2, L) (= entry r: the pad is the period) and 1 + mod(k - 1, L)
      if (c_prev == c_k) continue;
      // the smallest sample with index >= k lies in (i0, i_last]: index(i0) < k <= index(i_last)
      const int e = rp.boundary(k, i0, i_last);
      const float d = (float)(c_prev - c_k);
      const float2 v = P[e - i0];
      acc.x = fmaf(d, v.x, acc.x);
      acc.y = fmaf(d, v.y, acc.y);
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
      acc.x += __shfl_down(acc.x, sh, 64);
      acc.y += __shfl_down(acc.y, sh, 64);
    }
    if (lane == 0) {
      int r = (k_hi - 1) % L;
      if (r < 0) r += L;
      const float c_end = (float)tab[r + 1];
      prow[2 * pair] = (double)fmaf(c_end, P[n].x, acc.x);
      prow[2 * pair + 1] = (double)fmaf(c_end, P[n].y, acc.y);
    }
  }
}

// out[b][arm][tap][c] = the block's chunk partials in chunk order; arms the block's channel does not have are zero.
__global__ void bank_combine_kernel(const BankArgs p) {
  const long long row = (long long)p.arms * p.ntaps * 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)p.nblocks * row) return;
  const int b = (int)(i / row);
  const int v = (int)(i - (long long)b * row);
  const int arm = v / (2 * p.ntaps);
  double s = 0.0;
  if (arm < p.chans[p.blocks[b].channel].arms)
    for (int q = p.chunk_base[b]; q < p.chunk_base[b + 1]; ++q) s += p.partial[(long long)q * row + v];
  p.out[i] = s;
}

}  // namespace

int gc_launch_correlator_bank(gc_context* ctx, const gc_block* d_blocks, int nblocks, const int32_t* d_chunk_base, int total_chunks,
                              int ntaps, const double* d_offsets, int arms, double* d_partial, double* d_out) {
  if (nblocks <= 0 || total_chunks <= 0) return GC_OK;
  BankArgs a;
  a.if_base = ctx->d_if;
  a.blocks = d_blocks;
  a.chans = ctx->d_channels;
  a.chunk_base = d_chunk_base;
  a.offsets = d_offsets;
  a.partial = d_partial;
  a.out = d_out;
  a.fs = ctx->fs;
  a.nblocks = nblocks;
  a.ntaps = ntaps;
  a.arms = arms;
  const dim3 grid((unsigned int)total_chunks), block(kBankWG);
  switch (bank_record_mode(ctx)) {
    case I8_IQ: hipLaunchKernelGGL(bank_chunk_kernel<I8_IQ>, grid, block, 0, ctx->stream, a); break;
    case I8_QI: hipLaunchKernelGGL(bank_chunk_kernel<I8_QI>, grid, block, 0, ctx->stream, a); break;
    case I16_IQ: hipLaunchKernelGGL(bank_chunk_kernel<I16_IQ>, grid, block, 0, ctx->stream, a); break;
    case I16_QI: hipLaunchKernelGGL(bank_chunk_kernel<I16_QI>, grid, block, 0, ctx->stream, a); break;
    case I8_REAL: hipLaunchKernelGGL(bank_chunk_kernel<I8_REAL>, grid, block, 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL(bank_chunk_kernel<I16_REAL>, grid, block, 0, ctx->stream, a); break;
  }
  GC_HIP(hipGetLastError());
  const long long nout = (long long)nblocks * arms * ntaps * 2;
  hipLaunchKernelGGL(bank_combine_kernel, dim3((unsigned int)((nout + 255) / 256)), dim3(256), 0, ctx->stream, a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

extern "C" int gc_correlate_bank(gc_context* ctx, int nblocks, const gc_block* blocks, int ntaps, const double* tap_offsets, double* out) {
  if (!ctx || nblocks < 0 || !tap_offsets || (nblocks > 0 && (!blocks || !out))) {
    gc_set_error("gc_correlate_bank: bad arguments");
    return GC_E_INVALID;
  }
  int arms = 1;
  int rc = bank_validate("gc_correlate_bank", ctx, nblocks, blocks, ntaps, tap_offsets, &arms);
  if (rc) return rc;
  if (nblocks == 0) return GC_OK;
  GC_HIP(hipSetDevice(ctx->device));
  if ((rc = gc_sync_channels(ctx))) return rc;
  const long long row = (long long)arms * ntaps * 2;  // doubles per chunk (partials) and per block (results)
  const long long max_chunks = std::max<long long>(1, std::min<long long>(kBankPartialBytes / (row * 8), 0x40000000LL));
  GcBuf& bblk = ctx->bank[gc_context::BANK_BLOCKS];
  GcBuf& btap = ctx->bank[gc_context::BANK_TAPS];
  GcBuf& bchk = ctx->bank[gc_context::BANK_CHUNKS];
  GcBuf& bpar = ctx->bank[gc_context::BANK_PARTIAL];
  GcBuf& bout = ctx->bank[gc_context::BANK_OUT];
  if (gc_buf_reserve(btap, sizeof(double) * GC_BANK_MAX_TAPS, false) != hipSuccess) {
    gc_set_error("gc_correlate_bank: device allocation failed");
    return GC_E_NOMEM;
  }
  GC_HIP(hipMemcpyAsync(btap.p, tap_offsets, sizeof(double) * (size_t)ntaps, hipMemcpyHostToDevice, ctx->stream));
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
      gc_set_error("gc_correlate_bank: device allocation failed (%d blocks, %lld chunks, %d taps)", nb, chunks, ntaps);
      return GC_E_NOMEM;
    }
    GC_HIP(hipMemcpyAsync(bblk.p, blocks + first, sizeof(gc_block) * (size_t)nb, hipMemcpyHostToDevice, ctx->stream));
    GC_HIP(hipMemcpyAsync(bchk.p, base.data(), sizeof(int32_t) * (size_t)(nb + 1), hipMemcpyHostToDevice, ctx->stream));
    rc = gc_launch_correlator_bank(ctx, (const gc_block*)bblk.p, nb, (const int32_t*)bchk.p, (int)chunks, ntaps, (const double*)btap.p, arms,
                                   (double*)bpar.p, (double*)bout.p);
    if (rc) return rc;
    double* dst = out + (size_t)first * GC_MAX_ARMS * ntaps * 2;
    if (arms == GC_MAX_ARMS) {
      GC_HIP(hipMemcpyAsync(dst, bout.p, sizeof(double) * (size_t)(nb * row), hipMemcpyDeviceToHost, ctx->stream));
      GC_HIP(hipStreamSynchronize(ctx->stream));
    } else {  // the device rows hold the call's arms only: the others are zero on the host's side
      compact.resize((size_t)(nb * row));
      GC_HIP(hipMemcpyAsync(compact.data(), bout.p, sizeof(double) * compact.size(), hipMemcpyDeviceToHost, ctx->stream));
      GC_HIP(hipStreamSynchronize(ctx->stream));
      for (int b = 0; b < nb; ++b) {
        double* o = dst + (size_t)b * GC_MAX_ARMS * ntaps * 2;
        std::memcpy(o, compact.data() + (size_t)b * row, sizeof(double) * (size_t)row);
        std::memset(o + row, 0, sizeof(double) * (size_t)(GC_MAX_ARMS * ntaps * 2 - row));
      }
    }
    first += nb;
  }
  return GC_OK;
}
