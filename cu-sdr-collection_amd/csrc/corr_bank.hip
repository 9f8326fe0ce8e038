// corr_bank.hip — gc_correlate_bank: the correlation function of a block at up to GC_BANK_MAX_TAPS code offsets,
// gc_correlate_ddm: the same at up to GC_DDM_MAX_FREQS carrier offsets as well (a delay-Doppler map), and
// gc_correlate_ddm_integrate: those maps added coherently over runs of blocks, then as power over runs, where the chunk partials are,
// and gc_correlate_ddm_search: that integration under many hypotheses (shifts of the run grid, weight rows) from one chunk pass, every
// map's peak picked on the device (their kernels and drivers: the last two parts of this file).
//
// The DDM is defined as an identity: bin m of a block is what the bank returns for the block with carr_freq replaced by the
// float64 sum carr_freq + freq_offsets[m], bit for bit.  The code says so: one chunk kernel over (record format, G bins per work
// item), one combine kernel, one host driver.  The bank is G = 1 with no frequency offsets (none is added: -0.0 + 0.0 is +0.0);
// the DDM is G = GC_DDM_GROUP.
//
// The E/P/L kernels pay per sample and tap.  Here the samples of a block are read and converted ONCE, carrier-mixed once per bin,
// and every tap then costs work per table entry its ramp crosses, not per sample (GPS L1 C/A at 18 Msps: 1 023 entries against
// 18 000 samples):
//
//   work item   (block, chunk of kBankChunk consecutive samples, group of G consecutive bins), one workgroup of kBankWG threads
//   phase A     a thread's kBankSPT consecutive samples are loaded and converted once and stay in registers.  Per bin of the
//               group: phase ph0 + i * tau reduced in float64 (tau = carr_freq / fs, or (carr_freq + f_m) / fs), float32 sincospi
//               as the float32 correlators do, the two products, the thread's running sums, the wave's shuffle scan, the waves
//               before in index order: the inclusive prefix sums P_g[0 .. n] left in LDS as float pairs.  The sums restart at
//               every chunk: |P| stays below the chunk's sum |x|, which keeps float32 cancellation at the 1e-8 level - so the
//               chunk size is part of the identity.  No rotation recurrence across samples or bins: either would make a bin
//               depend on its neighbours.
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
//               The entry's two table values, their comparison and e(k) - the float64 search that is the expensive part of a
//               tap - do not depend on the carrier: computed once, then one read of P_g[e - i0] and two fmaf per bin.
//   sums        per chunk and (arm, bin, tap) over the float32 P values, a lane's terms in float64, the lanes by fixed shuffles - in
//               float64 too where the chunk crosses more than 64 entries, else in float32 -, written as float64 partials
//               [chunk][arm][bin][tap][2] and added over a block's chunks in index order by bank_combine_kernel.  No atomics:
//               the same input gives the same bits.
#include <cstring>

#include "bank_plan.h"
#include "replica_f64.h"

using namespace gcorr;

// Bins per work item of the DDM: G * (kBankChunk + 1) float2 of LDS (4: 32.9 KB, four workgroups per CU).  Measured at 4, 8 and 16
// (DESIGN.md 4.7): the smallest group won - phase A, per bin whatever the group, wants the waves the LDS leaves room for more than
// phase B wants its boundaries shared further.  A throw-away build sets another value (scripts/ddm_timing.py).
#ifndef GC_DDM_GROUP
#define GC_DDM_GROUP 4
#endif

namespace {

constexpr int kBankWG = 256;      // threads per workgroup: kBankChunk / kBankWG consecutive samples per thread in the prefix sums
constexpr int kBankSPT = kBankChunk / kBankWG;
constexpr int kBankWaves = kBankWG / 64;

// One (arm, tap) ramp of a block: the reference's colon element i and its table index (replica_f64.h).
struct BankRamp {
  Ramp64 r;
  double m;
  __device__ __forceinline__ int index(int i) const { return code_step(r.at(i), m); }
  // e(k): the smallest sample of the chunk [i0, i_last] whose index is >= k, for index(i0) < k <= index(i_last) - it lies in
  // (i0, i_last].  A candidate from a float64 division, corrected with the element rule itself: down while sample e - 1 already
  // has index >= k, up while sample e has index < k.
  __device__ __forceinline__ int boundary(int k, int i0, int i_last) const {
    const double x = ((double)(k - 1) / m - r.a) / r.sp;
    int e = (int)fmin(fmax(floor(x) + 1.0, (double)(i0 + 1)), (double)i_last);
    while (e > i0 + 1 && index(e - 1) >= k) --e;
    while (e < i_last && index(e) < k) ++e;
    return e;
  }
};

constexpr int kDdmGroup = GC_DDM_GROUP;
static_assert(kDdmGroup >= 1 && kDdmGroup * (kBankChunk + 1) * 8 + kDdmGroup * kBankWaves * 8 <= 160 * 1024, "a workgroup's LDS");

struct BankArgs {
  const uint8_t* if_base;
  const gc_block* blocks;
  const DevChannel* chans;
  const int32_t* chunk_base;  // [nblocks + 1]: chunks before block b
  const double* offsets;      // [ntaps] chips
  const double* freqs;        // [nfreq] Hz; nullptr (the bank): one bin at carr_freq as given, nothing added
  double* partial;            // [total chunks][arms][nfreq][ntaps][2]
  double* out;                // [nblocks][arms][nfreq][ntaps][2]
  double fs;
  int nblocks;
  int ntaps;
  int nfreq;
  int arms;  // arms of the partial / out layout: the most a channel of the call has
};

template <int MODE, int G>
__global__ __launch_bounds__(kBankWG) void bank_chunk_kernel(const BankArgs p) {
  __shared__ float2 P[G][kBankChunk + 1];
  __shared__ float2 wsum[G][kBankWaves];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  // uniform over the wavefront, which the compiler cannot prove by itself: with it phase B's per-pair values and branches are scalar
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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
  const int m0 = (int)blockIdx.y * G;
  const int gn = min(G, p.nfreq - m0);  // 1 .. G bins in this group (uniform)

  // ---- phase A: the thread's samples once, then per bin mix and prefix sums -------------------------------------------------
  // (Loading at stride kBankWG through LDS instead, as the bank did while it had a kernel of its own, gives the same values in
  // the same order and the same times: DESIGN.md 4.6 "compared across the move".)
  float xa[kBankSPT], xb[kBankSPT];
#pragma unroll
  for (int q = 0; q < kBankSPT; ++q) {
    const int li = kBankSPT * tid + q;
    xa[q] = 0.0f;
    xb[q] = 0.0f;
    if (li < n) record_sample<MODE>(p.if_base, blk.first_sample + i0 + li, xa[q], xb[q]);
  }
  const double ph0 = blk.rem_carr_phase * 0.15915494309189535;
  float2 s[G][kBankSPT];
  float2 before[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g < gn) {
      const double tau = (p.freqs ? __dadd_rn(blk.carr_freq, p.freqs[m0 + g]) : blk.carr_freq) / p.fs;
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
      // what precedes this thread's samples in its wave: the inclusive value of the lane below (no subtraction, no second rounding)
      const float ex = __shfl_up(incl.x, 1, 64), ey = __shfl_up(incl.y, 1, 64);
      before[g] = lane == 0 ? make_float2(0.0f, 0.0f) : make_float2(ex, ey);
    }
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < G; ++g) {
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
  const int i_last = i0 + n - 1;
  double* __restrict__ prow = p.partial + (long long)item * p.arms * p.nfreq * p.ntaps * 2;
  for (int pair = wave; pair < arms * p.ntaps; pair += kBankWaves) {
    const int arm = pair / p.ntaps, j = pair - arm * p.ntaps;
    const BankRamp rp = {ramp64(rem, p.offsets[j], step, R, N), chn->mult[arm]};
    const int8_t* __restrict__ tab = chn->tab[arm];
    const int L = chn->nent[arm] - 2;  // the code's period in entries
    const int k_lo = rp.index(i0), k_hi = rp.index(i_last);
    // A lane's terms add in float64.  The lanes of a pair take every 64th entry, so on a table that alternates (BOC(6,1): a
    // transition at every entry) a lane's terms all have one sign and add up to ten times |P|, and the lanes' totals alternate: in
    // float32 throughout that cost 2.4e-6 of sum |x| on a 1 024-sample block of an int16 record (tests/test_gpu_bank_edges.py).
    // Where the chunk crosses at most 64 entries (GPS L1 C/A at 18 Msps: 58) a lane holds at most one product, the same number in
    // either format, and the lanes are then added in float32, as they were while all of phase B was float32: the same bits.
    const bool one_pass = k_hi - k_lo <= 64;  // uniform over the wavefront
    double2 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = make_double2(0.0, 0.0);
    for (int k = k_lo + 1 + lane; k <= k_hi; k += 64) {
      int r = (k - 1) % L;
      if (r < 0) r += L;
      const int c_prev = tab[r], c_k = tab[r + 1];  // entries 1 + mod(k - 2, L) (= entry r: the pad is the period) and 1 + mod(k - 1, L)
      if (c_prev == c_k) continue;
      // the smallest sample with index >= k lies in (i0, i_last]: index(i0) < k <= index(i_last)
      const int e = rp.boundary(k, i0, i_last);
      const double d = (double)(c_prev - c_k);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (g < gn) {
          const float2 v = P[g][e - i0];
          acc[g].x = fma(d, (double)v.x, acc[g].x);
          acc[g].y = fma(d, (double)v.y, acc[g].y);
        }
      }
    }
    int r = (k_hi - 1) % L;
    if (r < 0) r += L;
    const double c_end = (double)tab[r + 1];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (g < gn) {
        double* dst = prow + 2 * (((long long)arm * p.nfreq + m0 + g) * p.ntaps + j);
        if (one_pass) {
          float2 a = make_float2((float)acc[g].x, (float)acc[g].y);
#pragma unroll
          for (int sh = 32; sh > 0; sh >>= 1) {
            a.x += __shfl_down(a.x, sh, 64);
            a.y += __shfl_down(a.y, sh, 64);
          }
          if (lane == 0) {
            dst[0] = (double)fmaf((float)c_end, P[g][n].x, a.x);
            dst[1] = (double)fmaf((float)c_end, P[g][n].y, a.y);
          }
        } else {
          double2 a = acc[g];
#pragma unroll
          for (int sh = 32; sh > 0; sh >>= 1) {
            a.x += __shfl_down(a.x, sh, 64);
            a.y += __shfl_down(a.y, sh, 64);
          }
          if (lane == 0) {
            dst[0] = fma(c_end, (double)P[g][n].x, a.x);
            dst[1] = fma(c_end, (double)P[g][n].y, a.y);
          }
        }
      }
    }
  }
}

// out[b][arm][bin][tap][c] = the block's chunk partials in chunk order; arms the block's channel does not have are zero.
__global__ void bank_combine_kernel(const BankArgs p) {
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

// The chunk kernel over `total_chunks` work items and the groups of G bins.
template <int G>
int bank_launch_chunks(gc_context* ctx, const BankArgs& a, int total_chunks) {
  const dim3 grid((unsigned int)total_chunks, (unsigned int)((a.nfreq + G - 1) / G)), block(kBankWG);
  gc_with_mode(gc_record_mode(ctx), [&](auto m) {
    hipLaunchKernelGGL((bank_chunk_kernel<decltype(m)::value, G>), grid, block, 0, ctx->stream, a);
  });
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ---- what gc_correlate_bank / gc_correlate_ddm (bank_run) and gc_correlate_ddm_integrate (ddm_integrate_run) share ------------------

// The channels, the tap offsets and the frequency offsets on the device.
int bank_upload_grids(const char* fn, gc_context* ctx, int ntaps, const double* tap_offsets, int nfreq, const double* freq_offsets) {
  GC_HIP(hipSetDevice(ctx->device));
  int rc = gc_sync_channels(ctx);
  if (rc) return rc;
  GcBuf& btap = ctx->bank[gc_context::BANK_TAPS];
  GcBuf& bfrq = ctx->bank[gc_context::BANK_FREQS];
  if (gc_buf_reserve(btap, sizeof(double) * GC_BANK_MAX_TAPS, false) != hipSuccess ||
      (freq_offsets && gc_buf_reserve(bfrq, sizeof(double) * GC_DDM_MAX_FREQS, false) != hipSuccess)) {
    gc_set_error("%s: device allocation failed", fn);
    return GC_E_NOMEM;
  }
  GC_HIP(hipMemcpyAsync(btap.p, tap_offsets, sizeof(double) * (size_t)ntaps, hipMemcpyHostToDevice, ctx->stream));
  if (freq_offsets) GC_HIP(hipMemcpyAsync(bfrq.p, freq_offsets, sizeof(double) * (size_t)nfreq, hipMemcpyHostToDevice, ctx->stream));
  return GC_OK;
}

int bank_nomem(const char* fn, bool ddm, int nb, long long chunks, int ntaps, int nfreq) {
  if (ddm) gc_set_error("%s: device allocation failed (%d blocks, %lld chunks, %d taps, %d bins)", fn, nb, chunks, ntaps, nfreq);
  else gc_set_error("%s: device allocation failed (%d blocks, %lld chunks, %d taps)", fn, nb, chunks, ntaps);
  return GC_E_NOMEM;
}

// A sub-batch's descriptors and chunk index to the device, room for its partial sums, and the chunk kernel.  *a: the arguments the
// kernels after it take (`out` is the caller's to set).
int bank_chunks(const char* fn, gc_context* ctx, const gc_block* blocks, int nb, const std::vector<int32_t>& base, int ntaps, int nfreq,
                bool ddm, int arms, BankArgs* a) {
  const long long row = (long long)arms * nfreq * ntaps * 2, chunks = base.back();
  GcBuf& bblk = ctx->bank[gc_context::BANK_BLOCKS];
  GcBuf& bchk = ctx->bank[gc_context::BANK_CHUNKS];
  GcBuf& bpar = ctx->bank[gc_context::BANK_PARTIAL];
  if (gc_buf_reserve(bblk, sizeof(gc_block) * (size_t)nb, false) != hipSuccess ||
      gc_buf_reserve(bchk, sizeof(int32_t) * (size_t)(nb + 1), false) != hipSuccess ||
      gc_buf_reserve(bpar, sizeof(double) * (size_t)(chunks * row), false) != hipSuccess)
    return bank_nomem(fn, ddm, nb, chunks, ntaps, nfreq);
  GC_HIP(hipMemcpyAsync(bblk.p, blocks, sizeof(gc_block) * (size_t)nb, hipMemcpyHostToDevice, ctx->stream));
  GC_HIP(hipMemcpyAsync(bchk.p, base.data(), sizeof(int32_t) * (size_t)(nb + 1), hipMemcpyHostToDevice, ctx->stream));
  a->if_base = ctx->d_if;
  a->blocks = (const gc_block*)bblk.p;
  a->chans = ctx->d_channels;
  a->chunk_base = (const int32_t*)bchk.p;
  a->offsets = (const double*)ctx->bank[gc_context::BANK_TAPS].p;
  a->freqs = ddm ? (const double*)ctx->bank[gc_context::BANK_FREQS].p : nullptr;
  a->partial = (double*)bpar.p;
  a->out = nullptr;
  a->fs = ctx->fs;
  a->nblocks = nb;
  a->ntaps = ntaps;
  a->nfreq = nfreq;
  a->arms = arms;
  return ddm ? bank_launch_chunks<kDdmGroup>(ctx, *a, (int)chunks) : bank_launch_chunks<1>(ctx, *a, (int)chunks);
}

// n compact rows of `row` elements to n rows of `full` >= row elements, the rest of each zero: the device rows hold the call's arms
// only, the caller's rows GC_MAX_ARMS of them.
template <typename T>
void bank_spread(T* dst, const T* src, long long n, long long row, long long full) {
  for (long long b = 0; b < n; ++b) {
    std::memcpy(dst + b * full, src + b * row, sizeof(T) * (size_t)row);
    std::memset(dst + b * full + row, 0, sizeof(T) * (size_t)(full - row));
  }
}

// n device rows of `row` doubles to host rows of `full` >= row doubles; waits for the stream.
int bank_fetch(gc_context* ctx, double* dst, const void* src, long long n, long long row, long long full, std::vector<double>& compact) {
  if (row != full) compact.resize((size_t)(n * row));
  GC_HIP(hipMemcpyAsync(row == full ? dst : compact.data(), src, sizeof(double) * (size_t)(n * row), hipMemcpyDeviceToHost, ctx->stream));
  GC_HIP(hipStreamSynchronize(ctx->stream));
  if (row != full) bank_spread(dst, compact.data(), n, row, full);
  return GC_OK;
}

// A sub-batch's cells [block][arm][bin][tap][2] in BANK_OUT: room for them, bank_chunks, and the combine kernel.  *a as bank_chunks
// leaves it, with `out` set.
int bank_cells(const char* fn, gc_context* ctx, const gc_block* blocks, int nb, const std::vector<int32_t>& base, int ntaps, int nfreq,
               bool ddm, int arms, BankArgs* a) {
  const long long row = (long long)arms * nfreq * ntaps * 2;
  GcBuf& bout = ctx->bank[gc_context::BANK_OUT];
  if (gc_buf_reserve(bout, sizeof(double) * (size_t)(nb * row), false) != hipSuccess) return bank_nomem(fn, ddm, nb, base.back(), ntaps, nfreq);
  const int rc = bank_chunks(fn, ctx, blocks, nb, base, ntaps, nfreq, ddm, arms, a);
  if (rc) return rc;
  a->out = (double*)bout.p;
  hipLaunchKernelGGL(bank_combine_kernel, dim3((unsigned int)((nb * row + 255) / 256)), dim3(256), 0, ctx->stream, *a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// gc_correlate_bank and gc_correlate_ddm after their argument check.  freq_offsets == nullptr is the bank: one bin (nfreq = 1) at
// carr_freq as given.
int bank_run(const char* fn, gc_context* ctx, int nblocks, const gc_block* blocks, int ntaps, const double* tap_offsets, int nfreq,
             const double* freq_offsets, double* out) {
  int arms = 1;
  int rc = bank_check(fn, ctx, nblocks, blocks, ntaps, tap_offsets, nfreq, freq_offsets, &arms);
  if (rc) return rc;
  if (nblocks == 0) return GC_OK;
  if ((rc = bank_upload_grids(fn, ctx, ntaps, tap_offsets, nfreq, freq_offsets))) return rc;
  const long long row = (long long)arms * nfreq * ntaps * 2;  // doubles per chunk (partials) and per block (results)
  const long long full = (long long)GC_MAX_ARMS * nfreq * ntaps * 2;
  const long long max_chunks = bank_max_chunks(row, BankBudget());
  std::vector<int32_t> base;
  std::vector<double> compact;
  for (int first = 0, nb; first < nblocks; first += nb) {
    nb = bank_cut(blocks, nblocks, first, max_chunks, base);
    BankArgs a;
    if ((rc = bank_cells(fn, ctx, blocks + first, nb, base, ntaps, nfreq, freq_offsets != nullptr, arms, &a))) return rc;
    if ((rc = bank_fetch(ctx, out + (size_t)first * full, a.out, nb, row, full, compact))) return rc;
  }
  return GC_OK;
}

// ---- gc_correlate_ddm_integrate: the DDM's cells added coherently over runs of blocks, then as power over runs ----------------------
//
// The chunk kernel's partials [chunk][arm][bin][tap] stay where they are.  ddm_integrate_kernel, a thread per cell (run, arm, bin,
// tap), adds each block's partials in chunk order - bank_combine_kernel's sum, so D is the DDM's bits -, rotates by the (block, bin)
// phasor ddm_rotation_kernel left in a scratch array, weights and accumulates in block order.  ddm_power_kernel, a thread per map
// cell, adds the runs' powers in run order.  A run or map the sub-batch walk cuts goes on from its own float64 accumulators in the
// next sub-batch: the additions are the same ones in the same order wherever the cut falls.

struct DdmArgs {
  const gc_block* blocks;
  const DevChannel* chans;
  const int32_t* chunk_base;  // [nblocks + 1]
  const double* freqs;        // [nfreq]
  const DdmBlockAux* aux;     // [nblocks]
  const double2* partial;     // [total chunks][arms][nfreq][ntaps]
  double2* rot;               // [nblocks][nfreq]: (cospi(2u), sinpi(2u))
  const int32_t* run_base;    // [nruns + 1]: the sub-batch's blocks before run r
  double2* coh;               // [nruns][arms][nfreq][ntaps]
  const int32_t* map_base;    // [nmaps + 1]: the sub-batch's finished runs before map q
  double* pow;                // [nmaps][arms][nfreq][ntaps]
  double fs;
  int nblocks, ntaps, nfreq, arms, nruns, nmaps;
  int carry_run;  // run 0 began in an earlier sub-batch: its cells go on from coh[0]
  int carry_map;  // map 0 likewise, from pow[0]
};

// (cospi(2u), sinpi(2u)) with x = (f * dn) / fs, u = x - rint(x): the rotation of bin f for a block dn samples after the first block
// of its run.
__device__ __forceinline__ double2 ddm_phasor(double f, long long dn, double fs) {
  const double x = __dmul_rn(f, (double)dn) / fs;
  const double u = x - rint(x);
  double s, c;
  sincospi(2.0 * u, &s, &c);
  return make_double2(c, s);
}

__global__ void ddm_rotation_kernel(const DdmArgs p) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)p.nblocks * p.nfreq) return;
  const int b = (int)(i / p.nfreq), m = (int)(i - (long long)b * p.nfreq);
  p.rot[i] = ddm_phasor(p.freqs[m], p.aux[b].dn, p.fs);
}

__global__ __launch_bounds__(256) void ddm_integrate_kernel(const DdmArgs p) {
  const int plane = p.nfreq * p.ntaps;
  const long long cells = (long long)p.arms * plane;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)p.nruns * cells) return;
  const int r = (int)(i / cells);
  const int v = (int)(i - (long long)r * cells);  // (arm, bin, tap), the tap fastest: a wavefront reads consecutive cells of a partial row
  const int arm = v / plane, m = (v - arm * plane) / p.ntaps;
  double re = 0.0, im = 0.0;
  if (r == 0 && p.carry_run) {
    re = p.coh[i].x;
    im = p.coh[i].y;
  }
  const int b0 = p.run_base[r], b1 = p.run_base[r + 1];
  if (arm < p.chans[p.blocks[b0].channel].arms)
    for (int b = b0; b < b1; ++b) {
      double dr = 0.0, di = 0.0;
      for (int q = p.chunk_base[b]; q < p.chunk_base[b + 1]; ++q) {
        const double2 t = p.partial[(long long)q * cells + v];
        dr += t.x;
        di += t.y;
      }
      const double2 cs = p.rot[(long long)b * p.nfreq + m];
      const double w = p.aux[b].w;
      re += w * (cs.x * dr + cs.y * di);
      im += w * (cs.x * di - cs.y * dr);
    }
  p.coh[i] = make_double2(re, im);
}

__global__ __launch_bounds__(256) void ddm_power_kernel(const DdmArgs p) {
  const long long cells = (long long)p.arms * p.nfreq * p.ntaps;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)p.nmaps * cells) return;
  const int q = (int)(i / cells);
  const long long v = i - (long long)q * cells;
  double acc = q == 0 && p.carry_map ? p.pow[i] : 0.0;
  for (int r = p.map_base[q]; r < p.map_base[q + 1]; ++r) {
    const double2 z = p.coh[(long long)r * cells + v];
    acc += (z.x * z.x + z.y * z.y);
  }
  p.pow[i] = acc;
}

// The kernel arguments of a step (bank_plan.h: DdmStep, DdmLaunch) from those bank_chunks returned.
DdmArgs ddm_args(gc_context* ctx, const BankArgs& a, const DdmStep& s, const DdmLaunch& l) {
  DdmArgs d;
  d.blocks = a.blocks;
  d.chans = a.chans;
  d.chunk_base = a.chunk_base;
  d.freqs = a.freqs;
  d.aux = (const DdmBlockAux*)ctx->bank[gc_context::BANK_AUX].p;
  d.partial = (const double2*)a.partial;
  d.rot = (double2*)ctx->bank[gc_context::BANK_ROT].p;
  d.run_base = (const int32_t*)ctx->bank[gc_context::BANK_RUNS].p;
  d.coh = (double2*)ctx->bank[gc_context::BANK_COH].p;
  d.map_base = (const int32_t*)ctx->bank[gc_context::BANK_MAPS].p;
  d.pow = (double*)ctx->bank[gc_context::BANK_POW].p;
  d.fs = a.fs;
  d.nblocks = s.nb;
  d.ntaps = a.ntaps;
  d.nfreq = a.nfreq;
  d.arms = a.arms;
  d.nruns = s.nr;
  d.nmaps = s.nm;
  d.carry_run = l.carry_run;
  d.carry_map = l.carry_map;
  return d;
}

// Check, plan (bank_plan.h), then per sub-batch upload, launch, fetch.
int ddm_integrate_run(const char* fn, gc_context* ctx, int nblocks, const gc_block* blocks, const double* weights, int ntaps,
                      const double* tap_offsets, int nfreq, const double* freq_offsets, int nruns, const int32_t* run_len, int nmaps,
                      const int32_t* map_len, double* coh, double* pow) {
  int arms = 1;
  BankPartition part;
  int rc = ddm_integrate_check(fn, ctx, nblocks, blocks, weights, ntaps, tap_offsets, nfreq, freq_offsets, nruns, run_len, nmaps, map_len,
                               coh != nullptr, pow != nullptr, &arms, &part);
  if (rc) return rc;
  if (nblocks == 0) return GC_OK;
  if ((rc = bank_upload_grids(fn, ctx, ntaps, tap_offsets, nfreq, freq_offsets))) return rc;
  const long long cells = (long long)arms * nfreq * ntaps, full = (long long)GC_MAX_ARMS * nfreq * ntaps;
  const long long max_chunks = bank_max_chunks(2 * cells, BankBudget());
  // The accumulators a cut run or map goes on from live in these buffers, so they are sized for the whole walk before it begins.
  const DdmSizes z = ddm_walk_sizes(blocks, nblocks, max_chunks, part);
  GcBuf& baux = ctx->bank[gc_context::BANK_AUX];
  GcBuf& brot = ctx->bank[gc_context::BANK_ROT];
  GcBuf& brun = ctx->bank[gc_context::BANK_RUNS];
  GcBuf& bcoh = ctx->bank[gc_context::BANK_COH];
  GcBuf& bmap = ctx->bank[gc_context::BANK_MAPS];
  GcBuf& bpow = ctx->bank[gc_context::BANK_POW];
  if (gc_buf_reserve(baux, sizeof(DdmBlockAux) * (size_t)z.nb, false) != hipSuccess ||
      gc_buf_reserve(brot, sizeof(double2) * (size_t)z.nb * (size_t)nfreq, false) != hipSuccess ||
      gc_buf_reserve(brun, sizeof(int32_t) * (size_t)(z.nr + 1), false) != hipSuccess ||
      gc_buf_reserve(bcoh, sizeof(double2) * (size_t)(z.nr * cells), false) != hipSuccess ||
      gc_buf_reserve(bmap, sizeof(int32_t) * (size_t)(z.nm + 1), false) != hipSuccess ||
      gc_buf_reserve(bpow, sizeof(double) * (size_t)(std::max(z.nm, 1) * cells), false) != hipSuccess) {
    gc_set_error("%s: device allocation failed (%d blocks, %d runs, %d maps in a sub-batch, %d taps, %d bins)", fn, z.nb, z.nr, z.nm, ntaps,
                 nfreq);
    return GC_E_NOMEM;
  }
  DdmLaunch l;
  std::vector<double> compact;
  for (DdmStep s; ddm_next_step(s, blocks, nblocks, max_chunks, part);) {
    BankArgs a;
    if ((rc = bank_chunks(fn, ctx, blocks + s.first, s.nb, s.chunk_base, ntaps, nfreq, true, arms, &a))) return rc;
    ddm_plan_step(s, blocks, weights, part, l);
    GC_HIP(hipMemcpyAsync(baux.p, l.aux.data(), sizeof(DdmBlockAux) * l.aux.size(), hipMemcpyHostToDevice, ctx->stream));
    GC_HIP(hipMemcpyAsync(brun.p, l.run_base.data(), sizeof(int32_t) * l.run_base.size(), hipMemcpyHostToDevice, ctx->stream));
    const DdmArgs d = ddm_args(ctx, a, s, l);
    hipLaunchKernelGGL(ddm_rotation_kernel, dim3((unsigned int)(((long long)s.nb * nfreq + 255) / 256)), dim3(256), 0, ctx->stream, d);
    GC_HIP(hipGetLastError());
    hipLaunchKernelGGL(ddm_integrate_kernel, dim3((unsigned int)((s.nr * cells + 255) / 256)), dim3(256), 0, ctx->stream, d);
    GC_HIP(hipGetLastError());
    if (s.nm > 0) {
      GC_HIP(hipMemcpyAsync(bmap.p, l.map_base.data(), sizeof(int32_t) * l.map_base.size(), hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(ddm_power_kernel, dim3((unsigned int)((s.nm * cells + 255) / 256)), dim3(256), 0, ctx->stream, d);
      GC_HIP(hipGetLastError());
      if (s.mfin > 0 && (rc = bank_fetch(ctx, pow + (size_t)s.q0 * full, bpow.p, s.mfin, cells, full, compact))) return rc;
      if (l.keep_map)  // the map that goes on: to the front
        GC_HIP(hipMemcpyAsync(bpow.p, (const double*)bpow.p + (size_t)l.keep_map * cells, sizeof(double) * (size_t)cells, hipMemcpyDeviceToDevice,
                              ctx->stream));
    }
    if (coh && s.nfin > 0 && (rc = bank_fetch(ctx, coh + (size_t)s.r0 * 2 * full, bcoh.p, s.nfin, 2 * cells, 2 * full, compact))) return rc;
    if (l.keep_run)  // the run that goes on: to the front
      GC_HIP(hipMemcpyAsync(bcoh.p, (const double2*)bcoh.p + (size_t)l.keep_run * cells, sizeof(double2) * (size_t)cells, hipMemcpyDeviceToDevice,
                            ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
  }
  return GC_OK;
}

// ---- gc_correlate_ddm_search: gc_correlate_ddm_integrate under many hypotheses, each map's peak picked here ---------------------------
//
// Per sub-batch of bank_cut's walk the chunk kernel runs once and bank_combine_kernel forms every block's cell D once
// ([block][arm][bin][tap], BANK_OUT).  The sub-batch's blocks are then taken in tiles of blocks (search_tile_blocks: what bounds the
// memory).  Per tile the host lays out one SearchAux per (hypothesis, block) - dn to the first block of the run the block has in THAT
// hypothesis, its weight there, and where runs and maps begin and end -, search_rotation_kernel forms the phasors per (hypothesis,
// block, bin) with ddm_rotation_kernel's expression, and search_integrate_kernel, a thread per (hypothesis, cell), walks the tile's
// blocks with its open run (re, im) and open map (p) in registers: ddm_integrate_kernel's and ddm_power_kernel's additions in their
// order.  The two accumulators are kept per (hypothesis, cell) between tiles and sub-batches, so a cut never shows; a finished run
// goes into its map at once and is stored only when the caller asked for coh.  search_peak_kernel reduces every finished plane.

struct SearchArgs {
  const gc_block* blocks;  // the sub-batch's
  const DevChannel* chans;
  const double* freqs;        // [nfreq]
  const SearchAux* aux;       // [nhyp][nt]
  const double2* cell;        // [sub-batch blocks][arms][nfreq][ntaps]: D
  double2* rot;               // [nhyp][nt][nfreq]: (cospi(2u), sinpi(2u))
  double2* racc;              // [nhyp][arms][nfreq][ntaps]: the open run
  double* macc;               // [nhyp][arms][nfreq][ntaps]: the open map
  double2* coh;               // [nhyp][nslot_r][arms][nfreq][ntaps]: the runs that end in this tile; nullptr: not asked for
  double* pow;                // [nhyp][nslot_m][arms][nfreq][ntaps]: the maps that end in this tile; nullptr: none asked for
  const int32_t* maps_done;   // [nhyp]: maps of the hypothesis that end in this tile
  gc_ddm_peak* peaks;         // [nhyp][nslot_m][arms]
  double fs;
  int t0, nt;  // the tile: blocks t0 .. t0 + nt - 1 of the sub-batch
  int ntaps, nfreq, arms, nhyp, nslot_r, nslot_m;
};

__global__ void search_rotation_kernel(const SearchArgs p) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)p.nhyp * p.nt * p.nfreq) return;
  const long long hk = i / p.nfreq;
  const int m = (int)(i - hk * p.nfreq);
  const SearchAux a = p.aux[hk];
  if (!(a.flags & SRCH_IN)) return;
  p.rot[i] = ddm_phasor(p.freqs[m], a.dn, p.fs);
}

__global__ __launch_bounds__(256) void search_integrate_kernel(const SearchArgs p) {
  const int plane = p.nfreq * p.ntaps;
  const int cells = p.arms * plane;
  const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);  // (arm, bin, tap), the tap fastest
  if (v >= cells) return;
  const int h = (int)blockIdx.y;
  const int arm = v / plane, m = (v - arm * plane) / p.ntaps;
  const SearchAux* __restrict__ ax = p.aux + (long long)h * p.nt;
  const double2* __restrict__ rot = p.rot + (long long)h * p.nt * p.nfreq + m;
  const long long sv = (long long)h * cells + v;
  double re = p.racc[sv].x, im = p.racc[sv].y, pw = p.macc[sv];  // the run / map that began in an earlier tile (else reset below)
  int sr = 0, sm = 0;
  for (int k = 0; k < p.nt; ++k) {
    const SearchAux a = ax[k];
    if (!(a.flags & SRCH_IN)) continue;
    if (a.flags & SRCH_RUN_START) re = im = 0.0;
    if (a.flags & SRCH_MAP_START) pw = 0.0;
    const int b = p.t0 + k;
    if (arm < p.chans[p.blocks[b].channel].arms) {
      const double2 d = p.cell[(long long)b * cells + v];
      const double2 cs = rot[(long long)k * p.nfreq];
      re += a.w * (cs.x * d.x + cs.y * d.y);
      im += a.w * (cs.x * d.y - cs.y * d.x);
    }
    if (a.flags & SRCH_RUN_END) {
      if (p.coh) p.coh[((long long)h * p.nslot_r + sr) * cells + v] = make_double2(re, im);
      ++sr;
      pw += (re * re + im * im);
      if (a.flags & SRCH_MAP_END) {
        if (p.pow) p.pow[((long long)h * p.nslot_m + sm) * cells + v] = pw;
        ++sm;
      }
    }
  }
  p.racc[sv] = make_double2(re, im);
  p.macc[sv] = pw;
}

// (value, linear index): the larger value wins, on equal values the smaller index - the sequential first maximum whatever the order
// of the combination.  Power is >= 0, so (-1, INT_MAX) loses against every cell.
__device__ __forceinline__ void search_better(double& bv, int& bi, double v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// A workgroup per finished (hypothesis, map, arm) plane.
__global__ __launch_bounds__(256) void search_peak_kernel(const SearchArgs p) {
  __shared__ double wv[4];
  __shared__ int wi[4];
  const int h = (int)blockIdx.y;
  const int s = (int)blockIdx.x / p.arms, arm = (int)blockIdx.x - s * p.arms;
  if (s >= p.maps_done[h]) return;  // uniform
  const int plane = p.nfreq * p.ntaps;
  const double* __restrict__ src = p.pow + (((long long)h * p.nslot_m + s) * p.arms + arm) * plane;
  const int tid = (int)threadIdx.x;
  double bv = -1.0;
  int bi = 0x7fffffff;
  for (int i = tid; i < plane; i += 256) search_better(bv, bi, src[i], i);
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) {
    const double ov = __shfl_down(bv, sh, 64);
    const int oi = __shfl_down(bi, sh, 64);
    search_better(bv, bi, ov, oi);
  }
  if ((tid & 63) == 0) {
    wv[tid >> 6] = bv;
    wi[tid >> 6] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) search_better(bv, bi, wv[w], wi[w]);
    gc_ddm_peak r;
    r.power = bv;
    r.bin = bi / p.ntaps;
    r.tap = bi - r.bin * p.ntaps;
    p.peaks[((long long)h * p.nslot_m + s) * p.arms + arm] = r;
  }
}

// What a tile's finished runs, maps and peaks pass through on the host.
struct SearchStage {
  std::vector<double> coh, pow;
  std::vector<gc_ddm_peak> peaks;
};

// The kernel arguments of the tile [t0, t0 + nt) of a sub-batch (bank_plan.h: SearchWalk) from those bank_cells returned.
SearchArgs search_args(gc_context* ctx, const BankArgs& a, const SearchWalk& w, int t0, int nt, int nhyp, bool out_coh, bool out_maps) {
  SearchArgs s;
  s.blocks = a.blocks;
  s.chans = a.chans;
  s.freqs = a.freqs;
  s.aux = (const SearchAux*)ctx->bank[gc_context::BANK_AUX].p;
  s.cell = (const double2*)a.out;
  s.rot = (double2*)ctx->bank[gc_context::BANK_ROT].p;
  s.racc = (double2*)ctx->bank[gc_context::BANK_RACC].p;
  s.macc = (double*)ctx->bank[gc_context::BANK_MACC].p;
  s.coh = out_coh ? (double2*)ctx->bank[gc_context::BANK_COH].p : nullptr;
  s.pow = out_maps ? (double*)ctx->bank[gc_context::BANK_POW].p : nullptr;
  s.maps_done = (const int32_t*)ctx->bank[gc_context::BANK_RUNS].p;
  s.peaks = (gc_ddm_peak*)ctx->bank[gc_context::BANK_PEAKS].p;
  s.fs = a.fs;
  s.t0 = t0;
  s.nt = nt;
  s.ntaps = a.ntaps;
  s.nfreq = a.nfreq;
  s.arms = a.arms;
  s.nhyp = nhyp;
  s.nslot_r = w.nslot_r;
  s.nslot_m = w.nslot_m;
  return s;
}

// One planned tile: its SearchAux to the device, the kernels, and the runs and maps that end in it back to their rows of the caller's.
int search_run_tile(const char* fn, gc_context* ctx, const BankArgs& a, const SearchWalk& w, int t0, int nt, int nhyp, int nruns, int nmaps,
                    double* coh, double* pow, gc_ddm_peak* peaks, SearchStage& st) {
  const int arms = a.arms, nfreq = a.nfreq, ntaps = a.ntaps, nslot_r = w.nslot_r, nslot_m = w.nslot_m;
  const long long cells = (long long)arms * nfreq * ntaps, full = (long long)GC_MAX_ARMS * nfreq * ntaps;
  const bool out_coh = coh && nslot_r > 0, out_maps = nslot_m > 0;
  GcBuf& baux = ctx->bank[gc_context::BANK_AUX];
  GcBuf& bdone = ctx->bank[gc_context::BANK_RUNS];
  GcBuf& bcoh = ctx->bank[gc_context::BANK_COH];
  GcBuf& bpow = ctx->bank[gc_context::BANK_POW];
  GcBuf& bpeak = ctx->bank[gc_context::BANK_PEAKS];
  if (gc_buf_reserve(baux, sizeof(SearchAux) * w.aux.size(), false) != hipSuccess ||
      gc_buf_reserve(ctx->bank[gc_context::BANK_ROT], sizeof(double2) * w.aux.size() * (size_t)nfreq, false) != hipSuccess ||
      (out_coh && gc_buf_reserve(bcoh, sizeof(double2) * (size_t)((long long)nhyp * nslot_r * cells), false) != hipSuccess) ||
      (out_maps && (gc_buf_reserve(bpow, sizeof(double) * (size_t)((long long)nhyp * nslot_m * cells), false) != hipSuccess ||
                    gc_buf_reserve(bpeak, sizeof(gc_ddm_peak) * (size_t)((long long)nhyp * nslot_m * arms), false) != hipSuccess))) {
    gc_set_error("%s: device allocation failed (%d hypotheses, %d blocks in a tile, %d taps, %d bins)", fn, nhyp, nt, ntaps, nfreq);
    return GC_E_NOMEM;
  }
  GC_HIP(hipMemcpyAsync(baux.p, w.aux.data(), sizeof(SearchAux) * w.aux.size(), hipMemcpyHostToDevice, ctx->stream));
  const SearchArgs s = search_args(ctx, a, w, t0, nt, nhyp, out_coh, out_maps);
  hipLaunchKernelGGL(search_rotation_kernel, dim3((unsigned int)((w.aux.size() * (size_t)nfreq + 255) / 256)), dim3(256), 0, ctx->stream, s);
  GC_HIP(hipGetLastError());
  hipLaunchKernelGGL(search_integrate_kernel, dim3((unsigned int)((cells + 255) / 256), (unsigned int)nhyp), dim3(256), 0, ctx->stream, s);
  GC_HIP(hipGetLastError());
  if (out_maps && peaks) {
    GC_HIP(hipMemcpyAsync(bdone.p, w.maps_now.data(), sizeof(int32_t) * (size_t)nhyp, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(search_peak_kernel, dim3((unsigned int)(nslot_m * arms), (unsigned int)nhyp), dim3(256), 0, ctx->stream, s);
    GC_HIP(hipGetLastError());
    st.peaks.resize((size_t)nhyp * nslot_m * arms);
    GC_HIP(hipMemcpyAsync(st.peaks.data(), bpeak.p, sizeof(gc_ddm_peak) * st.peaks.size(), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (out_coh) {
    st.coh.resize((size_t)((long long)nhyp * nslot_r * cells * 2));
    GC_HIP(hipMemcpyAsync(st.coh.data(), bcoh.p, sizeof(double) * st.coh.size(), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (out_maps && pow) {
    st.pow.resize((size_t)((long long)nhyp * nslot_m * cells));
    GC_HIP(hipMemcpyAsync(st.pow.data(), bpow.p, sizeof(double) * st.pow.size(), hipMemcpyDeviceToHost, ctx->stream));
  }
  GC_HIP(hipStreamSynchronize(ctx->stream));
  for (int h = 0; h < nhyp; ++h) {  // slot k of hypothesis h is its run runs_done[h] + k, its map maps_done[h] + k
    const size_t r = (size_t)h * nruns + w.runs_done[h], q = (size_t)h * nmaps + w.maps_done[h];
    if (out_coh) bank_spread(coh + r * (size_t)(2 * full), st.coh.data() + (size_t)h * nslot_r * (2 * cells), w.runs_now[h], 2 * cells, 2 * full);
    if (out_maps && pow) bank_spread(pow + q * (size_t)full, st.pow.data() + (size_t)h * nslot_m * cells, w.maps_now[h], cells, full);
    if (out_maps && peaks) bank_spread(peaks + q * GC_MAX_ARMS, st.peaks.data() + (size_t)h * nslot_m * arms, w.maps_now[h], arms, GC_MAX_ARMS);
  }
  return GC_OK;
}

// Check, plan (bank_plan.h), then per sub-batch the blocks' cells once and per tile of its blocks upload, launch, fetch.
int ddm_search_run(const char* fn, gc_context* ctx, int nblocks, const gc_block* blocks, int nhyp, const int32_t* block_shift,
                   const double* weights, int ntaps, const double* tap_offsets, int nfreq, const double* freq_offsets, int nruns,
                   const int32_t* run_len, int nmaps, const int32_t* map_len, double* coh, double* pow, gc_ddm_peak* peaks) {
  int arms = 1;
  BankPartition part;
  std::vector<int> shift;
  int rc = ddm_search_check(fn, ctx, nblocks, blocks, nhyp, block_shift, weights, ntaps, tap_offsets, nfreq, freq_offsets, nruns, run_len, nmaps,
                            map_len, coh != nullptr, pow != nullptr, peaks != nullptr, &arms, &part, &shift);
  if (rc) return rc;
  if (nblocks == 0) return GC_OK;
  if ((rc = bank_upload_grids(fn, ctx, ntaps, tap_offsets, nfreq, freq_offsets))) return rc;
  const bool want_maps = pow || peaks;
  const long long cells = (long long)arms * nfreq * ntaps;
  const BankBudget budget;
  const long long max_chunks = bank_max_chunks(2 * cells, budget);
  const int tile = search_tile_blocks(nhyp, nfreq, cells, arms, coh != nullptr, want_maps, budget);
  GcBuf& bracc = ctx->bank[gc_context::BANK_RACC];
  GcBuf& bmacc = ctx->bank[gc_context::BANK_MACC];
  // the accumulators a cut run or map goes on from: reserved once, before the walk
  if (gc_buf_reserve(bracc, sizeof(double2) * (size_t)(nhyp * cells), false) != hipSuccess ||
      gc_buf_reserve(bmacc, sizeof(double) * (size_t)(nhyp * cells), false) != hipSuccess ||
      gc_buf_reserve(ctx->bank[gc_context::BANK_RUNS], sizeof(int32_t) * (size_t)nhyp, false) != hipSuccess) {
    gc_set_error("%s: device allocation failed (%d hypotheses, %d taps, %d bins)", fn, nhyp, ntaps, nfreq);
    return GC_E_NOMEM;
  }
  GC_HIP(hipMemsetAsync(bracc.p, 0, sizeof(double2) * (size_t)(nhyp * cells), ctx->stream));
  GC_HIP(hipMemsetAsync(bmacc.p, 0, sizeof(double) * (size_t)(nhyp * cells), ctx->stream));
  SearchWalk w;
  search_walk_begin(w, part, nhyp, want_maps);
  SearchStage st;
  std::vector<int32_t> base;
  for (int first = 0, nb; first < nblocks; first += nb) {
    nb = bank_cut(blocks, nblocks, first, max_chunks, base);
    BankArgs a;
    if ((rc = bank_cells(fn, ctx, blocks + first, nb, base, ntaps, nfreq, true, arms, &a))) return rc;
    for (int t0 = 0; t0 < nb; t0 += tile) {
      const int nt = std::min(tile, nb - t0);
      if (!search_plan_tile(w, blocks, nblocks, weights, part, shift, first + t0, nt)) continue;  // a tile no hypothesis looks at
      if ((rc = search_run_tile(fn, ctx, a, w, t0, nt, nhyp, nruns, nmaps, coh, pow, peaks, st))) return rc;
    }
  }
  return GC_OK;
}

}  // namespace

extern "C" int gc_correlate_ddm_search(gc_context* ctx, int nblocks, const gc_block* blocks, int nhyp, const int32_t* block_shift,
                                       const double* block_weights, int ntaps, const double* tap_offsets, int nfreq,
                                       const double* freq_offsets, int nruns, const int32_t* run_len, int nmaps, const int32_t* map_len,
                                       double* coh, double* pow, gc_ddm_peak* peaks) {
  if (!ctx || nblocks < 0 || !tap_offsets || !freq_offsets || (nblocks > 0 && !blocks) || nruns < 0 || (nruns > 0 && !run_len) ||
      (nmaps > 0 && !map_len)) {
    gc_set_error("gc_correlate_ddm_search: bad arguments");
    return GC_E_INVALID;
  }
  return ddm_search_run("gc_correlate_ddm_search", ctx, nblocks, blocks, nhyp, block_shift, block_weights, ntaps, tap_offsets, nfreq,
                        freq_offsets, nruns, run_len, nmaps, map_len, coh, pow, peaks);
}

extern "C" int gc_correlate_bank(gc_context* ctx, int nblocks, const gc_block* blocks, int ntaps, const double* tap_offsets, double* out) {
  if (!ctx || nblocks < 0 || !tap_offsets || (nblocks > 0 && (!blocks || !out))) {
    gc_set_error("gc_correlate_bank: bad arguments");
    return GC_E_INVALID;
  }
  return bank_run("gc_correlate_bank", ctx, nblocks, blocks, ntaps, tap_offsets, 1, nullptr, out);
}

extern "C" int gc_correlate_ddm(gc_context* ctx, int nblocks, const gc_block* blocks, int ntaps, const double* tap_offsets, int nfreq,
                                const double* freq_offsets, double* out) {
  if (!ctx || nblocks < 0 || !tap_offsets || !freq_offsets || (nblocks > 0 && (!blocks || !out))) {
    gc_set_error("gc_correlate_ddm: bad arguments");
    return GC_E_INVALID;
  }
  return bank_run("gc_correlate_ddm", ctx, nblocks, blocks, ntaps, tap_offsets, nfreq, freq_offsets, out);
}

extern "C" int gc_correlate_ddm_integrate(gc_context* ctx, int nblocks, const gc_block* blocks, const double* block_weights, int ntaps,
                                          const double* tap_offsets, int nfreq, const double* freq_offsets, int nruns,
                                          const int32_t* run_len, int nmaps, const int32_t* map_len, double* coh, double* pow) {
  if (!ctx || nblocks < 0 || !tap_offsets || !freq_offsets || (nblocks > 0 && !blocks) || nruns < 0 || (nruns > 0 && !run_len) ||
      (nmaps > 0 && !map_len)) {
    gc_set_error("gc_correlate_ddm_integrate: bad arguments");
    return GC_E_INVALID;
  }
  return ddm_integrate_run("gc_correlate_ddm_integrate", ctx, nblocks, blocks, block_weights, ntaps, tap_offsets, nfreq, freq_offsets, nruns,
                           run_len, nmaps, map_len, coh, pow);
}
