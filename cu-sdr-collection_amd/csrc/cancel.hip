// cancel.hip — gc_cancel: the tracked components of a record rebuilt from their block descriptors and subtracted sample by sample
// (include/gnsscorr.h has the definition).  The replica is corr_f64.hip's prompt tap, by the same functions (replica_f64.h): the
// reference's float64 colon element, its table index, the carrier's angle and float64 sincos of it, every operation rounded by itself.
//
// Host: validates everything before anything is written, groups the blocks by channel (ascending channel index: the order the model
// is added in), sorts each group by first_sample, refuses overlaps inside a group, uploads the sorted descriptors, their starts and
// one CancelChan per channel.
// Pass 1 (cancel_project_kernel, only without amp_in): the prompt sums P and the integer E of every block.  A block is cut into
//   chunks of kCancelChunk samples, one workgroup each - a cut that depends on the block alone, so a block's sums are the same bits whatever
//   else is in the call.  Lanes by fixed shuffles, waves in index order, chunks in index order (cancel_amp_kernel, which also divides).
// Pass 2 (cancel_apply_kernel): one thread per 16 bytes of record (8 int8 I/Q samples, 4 int16 I/Q, 16 int8 real, 8 int16 real) as a
//   RecVec (record_fmt.h: one 16-byte load and store, byte by byte for the record's partial last vector), its samples one after the
//   other - for every channel of the call the block that covers the sample (a guess from the channel's mean block length, a binary
//   search over the sorted starts where the guess misses), the replica, the sum in channel order.  No atomics; a sample's output
//   depends on its own input and the blocks that cover it.
// What the call asks of its two records is record_check.h's check_record_pair.
#include <algorithm>
#include <cmath>

#include "corr_common.h"
#include "record_check.h"
#include "replica_f64.h"

using namespace gcorr;

namespace {

constexpr int kCancelWG = 256;
constexpr int kCancelChunk = 2048;  // samples of a block per projection workgroup: 8 per thread

struct CancelChan {  // one channel of the call (the list is in ascending channel index)
  const int8_t* tab[GC_MAX_ARMS];
  double mult[GC_MAX_ARMS];
  double R;
  double inv_mean;      // blocks per sample over the channel's span: the guess
  long long start0;     // first sample of its first block
  int32_t last[GC_MAX_ARMS];  // nent - 1
  int32_t arms;
  int32_t first, count;  // its blocks in the sorted list
};
static_assert(sizeof(CancelChan) % 8 == 0, "copied to LDS in 8-byte words");

struct CancelState {  // grow-only device buffers of the context (released by gc_destroy)
  GcBuf blocks, starts, chans, prefix, part_p, part_e, amp;
};

// What a block's samples share: corr_f64.hip's prompt tap - the same functions (replica_f64.h)
struct BlockRamp {
  Ramp64 code;
  Carrier64 carr;
};

__device__ __forceinline__ BlockRamp block_ramp(const gc_block& blk, double R) {
  return {ramp64(blk.rem_code_phase, 0.0, blk.code_phase_step, R, blk.blksize), carrier64(blk.carr_freq, blk.rem_carr_phase)};
}

__device__ __forceinline__ double code_at(const CancelChan& ch, const gc_block& blk, int arm, double t) {
  return (double)ch.tab[arm][code_index(t, ch.mult[arm], blk.table_offset[arm], ch.last[arm])];
}

struct ProjectArgs {
  const uint8_t* if_base;
  const gc_block* blocks;      // sorted; `reserved` holds the block's slot in chans
  const CancelChan* chans;
  const long long* prefix;     // [nblocks + 1]: chunks in front of each block
  double* part_p;              // [chunks][GC_MAX_ARMS][2]
  int32_t* part_e;             // [chunks][GC_MAX_ARMS]
  double fs;
  int nblocks;
};

// P = sum c (ib + j qb) and E = sum c^2 over one chunk of one block
template <int MODE>
__global__ __launch_bounds__(kCancelWG) void cancel_project_kernel(const ProjectArgs p) {
  __shared__ double red_p[kCancelWG / 64][2 * GC_MAX_ARMS];
  __shared__ int red_e[kCancelWG / 64][GC_MAX_ARMS];
  const long long g = blockIdx.x;
  int lo = 0, hi = p.nblocks;  // prefix[lo] <= g < prefix[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.prefix[mid] <= g) lo = mid;
    else hi = mid;
  }
  const gc_block blk = p.blocks[lo];
  const CancelChan ch = p.chans[blk.reserved];
  const BlockRamp k = block_ramp(blk, ch.R);
  const int i_beg = (int)(g - p.prefix[lo]) * kCancelChunk, i_end = min(blk.blksize, i_beg + kCancelChunk);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double acc[2 * GC_MAX_ARMS];
  int e[GC_MAX_ARMS];
#pragma unroll
  for (int a = 0; a < GC_MAX_ARMS; ++a) acc[2 * a] = acc[2 * a + 1] = 0.0, e[a] = 0;
  for (int i = i_beg + tid; i < i_end; i += kCancelWG) {
    double re, im, sn, cs, ib, qb;
    record_sample<MODE>(p.if_base, blk.first_sample + i, re, im);
    k.carr.at(i, p.fs, sn, cs);
    wipe_off(sn, cs, re, im, ib, qb);
    const double t = k.code.at(i);
#pragma unroll
    for (int a = 0; a < GC_MAX_ARMS; ++a)
      if (a < ch.arms) {
        const double c = code_at(ch, blk, a, t);
        acc[2 * a] += c * ib;
        acc[2 * a + 1] += c * qb;
        e[a] += (int)(c * c);
      }
  }
#pragma unroll
  for (int v = 0; v < 2 * GC_MAX_ARMS; ++v) {
    double x = acc[v];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if (lane == 0) red_p[wave][v] = x;
  }
#pragma unroll
  for (int a = 0; a < GC_MAX_ARMS; ++a) {
    int x = e[a];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if (lane == 0) red_e[wave][a] = x;
  }
  __syncthreads();
  if (tid < 2 * GC_MAX_ARMS) {
    double s = 0.0;
    for (int w = 0; w < kCancelWG / 64; ++w) s += red_p[w][tid];
    p.part_p[g * (2 * GC_MAX_ARMS) + tid] = s;
  } else if (tid < 3 * GC_MAX_ARMS) {
    const int a = tid - 2 * GC_MAX_ARMS;
    int s = 0;
    for (int w = 0; w < kCancelWG / 64; ++w) s += red_e[w][a];
    p.part_e[g * GC_MAX_ARMS + a] = s;
  }
}

// A = P / E per (block, arm): the chunks in index order; 0 where E == 0 and for arms the channel does not have
__global__ __launch_bounds__(kCancelWG) void cancel_amp_kernel(const long long* __restrict__ prefix, const double* __restrict__ part_p,
                                                         const int32_t* __restrict__ part_e, int nblocks, double* __restrict__ amp) {
  const long long t = (long long)blockIdx.x * kCancelWG + threadIdx.x;
  if (t >= (long long)nblocks * GC_MAX_ARMS) return;
  const int b = (int)(t / GC_MAX_ARMS), a = (int)(t - (long long)b * GC_MAX_ARMS);
  double pr = 0.0, pi = 0.0;
  long long e = 0;
  for (long long g = prefix[b]; g < prefix[b + 1]; ++g) {
    pr += part_p[g * (2 * GC_MAX_ARMS) + 2 * a];
    pi += part_p[g * (2 * GC_MAX_ARMS) + 2 * a + 1];
    e += part_e[g * GC_MAX_ARMS + a];
  }
  amp[2 * t] = e ? pr / (double)e : 0.0;
  amp[2 * t + 1] = e ? pi / (double)e : 0.0;
}

struct ApplyArgs {
  const uint8_t* src;
  uint8_t* dst;
  const gc_block* blocks;    // sorted
  const long long* starts;   // [nblocks] first_sample of the sorted blocks
  const CancelChan* chans;
  const double* amp;         // [nblocks][GC_MAX_ARMS][2], sorted order
  long long nsamples;
  double fs;
  int nchan;
  int mode;
};

template <int MODE>
__global__ __launch_bounds__(kCancelWG) void cancel_apply_kernel(const ApplyArgs p) {
  using F = Fmt<MODE>;
  __shared__ CancelChan sch[GC_CANCEL_MAX_CHANNELS];
  {
    const long long* g = (const long long*)p.chans;
    long long* s = (long long*)sch;
    const int words = p.nchan * (int)(sizeof(CancelChan) / 8);
    for (int i = (int)threadIdx.x; i < words; i += kCancelWG) s[i] = g[i];
  }
  __syncthreads();
  const long long nvec = (p.nsamples + F::per16 - 1) / F::per16, nbytes = p.nsamples * F::bps;
  for (long long v = (long long)blockIdx.x * kCancelWG + threadIdx.x; v < nvec; v += (long long)gridDim.x * kCancelWG) {
    const long long n0 = v * F::per16;
    const int cnt = (int)min((long long)F::per16, p.nsamples - n0);
    RecVec<MODE> w;
    w.load(p.src, v * 16, nbytes);
#pragma unroll 1
    for (int s = 0; s < cnt; ++s) {
      const long long n = n0 + s;
      int v0, v1;
      w.get(s, v0, v1);
      const double x_re = (double)(F::swap ? v1 : v0), x_im = (double)(F::swap ? v0 : v1);
      double m_re = 0.0, m_im = 0.0;
      for (int c = 0; c < p.nchan; ++c) {
        const CancelChan& ch = sch[c];
        const long long d = n - ch.start0;
        if (d < 0) continue;
        int j = (int)fmin((double)d * ch.inv_mean, (double)(ch.count - 1));
        long long sj = p.starts[ch.first + j];
        if (!(sj <= n && n < sj + p.blocks[ch.first + j].blksize)) {
          int lo = 0, hi = ch.count;  // starts[lo] <= n < starts[hi]
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (p.starts[ch.first + mid] <= n) lo = mid;
            else hi = mid;
          }
          j = lo;
          sj = p.starts[ch.first + j];
          if (n >= sj + p.blocks[ch.first + j].blksize) continue;  // in a gap of this channel
        }
        const gc_block blk = p.blocks[ch.first + j];
        const BlockRamp k = block_ramp(blk, ch.R);
        const int i = (int)(n - sj);
        double sn, cs;
        k.carr.at(i, p.fs, sn, cs);
        const double t = k.code.at(i);
        const double* A = p.amp + (long long)(ch.first + j) * (2 * GC_MAX_ARMS);
        double b_re = 0.0, b_im = 0.0;
#pragma unroll
        for (int a = 0; a < GC_MAX_ARMS; ++a)
          if (a < ch.arms) {
            const double cc = code_at(ch, blk, a, t);
            const double ar = A[2 * a], ai = A[2 * a + 1];
            b_re = __dadd_rn(b_re, __dmul_rn(cc, __dadd_rn(__dmul_rn(ar, cs), -__dmul_rn(ai, sn))));
            b_im = __dadd_rn(b_im, __dmul_rn(cc, __dadd_rn(__dmul_rn(ar, sn), __dmul_rn(ai, cs))));
          }
        if constexpr (F::values == 1) b_re = __dmul_rn(2.0, b_re);  // a real record holds half of the phasor
        m_re = __dadd_rn(m_re, b_re);
        m_im = __dadd_rn(m_im, b_im);
      }
      const double y_re = p.mode == GC_CANCEL_MODEL ? m_re : __dadd_rn(x_re, -m_re);
      const double y_im = p.mode == GC_CANCEL_MODEL ? m_im : __dadd_rn(x_im, -m_im);
      const int o_re = quantise<MODE>(y_re), o_im = quantise<MODE>(y_im);
      w.put(s, F::swap ? o_im : o_re, F::swap ? o_re : o_im);
    }
    w.store(p.dst, v * 16, nbytes);
  }
}

void launch_project(gc_context* ctx, long long chunks, const ProjectArgs& a) {
  gc_with_mode(gc_record_mode(ctx), [&](auto m) {
    hipLaunchKernelGGL(cancel_project_kernel<decltype(m)::value>, dim3((unsigned int)chunks), dim3(kCancelWG), 0, ctx->stream, a);
  });
}

void launch_apply(gc_context* ctx, unsigned int wgs, const ApplyArgs& a) {
  gc_with_mode(gc_record_mode(ctx), [&](auto m) {
    hipLaunchKernelGGL(cancel_apply_kernel<decltype(m)::value>, dim3(wgs), dim3(kCancelWG), 0, ctx->stream, a);
  });
}

// What gc_correlate asks of a descriptor (launch_plan.h gc_scope_from_blocks) with el_spacing taken as 0
int check_block(const gc_context* ctx, long long i, const gc_block& k) {
  if (k.channel < 0 || k.channel >= GC_MAX_CHANNELS || !ctx->ch[k.channel].configured) {
    gc_set_error("gc_cancel: block %lld: channel %d not configured", i, k.channel);
    return GC_E_STATE;
  }
  const HostChannel& c = ctx->ch[k.channel];
  for (int a = 0; a < c.arms; ++a) {
    if (!c.d_tab[a]) {
      gc_set_error("gc_cancel: block %lld: channel %d arm %d has no code table", i, k.channel, a);
      return GC_E_STATE;
    }
    if (k.table_offset[a] < 0 || k.table_offset[a] + 3 > c.nent[a]) {
      gc_set_error("gc_cancel: block %lld: table offset out of range", i);
      return GC_E_INVALID;
    }
  }
  if (k.blksize <= 0 || k.first_sample < 0 || !(k.code_phase_step > 0) || !(k.rem_code_phase > -1.0) || !std::isfinite(k.carr_freq) ||
      !std::isfinite(k.rem_carr_phase)) {
    gc_set_error("gc_cancel: block %lld: invalid descriptor", i);
    return GC_E_INVALID;
  }
  if ((uint64_t)k.first_sample + (uint64_t)k.blksize > ctx->if_nsamples) {
    gc_set_error("gc_cancel: block %lld: samples [%lld, %lld) exceed the IF buffer (%llu samples)", i, (long long)k.first_sample,
                 (long long)(k.first_sample + k.blksize), (unsigned long long)ctx->if_nsamples);
    return GC_E_RANGE;
  }
  for (int a = 0; a < c.arms; ++a) {
    const double tmin = k.rem_code_phase * c.index_scale * c.mult[a];
    if (!(std::ceil(tmin) >= 0.0)) {
      gc_set_error("gc_cancel: block %lld: code ramp starts at index %g, below the table entry at table_offset (arm %d)", i, std::ceil(tmin), a);
      return GC_E_INVALID;
    }
    const double tmax = ((k.blksize - 1) * k.code_phase_step + k.rem_code_phase) * c.index_scale * c.mult[a];
    const int stage = (c.window[a] > 0) ? std::min(c.window[a], c.nent[a]) : c.nent[a];
    const int avail = std::min(stage, c.nent[a] - k.table_offset[a]);
    if (!(std::ceil(tmax) <= avail - 1)) {
      gc_set_error("gc_cancel: block %lld: code ramp reaches index %g beyond table (%d entries)", i, std::ceil(tmax), avail);
      return GC_E_INVALID;
    }
  }
  return GC_OK;
}

}  // namespace

void gc_cancel_free(gc_context* ctx) {
  CancelState* s = static_cast<CancelState*>(ctx->cancel);
  if (!s) return;
  for (GcBuf* b : {&s->blocks, &s->starts, &s->chans, &s->prefix, &s->part_p, &s->part_e, &s->amp}) gc_buf_free(*b);
  delete s;
  ctx->cancel = nullptr;
}

extern "C" int gc_cancel(gc_context* src, gc_context* dst, int nblocks, const gc_block* blocks, const double* amp_in, double* amp_out, int mode) {
  if (!src || !dst || nblocks < 0 || (nblocks > 0 && !blocks)) {
    gc_set_error("gc_cancel: bad arguments");
    return GC_E_INVALID;
  }
  if (mode != GC_CANCEL_SUBTRACT && mode != GC_CANCEL_MODEL) {
    gc_set_error("gc_cancel: unknown mode %d", mode);
    return GC_E_INVALID;
  }
  if (nblocks > 0 && !(src->fs > 0)) {  // GC_E_STATE like a missing record, which check_record_pair names next
    gc_set_error("gc_cancel: sampling frequency not set (gc_set_sampling_freq)");
    return GC_E_STATE;
  }
  if (const int rc = check_record_pair("gc_cancel", src, dst)) return rc;
  const uint64_t bytes = src->if_nsamples * (uint64_t)gc_record_bps(src);
  // the blocks grouped by channel in ascending index, each group sorted by first_sample
  std::vector<int> order((size_t)nblocks);
  for (int i = 0; i < nblocks; ++i) {
    const int rc = check_block(src, i, blocks[i]);
    if (rc) return rc;
    order[(size_t)i] = i;
  }
  std::sort(order.begin(), order.end(), [&](int x, int y) {
    const gc_block &a = blocks[x], &b = blocks[y];
    if (a.channel != b.channel) return a.channel < b.channel;
    if (a.first_sample != b.first_sample) return a.first_sample < b.first_sample;
    return x < y;
  });
  std::vector<CancelChan> chans;
  std::vector<gc_block> sorted((size_t)nblocks);
  std::vector<long long> starts((size_t)nblocks), prefix((size_t)nblocks + 1, 0);
  for (int q = 0; q < nblocks; ++q) {
    const gc_block& k = blocks[order[(size_t)q]];
    if (q == 0 || k.channel != blocks[order[(size_t)q - 1]].channel) {
      const HostChannel& hc = src->ch[k.channel];
      CancelChan c;
      std::memset(&c, 0, sizeof c);
      for (int a = 0; a < hc.arms; ++a) {
        c.tab[a] = hc.d_tab[a];
        c.mult[a] = hc.mult[a];
        c.last[a] = hc.nent[a] - 1;
      }
      c.R = hc.index_scale;
      c.arms = hc.arms;
      c.first = q;
      c.start0 = k.first_sample;
      chans.push_back(c);
    } else {
      const gc_block& prev = blocks[order[(size_t)q - 1]];
      if (prev.first_sample + prev.blksize > k.first_sample) {
        gc_set_error("gc_cancel: blocks %d and %d of channel %d overlap", order[(size_t)q - 1], order[(size_t)q], k.channel);
        return GC_E_INVALID;
      }
    }
    CancelChan& c = chans.back();
    c.count = q - c.first + 1;
    c.inv_mean = (double)c.count / (double)(k.first_sample + k.blksize - c.start0);
    sorted[(size_t)q] = k;
    sorted[(size_t)q].reserved = (int32_t)chans.size() - 1;
    starts[(size_t)q] = k.first_sample;
    prefix[(size_t)q + 1] = prefix[(size_t)q] + (k.blksize + kCancelChunk - 1) / kCancelChunk;
  }
  if (chans.size() > GC_CANCEL_MAX_CHANNELS) {
    gc_set_error("gc_cancel: %d distinct channels in one call (at most %d)", (int)chans.size(), GC_CANCEL_MAX_CHANNELS);
    return GC_E_INVALID;
  }
  const long long chunks = prefix[(size_t)nblocks];
  if (chunks > 0x7fffffffLL) {
    gc_set_error("gc_cancel: %lld projection chunks in one call", chunks);
    return GC_E_INVALID;
  }
  const size_t namp = (size_t)nblocks * 2 * GC_MAX_ARMS;
  std::vector<double> amp(namp, 0.0);  // sorted order
  if (amp_in)
    for (int q = 0; q < nblocks; ++q)
      for (int v = 0; v < 2 * chans[(size_t)sorted[(size_t)q].reserved].arms; ++v) {  // the arms the block's channel has
        const double x = amp_in[(size_t)order[(size_t)q] * 2 * GC_MAX_ARMS + (size_t)v];
        if (!std::isfinite(x)) {
          gc_set_error("gc_cancel: block %d: amplitude is not finite", order[(size_t)q]);
          return GC_E_INVALID;
        }
        amp[(size_t)q * 2 * GC_MAX_ARMS + (size_t)v] = x;
      }

  // nothing has been written up to here
  GC_HIP(hipSetDevice(src->device));
  if (dst != src) GC_HIP(hipStreamSynchronize(dst->stream));  // the destination's own pending work comes first
  CancelState* s = gc_unit_state<CancelState>(src->cancel);
  if (!s) return gc_nomem("gc_cancel");
  if (nblocks > 0) {
    if (gc_buf_reserve(s->blocks, sizeof(gc_block) * (size_t)nblocks, false) != hipSuccess ||
        gc_buf_reserve(s->starts, sizeof(long long) * (size_t)nblocks, false) != hipSuccess ||
        gc_buf_reserve(s->chans, sizeof(CancelChan) * chans.size(), false) != hipSuccess ||
        gc_buf_reserve(s->amp, sizeof(double) * namp, false) != hipSuccess)
      return gc_nomem("gc_cancel");
    GC_HIP(hipMemcpyAsync(s->blocks.p, sorted.data(), sizeof(gc_block) * (size_t)nblocks, hipMemcpyHostToDevice, src->stream));
    GC_HIP(hipMemcpyAsync(s->starts.p, starts.data(), sizeof(long long) * (size_t)nblocks, hipMemcpyHostToDevice, src->stream));
    GC_HIP(hipMemcpyAsync(s->chans.p, chans.data(), sizeof(CancelChan) * chans.size(), hipMemcpyHostToDevice, src->stream));
    if (amp_in) {
      GC_HIP(hipMemcpyAsync(s->amp.p, amp.data(), sizeof(double) * namp, hipMemcpyHostToDevice, src->stream));
    } else {
      if (gc_buf_reserve(s->prefix, sizeof(long long) * ((size_t)nblocks + 1), false) != hipSuccess ||
          gc_buf_reserve(s->part_p, sizeof(double) * (size_t)chunks * 2 * GC_MAX_ARMS, false) != hipSuccess ||
          gc_buf_reserve(s->part_e, sizeof(int32_t) * (size_t)chunks * GC_MAX_ARMS, false) != hipSuccess)
        return gc_nomem("gc_cancel");
      GC_HIP(hipMemcpyAsync(s->prefix.p, prefix.data(), sizeof(long long) * ((size_t)nblocks + 1), hipMemcpyHostToDevice, src->stream));
      ProjectArgs pa;
      pa.if_base = src->d_if;
      pa.blocks = (const gc_block*)s->blocks.p;
      pa.chans = (const CancelChan*)s->chans.p;
      pa.prefix = (const long long*)s->prefix.p;
      pa.part_p = (double*)s->part_p.p;
      pa.part_e = (int32_t*)s->part_e.p;
      pa.fs = src->fs;
      pa.nblocks = nblocks;
      launch_project(src, chunks, pa);
      GC_HIP(hipGetLastError());
      const long long cells = (long long)nblocks * GC_MAX_ARMS;
      hipLaunchKernelGGL(cancel_amp_kernel, dim3((unsigned int)((cells + kCancelWG - 1) / kCancelWG)), dim3(kCancelWG), 0, src->stream, (const long long*)s->prefix.p,
                         (const double*)s->part_p.p, (const int32_t*)s->part_e.p, nblocks, (double*)s->amp.p);
      GC_HIP(hipGetLastError());
      GC_HIP(hipMemcpyAsync(amp.data(), s->amp.p, sizeof(double) * namp, hipMemcpyDeviceToHost, src->stream));
    }
  }
  ApplyArgs aa;
  aa.src = src->d_if;
  aa.dst = dst->d_if;
  aa.blocks = (const gc_block*)s->blocks.p;
  aa.starts = (const long long*)s->starts.p;
  aa.chans = (const CancelChan*)s->chans.p;
  aa.amp = (const double*)s->amp.p;
  aa.nsamples = (long long)src->if_nsamples;
  aa.fs = src->fs;
  aa.nchan = (int)chans.size();
  aa.mode = mode;
  const long long nvec = ((long long)bytes + 15) / 16;
  const long long wgs = std::min<long long>((nvec + kCancelWG - 1) / kCancelWG, 1LL << 20);  // grid-stride beyond
  if (wgs > 0) launch_apply(src, (unsigned int)wgs, aa);
  GC_HIP(hipGetLastError());
  GC_HIP(hipStreamSynchronize(src->stream));
  if (amp_out)
    for (int q = 0; q < nblocks; ++q)
      std::memcpy(amp_out + (size_t)order[(size_t)q] * 2 * GC_MAX_ARMS, amp.data() + (size_t)q * 2 * GC_MAX_ARMS, sizeof(double) * 2 * GC_MAX_ARMS);
  return GC_OK;
}
