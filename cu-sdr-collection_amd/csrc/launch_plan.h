// launch_plan.h — which correlator kernel a launch gets and with what geometry, decided on the host from integers: the scope of a
// launch (LaunchScope, gc_internal.h) built from its descriptors or its channels, the splits policies, and the planner that turns
// scope + block count + splits into a LaunchPlan.  Nothing here calls HIP, allocates or launches: the launchers (corr_kernel.hip and
// the kernels' own units) act on the plan, tests/launch_plan_shim.hip runs all of it without a device.
// From the context these functions read the channel tables' host side (ctx->ch) and facts of the device and the record only:
// compute_units, if_dtype, if_layout, force_generic, precision (the descriptor validation also d_if, fs, if_nsamples).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "corr_common.h"

// ---- channels ----------------------------------------------------------------------------------------------------------------
// Three arms {a, b, b'} where b' is b with a sign pattern at six times the ramp rate — BOC(6,1) next to BOC(1,1) (BDS B1C
// wide-band pilot, Galileo E1-C CBOC): entry k6 of b' (padded like every table) is entry p = (k6 + 5) / 6 of b times
// (-1)^(p + k6).  Then the lane kernel needs no third table (csrc/corr_lane.hip, DER).
inline bool gc_tables_derivable(const int8_t* t1, int nent1, const int8_t* t6, int nent6) {
  const int n1 = nent1 - 2, n6 = nent6 - 2;
  if (n1 < 1 || n6 != 6 * n1) return false;
  for (int k6 = 0; k6 < nent6; ++k6) {
    const int pidx = (k6 + 5) / 6;
    if (t6[k6] != t1[pidx] * (((pidx + k6) & 1) ? -1 : 1)) return false;
  }
  return true;
}

inline bool gc_channel_is_derived(const HostChannel& c) {  // cached in HostChannel::derived_state
  if (c.derived_state < 0) {
    bool der = !GC_TUNE_ENV("GC_NO_DERIVED_ARM") && c.arms == 3 && c.mult[0] == c.mult[1] && c.mult[2] == 6.0 * c.mult[1];
    for (int a = 0; a < 3 && der; ++a) der = c.window[a] == 0 && (int)c.h_tab[a].size() == c.nent[a];
    // the two interleaved arms must fit the lane kernel's LDS budget as f16 at least (f32 up to 96 KiB)
    der = der && ((size_t)std::max(c.nent[0], c.nent[1]) + 2 * gcorr::kGuard) * 2 * 2 + 2048 <= 160 * 1024;
    c.derived_state = (der && gc_tables_derivable(c.h_tab[1].data(), c.nent[1], c.h_tab[2].data(), c.nent[2])) ? 1 : 0;
  }
  return c.derived_state == 1;
}

// Which channels of a scope have arms of different ramp multipliers, and whether their odd arm can be derived from its neighbour.
struct ChannelMix {
  bool any_derived = false, any_plain_mixed = false, any_three_plain = false;
  void add(const HostChannel& c) {
    const bool der = gc_channel_is_derived(c);
    for (int a = 1; a < c.arms; ++a)
      if (c.mult[a] != c.mult[0]) (der ? any_derived : any_plain_mixed) = true;
    if (c.arms == 3 && !der) any_three_plain = true;
  }
  bool any_mixed() const { return any_derived || any_plain_mixed; }
};

// The derived third arm: every mixed channel's odd arm can be derived (BOC(6,1) from BOC(1,1)), there is no plain three-arm channel
// next to them and the record is int8 I/Q or Q/I - then the lane kernel's derived-arm instantiation (or the hybrid kernel) runs the
// launch; any other scope with mixed ramp multipliers takes the exact per-sample kernel.
inline bool gc_derived_arm_launch(const gc_context* ctx, const ChannelMix& m) {
  return m.any_derived && !m.any_plain_mixed && !m.any_three_plain && ctx->if_dtype == GC_I8 && ctx->if_layout != GC_REAL;
}

// ---- blocks ------------------------------------------------------------------------------------------------------------------
// Kernel class a block qualifies for: 0 = generic only, 1 = fast kernel with 8-sample lane-chunks,
// 2 = fast kernel with 16-sample lane-chunks (at most one table transition per chunk and tap).
inline int gc_block_lowrate_level(const gc_context* ctx, const gc_block& b) {
  const HostChannel& c = ctx->ch[b.channel];
  // at most one table transition per lane-chunk (8 or 16 samples), with a safety margin
  const double s = b.code_phase_step * c.index_scale * c.mult[0];
  return (15.0 * s < 0.995) ? 2 : (7.0 * s < 0.995) ? 1 : 0;
}

// corr_multi.hip: 1, 2, 4 transitions per 16-sample chunk at most; 0 = more
inline int gc_block_multi_kt(const gc_context* ctx, const gc_block& b) {
  const HostChannel& c = ctx->ch[b.channel];
  // (16 - 1) samples advance the table index by 15*s entries: at most KT integers are crossed when that stays below KT
  const double s = 15.0 * b.code_phase_step * c.index_scale * c.mult[0];
  return s < 0.995 ? 1 : s < 1.995 ? 2 : s < 3.995 ? 4 : 0;
}

// 2 * el_spacing * R * M == 1 exactly: early, prompt and late taps read table entries k and k + 1 of ONE ramp (lane kernel, HALF)
inline bool gc_block_shares_el_lane(const gc_context* ctx, const gc_block& b) {
  const HostChannel& c = ctx->ch[b.channel];
  return 2.0 * b.el_spacing * c.index_scale * c.mult[0] == 1.0;
}

// el_spacing * R * M == 1/2 exactly on a one-arm channel: early and late ramps differ by one whole table entry
inline bool gc_block_shares_el(const gc_context* ctx, const gc_block& b) {
  const HostChannel& c = ctx->ch[b.channel];
  return c.arms == 1 && b.el_spacing * c.index_scale * c.mult[0] == 0.5;
}

// ---- scope -------------------------------------------------------------------------------------------------------------------
// 0 = float2 tables / single-wave workgroups, 1 = WIDE (int8 pairs, four waves), -1 = tables too large for the fast kernel
inline int gc_fast_table_mode(const LaunchScope& s) {
  if (8 * s.lds_bytes + 512 <= 64 * 1024) return 0;                            // float2 tables, one wave per workgroup
  if (2 * s.lds_bytes + 512 <= 40 * 1024 && s.max_arms <= 2) return 1;  // int8 pairs, 4 waves share them
  return -1;
}

inline bool gc_fast_lds_ok(const gc_context* ctx, const LaunchScope& s) {
  const int m = gc_fast_table_mode(s);
  if (m == 0) return true;
  // WIDE is instantiated for int8 I/Q (Q/I) records and 8-sample chunks only
  return m == 1 && ctx->if_dtype == GC_I8 && ctx->if_layout != GC_REAL;
}

// LDS needs of a channel the launch references: the kernels size their staging areas for the largest table among THOSE channels,
// not among everything configured.
inline void gc_scope_add_channel(LaunchScope& s, const HostChannel& c) {
  int off = 0, maxn = 0;
  bool mixed = false;
  for (int a = 0; a < c.arms; ++a) {
    const int stage = (c.window[a] > 0) ? std::min(c.window[a], c.nent[a]) : c.nent[a];
    off += ((stage + 8 + 15) / 16) * 16;  // as DevChannel::lds_off in gc_sync_channels
    maxn = std::max(maxn, stage);
    mixed |= c.mult[a] != c.mult[0];
  }
  s.max_arms = std::max(s.max_arms, c.arms);
  if (mixed && gc_channel_is_derived(c)) {  // third arm derived from the second: only two tables go to LDS
    s.stage_len = std::max(s.stage_len, std::max(c.nent[0], c.nent[1]));
    return;
  }
  if (mixed) return;  // mixed-multiplier channels use the LDS-free exact kernel
  s.lds_bytes = std::max(s.lds_bytes, off);
  s.stage_len = std::max(s.stage_len, maxn);
}

// What the ramp multipliers of the scope's channels decide, once all channels are in: the derived-arm instantiation, or the exact
// kernel.  `lowrate` = the least lowrate level of the blocks (2 where they are not known yet).
inline void gc_scope_set_level(const gc_context* ctx, LaunchScope& s, const ChannelMix& m, int lowrate) {
  s.derived = gc_derived_arm_launch(ctx, m);
  if (s.derived) s.fast = 0;
  else if (m.any_mixed()) s.fast = -1;
  else s.fast = (gc_fast_lds_ok(ctx, s) && !ctx->force_generic) ? lowrate : 0;
}

// What depends on the blocks alone, once the channels are in: for a channel-set scope the per-epoch part (the tracking loop's launch per epoch).
inline void gc_scope_set_epoch(const gc_context* ctx, LaunchScope& s, const ChannelMix& m, const gc_block* b, int64_t nb) {
  int lowrate = 2;
  s.share_el = s.share_lane = true;
  for (int64_t k = 0; k < nb; ++k) {
    lowrate = std::min(lowrate, gc_block_lowrate_level(ctx, b[k]));
    s.share_el = s.share_el && gc_block_shares_el(ctx, b[k]);
    s.share_lane = s.share_lane && gc_block_shares_el_lane(ctx, b[k]);
  }
  gc_scope_set_level(ctx, s, m, lowrate);
  if (s.derived) s.share_lane = false;
}

// The closed loop's launch per epoch carries tagged records the host polls: not the exact per-sample kernel, and not the float64
// one (corr_f64.hip) - neither writes tagged records.  `poll`: the caller asked for polling.
inline bool gc_epoch_polled(const gc_context* ctx, const LaunchScope& s, bool poll) {
  return poll && s.fast >= 0 && ctx->precision != GC_PREC_F64;
}

// Validates descriptors on the host and fills the scope of their launch; returns GC_OK or a negative status.  `replay`: the list
// is a replay list, whose channel pattern period (blocks[i].channel == blocks[i % P].channel, epoch-major, all table offsets zero)
// the periodic geometries of the planner use.
inline int gc_scope_from_blocks(const gc_context* ctx, int64_t n, const gc_block* b, bool replay, LaunchScope* out) {
  LaunchScope s;
  ChannelMix mix;
  if (!ctx->d_if) {
    gc_set_error("no IF buffer loaded");
    return GC_E_STATE;
  }
  if (!(ctx->fs > 0)) {
    gc_set_error("sampling frequency not set (gc_set_sampling_freq)");
    return GC_E_STATE;
  }
  bool seen[GC_MAX_CHANNELS] = {false};
  s.min_blksize = 1 << 30;
  int kt = 1, kt6 = 1;
  for (int64_t i = 0; i < n; ++i) {
    const gc_block& k = b[i];
    if (k.channel < 0 || k.channel >= GC_MAX_CHANNELS || !ctx->ch[k.channel].configured) {
      gc_set_error("block %lld: channel %d not configured", (long long)i, k.channel);
      return GC_E_STATE;
    }
    const HostChannel& c = ctx->ch[k.channel];
    for (int a = 0; a < c.arms; ++a) {
      if (!c.d_tab[a]) {
        gc_set_error("block %lld: channel %d arm %d has no code table", (long long)i, k.channel, a);
        return GC_E_STATE;
      }
      if (k.table_offset[a] < 0 || k.table_offset[a] + 3 > c.nent[a]) {
        gc_set_error("block %lld: table offset out of range", (long long)i);
        return GC_E_INVALID;
      }
    }
    if (!seen[k.channel]) {
      seen[k.channel] = true;
      gc_scope_add_channel(s, c);
      mix.add(c);
    }
    double max_mult = c.mult[0];
    for (int a = 1; a < c.arms; ++a) max_mult = std::max(max_mult, c.mult[a]);
    if (k.blksize <= 0 || k.first_sample < 0 || !(k.code_phase_step > 0) ||
        !(k.el_spacing * c.index_scale * max_mult < 1.0) || !(k.el_spacing >= 0) ||
        !(k.rem_code_phase > -1.0) || !std::isfinite(k.carr_freq) || !std::isfinite(k.rem_carr_phase)) {
      gc_set_error("block %lld: invalid descriptor", (long long)i);
      return GC_E_INVALID;
    }
    if ((uint64_t)k.first_sample + (uint64_t)k.blksize > ctx->if_nsamples) {
      gc_set_error("block %lld: samples [%lld, %lld) exceed the IF buffer (%llu samples)", (long long)i,
                   (long long)k.first_sample, (long long)(k.first_sample + k.blksize),
                   (unsigned long long)ctx->if_nsamples);
      return GC_E_RANGE;  // tracking.m:241-245
    }
    // highest and lowest table index the ramps can reach must stay inside the staged window, which starts at the entry
    // table_offset names: the early ramp's first sample (rem - d) * R * mult > -1, i.e. index ceil(.) >= 0 (MATLAB index >= 1;
    // tracking.m would stop with an index error on 0)
    for (int a = 0; a < c.arms; ++a) {
      const double tmin = (k.rem_code_phase - k.el_spacing) * c.index_scale * c.mult[a];
      if (!(std::ceil(tmin) >= 0.0)) {
        gc_set_error("block %lld: early code ramp starts at index %g, below the table entry at table_offset (arm %d)", (long long)i,
                     std::ceil(tmin), a);
        return GC_E_INVALID;
      }
      const double tmax = ((k.blksize - 1) * k.code_phase_step + k.rem_code_phase + k.el_spacing) *
                          c.index_scale * c.mult[a];
      const int stage = (c.window[a] > 0) ? std::min(c.window[a], c.nent[a]) : c.nent[a];
      const int avail = std::min(stage, c.nent[a] - k.table_offset[a]);
      if (std::ceil(tmax) > avail - 1) {
        gc_set_error("block %lld: code ramp reaches index %g beyond table (%d entries)", (long long)i,
                     std::ceil(tmax), avail);
        return GC_E_INVALID;
      }
    }
    if (kt > 0) {  // corr_multi.hip: whole int8 tables of one ramp multiplier, one or two arms
      bool plain = c.arms <= 2;
      for (int a = 0; a < c.arms; ++a) plain = plain && c.mult[a] == c.mult[0] && c.window[a] == 0 && k.table_offset[a] == 0;
      const int need = plain ? gc_block_multi_kt(ctx, k) : 0;
      kt = need == 0 ? 0 : std::max(kt, need);
    }
    if (kt6 > 0) {  // corr_cboc.hip: whole tables, derived third arm, base ramp with at most two transitions per chunk
      bool der = c.arms == 3 && gc_channel_is_derived(c);
      for (int a = 0; a < c.arms; ++a) der = der && k.table_offset[a] == 0;
      const int need = der ? gc_block_multi_kt(ctx, k) : 0;
      kt6 = (need == 0 || need > 2) ? 0 : std::max(kt6, need);
    }
    s.min_blksize = std::min(s.min_blksize, k.blksize);
  }
  gc_scope_set_epoch(ctx, s, mix, b, n);
  s.kt = (kt >= 2 && ctx->if_layout != GC_REAL && !mix.any_mixed()) ? kt : 0;
  s.kt6 = s.derived ? kt6 : 0;
  if (replay) {
    for (int64_t i = 1; i < n && i <= GC_MAX_CHANNELS; ++i)
      if (b[i].channel == b[0].channel) {
        s.period = (int)i;
        break;
      }
    for (int64_t i = 0; i < n && s.period > 0; ++i)
      if ((i >= s.period && b[i].channel != b[i - s.period].channel) || b[i].table_offset[0] != 0 || b[i].table_offset[1] != 0 ||
          b[i].table_offset[2] != 0)
        s.period = 0;
  }
  *out = s;
  return GC_OK;
}

// ---- the multi-transition and the hybrid kernel's LDS (corr_multi.hip, corr_cboc.hip assert these against their own constants) --
constexpr int kPlanMaxLds = 160 * 1024;
constexpr int kPlanTabGuard = 8 + 8;      // zero guard entries below entry 0 and above the last staged one
constexpr int kPlanWaveSums = 8 * 1024;   // running sums a wave parks: [16 samples][64 lanes] float2

// LDS bytes of the interleaved int8 tables of a launch whose longest table has `max_entries` entries
inline int gc_multi_table_bytes(int max_entries, int arms) { return ((max_entries + kPlanTabGuard) * (arms <= 1 ? 1 : 2) + 15) / 16 * 16; }

// Wavefronts per workgroup of the multi-transition kernel: the most of {16, 12, 8, 4} whose LDS (tables + 8 KB of running sums per
// wave) fits the CU and that still leaves the list >= 2 workgroups per CU (GC_MULTI_WAVES overrides); 0 = the tables do not fit at all.
inline int gc_multi_waves(const gc_context* ctx, const LaunchScope& s, long long nblocks) {
  const int tb = gc_multi_table_bytes(s.stage_len, s.max_arms);
  int forced = 0;
  if (const char* e = GC_TUNE_ENV("GC_MULTI_WAVES")) forced = std::atoi(e);
  if (ctx->if_dtype == GC_I16) return tb + 4 * kPlanWaveSums <= kPlanMaxLds ? 4 : 0;  // the int16 instantiations: 4 waves
  // two transitions per chunk (short tables: Galileo E1, BDS B1I): three four-wave workgroups per CU measured 3 % ahead of one
  // sixteen-wave workgroup (e1x8: 1.40 against 1.44 ms); four transitions (GPS L5 at 50 Msps): the other way round (3.95 / 4.10 ms)
  if (forced == 0 && s.kt <= 2 && 3 * (tb + 4 * kPlanWaveSums) <= kPlanMaxLds) return 4;
  for (int w : {16, 12, 8, 4}) {
    if (tb + w * kPlanWaveSums > kPlanMaxLds) continue;
    if (w == 16 && s.max_arms == 2 && s.kt == 4 && !s.share_lane) continue;  // three ramps x four transitions x two arms: 135 VGPRs, over the 128 a 1024-thread workgroup gets
    if (forced == w) return w;
    if (forced == 0 && (w == 4 || nblocks / ((long long)w * std::max(1, s.period)) * s.period >= 2LL * ctx->compute_units)) return w;
  }
  return 0;
}

// Wavefronts per workgroup of the hybrid kernel: the most whose LDS (two interleaved int8 tables + 8 KB of running sums per wave)
// fits a CU; 0 = not even one (GC_CBOC_WAVES overrides)
inline int gc_cboc_waves(const LaunchScope& s) {
  const int tb = gc_multi_table_bytes(s.stage_len, 2);
  int forced = 0;
  if (const char* e = GC_TUNE_ENV("GC_CBOC_WAVES")) forced = std::atoi(e);
  for (int w : {16, 12, 8, 6, 4, 2, 1}) {
    if (tb + w * kPlanWaveSums > kPlanMaxLds) continue;
    if (forced == 0 || forced == w) return w;
  }
  return 0;
}

// The hybrid kernel takes a periodic replay list of `nblocks` blocks of scope `s`: every channel a three-arm channel with a derived
// six-fold arm, base ramp with <= 2 transitions per 16-sample chunk (kt6), int8 I/Q or Q/I record, tables + 8 KB of running sums per
// wave fit a CU, and the launch at least two rounds (of waves x CUs epochs), at least two thirds full
inline bool gc_cboc_takes(const gc_context* ctx, const LaunchScope& s, long long nblocks) {
  if (!(s.kt6 >= 1 && s.period > 0 && ctx->if_dtype == GC_I8 && ctx->if_layout != GC_REAL)) return false;
  const long long waves = gc_cboc_waves(s);
  if (waves <= 0) return false;
  // A wave takes one epoch and a workgroup fills a CU, so the launch runs in rounds of waves x CUs epochs and a part-filled last round
  // costs a whole one; a single round is as long as its slowest wave (a channel's first block sits on exact chip edges and takes the
  // float64 path chunk after chunk: ~0.2 ms more).  Measured on config 3's shape (eight channels, 1 - 10 s: lane kernel 97 ns per block;
  // the hybrid 0.47 ms for one round, 0.255 ms per round from two on): ahead from two rounds at least two thirds full on (3 s: 0.52
  // against 0.57 ms), up to 58 % behind below (1.5 s = 0.72 rounds: 0.47 / 0.30; 2.1 s = 1.02 rounds: 0.51 / 0.41).
  const long long cus = ctx->compute_units;
  const long long wgs = ((nblocks / s.period + waves - 1) / waves) * s.period;
  const long long rounds = (wgs + cus - 1) / cus;
  return rounds >= 2 && 3 * nblocks >= 2 * rounds * cus * waves;
}

// ---- splits ------------------------------------------------------------------------------------------------------------------
// WIDE fast kernel (gc_fast_table_mode 1): the four waves of a workgroup share a block, so a block is split in fours
inline int gc_wide_splits(int splits, int cap) { return std::max(4, std::min(cap, (splits / 4) * 4)); }

// Lane kernel (corr_lane.hip): one wavefront per (block, split) item, 16 items per workgroup sharing a block
// -> splits is a multiple of 16; aim at 16 wavefronts per CU, keep >= 8 samples per lane in every split.
inline int gc_lane_splits(const gc_context* ctx, int64_t nblocks, int min_blksize, int cap) {
  if (nblocks >= 2 * (int64_t)ctx->compute_units) return 1;  // one block per 16-wave workgroup, combined in LDS
  int64_t s = (16 * (int64_t)ctx->compute_units + nblocks - 1) / nblocks;
  s = std::min<int64_t>(s, std::max(1, min_blksize / 512));
  s = (s + 15) / 16 * 16;
  return (int)std::max<int64_t>(16, std::min<int64_t>(s, cap / 16 * 16));
}

// gc_correlate: workgroups per block for small launches, aiming at >= 2 workgroups per CU
inline int gc_correlate_splits(const gc_context* ctx, const LaunchScope& s, int64_t nblocks) {
  if (s.fast == 0) return gc_lane_splits(ctx, nblocks, s.min_blksize, 256);
  const int wg_threads = s.fast > 0 ? 64 : 256, spl = s.fast == 2 ? 16 : 8;
  if (nblocks * (wg_threads / 64) >= 8 * (int64_t)ctx->compute_units) return 1;
  const int min_chunks = s.min_blksize / spl + 1;
  // aim at ~8 wavefronts per CU, but keep at least two chunks per thread in every split
  int n = (int)((8 * (int64_t)ctx->compute_units * 64 / wg_threads + nblocks - 1) / nblocks);
  n = std::max(1, std::min({n, std::max(1, min_chunks / (2 * wg_threads)), 64}));
  return (s.fast > 0 && gc_fast_table_mode(s) == 1 && n > 1) ? gc_wide_splits(n, 64) : n;
}

// gc_replay_launch
inline int gc_replay_splits(const gc_context* ctx, const LaunchScope& s, int64_t nblocks) {
  if (s.fast == 0) {
    // lane kernel: periodic lists with enough blocks run one block per wavefront (bpw path of the planner),
    // everything else is split 16-fold or more
    const bool periodic = s.period > 0 && nblocks >= 8 * (int64_t)ctx->compute_units;
    return periodic ? 1 : gc_lane_splits(ctx, nblocks, s.min_blksize, 256);
  }
  const int wg_waves = s.fast > 0 ? 1 : 4;
  if (nblocks * wg_waves >= 8 * (int64_t)ctx->compute_units) return 1;
  // small replay sets: split blocks over several workgroups
  const int n = (int)std::min<int64_t>(8, (8 * (int64_t)ctx->compute_units / wg_waves + nblocks - 1) / nblocks);
  return (s.fast > 0 && gc_fast_table_mode(s) == 1 && n > 1) ? gc_wide_splits(n, 8) : n;
}

// ---- the planner -------------------------------------------------------------------------------------------------------------
// Periodic list (all table offsets zero): a workgroup stages its channel's tables once and walks bpw consecutive epochs of that
// channel, `period` descriptors apart.  Returns the workgroups that have work.
inline long long gc_plan_periodic(LaunchPlan& p, int64_t nblocks, int bpw, int period) {
  p.bpw = bpw;
  p.stride = period;
  return ((nblocks + (long long)bpw * period - 1) / ((long long)bpw * period)) * period;
}

// XCD-aware order of the workgroups (corr_fast.hip / corr_lane.hip: workgroup b runs on XCD b % 8; every XCD gets one contiguous
// range of the list, so that the channels of one epoch - neighbours in the list, readers of the same IF window - share an L2).
// Any grid: rounded up to a multiple of 8, the kernels send the workgroups past `total` home.  (It used to need total % 8 == 0:
// three channels x 20 s = 7 500 workgroups fetched the record three times, 2.13 GB per launch at 5.1 TB/s, HBM-bound.)
inline int gc_plan_grid(LaunchPlan& p, long long total, bool swizzle) {
  p.xcd_swizzle = 0;
  p.total_wg = 0;
  if (swizzle && total >= 64) {
    p.xcd_swizzle = 1;
    p.total_wg = total;
    total = (total + 7) / 8 * 8;
  }
  if (total > 0x7fffffffLL) {
    gc_set_error("too many workgroups (%lld)", total);
    return GC_E_INVALID;
  }
  p.grid = (unsigned int)total;
  return GC_OK;
}

// The kernel and the geometry of a launch of `nblocks` descriptors of scope `s`, each cut into `splits` items; `polled`: the host
// polls tagged records (the closed loop's launch per epoch).  Precedence: float64, hybrid, multi-transition, WIDE by necessity or
// choice, lane or fast.
inline int gc_plan_launch(const gc_context* ctx, const LaunchScope& s, int64_t nblocks, int splits, bool polled, LaunchPlan* out) {
  LaunchPlan p;
  if (ctx->precision == GC_PREC_F64) {  // float64 per-sample kernel (corr_f64.hip)
    p.kernel = 6;
    *out = p;
    return GC_OK;
  }
  int fast = s.fast;
  const int max_arms = s.max_arms, period = s.period, cus = ctx->compute_units;
  const bool i8c = ctx->if_dtype == GC_I8 && ctx->if_layout != GC_REAL;
  const bool replay_list = period > 0 && splits == 1 && !polled;  // what every periodic geometry needs
  p.share_el = s.share_el;
  p.derived = fast == 0 && s.derived;
  int want_bpw = 8;
  if (const char* e = GC_TUNE_ENV("GC_REPLAY_BPW")) want_bpw = std::max(1, std::atoi(e));
  // Hybrid kernel for channels with a derived six-fold arm (corr_cboc.hip): periodic replay lists of int8 I/Q records, all channels
  // derived, base ramp with <= 2 transitions per 16-sample chunk.  Round 5's version (all four running-sum streams parked side by side:
  // 4 - 8 waves per CU) measured slower than the lane kernel's derived-arm instantiation; round 6's phased parking at sixteen waves per CU
  // is ahead of it (config 3's shape over 20 s: 2.76 ms against 2.91 - DESIGN.md 4.2c), so it takes these lists.  GC_NO_CBOC=1 (tuning
  // build): the lane kernel as before.
  if (p.derived && replay_list && gc_cboc_takes(ctx, s, nblocks) && max_arms == 3 && !ctx->force_generic && !GC_TUNE_ENV("GC_NO_CBOC")) {
    p.kernel = 5;
    p.waves = gc_cboc_waves(s);
    p.wide = 1;
    // a staged table serves bpw epochs of its channel
    const long long total = gc_plan_periodic(p, nblocks, p.waves * (nblocks >= 64LL * p.waves * cus ? 2 : 1), period);
    const int rc = gc_plan_grid(p, total, true);
    if (rc == GC_OK) *out = p;
    return rc;
  }
  // Multi-transition kernel (corr_multi.hip): big periodic replay lists whose chunks of 16 samples see up to 2 or 4 table
  // transitions - lists the single-transition kernel takes with 8-sample chunks (fast == 1) or hands to the lane kernel
  // (fast == 0).  GC_NO_MULTI=1 keeps the old choice (A/B), GC_MULTI_MIN = epochs per CU from which it is taken.
  if ((fast == 0 || fast == 1) && s.kt >= 2 && replay_list && !p.derived && ctx->if_layout != GC_REAL && max_arms <= 2 &&
      !GC_TUNE_ENV("GC_NO_MULTI") && !ctx->force_generic) {
    const int multi_min = GC_TUNE_ENV("GC_MULTI_MIN") ? std::max(1, std::atoi(GC_TUNE_ENV("GC_MULTI_MIN"))) : 4;
    const int mwaves = gc_multi_waves(ctx, s, nblocks);
    // enough work to fill the device: epochs per CU, a block counted by its length in 16 384-sample units (two BDS B1C
    // channels x 10 s are 2 000 blocks of 180 000 samples)
    if (mwaves > 0 && nblocks * std::max<long long>(1, s.min_blksize / 16384) >= multi_min * (long long)period * cus) {
      // blocks per workgroup: a table staged once serves bpw epochs of its channel, but a short list cut into few workgroups ends in
      // a long tail (three Galileo E1 channels x 10 s: 940 workgroups of 8 blocks 0.450 ms, 1 875 of 4 blocks 0.406 ms)
      const int bpw4 = GC_TUNE_ENV("GC_REPLAY_BPW") ? std::max(4, want_bpw) / 4 * 4 : (nblocks / 8 >= 6LL * cus ? 8 : 4);
      p.kernel = 4;
      p.waves = mwaves;
      p.wide = 1;
      const long long total = gc_plan_periodic(p, nblocks, mwaves >= 8 ? mwaves * (nblocks / period >= 64LL * mwaves ? 2 : 1) : bpw4, period);
      const int rc = gc_plan_grid(p, total, true);
      if (rc == GC_OK) *out = p;
      return rc;
    }
  }
  const bool must_wide = fast > 0 && gc_fast_table_mode(s) == 1;  // tables too large for single-wave workgroups
  // by choice: every wave of the fast kernel parks 4-8 KB of running sums in LDS (corr_fast.hip), and
  // only four waves sharing an int8-pair table keep 16 waves per CU resident (big periodic replay lists, int8 I/Q, <= 2 arms)
  // (measured, scripts/replay_scaling.py: the four-wave float-table kernel wins from 4 epochs per CU on - 12 channels x 2 s: 0.70 of
  // the HBM figure against 0.52 with single-wave workgroups, 3 channels x 10 s: 0.55 against 0.39; the first version waited for 64)
  static const int wide_min = GC_TUNE_ENV("GC_WIDE_MIN") ? std::max(1, std::atoi(GC_TUNE_ENV("GC_WIDE_MIN"))) : 4;
  const bool choose_wide = fast > 0 && !must_wide && replay_list && nblocks >= wide_min * (long long)period * cus && i8c && max_arms <= 2 &&
                           2 * s.lds_bytes + 512 <= 40 * 1024;
  const bool wide_tables = must_wide || choose_wide;
  const bool big_list = choose_wide || nblocks >= 64 * (long long)period * cus;  // tables that MUST be shared: 8 epochs per workgroup only for long lists
  long long total = (long long)nblocks * splits;
  if (fast == 0) {
    // lane kernel: 16 wavefronts per workgroup, one (block, split) item each
    if (splits == 1 && period > 0) {
      // its waves walk consecutive epochs of the workgroup's channel
      int bpw = (nblocks / period >= 256) ? 2 * gcorr::kLaneWaves : gcorr::kLaneWaves;
      if (GC_TUNE_ENV("GC_REPLAY_BPW")) bpw = std::max(gcorr::kLaneWaves, want_bpw / gcorr::kLaneWaves * gcorr::kLaneWaves);
      total = gc_plan_periodic(p, nblocks, bpw, period);
      if (total < 2LL * cus && nblocks > total && !GC_TUNE_ENV("GC_REPLAY_BPW")) {
        // few, long blocks (two BDS B1C channels, 10-ms epochs: 996 blocks would make 32 workgroups): one block per
        // workgroup, split over its 16 waves, fills the device; the table is staged per block instead of per 16-32 blocks
        p.bpw = p.stride = 1;
        p.wide = 1;
        total = nblocks;
      }
    } else if (splits == 1) {
      p.wide = 1;  // one block per workgroup, split over its 16 waves in-kernel
    } else {
      if (splits % gcorr::kLaneWaves != 0) {
        gc_set_error("internal: lane correlator launch needs splits %% %d == 0 (got %d)", gcorr::kLaneWaves, splits);
        return GC_E_INVALID;
      }
      total = (long long)nblocks * (splits / gcorr::kLaneWaves);
    }
  } else if (want_bpw > 1 && fast > 0 && splits == 1 && period > 0 && (big_list || wide_tables)) {
    // 8 epochs per workgroup for big lists; the WIDE variant needs at least one block per wave, so 4 even for short lists
    total = gc_plan_periodic(p, nblocks, big_list ? std::max(want_bpw, wide_tables ? 4 : 1) : 4, period);
  }
  if (fast > 0 && wide_tables) {
    // WIDE fast kernel: four waves per workgroup, int8-pair tables (8-sample chunks and no early/late sharing unless
    // chosen for the prefix-sum variant, which is instantiated for both chunk sizes)
    p.wide = 1;
    if (!choose_wide) {
      fast = 1;
      p.share_el = false;
    } else if (max_arms == 1 && p.bpw > 1 && !GC_TUNE_ENV("GC_NO_TABF") &&
               4 * (size_t)s.lds_bytes + 4 * (size_t)(fast == 2 ? 8192 : 4096) + 64 <= 40 * 1024) {
      p.wide = 2;  // small single-arm table: plain float code values, no conversions in the chunk loop; still 4 workgroups per CU
    }
    if (p.bpw == 1) {
      if (splits % 4 != 0 && splits != 1) {
        gc_set_error("internal: WIDE correlator launch needs splits %% 4 == 0 (got %d)", splits);
        return GC_E_INVALID;
      }
      if (splits == 1) fast = 0;  // unrelated blocks cannot share a staged table: the lane kernel takes such lists, one block per workgroup
      else total = (total + 3) / 4;
    }
  }
  p.fast = fast;
  p.chunk = (fast == 2 && i8c) ? 16 : 8;  // 16-sample chunks exist for int8 I/Q and Q/I records
  p.kernel = fast < 0 ? -1 : fast == 0 ? 0 : p.wide == 2 ? 3 : p.wide ? 2 : 1;
  const int rc = gc_plan_grid(p, total, fast >= 0);
  if (rc == GC_OK) *out = p;
  return rc;
}
