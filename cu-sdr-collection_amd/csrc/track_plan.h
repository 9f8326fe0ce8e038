// track_plan.h — which kernel and which teams a closed-loop call gets (gc_track, gc_track_device and their window forms), decided
// on the host from integers before anything is reserved or launched: the tracking knobs, the team vocabulary, and one planner per
// loop.  Nothing here calls HIP, allocates or changes the context, and the planners read no environment variable: the knobs come
// in as a value (track_knobs_from_env, the one place that reads them).  track.hip acts on the plans; tests/track_plan_shim.hip runs
// all of it without a device.  What the planners decide also fixes the order of the float additions of every epoch (a team adds
// its members' partial sums in member order), so every formula here is held, integer for integer, by tests/test_track_plan_cpu.py.
#pragma once
#include <cstdio>

#include "launch_plan.h"

// ---- knobs -------------------------------------------------------------------------------------------------------------------
struct TrackKnob {  // an integer knob: whether it was given, and atoi of its text (each user clamps it to its own range)
  bool set = false;
  int v = 0;
};

struct TrackKnobs {
  TrackKnob track_splits;       // GC_TRACK_SPLITS: workgroups per block of a launch per epoch / members of a host-fed persistent team
  bool no_poll = false;         // GC_TRACK_NO_POLL: stream synchronise per epoch instead of polling tagged records
  int poll_timeout_ms = 2000;   // GC_TRACK_POLL_TIMEOUT_MS, per epoch (read by the shipping library too)
  bool persist_off = false;     // GC_TRACK_PERSIST=0: launch per epoch
  bool lockstep = false;        // GC_TRACK_LOCKSTEP: the persistent host loop closes all channels of an epoch before the next
  TrackKnob track_threads;      // GC_TRACK_THREADS: host threads that close the loops of a persistent kernel
  bool debug = false;           // GC_TRACK_DEBUG
  bool timing = false;          // GC_TRACK_TIMING
  TrackKnob devloop_members;    // GC_DEVLOOP_MEMBERS: members of a device-loop team
  TrackKnob devloop_waves;      // GC_DEVLOOP_WAVES: wavefronts per member workgroup of the lane device loop
  bool devloop_spread = false;  // GC_DEVLOOP_SPREAD: teams not pinned to one XCD each
  int devloop_scope = 0;        // GC_DEVLOOP_SCOPE: message scope (devloop.h): 0 system (default), 2 agent
  int devloop_timing = 0;       // GC_DEVLOOP_TIMING: 1 host + in-kernel phase clocks, 2 host only
  bool devloop_no_prefetch = false;  // GC_DEVLOOP_NO_PREFETCH
  bool devloop_one_writer = false;   // GC_DEVLOOP_ONE_WRITER
};

inline TrackKnob track_knob(const char* text) {
  TrackKnob k;
  if (text) {
    k.set = true;
    k.v = std::atoi(text);
  }
  return k;
}

// The tracking knobs of this process: tuning switches through GC_TUNE_ENV (null in the library that ships, so the defaults above
// are compile-time constants there), the poll timeout through plain getenv.
inline TrackKnobs track_knobs_from_env() {
  TrackKnobs k;
  k.track_splits = track_knob(GC_TUNE_ENV("GC_TRACK_SPLITS"));
  k.no_poll = GC_TUNE_ENV("GC_TRACK_NO_POLL") != nullptr;
  if (const char* ev = std::getenv("GC_TRACK_POLL_TIMEOUT_MS")) k.poll_timeout_ms = std::max(1, std::atoi(ev));
  const TrackKnob persist = track_knob(GC_TUNE_ENV("GC_TRACK_PERSIST"));
  k.persist_off = persist.set && persist.v == 0;
  k.lockstep = GC_TUNE_ENV("GC_TRACK_LOCKSTEP") != nullptr;
  k.track_threads = track_knob(GC_TUNE_ENV("GC_TRACK_THREADS"));
  k.debug = GC_TUNE_ENV("GC_TRACK_DEBUG") != nullptr;
  k.timing = GC_TUNE_ENV("GC_TRACK_TIMING") != nullptr;
  k.devloop_members = track_knob(GC_TUNE_ENV("GC_DEVLOOP_MEMBERS"));
  k.devloop_waves = track_knob(GC_TUNE_ENV("GC_DEVLOOP_WAVES"));
  k.devloop_spread = GC_TUNE_ENV("GC_DEVLOOP_SPREAD") != nullptr;
  k.devloop_scope = track_knob(GC_TUNE_ENV("GC_DEVLOOP_SCOPE")).v;
  k.devloop_timing = track_knob(GC_TUNE_ENV("GC_DEVLOOP_TIMING")).v;
  k.devloop_no_prefetch = GC_TUNE_ENV("GC_DEVLOOP_NO_PREFETCH") != nullptr;
  k.devloop_one_writer = GC_TUNE_ENV("GC_DEVLOOP_ONE_WRITER") != nullptr;
  return k;
}

// ---- the team vocabulary -----------------------------------------------------------------------------------------------------
constexpr int kTrackMsgBytes = 16;    // one message (devloop.h msg_t; track.hip asserts both)
constexpr int kTrackDescWords = 10;   // messages per descriptor (devloop.h kDescWords)
constexpr int kTrackFastTeamMax = 32; // the fast kernel's all-gather covers 32 members: its closer polls <= 62 messages
constexpr int kTrackLaneWaves = 8;    // wavefronts per member workgroup of a persistent lane kernel: measured best for the 1-ms and
                                      // the 4-ms packages (scripts/devloop_lane_sweep.py), and what the instantiations are bounded to

// Members of a lane-kernel team at most: its closer polls (members - 1) * 6 * arms messages, one per lane of a wavefront
inline int gc_lane_member_cap(int max_arms) { return max_arms == 1 ? 8 : max_arms == 2 ? 6 : 4; }

// Lane-chunks of `spl` samples in a nominal block (code_length chips at the nominal code rate), plus one
inline int gc_track_chunks(const gc_track_params& p, int spl) { return (int)(p.code_length / (p.code_freq_basis / p.sampling_freq) / spl) + 1; }
// ... the host loop's count for the fast kernel's chunk size (16 samples at lowrate level 2), from its 8-sample count
inline int gc_track_chunks_nominal(const gc_track_params& p, int fast_nominal) { return gc_track_chunks(p, 8) * 8 / (fast_nominal == 2 ? 16 : 8); }

// Channels that share the device during the call (gc_track_multi): teams are sized for all of them
inline int gc_track_nch_dev(const gc_context* ctx, int nch) { return ctx->concurrent_jobs ? std::max(nch, ctx->concurrent_channels) : nch; }

// A persistent grid the device cannot hold whole is refused by its launch (GC_E_NOFIT); the next try has teams of this size
inline int gc_team_halved(int team) { return (team + 1) / 2; }

// The teams' partial-sum messages: two alternating halves of two per member (fast kernel), six per arm and member (lane kernel)
inline size_t gc_track_part_bytes(int nch, int team, bool fast, int max_arms) {
  return (size_t)kTrackMsgBytes * (size_t)nch * team * (fast ? 2 * 2 : 6 * max_arms);
}

inline int gc_track_clamp(int lo, int hi, int v) { return std::max(lo, std::min(hi, v)); }

// ---- gc_track ----------------------------------------------------------------------------------------------------------------
enum TrackHostMode {
  GC_TRACK_PER_EPOCH = 0,     // one correlator launch per epoch, `splits` workgroups per block
  GC_TRACK_PERSIST_FAST = 1,  // one cooperative launch of the fast kernel's host-fed instantiation, `team` one-wave members per channel
  GC_TRACK_PERSIST_LANE = 2,  // ... of the lane kernel's, `team` member workgroups of kTrackLaneWaves waves per channel
  GC_TRACK_F64 = 3            // GC_PREC_F64: one launch of corr_f64.hip per epoch, the sums read after a stream synchronise
};

struct TrackHostPlan {
  int status = GC_OK;
  char message[160] = {0};      // of a refusal
  int fast_nominal = 0;         // fast-kernel class of the channels' nominal blocks (per-epoch blocks are re-checked by the launch)
  int splits = 1;               // launch per epoch
  int mode = GC_TRACK_PER_EPOCH;
  int team = 1;                 // persistent kernel, before any halving
  int max_arms = 1;
  bool share_lane_nominal = true, share_el = false, derived = false;
  bool poll = true;
  bool async = false;           // every channel at its own pace (persistent modes only)
  int nthreads = 1;             // host threads that close the loops when async
  bool persistent() const { return mode == GC_TRACK_PERSIST_FAST || mode == GC_TRACK_PERSIST_LANE; }
};

// `scope`, `mix`: of the call's channel set (track.hip track_preamble).  `pause_at_end`: the call is a window of a streamed record
// whose channels must all stop at the same epoch.
inline TrackHostPlan gc_plan_track_host(const gc_context* ctx, const LaunchScope& scope, const ChannelMix& mix, const gc_track_params& p, int nch,
                                        const gc_channel_init* init, bool pause_at_end, const TrackKnobs& k) {
  TrackHostPlan h;
  const int max_arms = h.max_arms = scope.max_arms;
  // B1C wide-band / E1 CBOC: the exact per-sample kernel, or the lane kernel's derived-arm instantiation when every such channel
  // allows it (three arms, the third derived, int8 I/Q or Q/I record)
  const bool any_mixed = mix.any_mixed(), derived = h.derived = scope.derived;
  const int nch_dev = gc_track_nch_dev(ctx, nch);
  if ((p.pilot_combine == 4 || p.pilot_combine == 5) && max_arms < 3) {
    h.status = GC_E_INVALID;
    std::snprintf(h.message, sizeof h.message, "gc_track: pilot_combine 4 / 5 need three arms {data, pilot BOC(1,1), pilot BOC(6,1)}");
    return h;
  }
  if (p.pilot_combine != 0 && max_arms < 2) {
    h.status = GC_E_INVALID;
    std::snprintf(h.message, sizeof h.message, "gc_track: pilot_combine requires a pilot arm");
    return h;
  }

  // nominal kernel choice: the fast kernel runs one wavefront per workgroup, the generic one four
  int fast_nominal = (gc_fast_lds_ok(ctx, scope) && !ctx->force_generic) ? 2 : 0;
  for (int c = 0; c < nch && fast_nominal; ++c) {
    gc_block probe;
    std::memset(&probe, 0, sizeof probe);
    probe.channel = init[c].channel;
    probe.code_phase_step = init[c].code_freq * 1.001 / p.sampling_freq;
    fast_nominal = std::min(fast_nominal, gc_block_lowrate_level(ctx, probe));
  }
  if (derived) fast_nominal = 0;  // derived-arm channels run on the lane kernel
  h.fast_nominal = fast_nominal;

  // launch per epoch: fill the device with one epoch's worth of blocks
  const int approx_chunks = gc_track_chunks(p, 8);
  const int chunks_nominal = gc_track_chunks_nominal(p, fast_nominal);
  int splits;
  if (fast_nominal) {
    splits = (8 * ctx->compute_units + nch_dev - 1) / nch_dev;
    splits = std::max(1, std::min(std::min(splits, 32), std::max(1, chunks_nominal / (2 * 64))));
    if (gc_fast_table_mode(scope) == 1) splits = gc_wide_splits(splits, 32);  // WIDE: 4 waves per workgroup
  } else {
    splits = gc_lane_splits(ctx, nch, approx_chunks * 8, 32);  // lane kernel: one wave per item, 16 items per workgroup
    if (splits == 1) splits = 16;  // the closed loop always goes through per-item records
  }
  if (k.track_splits.set) splits = gc_track_clamp(1, 32, k.track_splits.v);
  h.splits = splits;

  // Persistent mode: nothing is launched per epoch - one cooperative launch polls the descriptors the host loop writes into
  // host-mapped memory and answers with tagged records (devloop.h, host_loop).  On the fast kernel: single-arm R = 1 channels on
  // the transition-mask kernel with one-wave workgroups, any record format (GPS L1 C/A, BDS B1I, GLONASS) ...
  h.poll = !k.no_poll;
  bool persist = h.poll && !any_mixed && max_arms == 1 && fast_nominal > 0 && gc_fast_table_mode(scope) == 0 && p.pilot_combine == 0 &&
                 p.table_phase_count == 0 && p.n_epochs > 0 && !k.persist_off;
  for (int c = 0; c < nch && persist; ++c) {
    const HostChannel& hcn = ctx->ch[init[c].channel];
    persist = hcn.arms == 1 && hcn.index_scale == 1.0 && hcn.mult[0] == 1.0 && hcn.window[0] == 0;
  }
  // ... and on the lane kernel (corr_lane.hip, host_loop) for one- and two-arm channels of any rate and index scale (GPS L5, BDS
  // B2a / B3I, Galileo E5a / E5b / E1 B+C, BDS B1C narrow-band) and for derived third arms
  bool persist_lane = !persist && h.poll && ((!any_mixed && max_arms <= 2) || derived) && p.n_epochs > 0 && !k.persist_off;
  for (int c = 0; c < nch && persist_lane; ++c) {
    gc_block probe;
    std::memset(&probe, 0, sizeof probe);
    probe.channel = init[c].channel;
    probe.el_spacing = p.el_spacing;
    h.share_lane_nominal = h.share_lane_nominal && gc_block_shares_el_lane(ctx, probe);
  }
  if (ctx->precision == GC_PREC_F64) persist = persist_lane = false;
  h.mode = ctx->precision == GC_PREC_F64 ? GC_TRACK_F64 : persist ? GC_TRACK_PERSIST_FAST : persist_lane ? GC_TRACK_PERSIST_LANE : GC_TRACK_PER_EPOCH;
  h.share_el = !persist_lane && p.el_spacing == 0.5;

  // members per team of the persistent kernel; the host sees ONE record group per channel
  int team = std::max(1, std::min({kTrackFastTeamMax, (4 * ctx->compute_units + nch_dev - 1) / nch_dev, std::max(1, chunks_nominal / 48)}));
  const int lane_cap = gc_lane_member_cap(max_arms);
  if (persist_lane) team = std::max(1, std::min({lane_cap, approx_chunks * 8 / (64 * kTrackLaneWaves * 2), std::max(1, 2 * ctx->compute_units / nch_dev)}));
  if (k.track_splits.set) team = gc_track_clamp(1, persist_lane ? lane_cap : kTrackFastTeamMax, k.track_splits.v);
  h.team = team;

  // The channels share nothing (tracking.m:133), so the host need not wait for the slowest channel of an epoch before it closes
  // any - except in a window of a streamed record, which must end all channels at the same epoch.  One closing thread per 64
  // channels, four at most (at 12 channels more pollers only add traffic on the lines the device writes; at 96 / 192 the one
  // closer is what the epoch waits for: 14.2 / 20.4 us on one thread, 12.5 / 15.8 us on four).
  h.async = h.persistent() && !pause_at_end && !k.lockstep;
  h.nthreads = std::min(4, 1 + nch / 64);
  if (k.track_threads.set) h.nthreads = std::max(1, std::min({16, nch, k.track_threads.v}));
  return h;
}

// ---- gc_track_device ---------------------------------------------------------------------------------------------------------
// What gc_track_device asks of one configured channel before its blocks are validated; `text`: of the refusal
inline int gc_track_device_channel(const HostChannel& hcn, bool f64, const char** text) {
  const bool hder = gc_channel_is_derived(hcn);  // three arms, the third derived from the second inside the lane kernel
  for (int a = 0; a < hcn.arms; ++a)
    if (!hcn.d_tab[a] || (!f64 && hcn.mult[a] != 1.0 && !(hder && a == 2))) {
      *text = "gc_track_device: ramp multipliers other than a derived third arm are not covered (use gc_track)";
      return GC_E_UNSUPPORTED;
    }
  return GC_OK;
}

struct TrackDevicePlan {
  int status = GC_OK;  // GC_E_UNSUPPORTED: the caller uses gc_track
  char message[160] = {0};
  bool f64 = false;       // corr_f64.hip's device loop, one workgroup per channel: every configuration gc_track takes
  bool use_fast = false;  // transition-mask kernel (one-wave members), else the lane kernel (member workgroups of lane_waves waves)
  bool cboc = false;      // three arms, the third derived from the second: Galileo E1-C CBOC (fold 5), BDS B1C wide-band (fold 4)
  int lowrate = 2;        // least lowrate level of the channels' nominal blocks (2: 16-sample lane-chunks)
  bool share = true, share_lane = true;
  int team = 1, lane_waves = gcorr::kLaneWaves, msgs_per_member = 2;
  bool xcd_local = true;
  unsigned int grid = 0;
  size_t part_bytes = 0, desc_bytes = 0, rec_bytes = 0;
  int kernel() const { return f64 ? 6 : use_fast ? 1 : 0; }  // gc_debug_last_kernel: the device loop's float64 / fast / lane instantiation
};

// `first_blocks`: every channel's first block of the call (devloop_first).  `member_cap` > 0: the team may not be larger - the
// retry after a grid that did not fit.
inline TrackDevicePlan gc_plan_track_device(const gc_context* ctx, const LaunchScope& scope, const gc_track_params& p, int nch, const gc_channel_init* init,
                                            const gc_block* first_blocks, const TrackKnobs& k, int member_cap) {
  TrackDevicePlan d;
  d.f64 = ctx->precision == GC_PREC_F64;
  const int max_arms = scope.max_arms;
  const int nch_dev = gc_track_nch_dev(ctx, nch);
  bool single_r1 = true, all_derived = true, any_window = false;
  for (int c = 0; c < nch; ++c) {
    const HostChannel& hcn = ctx->ch[init[c].channel];
    all_derived = all_derived && gc_channel_is_derived(hcn);
    single_r1 = single_r1 && hcn.arms == 1 && hcn.index_scale == 1.0;
    for (int a = 0; a < hcn.arms; ++a) any_window = any_window || hcn.window[a] != 0;
  }
  d.cboc = max_arms == 3 && all_derived && (p.pilot_combine == 5 || p.pilot_combine == 4);
  const bool i8c = ctx->if_dtype == GC_I8 && ctx->if_layout != GC_REAL;  // int8 I/Q or Q/I record
  if (d.f64) {
    if (((p.pilot_combine == 4 || p.pilot_combine == 5) && max_arms < 3) || (p.pilot_combine != 0 && max_arms < 2)) {
      d.status = GC_E_INVALID;
      std::snprintf(d.message, sizeof d.message, "gc_track_device: pilot_combine %d does not match the channels' arms", p.pilot_combine);
      return d;
    }
  } else if ((max_arms > 2 && !d.cboc) || (p.pilot_combine > 3 && !d.cboc) || (p.pilot_combine != 0 && max_arms < 2) || (d.cboc && !i8c)) {
    d.status = GC_E_UNSUPPORTED;
    std::snprintf(d.message, sizeof d.message, "gc_track_device: configuration not covered by the persistent kernels (use gc_track)");
    return d;
  }
  // What selects the kernel and sizes the teams - hence the order of the float additions - comes from the channels' NOMINAL first
  // blocks (remainder 0, the acquired code frequency), which a resident call's first block is: every window of a record takes the
  // same kernel with the same teams as the whole record would
  int nominal_blksize = 0;
  for (int c = 0; c < nch; ++c) {
    gc_block nominal;
    std::memset(&nominal, 0, sizeof nominal);
    nominal.channel = init[c].channel;
    nominal.code_phase_step = init[c].code_freq / p.sampling_freq;
    nominal.blksize = (int)std::ceil(p.code_length / nominal.code_phase_step);
    nominal.el_spacing = p.el_spacing;
    if (c == 0) nominal_blksize = nominal.blksize;
    gc_block probe = nominal;
    probe.code_phase_step = nominal.code_phase_step * 1.001;  // head-room for the code NCO
    d.lowrate = std::min(d.lowrate, gc_block_lowrate_level(ctx, probe));
    d.share = d.share && gc_block_shares_el(ctx, nominal);
  }
  if (!i8c) d.lowrate = std::min(d.lowrate, 1);  // 16-sample chunks are an int8 I/Q format (corr_fast.hip)
  d.use_fast = single_r1 && d.lowrate > 0 && p.pilot_combine == 0 && gc_fast_table_mode(scope) == 0 && !ctx->force_generic && !any_window;
  if (d.use_fast) {
    // team size: just under one lane-chunk per lane and member - the epoch is a latency chain
    const int chunks = gc_track_chunks(p, d.lowrate == 2 ? 16 : 8);
    d.team = std::max(1, std::min({kTrackFastTeamMax, (4 * ctx->compute_units + nch_dev - 1) / nch_dev, std::max(1, chunks / 32)}));
    if (k.devloop_members.set) d.team = gc_track_clamp(1, kTrackFastTeamMax, k.devloop_members.v);
    d.msgs_per_member = 2;
  } else {
    for (int c = 0; c < nch; ++c) d.share_lane = d.share_lane && gc_block_shares_el_lane(ctx, first_blocks[c]);
    // member workgroups per channel: about four 64-sample steps per lane
    d.lane_waves = kTrackLaneWaves;
    if (k.devloop_waves.set) d.lane_waves = gc_track_clamp(1, kTrackLaneWaves, k.devloop_waves.v);
    const int lane_cap = gc_lane_member_cap(max_arms);
    d.team = std::max(1, std::min({lane_cap, nominal_blksize / (64 * d.lane_waves * 2), std::max(1, 2 * ctx->compute_units / nch_dev)}));
    if (k.devloop_members.set) d.team = gc_track_clamp(1, lane_cap, k.devloop_members.v);
    d.msgs_per_member = 6 * max_arms;
  }
  if (member_cap > 0) d.team = std::min(d.team, member_cap);
  // Teams on one XCD each (default).  Not next to other contexts' persistent kernels (gc_track_multi): two kernels that pin
  // their teams to the same XCDs were measured to run one after the other (E1 lane kernel 32 ms = its own 11 ms + the L1 C/A
  // kernel's 21 ms beside it), spread over the device they overlap completely and lose nothing alone (88.7 vs 89.7 ms).
  d.xcd_local = !k.devloop_spread && !ctx->concurrent_jobs;
  d.grid = d.xcd_local ? (unsigned int)(((nch + 7) / 8) * 8 * d.team) : (unsigned int)(nch * d.team);
  d.rec_bytes = sizeof(double) * (size_t)nch * GC_TRK_NFIELDS * p.n_epochs;
  d.part_bytes = gc_track_part_bytes(nch, d.team, d.use_fast, max_arms);
  d.desc_bytes = (size_t)kTrackMsgBytes * (size_t)nch * kTrackDescWords;
  return d;
}
