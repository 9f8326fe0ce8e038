// track.hip — gc_track: the reference's tracking loop (GPS/GPS_L1CA/include/tracking.m:133-368
// and the 3-state / pilot variants GPS_L5C/include/tracking.m:255-382,
// GAL_E1C/include/tracking.m:236-348) with the correlator (lines 247-300) on the GPU and the
// discriminators + loop filters (lines 302-335) on the host, as BASELINE.json's north_star
// prescribes.  All channels advance in lock step: one correlator launch per epoch covers every
// active channel; descriptors and partial sums live in host-mapped pinned memory so an epoch
// costs one kernel launch and one stream synchronisation.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <thread>

#include "devloop.h"
#include "launch_plan.h"

namespace {

// What gc_correlate checks per descriptor (gc_scope_from_blocks, launch_plan.h), for the blocks a tracking loop will cut from one
// channel: every ramp stays inside the reference's [c(end) c c(1)] padding (tracking.m:158,252-270) for ANY code step, because
// (blksize-1)*step + rem < codeLength by construction of blksize (:222): the largest index is ceil((codeLength + spacing)*R*M).
int validate_track_channel(const gc_context* ctx, const gc_track_params* p, const gc_channel_init& in, const char* who) {
  const HostChannel& c = ctx->ch[in.channel];
  if (!(p->sampling_freq > 0) || !(p->code_length > 0) || !(p->el_spacing >= 0) || !(p->int_time > 0) || !(in.code_freq > 0) ||
      !std::isfinite(in.code_freq) || !std::isfinite(in.acquired_freq) || in.code_phase < 0) {
    gc_set_error("%s: channel %d: invalid parameters (samplingFreq %g, codeLength %g, spacing %g, codeFreq %g, acquiredFreq %g)", who,
                 in.channel, p->sampling_freq, p->code_length, p->el_spacing, in.code_freq, in.acquired_freq);
    return GC_E_INVALID;
  }
  for (int a = 0; a < c.arms; ++a) {
    const double rm = c.index_scale * c.mult[a];
    if (!(p->el_spacing * rm < 1.0)) {
      gc_set_error("%s: channel %d arm %d: dllCorrelatorSpacing * index scale * ramp multiplier = %g table entries; the early/late "
                   "ramps must stay within one entry of the prompt ramp ([c(end) c c(1)] has one pad entry either side)", who,
                   in.channel, a, p->el_spacing * rm);
      return GC_E_INVALID;
    }
    int offset_max = 0;
    if (a == 1 && p->table_phase_count > 0) {  // GPS_L2C tracking.m:261: window offset codeLength*(CLCodePhase-1), CLCodePhase <= count
      if (in.table_phase < 0 || in.table_phase > p->table_phase_count) {
        gc_set_error("%s: channel %d: table_phase %d outside 1..%d", who, in.channel, in.table_phase, p->table_phase_count);
        return GC_E_INVALID;
      }
      offset_max = (int)p->code_length * (p->table_phase_count - 1);
    }
    const int stage = (c.window[a] > 0) ? std::min(c.window[a], c.nent[a]) : c.nent[a];
    const int avail = std::min(stage, c.nent[a] - offset_max);
    const double top = std::ceil((p->code_length + p->el_spacing) * rm);
    if (top > avail - 1) {
      gc_set_error("%s: channel %d arm %d: the code ramps reach table index %g but the table (window) holds %d entries - "
                   "settings.codeLength (%g) x index scale x multiplier does not match the table set with gc_set_code", who,
                   in.channel, a, top, avail, p->code_length);
      return GC_E_INVALID;
    }
  }
  return GC_OK;
}

// What gc_track and gc_track_device check before anything runs (`who` names the entry point in the error texts): the arguments, the
// IF buffer, every channel configured and fit for the blocks its loop will cut.  Fills the channel set's launch scope (`scope`, and
// `mix`: which channels mix ramp multipliers) on the way.
// per_channel(channel, index): the entry point's own checks of a configured channel, made before validate_track_channel.
template <class F>
int track_preamble(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init, const double* out, const int32_t* epochs_done,
                   GcTrackResume* r, const char* who, LaunchScope* scope, ChannelMix* mix, F&& per_channel) {
  if (r) r->paused = false;
  if (!ctx || !p || nch <= 0 || nch > GC_MAX_CHANNELS || !init || !out || !epochs_done || p->n_epochs <= 0 || (r && !r->state)) {
    gc_set_error("%s: bad arguments", who);
    return GC_E_INVALID;
  }
  if (!ctx->d_if) {
    gc_set_error("%s: no IF buffer loaded", who);
    return GC_E_STATE;
  }
  GC_HIP(hipSetDevice(ctx->device));
  ctx->fs = p->sampling_freq;
  int rc = gc_sync_channels(ctx);
  if (rc) return rc;
  *scope = LaunchScope();
  *mix = ChannelMix();
  for (int c = 0; c < nch; ++c) {
    const int ci = init[c].channel;
    if (ci < 0 || ci >= GC_MAX_CHANNELS || !ctx->ch[ci].configured) {
      gc_set_error("%s: channel %d not configured", who, ci);
      return GC_E_STATE;
    }
    if ((rc = per_channel(ctx->ch[ci], ci))) return rc;
    if ((rc = validate_track_channel(ctx, p, init[c], who))) return rc;
    gc_scope_add_channel(*scope, ctx->ch[ci]);
    mix->add(ctx->ch[ci]);
  }
  gc_scope_set_level(ctx, *scope, *mix, 2);
  return GC_OK;
}

}  // namespace

extern "C" int gc_track(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init,
                        double* out, int32_t* epochs_done) {
  const int rc = gc_track_window(ctx, p, nch, init, out, epochs_done, nullptr);
  if (rc == GC_OK || rc == GC_E_RANGE) gc_fill_cno_host(ctx, p, nch, out, epochs_done);
  return rc;
}

extern "C" int gc_set_cno_output(gc_context* ctx, double* cno, int64_t capacity) {
  if (!ctx || capacity < 0 || (cno && capacity == 0)) {
    gc_set_error("gc_set_cno_output: bad arguments");
    return GC_E_INVALID;
  }
  ctx->cno_out = cno;
  ctx->cno_cap = cno ? capacity : 0;
  return GC_OK;
}

// Calc_CNo_PLD.m (BDS/B2a, BDS/B1C) over the recorded prompt sums with the per-interval bookkeeping of BDS/B2a/include/
// tracking.m:409-432: two-pass mean and N-1 variance like MATLAB's mean / var, sqrt of a negative number complex, abs() of
// the complex quotient.
static void fill_cno_pld(gc_context* ctx, const gc_track_params* p, int nch, const double* out, const int32_t* epochs_done) {
  const int K = p->cno_interval, n_epochs = p->n_epochs, nk = n_epochs / K;
  if ((long long)nch * nk * GC_CNO_NPLD > ctx->cno_cap) return;
  const double T = p->cno_acc_time;
  auto arm = [&](const double* I, const double* Q, double& lin, double& pld) {  // Calc_CNo_PLD.m:47-68
    double zm = 0.0;
    for (int e = 0; e < K; ++e) zm += I[e] * I[e] + Q[e] * Q[e];
    zm /= K;
    double zv = 0.0, wiped = 0.0, sq = 0.0;
    for (int e = 0; e < K; ++e) {
      const double dz = I[e] * I[e] + Q[e] * Q[e] - zm;
      zv += dz * dz;
      wiped += std::fabs(I[e]);  // sum(I_P(I_P>0)) - sum(I_P(I_P<0))
      sq += Q[e];
    }
    zv /= (K - 1);
    lin = gcorr::cno_ratio(zm, zv) / T;
    pld = (wiped * wiped - sq * sq) / (wiped * wiped + sq * sq);
  };
  for (int c = 0; c < nch; ++c) {
    const double* rec = out + (size_t)c * GC_TRK_NFIELDS * n_epochs;
    double prev[3] = {0.0, 0.0, 0.0};  // tempCNoValue, tracking.m:192,432
    for (int k = 0; k < nk; ++k) {
      double* o = ctx->cno_out + ((size_t)c * nk + k) * GC_CNO_NPLD;
      for (int j = 0; j < GC_CNO_NPLD; ++j) o[j] = 0.0;
      if ((k + 1) * K > epochs_done[c]) continue;
      const size_t e0 = (size_t)k * K;
      double data = 0.0, pilot = 0.0, cur[3] = {0.0, 0.0, 0.0};
      arm(rec + (size_t)GC_TRK_I_P * n_epochs + e0, rec + (size_t)GC_TRK_Q_P * n_epochs + e0, data, o[3]);
      cur[0] = 10.0 * std::log10(data);
      if (p->cno_mode != GC_CNO_PLD) {
        const double* pi = rec + (size_t)GC_TRK_PILOT_I_P * n_epochs + e0;
        const double* pq = rec + (size_t)GC_TRK_PILOT_Q_P * n_epochs + e0;
        if (p->cno_mode == GC_CNO_PLD_PILOT_SWAPPED)
          arm(pq, pi, pilot, o[4]);
        else
          arm(pi, pq, pilot, o[4]);
        cur[1] = 10.0 * std::log10(pilot);
      }
      cur[2] = 10.0 * std::log10(data + pilot);
      for (int j = 0; j < 3; ++j) {
        o[j] = cur[j] * 0.5 + prev[j] * 0.5;
        prev[j] = cur[j];
      }
    }
  }
}

// CNoVSM over the recorded data-arm prompt sums, interval by interval, exactly as tracking.m:351-358 calls it (two-pass mean and
// N-1 variance like MATLAB's; Common/CNoVSM.m:38-47)
void gc_fill_cno_host(gc_context* ctx, const gc_track_params* p, int nch, const double* out, const int32_t* epochs_done) {
  const int K = p->cno_interval;
  if (!ctx->cno_out || K <= 1) return;
  const int n_epochs = p->n_epochs, nk = n_epochs / K;
  if (p->cno_mode != GC_CNO_VSM) {
    fill_cno_pld(ctx, p, nch, out, epochs_done);
    return;
  }
  if ((long long)nch * nk > ctx->cno_cap) return;
  for (int c = 0; c < nch; ++c) {
    const double* ip = out + ((size_t)c * GC_TRK_NFIELDS + GC_TRK_I_P) * n_epochs;
    const double* qp = out + ((size_t)c * GC_TRK_NFIELDS + GC_TRK_Q_P) * n_epochs;
    for (int k = 0; k < nk; ++k) {
      double v = 0.0;
      if ((k + 1) * K <= epochs_done[c]) {
        double zm = 0.0;
        for (int e = k * K; e < (k + 1) * K; ++e) zm += ip[e] * ip[e] + qp[e] * qp[e];
        zm /= K;
        double zv = 0.0;
        for (int e = k * K; e < (k + 1) * K; ++e) {
          const double dz = ip[e] * ip[e] + qp[e] * qp[e] - zm;
          zv += dz * dz;
        }
        zv /= (K - 1);
        v = 10.0 * std::log10(gcorr::cno_ratio(zm, zv) / p->cno_acc_time);
      }
      ctx->cno_out[(size_t)c * nk + k] = v;
    }
  }
}

// gc_track over one window of a record (GcTrackResume, gc_internal.h): channel state comes from / goes back to r->state,
// positions there count from the start of the RECORD (the IF buffer holds its samples from r->origin on), and with
// r->pause_at_end the call stops every channel, in lock step, at the first epoch whose block one of them cannot read from
// this window - more of the record follows - instead of ending that channel (tracking.m:241-245 is the END of the file).
int gc_track_window(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init, double* out,
                    int32_t* epochs_done, GcTrackResume* r) {
  LaunchScope scope;
  ChannelMix mix;
  int rc = track_preamble(ctx, p, nch, init, out, epochs_done, r, "gc_track", &scope, &mix, [&](const HostChannel& hcn, int ci) -> int {
    for (int a = 0; a < hcn.arms; ++a)
      if (!hcn.d_tab[a]) {
        gc_set_error("gc_track: channel %d arm %d has no code table", ci, a);
        return GC_E_STATE;
      }
    return GC_OK;
  });
  if (rc) return rc;
  const int max_arms = scope.max_arms;
  // B1C wide-band / E1 CBOC: the exact per-sample kernel, or the lane kernel's derived-arm instantiation when every such channel
  // allows it (three arms, the third derived, int8 I/Q or Q/I record)
  const bool any_mixed = mix.any_mixed(), derived = scope.derived;
  // channels that share the device during this call (gc_track_multi): teams are sized for all of them
  const int nch_dev = ctx->concurrent_jobs ? std::max(nch, ctx->concurrent_channels) : nch;
  if ((p->pilot_combine == 4 || p->pilot_combine == 5) && max_arms < 3) {
    gc_set_error("gc_track: pilot_combine 4 / 5 need three arms {data, pilot BOC(1,1), pilot BOC(6,1)}");
    return GC_E_INVALID;
  }
  if (p->pilot_combine != 0 && max_arms < 2) {
    gc_set_error("gc_track: pilot_combine requires a pilot arm");
    return GC_E_INVALID;
  }

  // splits: fill the device with one epoch's worth of blocks
  const int approx_chunks = (int)(p->code_length / (p->code_freq_basis / p->sampling_freq) / 8.0) + 1;
  // nominal kernel choice (per-epoch blocks are re-checked below): the fast kernel runs one
  // wavefront per workgroup, the generic one four
  int fast_nominal = (gc_fast_lds_ok(ctx, scope) && !ctx->force_generic) ? 2 : 0;
  for (int c = 0; c < nch && fast_nominal; ++c) {
    gc_block probe;
    std::memset(&probe, 0, sizeof probe);
    probe.channel = init[c].channel;
    probe.code_phase_step = init[c].code_freq * 1.001 / p->sampling_freq;
    fast_nominal = std::min(fast_nominal, gc_block_lowrate_level(ctx, probe));
  }
  if (derived) fast_nominal = 0;  // derived-arm channels run on the lane kernel
  int splits;
  if (fast_nominal) {
    const int chunks_nominal = approx_chunks * 8 / (fast_nominal == 2 ? 16 : 8);
    splits = (8 * ctx->compute_units + nch_dev - 1) / nch_dev;
    splits = std::max(1, std::min(std::min(splits, 32), std::max(1, chunks_nominal / (2 * 64))));
    if (gc_fast_table_mode(scope) == 1) splits = gc_wide_splits(splits, 32);  // WIDE: 4 waves per workgroup
  } else {
    splits = gc_lane_splits(ctx, nch, approx_chunks * 8, 32);  // lane kernel: one wave per item, 16 items per workgroup
    if (splits == 1) splits = 16;  // the closed loop always goes through per-item records
  }
  if (const char* e = GC_TUNE_ENV("GC_TRACK_SPLITS")) splits = std::max(1, std::min(32, std::atoi(e)));

  // pinned, device-visible descriptor and result buffers
  if (ctx->pinned_cap_blocks < nch * 32) {
    if (ctx->h_blocks_pinned) (void)hipHostFree(ctx->h_blocks_pinned);
    if (ctx->h_out_pinned) (void)hipHostFree(ctx->h_out_pinned);
    ctx->h_blocks_pinned = nullptr;
    ctx->h_out_pinned = nullptr;
    ctx->pinned_cap_blocks = 0;
    GC_HIP(hipHostMalloc((void**)&ctx->h_blocks_pinned, sizeof(gc_block) * (size_t)nch, hipHostMallocMapped));
    GC_HIP(hipHostMalloc((void**)&ctx->h_out_pinned, sizeof(double) * (size_t)nch * 32 * GC_OUT_STRIDE, hipHostMallocMapped));
    ctx->pinned_cap_blocks = nch * 32;
  }
  // Results of the fast kernel arrive as host-mapped tagged 16-byte records (corr_common.h TaggedSlot): a
  // stream synchronise costs ~15-20 us of wake-up latency per epoch, polling the tags does not.
  const bool poll = GC_TUNE_ENV("GC_TRACK_NO_POLL") == nullptr;
  int poll_timeout_ms = 2000;  // per epoch; GC_TRACK_POLL_TIMEOUT_MS overrides
  if (const char* ev = std::getenv("GC_TRACK_POLL_TIMEOUT_MS")) poll_timeout_ms = std::max(1, std::atoi(ev));
  const int64_t need_slots = (int64_t)nch * 32 * GC_OUT_STRIDE;
  if (ctx->tagged_cap < need_slots) {
    GC_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->h_tagged_pinned) (void)hipHostFree(ctx->h_tagged_pinned);
    ctx->h_tagged_pinned = nullptr;
    ctx->tagged_cap = 0;
    GC_HIP(hipHostMalloc(&ctx->h_tagged_pinned, sizeof(gcorr::TaggedSlot) * (size_t)need_slots, hipHostMallocMapped));
    ctx->tagged_cap = need_slots;
  }
  GC_HIP(hipStreamSynchronize(ctx->stream));
  std::memset(ctx->h_tagged_pinned, 0, sizeof(gcorr::TaggedSlot) * (size_t)ctx->tagged_cap);
  volatile gcorr::TaggedSlot* tagged = (volatile gcorr::TaggedSlot*)ctx->h_tagged_pinned;
  gc_block* blocks = ctx->h_blocks_pinned;
  double* partial = ctx->h_out_pinned;

  const int n_epochs = p->n_epochs;
  std::fill(out, out + (size_t)nch * GC_TRK_NFIELDS * n_epochs, 0.0);

  // Persistent mode: the loop is still closed HERE (tracking.m:302-335 below), but nothing is launched per epoch - one
  // cooperative launch of the fast kernel's persistent instantiation polls the descriptors this loop writes into
  // host-mapped memory and answers with tagged records (devloop.h, host_loop).  Launch-per-epoch costs ~5 us of dispatch
  // latency and ~13 us of kernel wall time per epoch; the persistent kernel answers in a few microseconds.  Covered:
  // single-arm R = 1 channels on the transition-mask kernel with one-wave workgroups, any record format (GPS L1 C/A, BDS B1I,
  // GLONASS); everything else keeps launching.
  ctx->last_track_mode = 0;
  ctx->last_track_team = ctx->precision == GC_PREC_F64 ? 1 : splits;  // gc_debug_last_track_team; a persistent kernel's team below
  bool persist = poll && !any_mixed && max_arms == 1 && fast_nominal > 0 && gc_fast_table_mode(scope) == 0 && p->pilot_combine == 0 &&
                 p->table_phase_count == 0 && n_epochs > 0 &&
                 !(GC_TUNE_ENV("GC_TRACK_PERSIST") && std::atoi(GC_TUNE_ENV("GC_TRACK_PERSIST")) == 0);
  for (int c = 0; c < nch && persist; ++c) {
    const HostChannel& hcn = ctx->ch[init[c].channel];
    persist = hcn.arms == 1 && hcn.index_scale == 1.0 && hcn.mult[0] == 1.0 && hcn.window[0] == 0;
  }
  // ... and on the lane kernel's persistent instantiation (corr_lane.hip, host_loop) for one- and two-arm channels of any
  // rate and index scale (GPS L5, BDS B2a / B3I, Galileo E5a / E5b / E1 B+C, BDS B1C narrow-band): member 0's first wave
  // gathers the team's sums, hands them to the host and relays the host's next descriptor
  bool persist_lane = !persist && poll && ((!any_mixed && max_arms <= 2) || derived) && n_epochs > 0 &&
                      !(GC_TUNE_ENV("GC_TRACK_PERSIST") && std::atoi(GC_TUNE_ENV("GC_TRACK_PERSIST")) == 0);
  bool share_lane_nominal = true;
  for (int c = 0; c < nch && persist_lane; ++c) {
    gc_block probe;
    std::memset(&probe, 0, sizeof probe);
    probe.channel = init[c].channel;
    probe.el_spacing = p->el_spacing;
    share_lane_nominal = share_lane_nominal && gc_block_shares_el_lane(ctx, probe);
  }
  // float64 (GC_PREC_F64): one launch of corr_f64.hip per epoch for all channels, the sums read after a stream synchronise
  if (ctx->precision == GC_PREC_F64) persist = persist_lane = false;
  if (persist_lane) persist = true;
  gcorr::DevLoopArgs pa;
  std::memset(&pa, 0, sizeof pa);
  gcorr::DevLoopArgs* d_pargs = nullptr;
  gcorr::msg_t* h_desc = nullptr;  // host-mapped descriptor messages [nch][kDescWords]
  auto persist_free = [&]() {  // the buffers stay with the context (GcBuf: freeing would wait for every stream of the device)
    gc_persistent_done(ctx);  // the kernel has ended (or was never launched): its grid leaves the device's ledger
    pa.chan = nullptr;
    pa.desc_msg = nullptr;
    pa.part_msg = nullptr;
    d_pargs = nullptr;
    h_desc = nullptr;
  };
  // descriptor of team c for epoch e (tag e + 1): payload first, tag last - a device read that sees the tag sees the payload
  auto write_desc = [&](int c, int e, const gc_block* b, unsigned long long status_word) {
    unsigned long long q[gcorr::kDescWords] = {0};
    if (b) std::memcpy(q, b, sizeof(gc_block));
    q[gcorr::kDescWords - 1] = status_word;
    volatile unsigned int* w = reinterpret_cast<volatile unsigned int*>(h_desc + (size_t)c * gcorr::kDescWords);
    for (int i = 0; i < gcorr::kDescWords; ++i) {
      w[4 * i + 0] = (unsigned int)q[i];
      w[4 * i + 1] = (unsigned int)(q[i] >> 32);
      w[4 * i + 3] = 0u;
    }
    std::atomic_thread_fence(std::memory_order_release);
    for (int i = 0; i < gcorr::kDescWords; ++i) w[4 * i + 2] = (unsigned int)e + 1u;
    std::atomic_thread_fence(std::memory_order_release);
  };
  // every team stops whatever epoch it is waiting for (tag 0xffffffff is accepted for any epoch)
  auto persist_stop = [&]() {
    for (int c = 0; c < nch; ++c) {
      volatile unsigned int* w = reinterpret_cast<volatile unsigned int*>(h_desc + (size_t)c * gcorr::kDescWords);
      for (int i = 0; i < gcorr::kDescWords; ++i) {
        w[4 * i + 0] = 3u;
        w[4 * i + 1] = 0u;
      }
      std::atomic_thread_fence(std::memory_order_release);
      for (int i = 0; i < gcorr::kDescWords; ++i) w[4 * i + 2] = 0xffffffffu;
    }
    std::atomic_thread_fence(std::memory_order_release);
  };
  // members per team of the persistent kernel (its all-gather covers up to 32); the host sees ONE record group per channel
  int psplits_dev = std::max(1, std::min({32, (4 * ctx->compute_units + nch_dev - 1) / nch_dev, std::max(1, approx_chunks * 8 / (fast_nominal == 2 ? 16 : 8) / 48)}));
  if (persist_lane)  // members of a lane-kernel team: workgroups of 8 waves (as gc_track_device)
    psplits_dev = std::max(1, std::min({max_arms == 1 ? 8 : max_arms == 2 ? 6 : 4, approx_chunks * 8 / (64 * 8 * 2), std::max(1, 2 * ctx->compute_units / nch_dev)}));
  if (const char* ev = GC_TUNE_ENV("GC_TRACK_SPLITS")) psplits_dev = std::max(1, std::min(persist_lane ? (max_arms == 1 ? 8 : max_arms == 2 ? 6 : 4) : 32, std::atoi(ev)));
  // A grid the device cannot hold whole (the teams spin on each other's messages) is refused by the launch: the teams are halved
  // until it fits - 192 channels x 1 member is still one launch for the whole call, where falling back to a launch per epoch cost
  // 33-90 us per epoch from 48 GPS L1 C/A channels on (bench.py closed_loop_sweep, round 4)
  while (persist) {
    bool refused = false;
    pa.n_epochs = n_epochs;
    pa.splits = psplits_dev;
    pa.if_nsamples = ctx->if_nsamples;
    pa.host_loop = 1;
    pa.host_tagged = ctx->h_tagged_pinned;
    std::vector<gcorr::DevLoopChan> hc((size_t)nch);
    std::memset(hc.data(), 0, sizeof(gcorr::DevLoopChan) * (size_t)nch);
    for (int c = 0; c < nch; ++c) {
      hc[c].blk.channel = init[c].channel;  // table staging needs the channel of each team
      hc[c].epoch_budget = n_epochs;        // the host ends the run
    }
    auto take = [&](int slot, size_t bytes, bool host) -> hipError_t { return gc_buf_reserve(ctx->trk[slot], bytes, host); };
    hipError_t e = take(gc_context::TRK_CHAN, sizeof(gcorr::DevLoopChan) * (size_t)nch, false);
    if (e == hipSuccess) e = take(gc_context::TRK_DESC, sizeof(gcorr::msg_t) * (size_t)nch * gcorr::kDescWords, false);
    const size_t ppart = sizeof(gcorr::msg_t) * (size_t)nch * psplits_dev * (persist_lane ? 6 * max_arms : 2 * 2);  // the teams' partial-sum messages
    if (e == hipSuccess) e = take(gc_context::TRK_PART, ppart, false);
    if (e == hipSuccess) e = take(gc_context::TRK_ARGS, sizeof pa, false);
    if (e == hipSuccess) e = take(gc_context::TRK_HDESC, sizeof(gcorr::msg_t) * (size_t)nch * gcorr::kDescWords, true);
    if (e == hipSuccess) {
      pa.chan = (gcorr::DevLoopChan*)ctx->trk[gc_context::TRK_CHAN].p;
      pa.desc_msg = (gcorr::msg_t*)ctx->trk[gc_context::TRK_DESC].p;
      pa.part_msg = (gcorr::msg_t*)ctx->trk[gc_context::TRK_PART].p;
      d_pargs = (gcorr::DevLoopArgs*)ctx->trk[gc_context::TRK_ARGS].p;
      h_desc = (gcorr::msg_t*)ctx->trk[gc_context::TRK_HDESC].p;
      e = hipMemsetAsync(pa.part_msg, 0, ppart, ctx->stream);
    }
    if (e == hipSuccess) {
      std::memset(h_desc, 0, sizeof(gcorr::msg_t) * (size_t)nch * gcorr::kDescWords);
      pa.host_desc = h_desc;
      e = hipMemsetAsync(pa.desc_msg, 0, sizeof(gcorr::msg_t) * (size_t)nch * gcorr::kDescWords, ctx->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(pa.chan, hc.data(), sizeof(gcorr::DevLoopChan) * (size_t)nch, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pargs, &pa, sizeof pa, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) {
      gcorr::KArgs a;
      std::memset(&a, 0, sizeof a);
      a.if_base = ctx->d_if;
      a.chans = ctx->d_channels;
      a.fs = ctx->fs;
      a.inv_fs = 1.0 / ctx->fs;
      a.nblocks = nch;
      a.splits = psplits_dev;
      a.bpw = 1;
      a.stride = 1;
      a.share_el = (p->el_spacing == 0.5) ? 1 : 0;
      a.devloop = d_pargs;
      a.xcd_swizzle = 0;
      if (persist_lane) {
        a.share_el = 0;
        a.derived = derived ? 1 : 0;
        const int lrc = gc_launch_devloop_lane(ctx, a, scope, (unsigned int)(nch * psplits_dev), share_lane_nominal && !derived, 8);
        if (lrc != GC_OK) e = hipErrorUnknown;
        refused = lrc == GC_E_NOFIT;   // (only a grid that did not fit is retried with smaller teams)
      } else {
        const int lrc = gc_launch_devloop(ctx, a, scope, (unsigned int)(nch * psplits_dev), fast_nominal == 2, a.share_el != 0);
        if (lrc != GC_OK) e = hipErrorUnknown;
        refused = lrc == GC_E_NOFIT;
      }
    }
    if (e != hipSuccess && refused && psplits_dev > 1) {
      (void)hipGetLastError();
      gc_persistent_done(ctx);
      psplits_dev = (psplits_dev + 1) / 2;
      continue;
    }
    ctx->last_track_mode = e == hipSuccess ? 1 : 0;
    if (e == hipSuccess) ctx->last_track_team = psplits_dev;
    if (e == hipSuccess && GC_TUNE_ENV("GC_TRACK_DEBUG"))
      std::fprintf(stderr, "gc_track: persistent kernel: %d channels x %d members (%s kernel)\n", nch, psplits_dev, persist_lane ? "lane" : "fast");
    if (e == hipSuccess) ctx->last_kernel = persist_lane ? 0 : 1;  // gc_debug_last_kernel: lane / fast kernel (persistent instantiation)
    if (e != hipSuccess) {  // could not set the persistent kernel up: launch per epoch
      if (GC_TUNE_ENV("GC_TRACK_DEBUG"))
        std::fprintf(stderr, "gc_track: persistent kernel refused (%s): %d channels x %d members, lane %d - launching per epoch\n", hipGetErrorString(e), nch,
                     psplits_dev, (int)persist_lane);
      (void)hipGetLastError();
      persist_free();
      persist = false;
      persist_lane = false;
    }
    break;
  }

  // The loop is closed by devloop.h's routine, the one the device loops run: its inputs go into `pa` (a persistent kernel took its
  // copy above), its state is one DevLoopChan per channel.  Positions count from the IF buffer's first sample, which is record
  // sample r->origin (gc_track_resume on a window: a run that starts in a window other than the record's first one must not read
  // from that window's start).
  const int64_t origin = r ? r->origin : 0;
  gcorr::devloop_set_loop(pa, *p, ctx->if_nsamples, origin, r && r->pause_at_end);
  std::vector<gcorr::DevLoopChan> st((size_t)nch);
  std::memset(st.data(), 0, sizeof(gcorr::DevLoopChan) * (size_t)nch);
  // A channel whose cutter found no block (2 the record holds no whole block any more, 4 its NCO left the finite numbers; MATLAB
  // then fails in fread(fid, NaN)) ends there; its team of a persistent kernel is told to stop instead of waiting for epoch e.
  auto tell_team = [&](int c, int e) {
    if (persist && (st[c].status == 2 || st[c].status == 4)) write_desc(c, e, nullptr, 2ull);
  };
  for (int c = 0; c < nch; ++c) {
    gcorr::DevLoopChan& s = st[c];
    gcorr::devloop_state_in(s, *p, init[c], (r && r->resume) ? &r->state[c] : nullptr, origin);
    s.epoch_budget = n_epochs;
    if (s.status != 0) continue;  // ended in an earlier window
    gcorr::devloop_first(&pa, s);
    tell_team(c, 0);
  }

  std::vector<int> slot((size_t)nch);
  double t_launch = 0.0, t_wait = 0.0;  // GC_TRACK_TIMING: host time in the launch call / until the records arrived
  const auto t_loop0 = std::chrono::steady_clock::now();

  // tracking.m:249-348 for channel c at epoch e: the records, the discriminators and loop filters, the next block in st[c].blk.
  // Returns the channel's status: 0 = st[c].blk is the block of epoch e + 1.
  auto advance = [&](int c, int e, const double (&sums)[GC_OUT_STRIDE]) -> int {
    gcorr::DevLoopChan& s = st[c];
    const HostChannel& hcn = ctx->ch[s.blk.channel];
    double* o = out + (size_t)c * GC_TRK_NFIELDS * n_epochs;
    // Arms: the device loops combine the pilot of a channel only when that channel HAS the arms the mode needs (gc_track_device tracks a
    // one-arm channel next to two-arm ones as data-only); this loop has always combined whenever pilot_combine is set - sums of arms
    // a channel lacks are zero, its discriminators NaN, the call ends with GC_E_INVALID.  Passing the arm count the mode needs keeps that (devloop_post then also records the
    // six Pilot_* fields of that one epoch: zeros, which is what the zero-filled `out` held there).
    const int arms = p->pilot_combine >= 4 ? 3 : p->pilot_combine != 0 ? std::max(hcn.arms, 2) : hcn.arms;
    const gcorr::DevLoopPre pre = gcorr::devloop_pre(&pa, s, s.blk, hcn.index_scale);
    gcorr::devloop_post<GC_MAX_ARMS>(&pa, s, s.blk, e, sums, arms, hcn.index_scale, pre, [&](int f, double v) { o[(size_t)f * n_epochs + e] = v; });
    tell_team(c, e + 1);
    return s.status;
  };

  // ---- persistent kernel, every channel at its own pace ---------------------------------------------------------------
  // The channels share nothing (tracking.m:133): each team of the persistent kernel waits for ITS descriptor and answers with
  // ITS record group.  So the host does not wait for the slowest channel of an epoch before it closes any: whichever record
  // group carries its channel's next tag is closed at once and that channel's next descriptor goes out, while the other teams
  // are still correlating or their records are on the way.  Lock step (the loop below) cost an epoch the sum of the PCIe round
  // trip, the team's work and the twelve closures; this way the round trip of one channel hides behind the others' work.
  // (Not under pause_at_end: a window of a streamed record must end all channels at the same epoch.)
  const bool async = persist && poll && !(r && r->pause_at_end) && GC_TUNE_ENV("GC_TRACK_LOCKSTEP") == nullptr;
  if (async) {
    const int arms6 = max_arms * 6;
    struct alignas(64) Slot {  // a channel's turn on a cache line of its own: neighbouring channels may belong to other threads
      int ep = 0;
      bool waiting = false;
      std::chrono::steady_clock::time_point sent;
    };
    std::vector<Slot> sl((size_t)nch);
    std::atomic<bool> lost{false};
    std::atomic<int> lost_epoch{0};
    // Is the one host thread that closes all loops what bounds the epoch?  Measured: no.  With the channels dealt out to 2, 3 and 4 host
    // threads (GC_TRACK_THREADS; a contiguous share each, this thread serves the first) twelve L1 C/A channels took 7.04 / 6.91 /
    // 6.93 us per epoch against 6.77 us on one thread, configs 3 and 4 lost 4-11 %: an epoch is one channel's own chain (descriptor
    // over PCIe, relay, correlate, all-gather, records back), and more pollers only add traffic on the lines the device writes.
    // So one thread is the default; the knob stays for hosts with slower cores.
    // ... at 12 channels.  With the closed_loop_sweep's 96 / 192 channels the one closer is what the epoch waits for: 14.2 / 20.4 us on
    // one thread, 12.5 / 15.8 us on four - so one more thread per 64 channels, four at most.
    int nthreads = std::min(4, 1 + nch / 64);
    if (const char* ev = GC_TUNE_ENV("GC_TRACK_THREADS")) nthreads = std::max(1, std::min({16, nch, std::atoi(ev)}));
    auto serve = [&](int t) {
      const int c0 = (int)((long long)t * nch / nthreads), c1 = (int)((long long)(t + 1) * nch / nthreads);
      int outstanding = 0;
      const auto now0 = std::chrono::steady_clock::now();
      for (int c = c0; c < c1; ++c) {
        if (st[c].status != 0) continue;
        write_desc(c, 0, &st[c].blk, 0ull);
        sl[c].waiting = true;
        sl[c].sent = now0;
        ++outstanding;
      }
      unsigned int idle = 0, turns = 0;
      // a descriptor's time of sending, to the precision the timeout needs: refreshed every 256 turns of the poll loop WHETHER OR NOT
      // records arrived (a stamp refreshed only while idle stays at now0 for a whole busy run, and the first stall after
      // poll_timeout_ms of wall time would then read as a lost epoch), and again whenever the loop has been idle for 1024 turns
      auto stamp = now0;
      while (outstanding > 0 && !lost.load(std::memory_order_relaxed)) {
        bool progress = false;
        if ((++turns & 255u) == 0) stamp = std::chrono::steady_clock::now();
        for (int c = c0; c < c1; ++c) {
          if (!sl[c].waiting) continue;
          const unsigned int tag = (unsigned int)sl[c].ep + 1u;
          volatile gcorr::TaggedSlot* grp = tagged + (size_t)c * GC_OUT_STRIDE;
          bool ready = true;
          for (int v = arms6 - 1; v >= 0 && ready; --v) ready = grp[v].tag == tag;
          if (!ready) continue;
          std::atomic_thread_fence(std::memory_order_acquire);
          double sums[GC_OUT_STRIDE];
          for (int v = 0; v < GC_OUT_STRIDE; ++v) sums[v] = v < arms6 ? grp[v].value : 0.0;
          const int status = advance(c, sl[c].ep, sums);
          progress = true;
          ++sl[c].ep;
          if (status == 0) {
            write_desc(c, sl[c].ep, &st[c].blk, 0ull);
            sl[c].sent = stamp;
          } else {
            sl[c].waiting = false;  // all epochs done (the team leaves by itself) or the channel ended (its team has been told)
            --outstanding;
          }
        }
        if (progress) {
          idle = 0;
        } else if ((++idle & 1023u) == 0) {
          // first epoch of the persistent kernel: code load + launch of the whole grid
          const auto now = stamp = std::chrono::steady_clock::now();
          for (int c = c0; c < c1; ++c)
            if (sl[c].waiting && now - sl[c].sent > std::chrono::milliseconds(sl[c].ep == 0 ? std::max(5000, poll_timeout_ms) : poll_timeout_ms)) {
              lost_epoch.store(sl[c].ep, std::memory_order_relaxed);
              lost.store(true, std::memory_order_relaxed);
              break;
            }
        }
      }
    };
    {
      std::vector<std::thread> helpers;
      for (int t = 1; t < nthreads; ++t) helpers.emplace_back(serve, t);
      serve(0);
      for (std::thread& h : helpers) h.join();
    }
    if (lost.load()) {
      persist_stop();
      GC_HIP(hipStreamSynchronize(ctx->stream));
      persist_free();
      gc_set_error("gc_track: result records of epoch %d did not arrive", lost_epoch.load());
      return GC_E_HIP;
    }
    t_wait = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_loop0).count();
  }

  for (int e = 0; e < n_epochs && !async; ++e) {
    if (r && r->pause_at_end) {  // some channel's block of this epoch lies beyond the window: all of them stop here
      for (int c = 0; c < nch; ++c) r->paused = r->paused || st[c].status == 5;
      if (r->paused) {
        // a channel that diverged in the epoch before has not ended in THIS window: the next window's call finds that out again, first thing
        // (tell_team has sent its persistent team the stop descriptor already: harmless, persist_stop follows this break)
        for (int c = 0; c < nch; ++c)
          if (st[c].status == 4 && st[c].epochs_done == e) st[c].status = 0;
        break;
      }
    }
    int nb = 0;
    for (int c = 0; c < nch; ++c) {
      if (st[c].status != 0) continue;
      blocks[nb] = st[c].blk;
      slot[nb] = c;
      ++nb;
    }
    if (nb == 0) break;
    gc_scope_set_epoch(ctx, scope, mix, blocks, nb);
    const unsigned int tag = (unsigned int)(e + 1);
    const bool polled = gc_epoch_polled(ctx, scope, poll);
    const auto tt0 = std::chrono::steady_clock::now();
    if (persist) {
      for (int k = 0; k < nb; ++k) write_desc(slot[k], e, &blocks[k], 0ull);
    } else {
      rc = gc_launch_correlator(ctx, scope, blocks, nb, splits, splits == 1 ? partial : nullptr, partial, polled ? tag : 0u);
      if (rc) return rc;
    }
    const auto tt1 = std::chrono::steady_clock::now();
    bool signalled = false;
    if (polled) {
      // wait until every record of this launch carries the epoch tag (bounded: never hang here).  A busy device (other
      // contexts' kernels in front of ours) can delay a launch by much more than its own few microseconds: when the poll
      // budget runs out, the launch-per-epoch mode falls back to a stream synchronise and looks once more before giving up.
      const int arms6 = max_arms * 6;
      const int hs = persist ? 1 : splits;  // record groups per block as the host sees them (the persistent kernel's teams add up on the device)
      auto wait_tags = [&](std::chrono::milliseconds budget) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < nb * hs; ++k)
          for (int v = 0; v < arms6; ++v) {
            // record group of (block, split): blocks are numbered per launch, teams of the persistent kernel per channel
            const size_t grp = persist ? (size_t)slot[k] : (size_t)k;
            volatile gcorr::TaggedSlot* s = tagged + grp * GC_OUT_STRIDE + v;
            unsigned int spins = 0;
            while (s->tag != tag)
              if ((++spins & 4095u) == 0 && std::chrono::steady_clock::now() - t0 > budget) return false;
          }
        return true;
      };
      // first epoch of the persistent kernel: code load + launch of the whole grid
      signalled = wait_tags(std::chrono::milliseconds((persist && e == 0) ? std::max(5000, poll_timeout_ms) : poll_timeout_ms));
      if (!signalled && !persist && hipStreamSynchronize(ctx->stream) == hipSuccess) signalled = wait_tags(std::chrono::milliseconds(1));
      std::atomic_thread_fence(std::memory_order_acquire);
    }
    const auto tt2 = std::chrono::steady_clock::now();
    t_launch += std::chrono::duration<double, std::micro>(tt1 - tt0).count();
    t_wait += std::chrono::duration<double, std::micro>(tt2 - tt1).count();
    if (!signalled) {
      if (persist && GC_TUNE_ENV("GC_TRACK_TIMING")) {
        const hipError_t q = hipStreamQuery(ctx->stream);
        std::fprintf(stderr, "gc_track persistent: epoch %d records missing; stream: %s; first tags:", e, hipGetErrorString(q));
        for (int k = 0; k < std::min(nb, 16); ++k) std::fprintf(stderr, " %u", tagged[(size_t)slot[k] * GC_OUT_STRIDE].tag);
        std::fprintf(stderr, "\n");
      }
      if (persist) persist_stop();
      GC_HIP(hipStreamSynchronize(ctx->stream));
      if (polled) {
        persist_free();
        gc_set_error("gc_track: result records of epoch %d did not arrive", e);
        return GC_E_HIP;
      }
    }

    for (int k = 0; k < nb; ++k) {
      const int c = slot[k];
      double sums[GC_OUT_STRIDE];
      for (int v = 0; v < GC_OUT_STRIDE; ++v) {
        double acc = 0.0;
        for (int sp = 0; sp < (persist ? 1 : splits); ++sp)
          acc += polled ? ((v < max_arms * 6) ? tagged[(persist ? (size_t)c : (size_t)k * splits + sp) * GC_OUT_STRIDE + v].value : 0.0)
                        : partial[((size_t)k * splits + sp) * GC_OUT_STRIDE + v];
        sums[v] = acc;
      }
      advance(c, e, sums);
    }
  }

  // The reference processes channels one after the other and returns from the whole function at
  // the first short read (tracking.m:241-245): channels after the first aborted one are never run.
  int first_aborted = nch;
  bool any_range = false, any_diverged = false;
  for (int c = 0; c < nch; ++c) {
    if ((st[c].status == 2 || st[c].status == 4) && first_aborted == nch) first_aborted = c;
    any_diverged |= st[c].status == 4;
    // a channel that came in ended (resumed state) is not this call's short read
    any_range |= st[c].status == 2 && !(r && r->resume && r->state[c].status != 0);
  }
  for (int c = 0; c < nch; ++c) {
    if (c > first_aborted) {
      double* o = out + (size_t)c * GC_TRK_NFIELDS * n_epochs;
      std::fill(o, o + (size_t)GC_TRK_NFIELDS * n_epochs, 0.0);
      epochs_done[c] = 0;
    } else {
      epochs_done[c] = st[c].epochs_done;
    }
  }
  if (r)  // the loop state the next window's call starts from, in record coordinates
    for (int c = 0; c < nch; ++c) gcorr::devloop_state_out(r->state[c], st[c], origin);
  const bool persist_was = persist;
  if (persist) {  // teams that were not told to stop leave after n_epochs by themselves; the others were stopped above
    persist_stop();
    (void)hipStreamSynchronize(ctx->stream);
    persist_free();
  }
  if (GC_TUNE_ENV("GC_TRACK_TIMING") && n_epochs > 0)
    std::fprintf(stderr, "gc_track: per epoch %.2f us in the launch call / descriptor writes, %.2f us until the records arrived, %.2f us total (%s, %d workgroups per block)\n",
                 t_launch / n_epochs, t_wait / n_epochs,
                 std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_loop0).count() / n_epochs,
                 persist_was ? (persist_lane ? "persistent lane kernel" : "persistent kernel") : "launch per epoch", persist_was ? psplits_dev : splits);
  if (any_diverged) {
    gc_set_error("gc_track: a channel's code / carrier NCO became non-finite (all-zero correlator sums?); its records end there");
    return GC_E_INVALID;
  }
  if (any_range) {
    gc_set_error("Not able to read the specified number of samples for tracking");
    return GC_E_RANGE;
  }
  return GC_OK;
}

// ---- device-side loop closure (devloop.h) -----------------------------------------------------------------------
// Same contract as gc_track for what the persistent kernels are instantiated for (tests/test_gpu_ref_vectors.py runs every
// package of the reference through it): single-arm R = 1 channels on the transition-mask kernel; one- and two-arm channels of
// any rate, index scale and record format (int8 / int16, I/Q, Q/I, real), windowed tables (GPS L2C CL) included, on the lane
// kernel; the three-arm folds with a derived third arm (Galileo E1-C CBOC, BDS B1C wide-band) on int8 I/Q records; everything
// gc_track takes under GC_PREC_F64.  Anything else returns GC_E_UNSUPPORTED and the caller uses gc_track.
//
// gc_track_device_window is that loop on one window of a record (GcTrackResume, as gc_track_window): the DevLoopChan of a
// channel is filled from r->state - the first block cut from it exactly as devloop_post cuts any later one - and converted
// back after the launch.  Positions on the device count from the buffer's first sample, absoluteSample is recorded from the
// record's (DevLoopArgs::origin).  With r->pause_at_end a channel whose next block does not fit the buffer stops with status 5
// instead of 2; channels pause independently, so `budget[c]` (null: p->n_epochs) is the number of epochs channel c runs at
// most.  `whole_call`: this is a caller's complete call - the channels after the first ended one are zeroed as gc_track does;
// gc_track_file_device, which assembles a call from many windows, does that once at its end.
int gc_track_device_window(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init, double* out,
                           int32_t* epochs_done, GcTrackResume* r, const int32_t* budget, bool whole_call) {
  if (r && r->origin < 0) {
    r->paused = false;
    gc_set_error("gc_track_device: bad arguments");
    return GC_E_INVALID;
  }
  const bool f64 = ctx && ctx->precision == GC_PREC_F64;  // corr_f64.hip's device loop: every configuration gc_track takes
  LaunchScope scope;
  ChannelMix mix;
  bool single_r1 = true, all_derived = true;
  int rc = track_preamble(ctx, p, nch, init, out, epochs_done, r, "gc_track_device", &scope, &mix, [&](const HostChannel& hcn, int ci) -> int {
    if (!hcn.d_tab[0]) {
      gc_set_error("gc_track_device: channel %d not configured", ci);
      return GC_E_STATE;
    }
    const bool hder = gc_channel_is_derived(hcn);  // three arms, the third derived from the second inside the lane kernel
    all_derived = all_derived && hder;
    for (int a = 0; a < hcn.arms; ++a)
      if (!hcn.d_tab[a] || (!f64 && hcn.mult[a] != 1.0 && !(hder && a == 2))) {
        gc_set_error("gc_track_device: ramp multipliers other than a derived third arm are not covered (use gc_track)");
        return GC_E_UNSUPPORTED;
      }
    single_r1 = single_r1 && hcn.arms == 1 && hcn.index_scale == 1.0;
    return GC_OK;
  });
  if (rc) return rc;
  const int max_arms = scope.max_arms;
  // channels that share the device during this call (gc_track_multi): teams are sized for all of them
  const int nch_dev = ctx->concurrent_jobs ? std::max(nch, ctx->concurrent_channels) : nch;
  // three arms, the third derived from the second: Galileo E1-C CBOC (fold 5), BDS B1C wide-band (fold 4)
  const bool cboc = max_arms == 3 && all_derived && (p->pilot_combine == 5 || p->pilot_combine == 4);
  const bool i8c = ctx->if_dtype == GC_I8 && ctx->if_layout != GC_REAL;  // int8 I/Q or Q/I record
  if (f64) {
    if (((p->pilot_combine == 4 || p->pilot_combine == 5) && max_arms < 3) || (p->pilot_combine != 0 && max_arms < 2)) {
      gc_set_error("gc_track_device: pilot_combine %d does not match the channels' arms", p->pilot_combine);
      return GC_E_INVALID;
    }
  } else if ((max_arms > 2 && !cboc) || (p->pilot_combine > 3 && !cboc) || (p->pilot_combine != 0 && max_arms < 2) || (cboc && !i8c)) {
    gc_set_error("gc_track_device: configuration not covered by the persistent kernels (use gc_track)");
    return GC_E_UNSUPPORTED;
  }
  const int n_epochs = p->n_epochs;
  std::vector<gcorr::DevLoopChan> hc((size_t)nch);
  std::memset(hc.data(), 0, sizeof(gcorr::DevLoopChan) * (size_t)nch);
  int nominal_blksize = 0;
  int lowrate = 2;
  bool share = true;
  const int64_t origin = r ? r->origin : 0;
  gcorr::DevLoopArgs ha;
  std::memset(&ha, 0, sizeof ha);
  gcorr::devloop_set_loop(ha, *p, ctx->if_nsamples, origin, r && r->pause_at_end);
  for (int c = 0; c < nch; ++c) {
    gcorr::DevLoopChan& s = hc[c];
    gcorr::devloop_state_in(s, *p, init[c], (r && r->resume) ? &r->state[c] : nullptr, origin);
    s.epoch_budget = budget ? std::max(0, std::min(budget[c], n_epochs)) : n_epochs;
    // the first block, cut as devloop_post cuts every later one; not even one block: tracking.m:241-245
    if (s.status == 0) gcorr::devloop_first(&ha, s);
    if (s.status == 0 && s.epoch_budget <= 0) s.status = 1;
    // what selects the kernel and sizes the teams - hence the order of the float additions - comes from the channel's NOMINAL first
    // block (remainder 0, the acquired code frequency), which a resident call's first block is: every window of a record takes the
    // same kernel with the same teams as the whole record would
    gc_block nominal;
    std::memset(&nominal, 0, sizeof nominal);
    nominal.channel = init[c].channel;
    nominal.code_phase_step = init[c].code_freq / p->sampling_freq;
    nominal.blksize = (int)std::ceil(p->code_length / nominal.code_phase_step);
    nominal.el_spacing = p->el_spacing;
    if (c == 0) nominal_blksize = nominal.blksize;
    gc_block probe = nominal;
    probe.code_phase_step = nominal.code_phase_step * 1.001;  // head-room for the code NCO
    lowrate = std::min(lowrate, gc_block_lowrate_level(ctx, probe));
    share = share && gc_block_shares_el(ctx, nominal);
  }
  if (!i8c) lowrate = std::min(lowrate, 1);  // 16-sample chunks are an int8 I/Q format (corr_fast.hip)
  // transition-mask kernel (one-wave members) where it applies, else the lane kernel (16-wave member workgroups)
  bool any_window = false;
  for (int c = 0; c < nch; ++c)
    for (int a = 0; a < ctx->ch[init[c].channel].arms; ++a) any_window = any_window || ctx->ch[init[c].channel].window[a] != 0;
  const bool use_fast = single_r1 && lowrate > 0 && p->pilot_combine == 0 && gc_fast_table_mode(scope) == 0 && !ctx->force_generic && !any_window;
  int splits, msgs_per_member, lane_waves = gcorr::kLaneWaves;
  bool share_lane = true;
  const int spl = lowrate == 2 ? 16 : 8;
  if (use_fast) {
    // team size: just under one lane-chunk per lane and member — the epoch is a latency chain
    const int chunks = (int)(p->code_length / (p->code_freq_basis / p->sampling_freq) / spl) + 1;
    splits = std::max(1, std::min({32, (4 * ctx->compute_units + nch_dev - 1) / nch_dev, std::max(1, chunks / 32)}));
    if (const char* e = GC_TUNE_ENV("GC_DEVLOOP_MEMBERS")) splits = std::max(1, std::min(32, std::atoi(e)));  // closer polls <= 62 messages
    if (ctx->persist_member_cap > 0) splits = std::min(splits, ctx->persist_member_cap);
    msgs_per_member = 2;
  } else {
    for (int c = 0; c < nch; ++c) share_lane = share_lane && gc_block_shares_el_lane(ctx, hc[c].blk);
    // member workgroups per channel: about four 64-sample steps per lane; the closer polls (members - 1) * 6 * arms <= 64 messages
    const int nsamp = nominal_blksize;
    lane_waves = 8;  // measured best for both the 1-ms and the 4-ms packages (scripts/devloop_lane_sweep.py)
    if (const char* e = GC_TUNE_ENV("GC_DEVLOOP_WAVES")) lane_waves = std::max(1, std::min(8, std::atoi(e)));  // the device-loop instantiations are bounded to 8 waves
    const int max_members = max_arms == 1 ? 8 : max_arms == 2 ? 6 : 4;  // (members - 1) * 6 * arms messages <= 64 lanes
    splits = std::max(1, std::min({max_members, nsamp / (64 * lane_waves * 2), std::max(1, 2 * ctx->compute_units / nch_dev)}));
    if (const char* e = GC_TUNE_ENV("GC_DEVLOOP_MEMBERS")) splits = std::max(1, std::min(max_members, std::atoi(e)));
    if (ctx->persist_member_cap > 0) splits = std::min(splits, ctx->persist_member_cap);
    msgs_per_member = 6 * max_arms;
  }
  // Teams on one XCD each (default).  Not next to other contexts' persistent kernels (gc_track_multi): two kernels that pin
  // their teams to the same XCDs were measured to run one after the other (E1 lane kernel 32 ms = its own 11 ms + the L1 C/A
  // kernel's 21 ms beside it), spread over the device they overlap completely and lose nothing alone (88.7 vs 89.7 ms).
  const bool xcd_local = GC_TUNE_ENV("GC_DEVLOOP_SPREAD") == nullptr && !ctx->concurrent_jobs;

  ha.n_epochs = n_epochs;
  ha.splits = splits;
  ha.code_index_scale_is_one = 1;
  if (const char* e = GC_TUNE_ENV("GC_DEVLOOP_SCOPE")) ha.reserved = std::atoi(e);  // message scope (devloop.h): 0 system (default), 2 agent
  ha.timing = GC_TUNE_ENV("GC_DEVLOOP_TIMING") ? std::atoi(GC_TUNE_ENV("GC_DEVLOOP_TIMING")) : 0;  // 1: host + in-kernel phase clocks, 2: host only
  ha.prefetch = GC_TUNE_ENV("GC_DEVLOOP_NO_PREFETCH") ? 0 : 1;  // the next epoch's first chunk fetched during the closure (corr_fast.hip)
  gcorr::DevLoopArgs* d_args = nullptr;
  const size_t rec_bytes = sizeof(double) * (size_t)nch * GC_TRK_NFIELDS * n_epochs;
  const size_t part_bytes = sizeof(gcorr::msg_t) * (size_t)nch * splits * msgs_per_member * (use_fast ? 2 : 1),  // fast kernel: two alternating halves
                desc_bytes = sizeof(gcorr::msg_t) * (size_t)nch * gcorr::kDescWords;
  hipError_t e = gc_buf_reserve(ctx->trk[gc_context::TRK_CHAN], sizeof(gcorr::DevLoopChan) * (size_t)nch, false);
  if (e == hipSuccess) e = gc_buf_reserve(ctx->trk[gc_context::TRK_PART], part_bytes, false);
  if (e == hipSuccess) e = gc_buf_reserve(ctx->trk[gc_context::TRK_DESC], desc_bytes, false);
  if (e == hipSuccess) e = gc_buf_reserve(ctx->trk[gc_context::TRK_RECORDS], rec_bytes, false);
  if (e == hipSuccess) e = gc_buf_reserve(ctx->trk[gc_context::TRK_ARGS], sizeof ha, false);
  // the estimator's running sums are local to the launch (e % K): a call on a window delivers no in-loop C/N0, as gc_track_resume
  const int cno_nk = (!r && p->cno_interval > 1 && ctx->cno_out && p->cno_mode == GC_CNO_VSM) ? n_epochs / p->cno_interval : 0;
  const bool want_cno = cno_nk > 0 && (long long)nch * cno_nk <= ctx->cno_cap;
  const size_t cno_bytes = sizeof(double) * (size_t)nch * (size_t)std::max(cno_nk, 1);
  if (e == hipSuccess && want_cno) e = gc_buf_reserve(ctx->trk[gc_context::TRK_CNO], cno_bytes, false);
  if (e != hipSuccess) {
    gc_set_error("gc_track_device: %s", hipGetErrorString(e));
    return GC_E_NOMEM;
  }
  ha.one_writer = GC_TUNE_ENV("GC_DEVLOOP_ONE_WRITER") != nullptr;
  if (want_cno) {
    ha.cno = (double*)ctx->trk[gc_context::TRK_CNO].p;
    ha.cno_nk = cno_nk;
    if (hipMemsetAsync(ha.cno, 0, cno_bytes, ctx->stream) != hipSuccess) return GC_E_HIP;
  }
  ha.chan = (gcorr::DevLoopChan*)ctx->trk[gc_context::TRK_CHAN].p;
  ha.part_msg = (gcorr::msg_t*)ctx->trk[gc_context::TRK_PART].p;
  ha.desc_msg = (gcorr::msg_t*)ctx->trk[gc_context::TRK_DESC].p;
  ha.records = (double*)ctx->trk[gc_context::TRK_RECORDS].p;
  d_args = (gcorr::DevLoopArgs*)ctx->trk[gc_context::TRK_ARGS].p;
  if (e == hipSuccess) e = hipMemsetAsync(ha.records, 0, rec_bytes, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(ha.part_msg, 0, part_bytes, ctx->stream);
  std::vector<gcorr::msg_t> hdesc((size_t)nch * gcorr::kDescWords);
  for (int c = 0; c < nch; ++c) {
    unsigned long long q[gcorr::kDescWords] = {0};
    std::memcpy(q, &hc[c].blk, sizeof(gc_block));
    q[gcorr::kDescWords - 1] = (unsigned long long)hc[c].status;  // not 0: the team leaves before its first epoch
    for (int i = 0; i < gcorr::kDescWords; ++i) hdesc[(size_t)c * gcorr::kDescWords + i] = gcorr::msg_t{(unsigned int)q[i], (unsigned int)(q[i] >> 32), 1u, 0u};
  }
  if (e == hipSuccess) e = hipMemcpyAsync(ha.desc_msg, hdesc.data(), desc_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(ha.chan, hc.data(), sizeof(gcorr::DevLoopChan) * (size_t)nch, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_args, &ha, sizeof ha, hipMemcpyHostToDevice, ctx->stream);
  auto cleanup = [&]() { gc_persistent_done(ctx); };  // the buffers stay with the context (GcBuf); the grid leaves the device's ledger
  if (e != hipSuccess) {
    cleanup();
    gc_set_error("gc_track_device: %s", hipGetErrorString(e));
    return GC_E_NOMEM;
  }
  gcorr::KArgs a;
  std::memset(&a, 0, sizeof a);
  a.if_base = ctx->d_if;
  a.blocks = nullptr;
  a.chans = ctx->d_channels;
  a.fs = ctx->fs;
  a.inv_fs = 1.0 / ctx->fs;
  a.nblocks = nch;
  a.splits = splits;
  a.bpw = 1;
  a.stride = 1;
  a.share_el = share ? 1 : 0;
  a.devloop = d_args;
  a.xcd_swizzle = xcd_local ? 1 : 0;
  const unsigned int grid = xcd_local ? (unsigned int)(((nch + 7) / 8) * 8 * splits) : (unsigned int)(nch * splits);
  a.derived = cboc ? 1 : 0;
  if (f64)  // one 16-wave workgroup per channel: no team, nothing to halve when the grid does not fit
    rc = gc_launch_devloop_f64(ctx, d_args, nch);
  else
    rc = use_fast ? gc_launch_devloop(ctx, a, scope, grid, lowrate == 2, share) : gc_launch_devloop_lane(ctx, a, scope, grid, share_lane && !cboc, lane_waves);
  if (rc == GC_E_NOFIT && splits > 1 && !f64) {
    // the grid does not fit the device whole: the same call again with teams half the size (see gc_track's persistent launch);
    // a structural refusal (no instantiation for these tables / arms) is not retried
    cleanup();
    const int cap0 = ctx->persist_member_cap;
    ctx->persist_member_cap = (splits + 1) / 2;
    rc = gc_track_device_window(ctx, p, nch, init, out, epochs_done, r, budget, whole_call);
    ctx->persist_member_cap = cap0;
    return rc;
  }
  if (rc == GC_E_NOFIT) rc = GC_E_UNSUPPORTED;  // one member per channel and still no room: the caller falls back to gc_track
  if (rc == GC_OK) {
    ctx->last_track_mode = 2;
    ctx->last_track_team = f64 ? 1 : splits;
    ctx->last_kernel = f64 ? 6 : use_fast ? 1 : 0;  // gc_debug_last_kernel: the device loop's float64 / fast / lane instantiation
    const auto t_l = std::chrono::steady_clock::now();
    e = hipStreamSynchronize(ctx->stream);
    const auto t_k = std::chrono::steady_clock::now();
    if (e == hipSuccess) e = hipMemcpy(out, ha.records, rec_bytes, hipMemcpyDeviceToHost);
    if (ha.timing)
      std::fprintf(stderr, "devloop: launch + kernel %.3f ms (%.2f us per epoch), records to host %.3f ms\n",
                   std::chrono::duration<double, std::milli>(t_k - t_l).count(),
                   std::chrono::duration<double, std::micro>(t_k - t_l).count() / n_epochs,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_k).count());
    if (e == hipSuccess) e = hipMemcpy(hc.data(), ha.chan, sizeof(gcorr::DevLoopChan) * (size_t)nch, hipMemcpyDeviceToHost);
    if (e == hipSuccess && want_cno) e = hipMemcpy(ctx->cno_out, ha.cno, cno_bytes, hipMemcpyDeviceToHost);  // computed by the closer (devloop.h)
    if (e != hipSuccess) {
      gc_set_error("gc_track_device: %s", hipGetErrorString(e));
      rc = GC_E_HIP;
    }
  }
  cleanup();
  if (rc) return rc;
  // same early-return semantics as gc_track: channels after the first exhausted one are never run
  int first_aborted = nch;
  bool timeout = false, diverged = false, ranged = false;
  for (int c = 0; c < nch; ++c) {
    timeout |= hc[c].status == 3;
    diverged |= hc[c].status == 4;
    if (ha.timing == 1 && hc[c].epochs_done > 0)
      std::fprintf(stderr, "devloop ch %d: correlate %.2f us, wait partials %.2f us, close+publish %.2f us per epoch (closer)\n", c,
                   hc[c].pad[0] / hc[c].epochs_done * 0.01, hc[c].pad[1] / hc[c].epochs_done * 0.01, hc[c].pad[2] / hc[c].epochs_done * 0.01);
    if ((hc[c].status == 2 || hc[c].status == 4) && first_aborted == nch) first_aborted = c;
    // a channel that came in ended (resumed state) is not this call's short read
    ranged |= hc[c].status == 2 && !(r && r->resume && r->state[c].status != 0);
    if (r && hc[c].status == 5) r->paused = true;
  }
  if (timeout) {
    gc_set_error("gc_track_device: a team member timed out waiting for its epoch descriptor");
    return GC_E_HIP;
  }
  for (int c = 0; c < nch; ++c) {
    if (whole_call && c > first_aborted) {
      double* o = out + (size_t)c * GC_TRK_NFIELDS * n_epochs;
      std::fill(o, o + (size_t)GC_TRK_NFIELDS * n_epochs, 0.0);
      epochs_done[c] = 0;
    } else {
      epochs_done[c] = hc[c].epochs_done;
    }
  }
  if (r)  // the loop state the next window's call starts from, in record coordinates
    for (int c = 0; c < nch; ++c) gcorr::devloop_state_out(r->state[c], hc[c], origin);
  if (!r && p->cno_mode != GC_CNO_VSM) gc_fill_cno_host(ctx, p, nch, out, epochs_done);  // Calc_CNo_PLD: from the records, as everywhere
  if (diverged) {
    gc_set_error("gc_track_device: a channel's code / carrier NCO became non-finite (all-zero correlator sums?); its records end there");
    return GC_E_INVALID;
  }
  if (ranged) {
    gc_set_error("Not able to read the specified number of samples for tracking (channel slot %d)", first_aborted);
    return GC_E_RANGE;
  }
  return GC_OK;
}

extern "C" int gc_track_device(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init,
                               double* out, int32_t* epochs_done) {
  return gc_track_device_window(ctx, p, nch, init, out, epochs_done, nullptr, nullptr, true);
}
