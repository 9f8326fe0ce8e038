// track.hip — gc_track: the reference's tracking loop (GPS/GPS_L1CA/include/tracking.m:133-368
// and the 3-state / pilot variants GPS_L5C/include/tracking.m:255-382,
// GAL_E1C/include/tracking.m:236-348) with the correlator (lines 247-300) on the GPU, and gc_track_device: the same loop with
// the discriminators + loop filters (lines 302-335) on the GPU too.  Both entry points are plan, session, loop, finish:
//   plan     track_plan.h decides kernel, mode and teams from the channel facts and the knobs, before anything is reserved;
//   session  the persistent kernel of the call: the context's tracking buffers, the upload, one cooperative launch - tried again
//            with halved teams while its grid does not fit the device - and the stop / release at the end;
//   loop     gc_track closes the loop on the host with devloop.h's routine.  Normally nothing is launched per epoch: the host
//            writes each channel's next descriptor into host-mapped memory, the persistent kernel answers with tagged records
//            the host polls, every channel at its own pace (run_async) or all of an epoch together (run_lockstep: windows of a
//            streamed record).  What no persistent kernel covers (mixed ramp multipliers, three plain arms, float64) takes
//            run_lockstep with one correlator launch per epoch, polled or followed by a stream synchronise.
//            gc_track_device's loop is the kernel itself; the host waits for it and reads records and state back;
//   finish   track_finish: the reference's early return at the first channel that ended, epochs_done, the state a next
//            window starts from, the call's status.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <thread>

#include "devloop.h"
#include "track_plan.h"

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

namespace {

static_assert(sizeof(gcorr::msg_t) == kTrackMsgBytes && gcorr::kDescWords == kTrackDescWords, "track_plan.h sizes the message buffers");

// ---- what both loops share: descriptor messages, the persistent launch, the ending ------------------------------------------------
// One descriptor, kDescWords messages {word lo, word hi, tag, 0}: payload first, tag last - a device read that sees the tag sees
// the payload.
inline void desc_store(gcorr::msg_t* m, const unsigned long long (&q)[gcorr::kDescWords], unsigned int tag) {
  volatile unsigned int* w = reinterpret_cast<volatile unsigned int*>(m);
  for (int i = 0; i < gcorr::kDescWords; ++i) {
    w[4 * i + 0] = (unsigned int)q[i];
    w[4 * i + 1] = (unsigned int)(q[i] >> 32);
    w[4 * i + 3] = 0u;
  }
  std::atomic_thread_fence(std::memory_order_release);
  for (int i = 0; i < gcorr::kDescWords; ++i) w[4 * i + 2] = tag;
  std::atomic_thread_fence(std::memory_order_release);
}
// The block of the epoch `tag` - 1 (null: none) and the channel's status word: not 0 = the team leaves instead of correlating
inline void desc_encode(gcorr::msg_t* m, const gc_block* b, unsigned long long status_word, unsigned int tag) {
  unsigned long long q[gcorr::kDescWords] = {0};
  if (b) std::memcpy(q, b, sizeof(gc_block));
  q[gcorr::kDescWords - 1] = status_word;
  desc_store(m, q, tag);
}
// The team stops whatever epoch it is waiting for (tag 0xffffffff is accepted for any epoch)
inline void desc_encode_stop(gcorr::msg_t* m) {
  unsigned long long q[gcorr::kDescWords];
  for (unsigned long long& v : q) v = 3ull;
  desc_store(m, q, 0xffffffffu);
}

// Kernel arguments of a persistent launch: `nch` teams of `team` members, the loop's arguments on the device in `d_args`
gcorr::KArgs persistent_kargs(const gc_context* ctx, int nch, int team, bool share_el, bool derived, bool xcd_local, const gcorr::DevLoopArgs* d_args) {
  gcorr::KArgs a;
  std::memset(&a, 0, sizeof a);
  a.if_base = ctx->d_if;
  a.chans = ctx->d_channels;
  a.fs = ctx->fs;
  a.inv_fs = 1.0 / ctx->fs;
  a.nblocks = nch;
  a.splits = team;
  a.bpw = 1;
  a.stride = 1;
  a.share_el = share_el ? 1 : 0;
  a.derived = derived ? 1 : 0;
  a.devloop = d_args;
  a.xcd_swizzle = xcd_local ? 1 : 0;
  return a;
}

// A persistent grid the device cannot hold whole (the teams spin on each other's messages) is refused by its launch: the teams
// are halved until it fits - 192 channels x 1 member is still one launch for the whole call, where a launch per epoch cost 33-90 us
// per epoch from 48 GPS L1 C/A channels on.  attempt(team) stages and launches; only GC_E_NOFIT is answered with smaller teams (a
// structural refusal - no instantiation for these tables / arms - no team size can fix), after the refused grid has left the
// device's ledger.  Returns the last attempt's status.
template <class Attempt>
int launch_halving(gc_context* ctx, int team, Attempt&& attempt) {
  for (;;) {
    const int rc = attempt(team);
    if (rc != GC_E_NOFIT || team <= 1) return rc;
    (void)hipGetLastError();
    gc_persistent_done(ctx);
    team = gc_team_halved(team);
  }
}

// The reference processes channels one after the other and returns from the whole function at the first short read
// (tracking.m:241-245): channels after the first aborted one are never run - zeroed here when this is a caller's `whole_call`
// (gc_track_file_device assembles one from many windows and does it once at its end).  Sets epochs_done and, for a window, the
// state the next one starts from (record coordinates); returns the call's status.
int track_finish(const char* who, bool device, const gc_track_params* p, int nch, double* out, int32_t* epochs_done, GcTrackResume* r,
                 const gcorr::DevLoopChan* st, int64_t origin, bool whole_call) {
  const int n_epochs = p->n_epochs;
  int first_aborted = nch;
  bool any_range = false, any_diverged = false;
  for (int c = 0; c < nch; ++c) {
    if ((st[c].status == 2 || st[c].status == 4) && first_aborted == nch) first_aborted = c;
    any_diverged |= st[c].status == 4;
    // a channel that came in ended (resumed state) is not this call's short read
    any_range |= st[c].status == 2 && !(r && r->resume && r->state[c].status != 0);
  }
  for (int c = 0; c < nch; ++c) {
    if (whole_call && c > first_aborted) {
      double* o = out + (size_t)c * GC_TRK_NFIELDS * n_epochs;
      std::fill(o, o + (size_t)GC_TRK_NFIELDS * n_epochs, 0.0);
      epochs_done[c] = 0;
    } else {
      epochs_done[c] = st[c].epochs_done;
    }
  }
  if (r)
    for (int c = 0; c < nch; ++c) gcorr::devloop_state_out(r->state[c], st[c], origin);
  if (any_diverged) {
    gc_set_error("%s: a channel's code / carrier NCO became non-finite (all-zero correlator sums?); its records end there", who);
    return GC_E_INVALID;
  }
  if (any_range) {
    if (device) gc_set_error("Not able to read the specified number of samples for tracking (channel slot %d)", first_aborted);
    else gc_set_error("Not able to read the specified number of samples for tracking");
    return GC_E_RANGE;
  }
  return GC_OK;
}

// ---- gc_track: session ---------------------------------------------------------------------------------------------------------
// Pinned, device-visible descriptor and result buffers of the launch per epoch, and the host-mapped tagged 16-byte records
// (corr_common.h TaggedSlot) every polled mode answers with: a stream synchronise costs ~15-20 us of wake-up latency per epoch,
// polling the tags does not.
int host_buffers(gc_context* ctx, int nch) {
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
  return GC_OK;
}

// The host-fed persistent kernel of one gc_track call (devloop.h, host_loop): the loop is still closed on the host, but one
// cooperative launch polls the descriptors the host writes (send) and answers with tagged records.  Launch-per-epoch costs ~5 us
// of dispatch latency and ~13 us of kernel wall time per epoch; the persistent kernel answers in a few microseconds.  Its buffers
// stay with the context (GcBuf: freeing would wait for every stream of the device).
struct HostSession {
  gc_context* ctx;
  const TrackHostPlan& plan;
  const LaunchScope& scope;
  const TrackKnobs& knobs;
  const gc_channel_init* init;
  int nch, n_epochs;
  gcorr::DevLoopArgs pa;            // what the kernel got a copy of; the loop's own inputs are added after the launch (HostLoop)
  gcorr::msg_t* h_desc = nullptr;   // host-mapped descriptor messages [nch][kDescWords]
  bool active = false;              // the kernel is running
  int team = 0;                     // members per team of the last attempt
  hipError_t err = hipSuccess;      // what kept the last attempt from launching

  HostSession(gc_context* c, const TrackHostPlan& pl, const LaunchScope& s, const TrackKnobs& k, const gc_channel_init* in, int n, int ne)
      : ctx(c), plan(pl), scope(s), knobs(k), init(in), nch(n), n_epochs(ne) {
    std::memset(&pa, 0, sizeof pa);
  }
  bool lane() const { return plan.mode == GC_TRACK_PERSIST_LANE; }

  // reserves, uploads and launches for teams of `members`: a launcher's status, GC_E_HIP when it did not get that far
  int attempt(int members) {
    team = members;
    pa.n_epochs = n_epochs;
    pa.splits = team;
    pa.if_nsamples = ctx->if_nsamples;
    pa.host_loop = 1;
    pa.host_tagged = ctx->h_tagged_pinned;
    std::vector<gcorr::DevLoopChan> hc((size_t)nch);
    std::memset(hc.data(), 0, sizeof(gcorr::DevLoopChan) * (size_t)nch);
    for (int c = 0; c < nch; ++c) {
      hc[c].blk.channel = init[c].channel;  // table staging needs the channel of each team
      hc[c].epoch_budget = n_epochs;        // the host ends the run
    }
    const size_t chan_bytes = sizeof(gcorr::DevLoopChan) * (size_t)nch, desc_bytes = sizeof(gcorr::msg_t) * (size_t)nch * gcorr::kDescWords;
    const size_t part_bytes = gc_track_part_bytes(nch, team, !lane(), plan.max_arms);
    auto take = [&](int slot, size_t bytes, bool host) -> hipError_t { return gc_buf_reserve(ctx->trk[slot], bytes, host); };
    hipError_t e = take(gc_context::TRK_CHAN, chan_bytes, false);
    if (e == hipSuccess) e = take(gc_context::TRK_DESC, desc_bytes, false);
    if (e == hipSuccess) e = take(gc_context::TRK_PART, part_bytes, false);
    if (e == hipSuccess) e = take(gc_context::TRK_ARGS, sizeof pa, false);
    if (e == hipSuccess) e = take(gc_context::TRK_HDESC, desc_bytes, true);
    gcorr::DevLoopArgs* d_args = nullptr;
    if (e == hipSuccess) {
      pa.chan = (gcorr::DevLoopChan*)ctx->trk[gc_context::TRK_CHAN].p;
      pa.desc_msg = (gcorr::msg_t*)ctx->trk[gc_context::TRK_DESC].p;
      pa.part_msg = (gcorr::msg_t*)ctx->trk[gc_context::TRK_PART].p;
      d_args = (gcorr::DevLoopArgs*)ctx->trk[gc_context::TRK_ARGS].p;
      h_desc = (gcorr::msg_t*)ctx->trk[gc_context::TRK_HDESC].p;
      e = hipMemsetAsync(pa.part_msg, 0, part_bytes, ctx->stream);
    }
    if (e == hipSuccess) {
      std::memset(h_desc, 0, desc_bytes);
      pa.host_desc = h_desc;
      e = hipMemsetAsync(pa.desc_msg, 0, desc_bytes, ctx->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(pa.chan, hc.data(), chan_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_args, &pa, sizeof pa, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    err = e;
    if (e != hipSuccess) return GC_E_HIP;
    const gcorr::KArgs a = persistent_kargs(ctx, nch, team, plan.share_el, lane() && plan.derived, false, d_args);
    const unsigned int grid = (unsigned int)(nch * team);
    const int rc = lane() ? gc_launch_devloop_lane(ctx, a, scope, grid, plan.share_lane_nominal && !plan.derived, kTrackLaneWaves)
                          : gc_launch_devloop(ctx, a, scope, grid, plan.fast_nominal == 2, plan.share_el);
    if (rc != GC_OK) err = hipErrorUnknown;
    return rc;
  }

  // Launches the plan's persistent kernel; where that cannot be set up the call launches per epoch (active stays false).
  void open() {
    active = launch_halving(ctx, plan.team, [&](int members) { return attempt(members); }) == GC_OK;
    ctx->last_track_mode = active ? 1 : 0;
    if (active) {
      ctx->last_track_team = team;
      ctx->last_kernel = lane() ? 0 : 1;  // gc_debug_last_kernel: lane / fast kernel (persistent instantiation)
      if (knobs.debug) std::fprintf(stderr, "gc_track: persistent kernel: %d channels x %d members (%s kernel)\n", nch, team, lane() ? "lane" : "fast");
      return;
    }
    if (knobs.debug)
      std::fprintf(stderr, "gc_track: persistent kernel refused (%s): %d channels x %d members, lane %d - launching per epoch\n", hipGetErrorString(err), nch,
                   team, (int)lane());
    (void)hipGetLastError();
    release();
  }

  // descriptor of team c for epoch e (tag e + 1)
  void send(int c, int e, const gc_block* b, unsigned long long status_word) const {
    desc_encode(h_desc + (size_t)c * gcorr::kDescWords, b, status_word, (unsigned int)e + 1u);
  }
  // every team stops: those that were not told to leave after n_epochs by themselves
  void stop() const {
    for (int c = 0; c < nch; ++c) desc_encode_stop(h_desc + (size_t)c * gcorr::kDescWords);
  }
  // the kernel has ended (or was never launched): its grid leaves the device's ledger
  void release() {
    gc_persistent_done(ctx);
    h_desc = nullptr;
    active = false;
  }
};

// ---- gc_track: loop ------------------------------------------------------------------------------------------------------------
// The loop is closed by devloop.h's routine, the one the device loops run: its inputs are in ses.pa, its state is one DevLoopChan
// per channel.  Positions count from the IF buffer's first sample, which is record sample `origin` (gc_track_resume on a window: a
// run that starts in a window other than the record's first one must not read from that window's start).
struct HostLoop {
  gc_context* ctx;
  const gc_track_params* p;
  int nch;
  double* out;
  GcTrackResume* r;
  const TrackKnobs& knobs;
  const TrackHostPlan& plan;
  LaunchScope& scope;
  const ChannelMix& mix;
  HostSession& ses;
  const int n_epochs = p->n_epochs;
  const int64_t origin = r ? r->origin : 0;
  volatile gcorr::TaggedSlot* tagged = (volatile gcorr::TaggedSlot*)ctx->h_tagged_pinned;
  std::vector<gcorr::DevLoopChan> st = std::vector<gcorr::DevLoopChan>((size_t)nch);
  double t_launch = 0.0, t_wait = 0.0;  // GC_TRACK_TIMING: host time in the launch call / until the records arrived
  std::chrono::steady_clock::time_point t_loop0;

  // A channel whose cutter found no block (2 the record holds no whole block any more, 4 its NCO left the finite numbers; MATLAB
  // then fails in fread(fid, NaN)) ends there; its team of a persistent kernel is told to stop instead of waiting for epoch e.
  void tell_team(int c, int e) {
    if (ses.active && (st[c].status == 2 || st[c].status == 4)) ses.send(c, e, nullptr, 2ull);
  }

  // every channel's state and first block
  void start(const gc_channel_init* init) {
    gcorr::devloop_set_loop(ses.pa, *p, ctx->if_nsamples, origin, r && r->pause_at_end);
    std::memset(st.data(), 0, sizeof(gcorr::DevLoopChan) * (size_t)nch);
    for (int c = 0; c < nch; ++c) {
      gcorr::DevLoopChan& s = st[c];
      gcorr::devloop_state_in(s, *p, init[c], (r && r->resume) ? &r->state[c] : nullptr, origin);
      s.epoch_budget = n_epochs;
      if (s.status != 0) continue;  // ended in an earlier window
      gcorr::devloop_first(&ses.pa, s);
      tell_team(c, 0);
    }
    t_loop0 = std::chrono::steady_clock::now();
  }

  // tracking.m:249-348 for channel c at epoch e: the records, the discriminators and loop filters, the next block in st[c].blk.
  // Returns the channel's status: 0 = st[c].blk is the block of epoch e + 1.
  int advance(int c, int e, const double (&sums)[GC_OUT_STRIDE]) {
    gcorr::DevLoopChan& s = st[c];
    const HostChannel& hcn = ctx->ch[s.blk.channel];
    double* o = out + (size_t)c * GC_TRK_NFIELDS * n_epochs;
    // Arms: the device loops combine the pilot of a channel only when that channel HAS the arms the mode needs (gc_track_device tracks a
    // one-arm channel next to two-arm ones as data-only); this loop has always combined whenever pilot_combine is set - sums of arms
    // a channel lacks are zero, its discriminators NaN, the call ends with GC_E_INVALID.  Passing the arm count the mode needs keeps that
    // (devloop_post then also records the six Pilot_* fields of that one epoch: zeros, which is what the zero-filled `out` held there).
    const int arms = p->pilot_combine >= 4 ? 3 : p->pilot_combine != 0 ? std::max(hcn.arms, 2) : hcn.arms;
    const int ne = n_epochs;
    const gcorr::DevLoopPre pre = gcorr::devloop_pre(&ses.pa, s, s.blk, hcn.index_scale);
    gcorr::devloop_post<GC_MAX_ARMS>(&ses.pa, s, s.blk, e, sums, arms, hcn.index_scale, pre, [o, ne, e](int f, double v) { o[(size_t)f * ne + e] = v; });
    tell_team(c, e + 1);
    return s.status;
  }

  // the persistent kernel is stopped and the call is lost: the records of `epoch` did not arrive
  int lost(int epoch) {
    ses.release();
    gc_set_error("gc_track: result records of epoch %d did not arrive", epoch);
    return GC_E_HIP;
  }

  int run_async();
  int run_lockstep();
};

// Persistent kernel, every channel at its own pace.  The channels share nothing (tracking.m:133): each team waits for ITS
// descriptor and answers with ITS record group.  So the host does not wait for the slowest channel of an epoch before it closes
// any: whichever record group carries its channel's next tag is closed at once and that channel's next descriptor goes out, while
// the other teams are still correlating or their records are on the way.  Lock step cost an epoch the sum of the PCIe round trip,
// the team's work and the twelve closures; this way the round trip of one channel hides behind the others' work.  The channels are
// dealt out to plan.nthreads host threads, a contiguous share each; this thread serves the first.
int HostLoop::run_async() {
  const int arms6 = plan.max_arms * 6, nthreads = plan.nthreads, poll_timeout_ms = knobs.poll_timeout_ms;
  struct alignas(64) Slot {  // a channel's turn on a cache line of its own: neighbouring channels may belong to other threads
    int ep = 0;
    bool waiting = false;
    std::chrono::steady_clock::time_point sent;
  };
  std::vector<Slot> sl((size_t)nch);
  std::atomic<bool> is_lost{false};
  std::atomic<int> lost_epoch{0};
  auto serve = [&](int t) {
    const int c0 = (int)((long long)t * nch / nthreads), c1 = (int)((long long)(t + 1) * nch / nthreads);
    int outstanding = 0;
    const auto now0 = std::chrono::steady_clock::now();
    for (int c = c0; c < c1; ++c) {
      if (st[c].status != 0) continue;
      ses.send(c, 0, &st[c].blk, 0ull);
      sl[c].waiting = true;
      sl[c].sent = now0;
      ++outstanding;
    }
    unsigned int idle = 0, turns = 0;
    // a descriptor's time of sending, to the precision the timeout needs: refreshed every 256 turns of the poll loop WHETHER OR NOT
    // records arrived (a stamp refreshed only while idle stays at now0 for a whole busy run, and the first stall after
    // poll_timeout_ms of wall time would then read as a lost epoch), and again whenever the loop has been idle for 1024 turns
    auto stamp = now0;
    while (outstanding > 0 && !is_lost.load(std::memory_order_relaxed)) {
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
          ses.send(c, sl[c].ep, &st[c].blk, 0ull);
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
            is_lost.store(true, std::memory_order_relaxed);
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
  if (is_lost.load()) {
    ses.stop();
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return lost(lost_epoch.load());
  }
  t_wait = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_loop0).count();
  return GC_OK;
}

// All channels of an epoch together: a correlator launch per epoch, or the persistent kernel in a window of a streamed record
// (r->pause_at_end: all channels must end at the same epoch) and under GC_TRACK_LOCKSTEP.
int HostLoop::run_lockstep() {
  const bool persist = ses.active;
  const int splits = plan.splits, arms6 = plan.max_arms * 6, poll_timeout_ms = knobs.poll_timeout_ms;
  const int hs = persist ? 1 : splits;  // record groups per block as the host sees them (the persistent kernel's teams add up on the device)
  gc_block* blocks = ctx->h_blocks_pinned;
  double* partial = ctx->h_out_pinned;
  std::vector<int> slot((size_t)nch);
  for (int e = 0; e < n_epochs; ++e) {
    if (r && r->pause_at_end) {  // some channel's block of this epoch lies beyond the window: all of them stop here
      for (int c = 0; c < nch; ++c) r->paused = r->paused || st[c].status == 5;
      if (r->paused) {
        // a channel that diverged in the epoch before has not ended in THIS window: the next window's call finds that out again, first thing
        // (tell_team has sent its persistent team the stop descriptor already: harmless, the session's stop follows this break)
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
    const bool polled = gc_epoch_polled(ctx, scope, plan.poll);
    const auto tt0 = std::chrono::steady_clock::now();
    if (persist) {
      for (int k = 0; k < nb; ++k) ses.send(slot[k], e, &blocks[k], 0ull);
    } else {
      const int rc = gc_launch_correlator(ctx, scope, blocks, nb, splits, splits == 1 ? partial : nullptr, partial, polled ? tag : 0u);
      if (rc) return rc;
    }
    const auto tt1 = std::chrono::steady_clock::now();
    bool signalled = false;
    if (polled) {
      // wait until every record of this launch carries the epoch tag (bounded: never hang here).  A busy device (other
      // contexts' kernels in front of ours) can delay a launch by much more than its own few microseconds: when the poll
      // budget runs out, the launch-per-epoch mode falls back to a stream synchronise and looks once more before giving up.
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
      if (persist && knobs.timing) {
        const hipError_t q = hipStreamQuery(ctx->stream);
        std::fprintf(stderr, "gc_track persistent: epoch %d records missing; stream: %s; first tags:", e, hipGetErrorString(q));
        for (int k = 0; k < std::min(nb, 16); ++k) std::fprintf(stderr, " %u", tagged[(size_t)slot[k] * GC_OUT_STRIDE].tag);
        std::fprintf(stderr, "\n");
      }
      if (persist) ses.stop();
      GC_HIP(hipStreamSynchronize(ctx->stream));
      if (polled) return lost(e);
    }

    for (int k = 0; k < nb; ++k) {
      const int c = slot[k];
      double sums[GC_OUT_STRIDE];
      for (int v = 0; v < GC_OUT_STRIDE; ++v) {
        double acc = 0.0;
        for (int sp = 0; sp < hs; ++sp)
          acc += polled ? ((v < arms6) ? tagged[(persist ? (size_t)c : (size_t)k * splits + sp) * GC_OUT_STRIDE + v].value : 0.0)
                        : partial[((size_t)k * splits + sp) * GC_OUT_STRIDE + v];
        sums[v] = acc;
      }
      advance(c, e, sums);
    }
  }
  return GC_OK;
}

}  // namespace

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
  const TrackKnobs knobs = track_knobs_from_env();
  const TrackHostPlan plan = gc_plan_track_host(ctx, scope, mix, *p, nch, init, r && r->pause_at_end, knobs);
  if (plan.status) {
    gc_set_error("%s", plan.message);
    return plan.status;
  }
  if ((rc = host_buffers(ctx, nch))) return rc;
  const int n_epochs = p->n_epochs;
  std::fill(out, out + (size_t)nch * GC_TRK_NFIELDS * n_epochs, 0.0);
  ctx->last_track_mode = 0;
  ctx->last_track_team = plan.mode == GC_TRACK_F64 ? 1 : plan.splits;  // gc_debug_last_track_team; a persistent kernel's team below

  HostSession ses(ctx, plan, scope, knobs, init, nch, n_epochs);
  if (plan.persistent()) ses.open();
  const bool persist_was = ses.active, lane_was = ses.active && ses.lane();

  HostLoop loop{ctx, p, nch, out, r, knobs, plan, scope, mix, ses};
  loop.start(init);
  rc = (plan.async && ses.active) ? loop.run_async() : loop.run_lockstep();
  if (rc) return rc;

  if (ses.active) {  // teams that were not told to stop leave after n_epochs by themselves; the others were stopped in the loop
    ses.stop();
    (void)hipStreamSynchronize(ctx->stream);
    ses.release();
  }
  if (knobs.timing && n_epochs > 0)
    std::fprintf(stderr, "gc_track: per epoch %.2f us in the launch call / descriptor writes, %.2f us until the records arrived, %.2f us total (%s, %d workgroups per block)\n",
                 loop.t_launch / n_epochs, loop.t_wait / n_epochs,
                 std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - loop.t_loop0).count() / n_epochs,
                 persist_was ? (lane_was ? "persistent lane kernel" : "persistent kernel") : "launch per epoch", persist_was ? ses.team : plan.splits);
  return track_finish("gc_track", false, p, nch, out, epochs_done, r, loop.st.data(), loop.origin, true);
}

// ---- device-side loop closure (devloop.h) -----------------------------------------------------------------------
// Same contract as gc_track for what the persistent kernels are instantiated for (tests/test_gpu_ref_vectors.py runs every
// package of the reference through it): single-arm R = 1 channels on the transition-mask kernel; one- and two-arm channels of
// any rate, index scale and record format (int8 / int16, I/Q, Q/I, real), windowed tables (GPS L2C CL) included, on the lane
// kernel; the three-arm folds with a derived third arm (Galileo E1-C CBOC, BDS B1C wide-band) on int8 I/Q records; everything
// gc_track takes under GC_PREC_F64.  Anything else returns GC_E_UNSUPPORTED and the caller uses gc_track.
namespace {

// The in-loop C/N0 of a device loop (variance-summing method).  The estimator's running sums are local to the launch (e % K): a
// call on a window delivers no in-loop C/N0, as gc_track_resume.
struct DevCno {
  int nk = 0;
  bool want = false;
  size_t bytes = 0;
  DevCno(const gc_context* ctx, const gc_track_params* p, int nch, const GcTrackResume* r) {
    nk = (!r && p->cno_interval > 1 && ctx->cno_out && p->cno_mode == GC_CNO_VSM) ? p->n_epochs / p->cno_interval : 0;
    want = nk > 0 && (long long)nch * nk <= ctx->cno_cap;
    bytes = sizeof(double) * (size_t)nch * (size_t)std::max(nk, 1);
  }
};

// One attempt at the device loop's persistent launch with the plan's teams: the context's tracking buffers reserved, the channel
// states `hc` (untouched here), their first descriptors and the loop's arguments `ha` uploaded, the kernel launched.
int devloop_launch(gc_context* ctx, const LaunchScope& scope, const TrackDevicePlan& plan, const TrackKnobs& knobs, const DevCno& cno, int nch, int n_epochs,
                   const std::vector<gcorr::DevLoopChan>& hc, gcorr::DevLoopArgs& ha) {
  ha.n_epochs = n_epochs;
  ha.splits = plan.team;
  ha.code_index_scale_is_one = 1;
  ha.reserved = knobs.devloop_scope;
  ha.timing = knobs.devloop_timing;
  ha.prefetch = knobs.devloop_no_prefetch ? 0 : 1;  // the next epoch's first chunk fetched during the closure (corr_fast.hip)
  ha.one_writer = knobs.devloop_one_writer;
  const size_t chan_bytes = sizeof(gcorr::DevLoopChan) * (size_t)nch;
  hipError_t e = gc_buf_reserve(ctx->trk[gc_context::TRK_CHAN], chan_bytes, false);
  if (e == hipSuccess) e = gc_buf_reserve(ctx->trk[gc_context::TRK_PART], plan.part_bytes, false);
  if (e == hipSuccess) e = gc_buf_reserve(ctx->trk[gc_context::TRK_DESC], plan.desc_bytes, false);
  if (e == hipSuccess) e = gc_buf_reserve(ctx->trk[gc_context::TRK_RECORDS], plan.rec_bytes, false);
  if (e == hipSuccess) e = gc_buf_reserve(ctx->trk[gc_context::TRK_ARGS], sizeof ha, false);
  if (e == hipSuccess && cno.want) e = gc_buf_reserve(ctx->trk[gc_context::TRK_CNO], cno.bytes, false);
  if (e != hipSuccess) {
    gc_set_error("gc_track_device: %s", hipGetErrorString(e));
    return GC_E_NOMEM;
  }
  if (cno.want) {
    ha.cno = (double*)ctx->trk[gc_context::TRK_CNO].p;
    ha.cno_nk = cno.nk;
    if (hipMemsetAsync(ha.cno, 0, cno.bytes, ctx->stream) != hipSuccess) return GC_E_HIP;
  }
  ha.chan = (gcorr::DevLoopChan*)ctx->trk[gc_context::TRK_CHAN].p;
  ha.part_msg = (gcorr::msg_t*)ctx->trk[gc_context::TRK_PART].p;
  ha.desc_msg = (gcorr::msg_t*)ctx->trk[gc_context::TRK_DESC].p;
  ha.records = (double*)ctx->trk[gc_context::TRK_RECORDS].p;
  gcorr::DevLoopArgs* d_args = (gcorr::DevLoopArgs*)ctx->trk[gc_context::TRK_ARGS].p;
  e = hipMemsetAsync(ha.records, 0, plan.rec_bytes, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(ha.part_msg, 0, plan.part_bytes, ctx->stream);
  std::vector<gcorr::msg_t> hdesc((size_t)nch * gcorr::kDescWords);
  for (int c = 0; c < nch; ++c)  // epoch 0's descriptors; a status that is not 0: the team leaves before its first epoch
    desc_encode(hdesc.data() + (size_t)c * gcorr::kDescWords, &hc[c].blk, (unsigned long long)hc[c].status, 1u);
  if (e == hipSuccess) e = hipMemcpyAsync(ha.desc_msg, hdesc.data(), plan.desc_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(ha.chan, hc.data(), chan_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_args, &ha, sizeof ha, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) {
    gc_set_error("gc_track_device: %s", hipGetErrorString(e));
    return GC_E_NOMEM;
  }
  if (plan.f64) {  // one 16-wave workgroup per channel: no team, nothing to halve when the grid does not fit
    const int rc = gc_launch_devloop_f64(ctx, d_args, nch);
    return rc == GC_E_NOFIT ? GC_E_UNSUPPORTED : rc;
  }
  const gcorr::KArgs a = persistent_kargs(ctx, nch, plan.team, plan.share, plan.cboc, plan.xcd_local, d_args);
  return plan.use_fast ? gc_launch_devloop(ctx, a, scope, plan.grid, plan.lowrate == 2, plan.share)
                       : gc_launch_devloop_lane(ctx, a, scope, plan.grid, plan.share_lane && !plan.cboc, plan.lane_waves);
}

// Waits for the device loop and reads back its records, the channels' end states and the in-loop C/N0
int devloop_collect(gc_context* ctx, const gcorr::DevLoopArgs& ha, const TrackDevicePlan& plan, const DevCno& cno, int nch, double* out,
                    std::vector<gcorr::DevLoopChan>& hc) {
  const auto t_l = std::chrono::steady_clock::now();
  hipError_t e = hipStreamSynchronize(ctx->stream);
  const auto t_k = std::chrono::steady_clock::now();
  if (e == hipSuccess) e = hipMemcpy(out, ha.records, plan.rec_bytes, hipMemcpyDeviceToHost);
  if (ha.timing)
    std::fprintf(stderr, "devloop: launch + kernel %.3f ms (%.2f us per epoch), records to host %.3f ms\n",
                 std::chrono::duration<double, std::milli>(t_k - t_l).count(),
                 std::chrono::duration<double, std::micro>(t_k - t_l).count() / ha.n_epochs,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_k).count());
  if (e == hipSuccess) e = hipMemcpy(hc.data(), ha.chan, sizeof(gcorr::DevLoopChan) * (size_t)nch, hipMemcpyDeviceToHost);
  if (e == hipSuccess && cno.want) e = hipMemcpy(ctx->cno_out, ha.cno, cno.bytes, hipMemcpyDeviceToHost);  // computed by the closer (devloop.h)
  if (e != hipSuccess) {
    gc_set_error("gc_track_device: %s", hipGetErrorString(e));
    return GC_E_HIP;
  }
  return GC_OK;
}

}  // namespace

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
  const bool f64 = ctx && ctx->precision == GC_PREC_F64;
  LaunchScope scope;
  ChannelMix mix;
  int rc = track_preamble(ctx, p, nch, init, out, epochs_done, r, "gc_track_device", &scope, &mix, [&](const HostChannel& hcn, int ci) -> int {
    if (!hcn.d_tab[0]) {
      gc_set_error("gc_track_device: channel %d not configured", ci);
      return GC_E_STATE;
    }
    const char* text = nullptr;
    const int crc = gc_track_device_channel(hcn, f64, &text);
    if (crc) gc_set_error("%s", text);
    return crc;
  });
  if (rc) return rc;
  const TrackKnobs knobs = track_knobs_from_env();
  const int n_epochs = p->n_epochs;
  const int64_t origin = r ? r->origin : 0;
  gcorr::DevLoopArgs ha;
  std::memset(&ha, 0, sizeof ha);
  gcorr::devloop_set_loop(ha, *p, ctx->if_nsamples, origin, r && r->pause_at_end);
  std::vector<gcorr::DevLoopChan> hc((size_t)nch);
  std::memset(hc.data(), 0, sizeof(gcorr::DevLoopChan) * (size_t)nch);
  std::vector<gc_block> first((size_t)nch);
  for (int c = 0; c < nch; ++c) {
    gcorr::DevLoopChan& s = hc[c];
    gcorr::devloop_state_in(s, *p, init[c], (r && r->resume) ? &r->state[c] : nullptr, origin);
    s.epoch_budget = budget ? std::max(0, std::min(budget[c], n_epochs)) : n_epochs;
    // the first block, cut as devloop_post cuts every later one; not even one block: tracking.m:241-245
    if (s.status == 0) gcorr::devloop_first(&ha, s);
    if (s.status == 0 && s.epoch_budget <= 0) s.status = 1;
    first[c] = s.blk;
  }
  TrackDevicePlan plan = gc_plan_track_device(ctx, scope, *p, nch, init, first.data(), knobs, 0);
  if (plan.status) {
    gc_set_error("%s", plan.message);
    return plan.status;
  }
  const DevCno cno(ctx, p, nch, r);
  // a grid that does not fit the device whole: again with teams half the size, planned as the first (see launch_halving)
  rc = launch_halving(ctx, plan.team, [&](int members) {
    plan = gc_plan_track_device(ctx, scope, *p, nch, init, first.data(), knobs, members);
    return devloop_launch(ctx, scope, plan, knobs, cno, nch, n_epochs, hc, ha);
  });
  if (rc == GC_E_NOFIT) rc = GC_E_UNSUPPORTED;  // one member per channel and still no room: the caller falls back to gc_track
  if (rc == GC_OK) {
    ctx->last_track_mode = 2;
    ctx->last_track_team = plan.f64 ? 1 : plan.team;
    ctx->last_kernel = plan.kernel();
    rc = devloop_collect(ctx, ha, plan, cno, nch, out, hc);
  }
  gc_persistent_done(ctx);  // the buffers stay with the context (GcBuf); the grid leaves the device's ledger
  if (rc) return rc;
  bool timeout = false;
  for (int c = 0; c < nch; ++c) {
    timeout |= hc[c].status == 3;
    if (ha.timing == 1 && hc[c].epochs_done > 0)
      std::fprintf(stderr, "devloop ch %d: correlate %.2f us, wait partials %.2f us, close+publish %.2f us per epoch (closer)\n", c,
                   hc[c].pad[0] / hc[c].epochs_done * 0.01, hc[c].pad[1] / hc[c].epochs_done * 0.01, hc[c].pad[2] / hc[c].epochs_done * 0.01);
    if (r && hc[c].status == 5) r->paused = true;
  }
  if (timeout) {
    gc_set_error("gc_track_device: a team member timed out waiting for its epoch descriptor");
    return GC_E_HIP;
  }
  rc = track_finish("gc_track_device", true, p, nch, out, epochs_done, r, hc.data(), origin, whole_call);
  if (!r && p->cno_mode != GC_CNO_VSM) gc_fill_cno_host(ctx, p, nch, out, epochs_done);  // Calc_CNo_PLD: from the records, as everywhere
  return rc;
}

extern "C" int gc_track_device(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init,
                               double* out, int32_t* epochs_done) {
  return gc_track_device_window(ctx, p, nch, init, out, epochs_done, nullptr, nullptr, true);
}
