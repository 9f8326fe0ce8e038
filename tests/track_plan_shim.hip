// The closed loops' planners of csrc/track_plan.h on the CPU: gc_plan_track_host and gc_plan_track_device over the context of channel
// FACTS that launch_plan_shim.hip makes (included: plan_shim_create, plan_shim_set_channel), the knobs as track_knobs_from_env reads
// them - nothing in the shim built like the library that ships, the process environment in the one built with -DGC_TUNING=1.
// Built by tests/test_track_plan_cpu.py with the flags of track.hip; no GPU is touched.
#include "launch_plan_shim.hip"

extern "C" {

// gc_track_multi: this context's call runs next to other contexts' with `channels` channels on the device in all
void tplan_shim_concurrent(void* vctx, int jobs, int channels) {
  gc_context* ctx = static_cast<gc_context*>(vctx);
  ctx->concurrent_jobs = jobs != 0;
  ctx->concurrent_channels = channels;
}

struct TplanCall {  // the fields of gc_track_params and gc_channel_init the planners read
  double sampling_freq, code_freq_basis, code_length, el_spacing;
  int pilot_combine, table_phase_count, n_epochs, nch;
  const int* channel;       // [nch]
  const double* code_freq;  // [nch]
};

struct TplanOut {
  int status;
  char message[160];
  // host
  int fast_nominal, splits, mode, team, share_lane_nominal, share_el, derived, poll, async, nthreads;
  // device
  int kernel, lowrate, share, share_lane, cboc, lane_waves, msgs_per_member, xcd_local;
  unsigned int grid;
  long long part_bytes, desc_bytes, rec_bytes;
};

}  // extern "C"

namespace {
struct Call {
  gc_track_params p = gc_track_params();
  std::vector<gc_channel_init> init;
  LaunchScope scope;
  ChannelMix mix;
  Call(const gc_context* ctx, const TplanCall& c) : init((size_t)c.nch) {
    p.sampling_freq = c.sampling_freq;
    p.code_freq_basis = c.code_freq_basis;
    p.code_length = c.code_length;
    p.el_spacing = c.el_spacing;
    p.pilot_combine = c.pilot_combine;
    p.table_phase_count = c.table_phase_count;
    p.n_epochs = c.n_epochs;
    for (int k = 0; k < c.nch; ++k) {  // as track.hip's track_preamble
      init[k] = gc_channel_init();
      init[k].channel = c.channel[k];
      init[k].code_freq = c.code_freq[k];
      gc_scope_add_channel(scope, ctx->ch[c.channel[k]]);
      mix.add(ctx->ch[c.channel[k]]);
    }
    gc_scope_set_level(ctx, scope, mix, 2);
  }
};
}  // namespace

extern "C" {

void tplan_shim_host(void* vctx, const TplanCall* c, int pause_at_end, TplanOut* o) {
  const gc_context* ctx = static_cast<const gc_context*>(vctx);
  const Call call(ctx, *c);
  const TrackHostPlan h = gc_plan_track_host(ctx, call.scope, call.mix, call.p, c->nch, call.init.data(), pause_at_end != 0, track_knobs_from_env());
  *o = TplanOut();
  o->status = h.status;
  std::memcpy(o->message, h.message, sizeof o->message);
  o->fast_nominal = h.fast_nominal;
  o->splits = h.splits;
  o->mode = h.mode;
  o->team = h.team;
  o->share_lane_nominal = h.share_lane_nominal;
  o->share_el = h.share_el;
  o->derived = h.derived;
  o->poll = h.poll;
  o->async = h.async;
  o->nthreads = h.nthreads;
}

// gc_track_device up to the launch: each channel's own check in the channels' order, then the plan.  member_cap: of a retry (0: none)
void tplan_shim_device(void* vctx, const TplanCall* c, int member_cap, TplanOut* o) {
  const gc_context* ctx = static_cast<const gc_context*>(vctx);
  *o = TplanOut();
  for (int k = 0; k < c->nch; ++k) {
    const char* text = nullptr;
    if ((o->status = gc_track_device_channel(ctx->ch[c->channel[k]], ctx->precision == GC_PREC_F64, &text)) != GC_OK) {
      std::snprintf(o->message, sizeof o->message, "%s", text);
      return;
    }
  }
  const Call call(ctx, *c);
  std::vector<gc_block> first((size_t)c->nch);
  for (int k = 0; k < c->nch; ++k) {  // what devloop_state_in puts there before the first block is cut
    first[k] = gc_block();
    first[k].channel = c->channel[k];
    first[k].el_spacing = c->el_spacing;
  }
  const TrackDevicePlan d = gc_plan_track_device(ctx, call.scope, call.p, c->nch, call.init.data(), first.data(), track_knobs_from_env(), member_cap);
  o->status = d.status;
  std::memcpy(o->message, d.message, sizeof o->message);
  o->kernel = d.kernel();
  o->lowrate = d.lowrate;
  o->share = d.share;
  o->share_lane = d.share_lane;
  o->cboc = d.cboc;
  o->team = d.team;
  o->lane_waves = d.lane_waves;
  o->msgs_per_member = d.msgs_per_member;
  o->xcd_local = d.xcd_local;
  o->grid = d.grid;
  o->part_bytes = (long long)d.part_bytes;
  o->desc_bytes = (long long)d.desc_bytes;
  o->rec_bytes = (long long)d.rec_bytes;
}

int tplan_shim_lane_member_cap(int max_arms) { return gc_lane_member_cap(max_arms); }
int tplan_shim_team_halved(int team) { return gc_team_halved(team); }
int tplan_shim_nch_dev(void* vctx, int nch) { return gc_track_nch_dev(static_cast<const gc_context*>(vctx), nch); }
int tplan_shim_poll_timeout_ms() { return track_knobs_from_env().poll_timeout_ms; }

}  // extern "C"
