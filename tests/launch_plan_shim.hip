// The launch planner of csrc/launch_plan.h on the CPU: a context that holds channel FACTS only (arms, table lengths, multipliers,
// windows - no device memory), the scope builder over a descriptor list, the splits policies of gc_correlate / gc_replay_launch and
// gc_plan_launch.  Built by tests/test_launch_plan_cpu.py with the flags of corr_kernel.hip; no GPU is touched.
#include <cstdarg>

#include "../cu-sdr-collection_amd/csrc/track_plan.h"  // launch_plan.h + the closed loops' planners

void gc_set_error(const char*, ...) {}

extern "C" {

// device and record facts; the IF buffer "holds" if_nsamples samples
void* plan_shim_create(int compute_units, int dtype, int layout, int force_generic, int precision, unsigned long long if_nsamples) {
  static uint8_t no_record;
  gc_context* ctx = new gc_context();
  ctx->compute_units = compute_units;
  ctx->if_dtype = dtype;
  ctx->if_layout = layout;
  ctx->force_generic = force_generic != 0;
  ctx->precision = precision;
  ctx->d_if = &no_record;  // never read
  ctx->if_nsamples = if_nsamples;
  ctx->fs = 1.0;
  return ctx;
}

void plan_shim_destroy(void* ctx) { delete static_cast<gc_context*>(ctx); }

// six_fold: arm 2's table is the six-fold replica of arm 1's (what gc_set_code would find in BOC(6,1) next to BOC(1,1) tables)
void plan_shim_set_channel(void* vctx, int channel, int arms, double index_scale, const int* nent, const double* mult, const int* window,
                           int six_fold) {
  static int8_t no_table;
  HostChannel& c = static_cast<gc_context*>(vctx)->ch[channel];
  c = HostChannel();
  c.configured = true;
  c.arms = arms;
  c.index_scale = index_scale;
  for (int a = 0; a < arms; ++a) {
    c.nent[a] = nent[a];
    c.mult[a] = mult[a];
    c.window[a] = window[a];
    c.d_tab[a] = &no_table;  // never read
    c.h_tab[a].assign((size_t)nent[a], (int8_t)1);
  }
  if (six_fold && arms == 3)
    for (int k6 = 0; k6 < nent[2]; ++k6) c.h_tab[2][k6] = (((k6 + 5) / 6 + k6) & 1) ? -1 : 1;
}

struct PlanShimOut {
  int status;  // of the scope builder or the planner
  int kernel, fast, chunk, bpw, stride, wide, share_el, derived, waves, xcd_swizzle;
  int splits, period;
  unsigned int grid;
  long long total_wg;
};

static void put(PlanShimOut* o, const LaunchPlan& p) {
  o->kernel = p.kernel;
  o->fast = p.fast;
  o->chunk = p.chunk;
  o->bpw = p.bpw;
  o->stride = p.stride;
  o->wide = p.wide;
  o->share_el = p.share_el;
  o->derived = p.derived;
  o->waves = p.waves;
  o->xcd_swizzle = p.xcd_swizzle;
  o->grid = p.grid;
  o->total_wg = p.total_wg;
}

// gc_correlate (replay = 0) or gc_replay_prepare + gc_replay_launch (replay = 1) up to the launch; splits < 1: the caller's policy
void plan_shim_plan(void* vctx, long long n, const gc_block* blocks, int replay, int splits, int polled, PlanShimOut* o) {
  const gc_context* ctx = static_cast<const gc_context*>(vctx);
  *o = PlanShimOut();
  o->kernel = -2;
  LaunchScope s;
  if ((o->status = gc_scope_from_blocks(ctx, n, blocks, replay != 0, &s)) != GC_OK) return;
  if (splits < 1) splits = replay ? gc_replay_splits(ctx, s, n) : gc_correlate_splits(ctx, s, n);
  o->splits = splits;
  o->period = s.period;
  LaunchPlan p;
  if ((o->status = gc_plan_launch(ctx, s, n, splits, polled != 0, &p)) != GC_OK) return;
  put(o, p);
}

// gc_track's launch per epoch: the channel-set scope of `nch` channels, then the epoch's blocks (one per channel here)
void plan_shim_plan_epoch(void* vctx, int nb, const gc_block* blocks, int splits, int polled, PlanShimOut* o) {
  const gc_context* ctx = static_cast<const gc_context*>(vctx);
  *o = PlanShimOut();
  o->kernel = -2;
  LaunchScope s;
  ChannelMix mix;
  for (int k = 0; k < nb; ++k) {
    gc_scope_add_channel(s, ctx->ch[blocks[k].channel]);
    mix.add(ctx->ch[blocks[k].channel]);
  }
  gc_scope_set_level(ctx, s, mix, 2);
  gc_scope_set_epoch(ctx, s, mix, blocks, nb);
  o->splits = splits;
  LaunchPlan p;
  if ((o->status = gc_plan_launch(ctx, s, nb, splits, gc_epoch_polled(ctx, s, polled != 0), &p)) != GC_OK) return;
  put(o, p);
}

// ... and the splits gc_track gives that launch (gc_plan_track_host, track_plan.h) when the epoch's blocks are its channels' first:
// blocks of `code_length` chips of a code of rate `code_freq_basis`, the channels' code frequencies taken back from the blocks' steps
int plan_shim_track_splits(void* vctx, int nb, const gc_block* blocks, double sampling_freq, double code_freq_basis, double code_length) {
  const gc_context* ctx = static_cast<const gc_context*>(vctx);
  LaunchScope s;
  ChannelMix mix;
  std::vector<gc_channel_init> init((size_t)nb);
  for (int k = 0; k < nb; ++k) {
    gc_scope_add_channel(s, ctx->ch[blocks[k].channel]);
    mix.add(ctx->ch[blocks[k].channel]);
    init[k] = gc_channel_init();
    init[k].channel = blocks[k].channel;
    init[k].code_freq = blocks[k].code_phase_step * sampling_freq;
  }
  gc_scope_set_level(ctx, s, mix, 2);
  gc_track_params p = gc_track_params();
  p.sampling_freq = sampling_freq;
  p.code_freq_basis = code_freq_basis;
  p.code_length = code_length;
  p.el_spacing = blocks[0].el_spacing;
  p.n_epochs = 1;
  return gc_plan_track_host(ctx, s, mix, p, nb, init.data(), false, TrackKnobs()).splits;
}

}  // extern "C"
