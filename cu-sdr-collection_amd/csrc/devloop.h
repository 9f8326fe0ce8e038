// devloop.h — device-side loop closure: the tracking loop of tracking.m:184-348 without the
// per-epoch host round trip.  ONE persistent launch runs all epochs; the workgroups that share a channel (its
// "team": one per split) exchange two kinds of self-validating 16-byte messages per epoch — {payload, epoch tag}
// written by ONE store instruction and read by ONE load instruction, both at system scope (sc0 sc1: no cache on the
// way), so no flag, counter, atomic or fence is needed:
//   fast kernel (corr_fast.hip): all-gather - every member stores its six partial sums as two messages {f, f, f, tag}, polls the
//   whole team's messages (one per lane), adds them in double in a fixed order and closes the loop ITSELF (devloop_pre /
//   devloop_post below); identical inputs give identical descriptors, so nothing is broadcast: ONE one-way propagation delay
//   per epoch.  Member 0 writes the epoch's records.
//   lane kernel (corr_lane.hip): gather and broadcast - member 0 (the closer) polls the other members' messages, closes the
//   loop, writes the records and publishes the next descriptor as ten messages {word, tag} that the other members poll.
// Channels never wait for each other.  All team workgroups must be co-resident: the launch is cooperative.  Polls are bounded.
//
// The closure itself - tracking.m:219-222, 241-245, 273-283, 302-348 in float64, statement for statement in the reference's
// operation order - exists ONCE, here, as __host__ __device__ code: devloop_cut (the next block), devloop_pre / devloop_post
// (one epoch), gcorr::cno_ratio (the C/N0 tail) and the loop state DevLoopChan with its conversion from and to the public
// gc_channel_state.  The device loops call it from their kernels, gc_track's host loop (track.hip) from the thread that polls
// the records, tests/loop_closure_shim.hip from a CPU test that replays the reference's recorded sums through it.
#pragma once
#include "gc_internal.h"
#include "replica_f64.h"  // kPi

namespace gcorr {

constexpr int kDescWords = 10;  // gc_block (9 x 8 bytes) + status word

typedef unsigned int msg_t __attribute__((ext_vector_type(4)));  // one 16-byte message

struct DevLoopChan {
  gc_block blk;              // initial descriptor (host) / last descriptor (closer)
  int status;                // 0 running, 1 all epochs done, 2 record exhausted (tracking.m:241-245), 3 wait timed out,
                             // 4 code NCO diverged: codeFreq not finite / not positive (MATLAB's fread(fid, NaN) errors there),
                             // 5 paused: the next block does not fit this window of the record (DevLoopArgs::pause)
  int epochs_done;
  int epoch_budget;          // epochs this launch runs for THIS channel (<= DevLoopArgs::n_epochs): channels pause at different epochs of
                             // a windowed record, so the calls that follow owe them different numbers of epochs
  int pad0;
  // loop state, touched by the closing member only
  long long pos;
  double code_freq, code_freq_basis, rem_code;
  double carr_freq, carr_basis, rem_carr;
  double old_code_nco, old_code_err, old_carr_nco, old_carr_err;  // 2nd-order PLL / DLL
  double d2_carr_err, d_carr_err;                                 // 3-state PLL
  double pad[3];
  int table_phase;  // GPS L2C CLCodePhase (1-based segment of the CL code; 0: none), GPS_L2C/include/tracking.m:261,357-360
  int cno_n;        // C/N0 intervals completed; cno_value is the latest one when cno_ready
  double cno_z0, cno_s1, cno_s2, cno_value;  // running sums of Z - Z0 and (Z - Z0)^2 over the current interval (Z = I_P^2 + Q_P^2)
  int cno_ready, pad_i;
};

struct DevLoopArgs {
  DevLoopChan* chan;   // [nch]
  msg_t* desc_msg;     // [nch][kDescWords]   {word lo, word hi, tag, 0}, tag = epoch + 1
  msg_t* part_msg;     // [nch][splits][2]    {f, f, f, tag}  (fast kernel) | [nch][members][12] {double, tag, 0} (lane kernel)
  double* records;     // [nch][GC_TRK_NFIELDS][n_epochs]
  gc_track_params prm;
  double tau1code, tau2code, tau1carr, tau2carr;
  // the loop filters' quotients (tau2/tau1, int_time/tau1: tracking.m:308-309,327-328), formed once on the host - four
  // dependent float64 divisions per epoch otherwise
  double k1code, k2code, k1carr, k2carr;
  unsigned long long if_nsamples;
  int n_epochs;
  int splits;
  int code_index_scale_is_one;  // R == 1 (the only case wired up)
  int reserved;                 // message scope (msg_load / msg_store): 0 = system
  int timing;                   // GC_DEVLOOP_TIMING: the closer accumulates its phase clocks in DevLoopChan::pad (costs ~1 us per epoch)
  int prefetch;                 // fast kernel: fetch the next epoch's first chunk during the closure (corr_fast.hip; GC_DEVLOOP_NO_PREFETCH=1 in the tuning build: 0)
  int pause;                    // a windowed record (gc_track_device_resume): a channel whose next block does not fit the buffer stops with
                                // status 5 (more of the record follows) instead of 2 (tracking.m:241-245 is the END of the file)
  long long origin;             // record index of the buffer's sample 0: positions (DevLoopChan::pos, gc_block::first_sample) count from the
                                // buffer's start, absoluteSample is recorded from the record's
  // Host-fed variant (gc_track's persistent mode): the HOST closes the loop (tracking.m:302-335 stay where the reference has
  // them) but nothing is launched per epoch: member 0 of a team polls the channel's descriptor messages in host-mapped
  // memory (tag = epoch + 1), relays them to its team through desc_msg, and every member writes its six partial sums as
  // tagged 16-byte records straight into host-mapped memory, where the host polls them.
  // C/N0 by the variance-summing method inside the loop (gc_track_params::cno_interval): [nch][cno_nk], device memory
  double* cno;
  int cno_nk, one_writer;  // GC_DEVLOOP_ONE_WRITER (tuning): member 0 stores the whole record
  int host_loop;
  const msg_t* host_desc;       // [nch][kDescWords], host-mapped
  void* host_tagged;            // TaggedSlot [nch][splits][GC_OUT_STRIDE], host-mapped
};

// ---- host: what an entry point fills in before the loop runs -------------------------------------------------------
// Common/calcLoopCoef.m:41-45
inline void calc_loop_coef(double lbw, double zeta, double k, double* tau1, double* tau2) {
  const double wn = lbw * 8 * zeta / (4 * zeta * zeta + 1);
  *tau1 = k / (wn * wn);
  *tau2 = 2.0 * zeta / wn;
}

// The closure's own inputs of DevLoopArgs: the parameters, the loop coefficients and their quotients, the window of the record.
inline void devloop_set_loop(DevLoopArgs& a, const gc_track_params& p, unsigned long long if_nsamples, long long origin, bool pause) {
  a.prm = p;
  calc_loop_coef(p.dll_noise_bw, p.dll_damping, 1.0, &a.tau1code, &a.tau2code);   // tracking.m:100-102
  calc_loop_coef(p.pll_noise_bw, p.pll_damping, 0.25, &a.tau1carr, &a.tau2carr);  // tracking.m:109-110
  a.k1code = a.tau2code / a.tau1code;
  a.k2code = p.int_time / a.tau1code;
  a.k1carr = a.tau2carr / a.tau1carr;
  a.k2carr = p.int_time / a.tau1carr;
  a.if_nsamples = if_nsamples;
  a.origin = origin;
  a.pause = pause ? 1 : 0;
}

// Loop state of a channel that starts (g == nullptr: tracking.m:150-168) or continues where the previous window stopped.
// gc_channel_state counts positions from the start of the record, DevLoopChan from the buffer's sample 0 = record sample `origin`.
inline void devloop_state_in(DevLoopChan& s, const gc_track_params& p, const gc_channel_init& in, const gc_channel_state* g, long long origin) {
  s.pos = p.skip_samples + in.code_phase - 1 - origin;       // :150-152
  s.code_freq = s.code_freq_basis = in.code_freq;           // :163 / GPS_L5C :165
  s.carr_freq = s.carr_basis = in.acquired_freq;            // :167-168
  s.table_phase = in.table_phase;
  s.blk.channel = in.channel;
  s.blk.el_spacing = p.el_spacing;
  if (!g) return;
  if (g->status != 0) s.status = 2;  // ended before: does not run
  s.pos = g->next_sample - origin;
  s.code_freq = g->code_freq;
  s.rem_code = g->rem_code_phase;
  s.carr_freq = g->carr_freq;
  s.rem_carr = g->rem_carr_phase;
  s.old_code_nco = g->old_code_nco;
  s.old_code_err = g->old_code_error;
  s.old_carr_nco = g->old_carr_nco;
  s.old_carr_err = g->old_carr_error;
  s.d_carr_err = g->d_carr_error;
  s.d2_carr_err = g->d2_carr_error;
  s.table_phase = g->table_phase;
}
inline void devloop_state_out(gc_channel_state& g, const DevLoopChan& s, long long origin) {
  g.next_sample = s.pos + origin;
  g.code_freq = s.code_freq;
  g.rem_code_phase = s.rem_code;
  g.carr_freq = s.carr_freq;
  g.rem_carr_phase = s.rem_carr;
  g.old_code_nco = s.old_code_nco;
  g.old_code_error = s.old_code_err;
  g.old_carr_nco = s.old_carr_nco;
  g.old_carr_error = s.old_carr_err;
  g.d_carr_error = s.d_carr_err;
  g.d2_carr_error = s.d2_carr_err;
  g.table_phase = s.table_phase;
  g.status = (s.status == 2 || s.status == 4) ? 2 : 0;  // ended | running, paused or out of epochs
  g.reserved = 0;
}

// ---- host and device: the closure ----------------------------------------------------------------------------------
// |Pav / (2*Nv)| of CNoVSM.m:38-47 / Calc_CNo_PLD.m:47-68 from the mean and the N-1 variance of Z = I^2 + Q^2:
// Pav = sqrt(Zm^2 - Zv), Nv = (Zm - Pav)/2; the square root of a negative number is imaginary, abs() of the complex quotient
__host__ __device__ inline double cno_ratio(double zm, double zv) {
  const double d = zm * zm - zv;
  if (d >= 0.0) {
    const double pav = sqrt(d);
    return fabs(pav / (zm - pav));
  }
  const double s2 = -d;  // Pav imaginary: |i*s / (Zm - i*s)|
  return sqrt(s2 / (zm * zm + s2));
}

// The block a channel correlates next (tracking.m:219-222), cut from the four numbers of its loop state that decide it.  status: 0,
// or why there is no such block: 4 the code step is not finite / not positive or the carrier frequency NaN (all-zero sums give
// atan(0/0)): no block can be cut from it; 2 the block does not lie inside the buffer (:241-245), 5 instead when more of the record
// follows this window (DevLoopArgs::pause).  `spent`: the channel has run its epochs, 1 whatever the block is like.  Of dl it reads
// prm, if_nsamples and pause.  Arguments and result are values: devloop_post calls it on the epoch's new state while the old one is
// still in `st`, which keeps the device loops' instruction stream what it was when these statements stood there.
struct DevLoopCut {
  double step;  // code chips per sample
  int n;        // samples
  int status;
};

// (int)ceil(x).  Host C++ leaves the conversion of a NaN or of a value beyond int undefined - a diverged code NCO gets here -
// where the device's instruction saturates: the host saturates by hand, the device loops keep the instruction they had.
__host__ __device__ inline int ceil_to_int(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)ceil(x);
#else
  return (x >= -2147483648.0 && x < 2147483647.0) ? (int)ceil(x) : 2147483647;
#endif
}

__host__ __device__ inline DevLoopCut devloop_cut(const DevLoopArgs* __restrict__ dl, long long pos, double rem_code, double code_freq, double carr_freq,
                                                  int epochs_done = 0, int epoch_budget = 1) {
  const gc_track_params& p = dl->prm;
  const double step = code_freq / p.sampling_freq;
  const int n = ceil_to_int((p.code_length - rem_code) / step);
  int status = 0;
  if (epochs_done >= epoch_budget)
    status = 1;
  else if (!(step > 0.0) || !(step < 1e6) || !(carr_freq == carr_freq))
    status = 4;
  else if (pos < 0 || (unsigned long long)(pos + n) > dl->if_nsamples)
    status = dl->pause ? 5 : 2;  // paused: the state is the one the next window's call starts from
  return DevLoopCut{step, n, status};
}

// The cut block's geometry into the descriptor; channel, correlator spacing and table offsets of b stay as they are.
__host__ __device__ inline void devloop_put(gc_block& b, const DevLoopCut& c, long long pos, double rem_code, double carr_freq, double rem_carr) {
  b.blksize = c.n;
  b.first_sample = pos;
  b.rem_code_phase = rem_code;
  b.code_phase_step = c.step;
  b.carr_freq = carr_freq;
  b.rem_carr_phase = rem_carr;
}

// A channel's first block of a call, cut from the state devloop_state_in left, as devloop_post cuts every later one.
inline void devloop_first(const DevLoopArgs* dl, DevLoopChan& s) {
  const DevLoopCut c = devloop_cut(dl, s.pos, s.rem_code, s.code_freq, s.carr_freq);
  if (dl->prm.table_phase_count > 0 && s.table_phase > 0) s.blk.table_offset[1] = (int)dl->prm.code_length * (s.table_phase - 1);  // GPS_L2C tracking.m:261
  devloop_put(s.blk, c, s.pos, s.rem_code, s.carr_freq, s.rem_carr);
  s.status = c.status;
}

// One channel, one epoch: lane-uniform float64 restatement of tracking.m:273-348, every pilot handling mode included, in two
// parts, so that the closer of the fast kernel can run the first one while the other members' partial sums are still on their way:
//   devloop_pre   what depends only on the epoch's own geometry and NCO state: the remainders the next block starts from
//                 (tracking.m:273-283: one fmod, one division);
//   devloop_post  what needs the sums: discriminators, loop filters, records, the next block (tracking.m:302-335, 219-222).
// `st` is the caller's copy of the loop state (the fast kernel keeps it in registers across epochs; the host loop's own).
// `sums`: 6 per arm; R: the channel's index scale.  On return b holds the next epoch's block geometry; the return value is the
// channel status (0 = keep going).
struct DevLoopPre {
  double rem_code_new, rem_carr_new;
};

__host__ __device__ inline DevLoopPre devloop_pre(const DevLoopArgs* __restrict__ dl, const DevLoopChan& st, const gc_block& b, double R) {
  const gc_track_params& p = dl->prm;
  const int n = b.blksize;
  const double step = b.code_phase_step;
  DevLoopPre r;
  const double t_last = ((n - 1) * step + st.rem_code) * R;                    // tcode(blksize), :273 / GAL_E1C :268
  r.rem_code_new = (R != 1.0) ? (t_last / R + step) - p.code_length : (t_last + step) - p.code_length;
  const double time_n = (double)n / p.sampling_freq;                            // :280-283
  const double trig_n = ((st.carr_freq * 2.0 * kPi) * time_n) + st.rem_carr;
  r.rem_carr_new = fmod(trig_n, 2 * kPi);
  return r;
}

template <int MAXARMS, class Rec>
__host__ __device__ inline int devloop_post(const DevLoopArgs* __restrict__ dl, DevLoopChan& st, gc_block& b, int e, const double (&sums)[6 * MAXARMS],
                                   int arms, double R, const DevLoopPre& pre, Rec&& rec, bool do_cno = true, long long cno_slot = -1) {
  // rec(field, value) takes the epoch's record: straight to device memory (lane kernel) or into registers, to be stored by
  // devloop_commit AFTER the next descriptor is on its way (fast kernel)
  const gc_track_params& p = dl->prm;
  const int n = b.blksize;
  const double i_e = sums[0], q_e = sums[1], i_p = sums[2], q_p = sums[3], i_l = sums[4], q_l = sums[5];
  // do_cno: in an all-gather team every member runs this closure, ONE of them (not the one that writes the records) keeps the
  // C/N0 sums - they feed nothing back, so the other members need not carry them on the epoch's critical path; that member
  // stores the finished value itself (cno_slot >= 0), the single closer of the lane kernel leaves it to devloop_commit
  if (do_cno && p.cno_interval > 0 && dl->cno) {
    // CNoVSM(I_P(loopCnt-K+1:loopCnt), Q_P(...), T) when rem(loopCnt, K) == 0 (tracking.m:351-358; Common/CNoVSM.m:38-47):
    // Z = I^2 + Q^2, Zm = mean(Z), Zv = var(Z) (N-1), Pav = sqrt(Zm^2 - Zv), Nv = (Zm - Pav)/2, 10*log10(|Pav/(2*Nv)/T|).
    // Sums of Z - Z0 (Z0 = the interval's first Z) keep the one-pass variance free of cancellation.
    const int K = p.cno_interval, kk = e % K;
    const double z = i_p * i_p + q_p * q_p;
    if (kk == 0) {
      st.cno_z0 = z;
      st.cno_s1 = 0.0;
      st.cno_s2 = 0.0;
    }
    const double dz = z - st.cno_z0;
    st.cno_s1 += dz;
    st.cno_s2 += dz * dz;
    st.cno_ready = 0;
    if (kk == K - 1 && K > 1) {
      const double m = st.cno_s1 / K, zm = st.cno_z0 + m, zv = (st.cno_s2 - st.cno_s1 * m) / (K - 1);
      st.cno_value = 10.0 * log10(cno_ratio(zm, zv) / p.cno_acc_time);
      st.cno_n = (e + 1) / K;
      st.cno_ready = 1;
      if (cno_slot >= 0 && st.cno_n >= 1 && st.cno_n <= dl->cno_nk) {
        dl->cno[cno_slot * dl->cno_nk + st.cno_n - 1] = st.cno_value;
        st.cno_ready = 0;
      }
    }
  }
  rec(GC_TRK_ABSOLUTE_SAMPLE, (double)(st.pos + dl->origin));
  rec(GC_TRK_REM_CODE_PHASE, st.rem_code);
  rec(GC_TRK_REM_CARR_PHASE, st.rem_carr);
  const double rem_code_new = pre.rem_code_new;
  const double rem_carr_new = pre.rem_carr_new;
  double carr_err = atan(q_p / i_p) / (2.0 * kPi);                              // :305
  double code_err = (sqrt(i_e * i_e + q_e * q_e) - sqrt(i_l * i_l + q_l * q_l)) /
                    (sqrt(i_e * i_e + q_e * q_e) + sqrt(i_l * i_l + q_l * q_l));  // :322-323
  if constexpr (MAXARMS >= 2) {
  if (p.pilot_combine != 0 && arms >= 2) {
    double p6[6] = {sums[6], sums[7], sums[8], sums[9], sums[10], sums[11]};  // the pilot arm as correlated
    if constexpr (MAXARMS >= 3) {
      if (p.pilot_combine == 5 && arms >= 3) {
        // Galileo E1-C CBOC(6,1,1/11): arms {data, pilot BOC(1,1), pilot BOC(6,1)} folded in phase, then as mode 2 (track.hip)
        const double a11 = sqrt(10.0 / 11.0), a61 = -sqrt(1.0 / 11.0);
#pragma unroll
        for (int v = 0; v < 6; ++v) p6[v] = a11 * sums[6 + v] + a61 * sums[12 + v];
      } else if (p.pilot_combine == 4 && arms >= 3) {
        // BDS B1C wide-band: arms {data, pilot BOC(1,1), pilot BOC(6,1)} -> one pilot (WB_tracking.m:364-369; track.hip)
        const double a61 = -sqrt(4.0 / 33.0), a11 = sqrt(29.0 / 33.0);
#pragma unroll
        for (int x = 0; x < 3; ++x) {
          const double i11 = sums[6 + 2 * x], q11 = sums[7 + 2 * x], i61 = sums[12 + 2 * x], q61 = sums[13 + 2 * x];
          p6[2 * x] = a61 * i61 + a11 * q11;
          p6[2 * x + 1] = a61 * q61 - a11 * i11;
        }
      }
    }
    const double pi_e = p6[0], pq_e = p6[1], pi_p = p6[2], pq_p = p6[3], pi_l = p6[4], pq_l = p6[5];
    double carr_err_q;
    if (p.pilot_combine == 1) {  // QI = (I_PQ + 1i*Q_PQ) * exp(-1i*pi/2), GPS_L5C tracking.m:340
      const double cr = cos(kPi / 2), ci = -sin(kPi / 2);
      const double re = pi_p * cr - pq_p * ci;
      const double im = pi_p * ci + pq_p * cr;
      carr_err_q = atan(im / re) / (2.0 * kPi);
    } else if (p.pilot_combine == 3) {
      carr_err_q = atan(-pi_p / pq_p) / (2.0 * kPi);  // BDS/B1C NB_tracking.m:341
    } else {
      carr_err_q = atan(pq_p / pi_p) / (2.0 * kPi);   // GAL_E1C tracking.m:309
    }
    double code_err_q = (sqrt(pi_e * pi_e + pq_e * pq_e) - sqrt(pi_l * pi_l + pq_l * pq_l)) /
                        (sqrt(pi_e * pi_e + pq_e * pq_e) + sqrt(pi_l * pi_l + pq_l * pq_l));
    const bool pll_w = p.pll_weight[0] != 0.0 || p.pll_weight[1] != 0.0;
    const bool dll_w = p.dll_weight[0] != 0.0 || p.dll_weight[1] != 0.0;
    if (p.dll_scale != 0.0) {
      code_err = code_err * p.dll_scale;
      code_err_q = code_err_q * p.dll_scale;
    }
    carr_err = pll_w ? (carr_err * p.pll_weight[0] + carr_err_q * p.pll_weight[1]) / (p.pll_weight[0] + p.pll_weight[1])
                     : (carr_err + carr_err_q) / 2;
    if (dll_w && p.pilot_combine == 4)  // codeError*factor + p_codeError*(1-factor), WB_tracking.m:403
      code_err = code_err * p.dll_weight[0] + code_err_q * p.dll_weight[1];
    else
      code_err = dll_w ? (code_err * p.dll_weight[0] + code_err_q * p.dll_weight[1]) / (p.dll_weight[0] + p.dll_weight[1])
                       : (code_err + code_err_q) / 2;
    rec(GC_TRK_PILOT_I_E, pi_e);
    rec(GC_TRK_PILOT_Q_E, pq_e);
    rec(GC_TRK_PILOT_I_P, pi_p);
    rec(GC_TRK_PILOT_Q_P, pq_p);
    rec(GC_TRK_PILOT_I_L, pi_l);
    rec(GC_TRK_PILOT_Q_L, pq_l);
  } else if (arms >= 2) {
#pragma unroll
    for (int v = 0; v < 6; ++v) rec(GC_TRK_PILOT_I_E + v, sums[6 + v]);
  }
  }
  double carr_nco;
  double old_carr_nco = st.old_carr_nco, old_carr_err = st.old_carr_err, d2 = st.d2_carr_err, d1 = st.d_carr_err;
  if (p.pll_kind == GC_PLL_2ND_ORDER) {
    carr_nco = old_carr_nco + dl->k1carr * (carr_err - old_carr_err) + carr_err * dl->k2carr;  // :308-309
    old_carr_nco = carr_nco;
    old_carr_err = carr_err;
  } else {
    d2 = d2 + carr_err * p.pf3;  // GPS_L5C tracking.m:351-353
    d1 = d2 + carr_err * p.pf2 + d1;
    carr_nco = d1 + carr_err * p.pf1;
  }
  rec(GC_TRK_CARR_FREQ, st.carr_freq);
  const double carr_freq_new = st.carr_basis + carr_nco;                        // :317
  const double code_nco = st.old_code_nco + dl->k1code * (code_err - st.old_code_err) + code_err * dl->k2code;
  rec(GC_TRK_CODE_FREQ, st.code_freq);
  const double code_freq_new = st.code_freq_basis - code_nco;                   // :335
  rec(GC_TRK_DLL_DISCR, code_err);
  rec(GC_TRK_DLL_DISCR_FILT, code_nco);
  rec(GC_TRK_PLL_DISCR, carr_err);
  rec(GC_TRK_PLL_DISCR_FILT, carr_nco);
  rec(GC_TRK_I_E, i_e);
  rec(GC_TRK_Q_E, q_e);
  rec(GC_TRK_I_P, i_p);
  rec(GC_TRK_Q_P, q_p);
  rec(GC_TRK_I_L, i_l);
  rec(GC_TRK_Q_L, q_l);
  // next block geometry (:219-222) or the end
  const long long pos_new = st.pos + n;
  const DevLoopCut cut = devloop_cut(dl, pos_new, rem_code_new, code_freq_new, carr_freq_new, e + 1, st.epoch_budget);
  const int status = cut.status;
  st.pos = pos_new;
  st.rem_code = rem_code_new;
  st.rem_carr = rem_carr_new;
  st.carr_freq = carr_freq_new;
  st.code_freq = code_freq_new;
  st.old_code_nco = code_nco;
  st.old_code_err = code_err;
  st.old_carr_nco = old_carr_nco;
  st.old_carr_err = old_carr_err;
  st.d2_carr_err = d2;
  st.d_carr_err = d1;
  st.epochs_done = e + 1;
  st.status = status;
  if (p.table_phase_count > 0 && st.table_phase > 0) {  // GPS_L2C tracking.m:357-360, then :261 for the next block
    if (p.pilot_combine != 0) {
      st.table_phase += 1;
      if (st.table_phase >= p.table_phase_count + 1) st.table_phase = 1;
    }
    b.table_offset[1] = (int)p.code_length * (st.table_phase - 1);
  }
  devloop_put(b, cut, pos_new, rem_code_new, carr_freq_new, rem_carr_new);
  return status;
}

// ---- device only: the teams' messages and the closer's stores -------------------------------------------------------
#if defined(__HIPCC__)
// Message scope (g_msg_scope, set per launch from DevLoopArgs::reserved): 0 = system (sc0 sc1: past every cache),
// 1 = workgroup (sc0: past the CU's L1 only — the team's L2 is the meeting point; valid when the whole team runs on ONE
// XCD, which the launch arranges and the kernel verifies through HW_REG_XCC_ID before switching to it), 2 = agent (sc1).
__device__ __forceinline__ msg_t msg_load(const msg_t* p, int scope = 0) {
  msg_t v;
  if (scope == 1)
    asm volatile("global_load_dwordx4 %0, %1, off sc0\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  else if (scope == 2)
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  else
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ void msg_store(msg_t* p, msg_t v, int scope = 0) {
  if (scope == 1)
    asm volatile("global_store_dwordx4 %0, %1, off sc0" : : "v"(p), "v"(v) : "memory");
  else if (scope == 2)
    asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
  else
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}

// The epoch's record and the loop state to device memory (lane 0), off the critical path.
// spread: every member of an all-gather team holds the same record (it ran the same closure on the same sums), so in teams of
// 17 members or more member f + 2 stores field f - one store instead of fifteen by the member whose partial sums the next epoch
// then waits for (5.77 us per epoch against 5.90; selecting the fields with a runtime modulo instead of a compare cost 0.5 us).
// Member 0 keeps the state.
__device__ inline void devloop_commit(const DevLoopArgs* __restrict__ dl, DevLoopChan* gch, const DevLoopChan& st, long long slot, int e,
                                      const double (&rv)[GC_TRK_NFIELDS], int arms, int lane, int member = 0, bool spread = false) {
  if (lane != 0) return;
  double* o = dl->records + (size_t)slot * GC_TRK_NFIELDS * dl->n_epochs;
  const int nf = (arms >= 2) ? GC_TRK_NFIELDS : GC_TRK_PILOT_I_E;  // the pilot fields follow the fifteen common ones
#pragma unroll
  for (int f = 0; f < GC_TRK_NFIELDS; ++f)
    if (f < nf && (!spread || f + 2 == member)) o[(size_t)f * dl->n_epochs + e] = rv[f];
  if (member != 0) return;
  // the state in device memory is what the host reads when the launch has ended (status, epochs done, the loop state a resumed
  // call starts from): the last epoch's is the one that counts; every 256th keeps a hung run diagnosable
  if (spread && st.status == 0 && (e & 255) != 255) return;
  gch->pos = st.pos;
  gch->rem_code = st.rem_code;
  gch->rem_carr = st.rem_carr;
  gch->carr_freq = st.carr_freq;
  gch->code_freq = st.code_freq;
  gch->old_code_nco = st.old_code_nco;
  gch->old_code_err = st.old_code_err;
  gch->old_carr_nco = st.old_carr_nco;
  gch->old_carr_err = st.old_carr_err;
  gch->d2_carr_err = st.d2_carr_err;
  gch->d_carr_err = st.d_carr_err;
  gch->epochs_done = st.epochs_done;
  gch->status = st.status;
  gch->table_phase = st.table_phase;
  if (dl->cno && st.cno_ready && st.cno_n >= 1 && st.cno_n <= dl->cno_nk) dl->cno[slot * dl->cno_nk + st.cno_n - 1] = st.cno_value;
}

#endif

}  // namespace gcorr
