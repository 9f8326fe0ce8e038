// replica_f64.h — what a per-sample float64 replica of tracking.m:247-300 is made of, written once: the reference's colon element
// and its table index, the carrier's angle and the baseband rotation.  Every operation is rounded by itself - the explicit
// __dadd_rn / __dmul_rn / __ddiv_rn say so, and keep saying it in a unit compiled without -ffp-contract=off (build.py).
// corr_f64.hip (three taps), cancel.hip (the prompt tap), corr_kernel.hip's mixed kernel and corr_bank.hip's BankRamp (ramp and index)
// call these functions; the exact fallback paths of corr_fast.hip, corr_multi.hip and corr_cboc.hip restate colon_at in place (their
// register allocation is tuned around those lines) and point here.
#pragma once
#include <hip/hip_runtime.h>

namespace gcorr {

constexpr double kPi = 3.141592653589793;  // MATLAB's pi

// Element i of colon(a, sp, b) with N elements, as MATLAB forms it: a + i*sp from the start below the middle, b - (N-1-i)*sp from
// the end above it, the mean of both ends in the middle (odd N only).
__device__ __forceinline__ double colon_at(double a, double b, double sp, int N, int i) {
  const int back = N - 1 - i;  // elements after this one
  double t;
  if (i < back)
    t = __dadd_rn(a, __dmul_rn((double)i, sp));
  else if (i > back)
    t = __dadd_rn(b, -__dmul_rn((double)back, sp));
  else
    t = __dadd_rn(a, b) / 2.0;
  return t;
}

// ceil(t * arm_mult): the table entry of ramp value t before the block's table_offset
__device__ __forceinline__ int code_step(double t, double mult) { return (int)ceil(__dmul_rn(t, mult)); }

// ... and with it, clamped to the table's entries 0 .. last
__device__ __forceinline__ int code_index(double t, double mult, int off, int last) { return min(max(code_step(t, mult) + off, 0), last); }

// The code ramp of one tap of a block: colon(a, step*R, b) of tracking.m:252-270 (GAL_E1C tracking.m:236-262).
struct Ramp64 {
  double a, b, sp;
  int N;
  __device__ __forceinline__ double at(int i) const { return colon_at(a, b, sp, N, i); }
};

// The ramp of the tap `tap` chips from the prompt one (-el_spacing, 0, +el_spacing; any offset for the bank).  The prompt tap's
// + 0.0 changes no value.  The end the second half is built from is MATLAB's: c = a + (N-1)*sp, and the written end point b in its
// place only when c - b > -tol, tol = 2 eps max(|a|, |b|).  Where rem and tap nearly cancel, a and b carry the rounding of
// intermediates many times their size and c < b - tol: the colon then ends at c, a few 1e-14 before b, and a sample on a table edge
// gets the other index (tests/test_bank_edges_cpu.py).  A colon with N - 1 elements is outside every definition that uses this ramp.
__device__ __forceinline__ Ramp64 ramp64(double rem, double tap, double step, double R, int N) {
  Ramp64 r;
  r.N = N;
  r.sp = __dmul_rn(step, R);
  r.a = __dmul_rn(__dadd_rn(rem, tap), R);
  const double b = __dmul_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)(N - 1), step), rem), tap), R);
  const double c = __dadd_rn(r.a, __dmul_rn((double)(N - 1), r.sp));
  const double tol = __dmul_rn(2.0 * 2.220446049250313e-16, fmax(fabs(r.a), fabs(b)));
  r.b = __dadd_rn(c, -b) > -tol ? b : c;
  return r;
}

// The carrier of a block: trig = (carrFreq * 2 * pi) * (i / fs) + remCarrPhase (:280-281: time = (0:blksize) ./ fs is a division),
// float64 sin / cos of trig itself - no phase recurrence, no reduced phase.
struct Carrier64 {
  double w, rc;
  __device__ __forceinline__ double trig(int i, double fs) const { return __dadd_rn(__dmul_rn(w, __ddiv_rn((double)i, fs)), rc); }
  __device__ __forceinline__ void at(int i, double fs, double& sn, double& cs) const { sincos(trig(i, fs), &sn, &cs); }
};

__device__ __forceinline__ Carrier64 carrier64(double carr_freq, double rem_carr_phase) {
  Carrier64 c;
  c.w = __dmul_rn(__dmul_rn(carr_freq, 2.0), kPi);  // carrFreq * 2.0 * pi
  c.rc = rem_carr_phase;
  return c;
}

// (ib, qb) = real / imag(exp(-1i * trig) .* (re + 1i * im)), :287-292 (oracle/gnss_oracle.c orc_correlate_block)
__device__ __forceinline__ void wipe_off(double sn, double cs, double re, double im, double& ib, double& qb) {
  ib = __dadd_rn(__dmul_rn(cs, re), __dmul_rn(sn, im));
  qb = __dadd_rn(__dmul_rn(cs, im), -__dmul_rn(sn, re));
}

}  // namespace gcorr
