"""The teacher-forced oracle: every epoch of a closed loop's trackResults against the float64 oracle of ITS OWN block.

The oracle's tracking loops (oracle/gnss_oracle.py: tracking_l1ca, tracking_generic, tracking_l2c) take a `correlate` hook for
tracking.m:247-300.  check() runs them with a hook that, for every channel and epoch,

  1. forms the float64 sums of the descriptor the oracle holds (pos, n, rem_code, step, d, carr_freq, rem_carr) with
     oracle.c_oracle.correlate_block where it applies (int8 I/Q or Q/I record, equal-length tables, one ramp multiplier, no table
     offset) and oracle.gnss_oracle.correlate_block on raw_from_if otherwise - the rule of tests/test_gpu_correlator_edges.py;
  2. records |have - want| / (TOL * sum|x| of the block) per output, `have` being what the loop under test RECORDED for that epoch
     (for pilot_combine 4 / 5 the recorded pilot is the fold of two arms: compared with oracle.fold_pilot of the float64 arms, the
     bound times the sum of the fold's absolute coefficients);
  3. hands the oracle the RECORDED sums, with the float64 rem_code_new and rem_carr_new.

So the oracle's state at epoch e + 1 is the float64 closure (tracking.m:302-348) of the loop's own sums at epoch e: it follows the
loop under test, not the reference's trajectory, and no bound has to leave room for drift.  After the run the oracle's state
fields are compared with the recorded ones.

Bounds, the project's own: sums TOL = 2e-6 * sum(|I_n| + |Q_n|) per output (test_gpu_correlator.py); absoluteSample equal (GPS
L2C, which records a fractional position, < 1e-6); the eight state fields of test_loop_closure_cpu._CHECKED within 1e-10 of
max|want| of the channel's record, remCarrPhase modulo 2 pi.  Ratios are errors over these bounds: <= 1 passes.

No GPU here: trackResults come from any loop (tests/test_loop_epochs_cpu.py feeds the oracle's and the reference's own)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from oracle import c_oracle as CO
from oracle import gnss_oracle as O

TOL = 2e-6                       # test_gpu_correlator.py, test_gpu_correlator_edges.py
STATE_TOL = 1e-10                # test_loop_closure_cpu.py, test_gpu_tracking_f64.py::_against_the_reference
L2C_ABS_TOL = 1e-6               # test_gpu_ref_vectors.py: GPS L2C records a fractional sample position
SUMS = ("I_E", "Q_E", "I_P", "Q_P", "I_L", "Q_L")
PILOT_SUMS = tuple("Pilot_" + f for f in SUMS)
STATE = ("carrFreq", "codeFreq", "remCodePhase", "remCarrPhase", "dllDiscr", "dllDiscrFilt", "pllDiscr", "pllDiscrFilt")
GC_REAL, GC_IQ, GC_QI = 0, 1, 2


def l1ca_spec():
    """check()'s first argument for channels of GPS L1 C/A tracked outside a ref_scenes.TrackScene."""
    return SimpleNamespace(kind="l1ca")


def generic_spec(**kw):
    """check()'s first argument for oracle.tracking_generic: its spec fields as keywords."""
    return SimpleNamespace(kind="generic", **kw)


def _rems(n, rem, step, carr_freq, rem_carr, fs, code_length, r):
    """rem_code_new, rem_carr_new exactly as gnss_oracle.correlate_block forms them (tracking.m:273,280-283)."""
    t_last = O.colon(rem * r, step * r, ((n - 1) * step + rem) * r)[n - 1]
    rem_code_new = (t_last / r + step) - code_length if r != 1.0 else (t_last + step) - code_length
    trig_n = ((carr_freq * 2.0 * math.pi) * (float(n) / fs)) + rem_carr
    return float(rem_code_new), O.matlab_rem(float(trig_n), O.TWO_PI)


class _Hook:
    """hook(kind, spec, S, channels) of tests/ref_scenes.py's oracle runners; the callable it returns is the oracle's `correlate`."""

    def __init__(self, rec, layout, tr, n_done, feed=None):
        self.rec, self.layout, self.tr, self.n_done, self.feed = rec, layout, tr, n_done, feed
        comp = 1 if layout == GC_REAL else 2
        self.comp = comp
        self.cum = np.concatenate([[0.0], np.cumsum(np.abs(np.asarray(rec, dtype=np.float64)))])
        self.ratio = {}              # channel -> [epochs, 6 or 12]
        self.want = {}               # channel -> float64 sums [epochs, 6 or 12]
        self.scale = {}              # channel -> sum|x| of each block
        self.compared = 0
        self.pilot_combine = 0

    def __call__(self, kind, spec, S, channels):
        self.kind, self.spec, self.S = kind, spec, S
        self.index = {id(c): i for i, c in enumerate(channels)}
        self.epoch = [0] * len(channels)
        self.tables = {}
        self.fs = float(S.samplingFreq)
        self.code_length = float(S.codeLength) * (2.0 if kind == "l2c" else 1.0)
        self.r = float(getattr(spec, "r", 1.0)) if kind == "generic" else 1.0
        self.arm_mult = getattr(spec, "arm_mult", None) if kind == "generic" else None
        self.swap = bool(getattr(spec, "swap_iq", False)) if kind == "generic" else False
        self.pilot_combine = int(getattr(spec, "pilot_combine", 0)) if kind == "generic" else 0
        self.file_type = int(getattr(S, "fileType", 2)) if kind == "l1ca" else int(getattr(spec, "file_type", 2)) if kind == "generic" else 2
        assert (self.file_type == 1) == (self.layout == GC_REAL) and self.swap == (self.layout == GC_QI), "record layout and oracle disagree"
        return self.correlate

    def _tables(self, ch):
        prn = ch.PRN
        if prn not in self.tables:
            if self.kind == "l1ca":
                t = [O.pad_code(O.generate_ca_code(prn))]
            elif self.kind == "generic":
                t = self.spec.tables(prn)
            else:
                t = [O.pad_code(O.generate_l2c_code(prn, "CM", int(self.S.codeLength)))]
                if getattr(self.S, "pilotTRKflag", 0):
                    t.append(O.pad_code(O.generate_l2c_code(prn, "CL", int(self.S.CLCodeLength))))
            self.tables[prn] = [np.asarray(x, dtype=np.float64) for x in t]
        return self.tables[prn]

    def _float64(self, tables, pos, n, rem, step, d, carr_freq, rem_carr, table_offset):
        mult = list(self.arm_mult) if self.arm_mult else [1.0] * len(tables)
        c_applies = (self.rec.dtype == np.int8 and self.layout != GC_REAL and len({len(t) for t in tables}) == 1 and
                     len(set(mult)) == 1 and not (table_offset and any(table_offset)))
        if c_applies:
            sums, _, _ = CO.correlate_block(self.rec, pos, n, tables, rem, step, d, carr_freq, rem_carr, self.fs, self.code_length,
                                            r=self.r, mult=mult[0], swap_iq=self.swap)
            return sums, _rems(n, rem, step, carr_freq, rem_carr, self.fs, self.code_length, self.r)
        raw = O.raw_from_if(self.rec, pos, n, self.file_type, swap_iq=self.swap)
        sums, rc, rp = O.correlate_block(raw, tables, rem, step, d, carr_freq, rem_carr, self.fs, self.code_length, r=self.r,
                                         arm_mult=self.arm_mult, table_offset=table_offset)
        return sums, (rc, rp)

    def correlate(self, ch, pos, n, rem, step, d, carr_freq, rem_carr, table_offset=None):
        i = self.index[id(ch)]
        e = self.epoch[i]
        self.epoch[i] += 1
        tables = self._tables(ch)
        sums64, rems = self._float64(tables, pos, n, rem, step, d, carr_freq, rem_carr, table_offset)
        want = [sums64[0]]
        gain = [1.0]
        if len(tables) >= 2:
            if self.pilot_combine in (4, 5):
                want.append(np.array(O.fold_pilot(self.pilot_combine, sums64[1], sums64[2])))
                gain.append(O.fold_pilot_gain(self.pilot_combine))
            else:
                want.append(sums64[1])
                gain.append(1.0)
        want = np.array(want)
        if e >= self.n_done[i]:          # the loop under test did not get this far: the oracle goes on by itself, nothing to compare
            return want, rems[0], rems[1]
        t = self.tr[i]
        have = np.array([[getattr(t, f)[e] for f in names] for names in (SUMS, PILOT_SUMS)[:len(want)]], dtype=np.float64)
        scale = float(self.cum[self.comp * (pos + n)] - self.cum[self.comp * pos])
        bound = TOL * scale * np.array(gain)[:, None]
        diff = np.abs(have - want)
        with np.errstate(divide="ignore", invalid="ignore"):     # an all-zero block: bound 0, passes with exact zeros only
            ratio = np.where(diff == 0.0, 0.0, diff / bound)
        rows = self.ratio.setdefault(i, np.full((self.n_done[i], 6 * len(want)), np.nan))
        rows[e] = ratio.reshape(-1)
        self.want.setdefault(i, np.full((self.n_done[i], 6 * len(want)), np.nan))[e] = want.reshape(-1)
        self.scale.setdefault(i, np.full(self.n_done[i], np.nan))[e] = scale
        self.compared += 1
        fed = have if self.feed is None else self.feed(i, e, have, want, dict(pos=pos, n=n, rem=rem, step=step, d=d, carr_freq=carr_freq,
                                                                              rem_carr=rem_carr, tables=tables, scale=scale))
        return fed, rems[0], rems[1]


def check(sc_or_spec, rec, layout, ch, S, tr, done=None, feed=None):
    """Every epoch of `tr` (a list of trackResults parallel to `ch`, from any loop over record `rec`) against the teacher-forced oracle.

    sc_or_spec  a ref_scenes.TrackScene (its oracle runner is used), l1ca_spec() or generic_spec(...)
    done        epochs done per entry of `tr` (default: all of a channel whose status is not '-', none of the others)
    feed        test hook: (channel, epoch, have, want, descriptor) -> the sums handed to the oracle instead of `have`
    Returns a namespace:
      compared            epochs that went through the hook and were compared
      sum_ratio[c]        [epochs, 6 (12 with a pilot)] error / bound per output, order SUMS then PILOT_SUMS
      state_ratio[c][f]   [epochs] error / bound of state field f; f = "absoluteSample": 0 where equal, else the difference (L2C: / 1e-6)
      worst_sum, worst_state   (ratio, epoch, channel, field) of the largest ratio; ratio 0 and None's where nothing was compared
      failures            every (kind, ratio, epoch, channel, field) with ratio > 1, or not finite, in channel / epoch order"""
    rec = np.asarray(rec)
    n_ep = max((len(t.carrFreq) for t in tr), default=0)
    if done is None:
        done = [len(t.carrFreq) if t.status != "-" else 0 for t in tr]
    n_done = [int(v) for v in done]
    hook = _Hook(rec, layout, tr, n_done, feed)
    if hasattr(sc_or_spec, "oracle"):
        ora = sc_or_spec.oracle(O, rec, ch, S, hook=hook)
        l2c = sc_or_spec.signal == "GPS_L2C"
    elif sc_or_spec.kind == "l1ca":
        ora, l2c = O.tracking_l1ca(rec, ch, S, correlate=hook("l1ca", None, S, ch)), False
    else:
        ora, l2c = O.tracking_generic(rec, ch, S, sc_or_spec, correlate=hook("generic", sc_or_spec, S, ch)), False
    res = SimpleNamespace(compared=hook.compared, sum_ratio=hook.ratio, want=hook.want, scale=hook.scale, state_ratio={}, oracle=ora, failures=[],
                          worst_sum=(0.0, None, None, None), worst_state=(0.0, None, None, None))
    names = SUMS + PILOT_SUMS
    for c in sorted(hook.ratio):
        r = hook.ratio[c]
        assert not np.isnan(r).any(), f"channel {c}: the oracle ended before the loop under test did"
        for e, v in zip(*np.nonzero(~(r <= 1.0))):
            res.failures.append(("sum", float(r[e, v]), int(e), c, names[v]))
        e, v = np.unravel_index(int(np.argmax(r)), r.shape)
        if r[e, v] > res.worst_sum[0]:
            res.worst_sum = (float(r[e, v]), int(e), c, names[v])
    for c, t in enumerate(tr):
        n = n_done[c]
        if n == 0:
            continue
        o = ora[c]
        out = {}
        da = np.abs(np.asarray(t.absoluteSample[:n], dtype=np.float64) - o.absoluteSample[:n])
        out["absoluteSample"] = da / L2C_ABS_TOL if l2c else da
        for f in STATE:
            want, have = getattr(o, f)[:n], np.asarray(getattr(t, f)[:n], dtype=np.float64)
            dd = np.abs(have - want)
            if f == "remCarrPhase":
                dd = np.minimum(dd, np.abs(dd - 2 * np.pi))
            scale = float(np.max(np.abs(want)))
            assert np.all(np.isfinite(want)), (c, f)
            out[f] = dd / (STATE_TOL * scale) if scale > 0 else dd / STATE_TOL
        res.state_ratio[c] = out
        for f, r in out.items():
            bad = ~(r < 1.0) if (f == "absoluteSample" and l2c) else (r != 0) if f == "absoluteSample" else ~(r <= 1.0)
            for e in np.flatnonzero(bad):
                res.failures.append(("state", float(r[e]), int(e), c, f))
            e = int(np.argmax(np.where(np.isfinite(r), r, np.inf)))
            if f != "absoluteSample" and not r[e] <= res.worst_state[0]:
                res.worst_state = (float(r[e]), e, c, f)
    res.n_epochs = n_ep
    return res


def describe(res):
    ws, wt = res.worst_sum, res.worst_state
    return (f"{res.compared} epochs; sums {ws[0]:.3f} of the bound (epoch {ws[1]}, channel {ws[2]}, {ws[3]}); "
            f"state {wt[0] * STATE_TOL:.1e} relative (epoch {wt[1]}, channel {wt[2]}, {wt[3]}); {len(res.failures)} beyond a bound")
