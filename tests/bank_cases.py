"""What the tests of gc_correlate_bank and gc_correlate_ddm (csrc/corr_bank.hip) share: the records and offsets they run at, the
descriptors of a call, and the float64 per-sample restatement of the definition (include/gnsscorr.h) written with the oracle's
colon().  The DDM is the bank at carr_freq + f_m, so there is one restatement, over (tap offsets, carrier frequencies)."""
import math

import numpy as np
import pytest

from oracle import gnss_oracle as O

FS = 18e6
PERIOD_L1 = 1023.0
# the offsets the shapes are run at: 0, thirds, halves, whole chips, several chips, and just under a period of the 1 023-chip code
POOL = [0.0, 1.0 / 3, -1.0 / 3, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 17.25, -17.25, 1022.9, -1022.9]


def _raw(rec, s0, n, layout="IQ"):
    """raw = data1 + 1i*data2 of tracking.m:233-235 for the record's sample order (GLONASS: swapped; real: no imaginary part)."""
    if layout == "REAL":
        return rec[s0:s0 + n].astype(np.float64).astype(np.complex128)
    seg = rec[2 * s0:2 * (s0 + n)].astype(np.float64)
    return seg[1::2] + 1j * seg[0::2] if layout == "QI" else seg[0::2] + 1j * seg[1::2]


def reference(raw, tables, rem, step, offsets, carriers, rem_carr, fs, r=1.0, arm_mult=None):
    """The definition, per sample, in float64, at every carrier frequency of `carriers`, each taken as given.  Returns (complex128
    [arms, len(carriers), ntaps], number of samples with an integer t_i over the taps)."""
    n = raw.shape[0]
    arm_mult = arm_mult or [1.0] * len(tables)
    code = np.zeros((len(tables), len(offsets), n))
    ties = 0
    for j, o in enumerate(offsets):
        t = O.colon((rem + o) * r, step * r, (((n - 1) * step + rem) + o) * r)
        assert t.shape[0] == n
        ties += int(np.sum(t == np.rint(t)))
        for a, tab in enumerate(tables):
            p = np.ceil(t * arm_mult[a]).astype(np.int64)           # index into the padded table [c(end) c c(1)] ...
            code[a, j] = np.asarray(tab, dtype=np.float64)[1 + np.mod(p - 1, len(tab) - 2)]     # ... read periodically
    out = np.zeros((len(tables), len(carriers), len(offsets)), dtype=np.complex128)
    for m, cf in enumerate(carriers):
        trig = ((cf * 2.0 * math.pi) * (np.arange(n, dtype=np.float64) / fs)) + rem_carr
        mixed = np.exp(-1j * trig) * raw
        out[:, m, :] = code @ mixed
    return out, ties


def bank_reference(raw, tables, rem, step, offsets, carr_freq, rem_carr, fs, r=1.0, arm_mult=None):
    """gc_correlate_bank: one carrier, carr_freq itself.  Returns (complex128 [arms, ntaps], ties)."""
    out, ties = reference(raw, tables, rem, step, offsets, [carr_freq], rem_carr, fs, r, arm_mult)
    return out[:, 0], ties


def ddm_reference(raw, tables, rem, step, offsets, carr_freq, freqs, rem_carr, fs, r=1.0, arm_mult=None):
    """gc_correlate_ddm: the bank's with the float64 sums carr_freq + f_m.  Returns (complex128 [arms, nfreq, ntaps], ties)."""
    carriers = [float(np.float64(carr_freq) + np.float64(f)) for f in freqs]
    return reference(raw, tables, rem, step, offsets, carriers, rem_carr, fs, r, arm_mult)


def _colon_has_n_elements(d, o, r=1.0):
    """The definition takes element i of MATLAB's colon vector, so that vector must have N elements.  A block of two or three
    samples whose start (rem + o) cancels to a few hundredths of a chip has end points that carry more rounding (an ulp of 1) than
    the colon's own end-point tolerance (2 eps of the LARGER END POINT) forgives: MATLAB then builds N - 1 elements and tracking.m
    would stop on the size mismatch.  Such a draw is outside the definition and is drawn again; blocks of a code period are never
    near it (their end point is ~1e3 chips)."""
    n, rem, step = d["n"], d["rem"], d["step"]
    return O.colon((rem + o) * r, step * r, (((n - 1) * step + rem) + o) * r).shape[0] == n


def ramp_model(rem, o, step, n, r=1.0, matlab_end=True):
    """csrc/replica_f64.h restated in numpy, every operation rounded by itself: ramp64's start, end and spacing, then colon_at's
    element i - forwards from the start below the middle, backwards from the end above it, the mean of both in the middle.
    matlab_end: the end point is MATLAB's (c = a + (N-1)*sp, snapped to b when c - b > -tol); False: b itself, as ramp64 took it
    before the tap bank's edge sweep."""
    f = np.float64
    rem, o, step, r = f(rem), f(o), f(step), f(r)
    sp = step * r
    a = (rem + o) * r
    b = (((f(n - 1) * step) + rem) + o) * r
    if matlab_end:
        c = a + f(n - 1) * sp
        tol = 2.0 * np.finfo(np.float64).eps * max(abs(a), abs(b))
        b = b if c - b > -tol else c
    i = np.arange(n, dtype=np.int64)
    back = n - 1 - i
    fi, fb = i.astype(np.float64), back.astype(np.float64)
    return np.where(i < back, a + fi * sp, np.where(i > back, b - fb * sp, (a + b) / 2.0))


def ramp_index(t, mult=1.0):
    """code_step of csrc/replica_f64.h: ceil(fl(t * arm_mult))."""
    return np.ceil(np.asarray(t, dtype=np.float64) * np.float64(mult)).astype(np.int64)


def oracle_ramp(rem, o, step, n, r=1.0):
    """The definition's ramp of a tap: MATLAB's colon, as `reference` takes it (N or N - 1 elements)."""
    return O.colon((rem + o) * r, step * r, (((n - 1) * step + rem) + o) * r)


def bank_refusal(tables_len, mult, r, n, rem, step, offsets):
    """bank_validate's numeric conditions (csrc/bank_plan.h) restated, in its order: the status name a descriptor is refused with
    and the class of the refusal, or None where the library accepts it.  tables_len: entries of each arm's padded table."""
    omax = max(abs(float(o)) for o in offsets)
    for nent, m in zip(tables_len, mult):
        if not omax * r * m < float(nent - 2):
            return "GC_E_INVALID", "period"
    if not (n >= 1 and step > 0 and rem > -1.0 and math.isfinite(rem)):
        return "GC_E_INVALID", "descriptor"
    rate = step * r * max(max(mult), 1.0)
    if rate > 1.0:
        return "GC_E_UNSUPPORTED", "rate_high"
    if not rate >= 1.0 / 65536.0:
        return "GC_E_INVALID", "rate_low"
    if not ((float(n) * step + abs(rem) + omax) * r * max(max(mult), 1.0)) < 2147483000.0:
        return "GC_E_INVALID", "int32"
    return None


def _blocks(engine, descs, df=None):
    """The descriptors of a call; `df`: carr_freq replaced by the float64 sum carr_freq + df (None: carr_freq as it is)."""
    b = engine.make_blocks(len(descs))
    for k, d in enumerate(descs):
        b[k].channel = d.get("channel", 0)
        b[k].blksize = d["n"]
        b[k].first_sample = d["s0"]
        b[k].rem_code_phase = d["rem"]
        b[k].code_phase_step = d["step"]
        b[k].el_spacing = d.get("d", 0.0)
        b[k].carr_freq = d["f"] if df is None else float(np.float64(d["f"]) + np.float64(df))
        b[k].rem_carr_phase = d["phi"]
    return b


@pytest.fixture(scope="module")
def noise_record():
    """Random full-range int8 I/Q samples."""
    return np.random.default_rng(20241018).integers(-128, 128, size=2 * 60000, dtype=np.int8)


@pytest.fixture(scope="module")
def ca_table():
    return O.pad_code(O.generate_ca_code(7)).astype(np.int8)
