"""The float64 numpy model of gc_resample's definition (include/gnsscorr.h), operation by operation: the loop runs over the branch
index j, every numpy operation below is vectorised over the outputs and rounds by itself, the NCO is np.uint64 arithmetic modulo
2^64 addressed by the tick.  A tap j L + p_m >= T is SKIPPED (the kernel adds a zero tap there: +-0 to a sum that started at +0.0).
Everything from the angle on is ddc_model's, restated on the tick.  What may differ from the library: one ulp in each of sin and cos."""
import math

import numpy as np

from ddc_model import HALF_EPS, TWO_PI, REAL, IQ, QI, components, phase0, phase_step, signed, taps_pair, nco_freq  # noqa: F401


def rs_phase_step(carr_freq, fs, interp):
    """phase_step per TICK: the rate of the ticks is fs * (double) L, one rounding."""
    return phase_step(carr_freq, fs * float(interp))


def rs_nco_freq(step, fs, interp):
    return math.ldexp(float(signed(step)), -64) * (fs * float(interp))


def out_rate(fs, interp, decim):
    return (fs * float(interp)) / float(decim)


def full_outputs(ns, ntaps, interp, decim, first_tick=0):
    """Outputs that still have a record sample under them: n_m - (J - 1) <= ns - 1."""
    J = -(-ntaps // interp)
    return ((ns + J - 1) * interp - 1 - first_tick) // decim + 1


def resample(raw, src_layout, taps, interp, decim, fs, dst_dtype, dst_layout, carr_freq=0.0, carr_phase=0.0, first_tick=0, noutputs=None):
    """gc_resample of the record `raw` (file order, integer dtype).  Returns ddc_model.downconvert's tuple: (the stored integers in
    dst's file order, clipped, sum_sq, near: bool per stored integer - within HALF_EPS of a half-integer -, (yr, yi) before rounding)."""
    re, im = components(raw, src_layout)
    ns = re.shape[0]
    gr, gi = taps_pair(taps)
    T, L, M = gr.shape[0], int(interp), int(decim)
    J = -(-T // L)
    if noutputs is None:
        noutputs = full_outputs(ns, T, L, M, first_tick)
    m = np.arange(noutputs, dtype=np.int64)
    u = first_tick + m * M
    n, p = u // L, u % L
    # x[n] = 0 outside the record: J - 1 zeros in front, enough behind
    back = max(0, int(n[-1]) + 1 - ns)
    xr = np.concatenate([np.zeros(J - 1), re, np.zeros(back)])
    xi = np.concatenate([np.zeros(J - 1), im, np.zeros(back)])
    a_r, a_i = np.zeros(noutputs), np.zeros(noutputs)
    for j in range(J):
        k = j * L + p
        on = k < T
        kk = np.where(on, k, 0)
        idx = n - j + (J - 1)
        sr, si = xr[idx], xi[idx]
        pr = gr[kk] * sr - gi[kk] * si
        pi = gr[kk] * si + gi[kk] * sr
        a_r = np.where(on, a_r + pr, a_r)
        a_i = np.where(on, a_i + pi, a_i)
    step, p0 = np.uint64(rs_phase_step(carr_freq, fs, L)), np.uint64(phase0(carr_phase))
    with np.errstate(over="ignore"):
        ph = p0 + step * u.astype(np.uint64)
    ang = ph.view(np.int64).astype(np.float64) * (TWO_PI * 2.0 ** -64)
    sn, cs = np.sin(ang), np.cos(ang)
    yr = cs * a_r + sn * a_i
    yi = cs * a_i - sn * a_r
    info = np.iinfo(dst_dtype)
    rr, ri = np.rint(yr), np.rint(yi)
    o_r, o_i = np.clip(rr, info.min, info.max).astype(np.int64), np.clip(ri, info.min, info.max).astype(np.int64)
    c_r, c_i = (rr < info.min) | (rr > info.max), (ri < info.min) | (ri > info.max)
    near_r = (np.abs(yr - np.floor(yr) - 0.5) <= HALF_EPS) & (yr != 0.0)
    near_i = (np.abs(yi - np.floor(yi) - 0.5) <= HALF_EPS) & (yi != 0.0)
    if dst_layout == REAL:
        out, near = o_r.astype(dst_dtype), near_r
        clipped, sum_sq = int(c_r.sum()), int(np.sum(o_r * o_r))
    else:
        out = np.empty(2 * noutputs, dtype=dst_dtype)
        near = np.empty(2 * noutputs, dtype=bool)
        first, second = (o_i, o_r) if dst_layout == QI else (o_r, o_i)
        out[0::2], out[1::2] = first, second
        near[0::2], near[1::2] = (near_i, near_r) if dst_layout == QI else (near_r, near_i)
        clipped, sum_sq = int(c_r.sum() + c_i.sum()), int(np.sum(o_r * o_r) + np.sum(o_i * o_i))
    return out, clipped, sum_sq, near, (yr, yi)
