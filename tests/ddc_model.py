"""The float64 numpy model of gc_downconvert's definition (include/gnsscorr.h), operation by operation: the loop runs over the taps,
every numpy operation below is vectorised over the outputs and rounds by itself, the NCO is np.uint64 arithmetic modulo 2^64.  What
may differ from the library: one ulp in each of sin and cos."""
import math
from fractions import Fraction

import numpy as np

REAL, IQ, QI = 0, 1, 2
HALF_EPS = 1e-9          # a component whose value lies this close to a half-integer may round either way
TWO_PI = 6.283185307179586
MASK = (1 << 64) - 1


def components(raw, layout):
    """(re, im) as float64 of a record in file order: I/Q as stored, Q/I swapped, real records im = 0."""
    x = np.asarray(raw).astype(np.float64)
    if layout == REAL:
        return x, np.zeros_like(x)
    return (x[1::2], x[0::2]) if layout == QI else (x[0::2], x[1::2])


def phase_step(carr_freq, fs):
    """phase_step = (uint64)(int64) llrint(ldexp(carr_freq / fs, 64)), in Python integers (round: to nearest, ties to even)."""
    return int(round(Fraction(math.ldexp(carr_freq / fs, 64)))) & MASK


def phase0(carr_phase):
    q = carr_phase / TWO_PI
    r = q - float(np.rint(q))
    X = math.ldexp(r, 64)
    if abs(X) == 2.0 ** 63:
        return 1 << 63
    return int(round(Fraction(X))) & MASK


def signed(u):
    return u - (1 << 64) if u >= 1 << 63 else u


def nco_freq(step, fs):
    """gc_ddc_result.carr_freq: (double)(int64) phase_step * 2^-64 * fs."""
    return math.ldexp(float(signed(step)), -64) * fs


def taps_pair(taps):
    g = np.asarray(taps)
    if g.ndim == 2:
        return g[:, 0].astype(np.float64), g[:, 1].astype(np.float64)
    g = g.astype(np.complex128)
    return g.real.copy(), g.imag.copy()


def downconvert(raw, src_layout, taps, decim, fs, dst_dtype, dst_layout, carr_freq=0.0, carr_phase=0.0, first_sample=0, noutputs=None):
    """gc_downconvert of the record `raw` (file order, integer dtype).  Returns (the stored integers in dst's file order - an array
    of dst_dtype, 2 per output for I/Q and Q/I -, clipped, sum_sq, near: bool per stored integer - within HALF_EPS of a half-integer;
    an exact zero never is -, (yr, yi) before rounding)."""
    re, im = components(raw, src_layout)
    ns = re.shape[0]
    gr, gi = taps_pair(taps)
    T, D = gr.shape[0], int(decim)
    if noutputs is None:
        noutputs = (ns + T - 2 - first_sample) // D + 1
    m = np.arange(noutputs, dtype=np.int64)
    n = first_sample + m * D
    # x[n] = 0 outside the record: T - 1 zeros in front, enough behind
    back = max(0, int(n[-1]) + 1 - ns)
    xr = np.concatenate([np.zeros(T - 1), re, np.zeros(back)])
    xi = np.concatenate([np.zeros(T - 1), im, np.zeros(back)])
    a_r, a_i = np.zeros(noutputs), np.zeros(noutputs)
    for k in range(T):
        idx = n - k + (T - 1)
        sr, si = xr[idx], xi[idx]
        pr = gr[k] * sr - gi[k] * si
        pi = gr[k] * si + gi[k] * sr
        a_r = a_r + pr
        a_i = a_i + pi
    step, p0 = np.uint64(phase_step(carr_freq, fs)), np.uint64(phase0(carr_phase))
    with np.errstate(over="ignore"):
        ph = p0 + step * n.astype(np.uint64)
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
