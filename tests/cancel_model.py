"""The float64 numpy model of gc_cancel's definition (include/gnsscorr.h), operation by operation: every numpy operation below rounds
by itself, as the header asks.  What may differ from the library: one ulp in each of sin and cos, and the order of additions in P.

A channel is a dict {"tables": [int arrays], "r": index_scale, "mult": [arm_mult]}; a block a dict {"ch": channel index, "s0", "n",
"rem", "step", "f", "phi"} and optionally "off": [table_offset per arm].

The code ramp is csrc/replica_f64.h's, restated in bank_cases.ramp_model: the colon's element rule with MATLAB's end point (c = a +
(N-1)*sp, the written end point b in its place only where c - b > -tol).  Where MATLAB's colon of the block has N elements
(oracle_ok) that ramp is the colon element for element (tests/test_cancel_edges_cpu.py); a block whose colon has N - 1 elements is
outside the definition."""
import numpy as np

from bank_cases import oracle_ramp, ramp_index, ramp_model

REAL, IQ, QI = 0, 1, 2
HALF_EPS = 1e-9          # a sample whose value lies this close to a half-integer may round either way


def components(raw, layout):
    """(re, im) as float64 of a record in file order: I/Q as stored, Q/I swapped, real records im = 0."""
    x = np.asarray(raw).astype(np.float64)
    if layout == REAL:
        return x, np.zeros_like(x)
    return (x[1::2], x[0::2]) if layout == QI else (x[0::2], x[1::2])


def pack(re, im, dtype, layout):
    if layout == REAL:
        return np.ascontiguousarray(re.astype(dtype))
    out = np.empty(2 * re.shape[0], dtype=dtype)
    out[0::2], out[1::2] = (im, re) if layout == QI else (re, im)
    return out


def oracle_ok(blk, chan):
    """MATLAB's colon of the block's ramp has N elements: the definition covers the block."""
    return oracle_ramp(float(blk["rem"]), 0.0, float(blk["step"]), int(blk["n"]), float(chan["r"])).shape[0] == int(blk["n"])


def replica(blk, chan, fs, matlab_end=True):
    """(sn, cs, c[arms, N]) of a block: the carrier and every arm's code on its N samples.  matlab_end=False: the ramp's second half
    from the written end point b, as this model took it before the tap bank's edge sweep."""
    n, rem, step, r = int(blk["n"]), float(blk["rem"]), float(blk["step"]), float(chan["r"])
    i = np.arange(n, dtype=np.float64)
    trig = ((blk["f"] * 2.0) * np.pi) * (i / fs) + blk["phi"]
    sn, cs = np.sin(trig), np.cos(trig)
    t = ramp_model(rem, 0.0, step, n, r, matlab_end=matlab_end)                                        # the colon's element rule
    off = blk.get("off") or [0] * len(chan["tables"])
    c = np.empty((len(chan["tables"]), n))
    for arm, tab in enumerate(chan["tables"]):
        k = ramp_index(t, float(chan["mult"][arm])) + int(off[arm])
        c[arm] = np.asarray(tab, dtype=np.float64)[np.clip(k, 0, len(tab) - 1)]
    return sn, cs, c


def project(re, im, blk, chan, fs, rep=None):
    """(P complex [arms], E int [arms], sum |re| + |im| over the block) of one block on the record (re, im); rep: the block's
    replica() where the caller has it."""
    s0, n = int(blk["s0"]), int(blk["n"])
    sn, cs, c = replica(blk, chan, fs) if rep is None else rep
    x_re, x_im = re[s0:s0 + n], im[s0:s0 + n]
    ib = cs * x_re + sn * x_im
    qb = cs * x_im - sn * x_re
    P = np.array([np.sum(ca * ib) + 1j * np.sum(ca * qb) for ca in c])
    E = np.array([int(np.sum(ca * ca)) for ca in c])
    return P, E, float(np.sum(np.abs(x_re) + np.abs(x_im)))


def cancel(raw, dtype, layout, blocks, chans, fs, amp=None, mode="subtract", reps=None):
    """gc_cancel on the record `raw` (file order, integer dtype).  amp: complex [nblocks, 3] or None (the projection).
    reps: a dict the replicas of `blocks` are kept in from one call to the next on the same list (they do not depend on the record,
    the amplitudes or the mode), or None.
    Returns (out record, amp used complex [nblocks, 3], P [nblocks, 3], E [nblocks, 3], sum|x| [nblocks],
    near: bool per sample - a component within HALF_EPS of a half-integer, covered: bool per sample)."""
    re, im = components(raw, layout)
    ns = re.shape[0]
    nb = len(blocks)
    used = np.zeros((nb, 3), dtype=np.complex128)
    P_all, E_all, sx = np.zeros((nb, 3), dtype=np.complex128), np.zeros((nb, 3), dtype=np.int64), np.zeros(nb)
    m_re, m_im = np.zeros(ns), np.zeros(ns)
    covered = np.zeros(ns, dtype=bool)
    for k in sorted(range(nb), key=lambda q: (blocks[q]["ch"], blocks[q]["s0"])):      # ascending channel index
        blk = blocks[k]
        chan = chans[blk["ch"]]
        arms = len(chan["tables"])
        s0, n = int(blk["s0"]), int(blk["n"])
        if reps is None or k not in reps:
            rep = replica(blk, chan, fs)
            if reps is not None:
                reps[k] = rep
        else:
            rep = reps[k]
        sn, cs, c = rep
        P, E, sx[k] = project(re, im, blk, chan, fs, rep)
        P_all[k, :arms], E_all[k, :arms] = P, E
        if amp is None:
            # per component, one division each (a complex quotient would multiply by 1 / E: an ulp off now and then)
            used[k, :arms] = [complex(P[a].real / float(E[a]), P[a].imag / float(E[a])) if E[a] else 0.0 for a in range(arms)]
        else:
            used[k, :arms] = np.asarray(amp)[k, :arms]
        b_re, b_im = np.zeros(n), np.zeros(n)
        for a in range(arms):
            ar, ai = used[k, a].real, used[k, a].imag
            b_re = b_re + c[a] * (ar * cs - ai * sn)
            b_im = b_im + c[a] * (ar * sn + ai * cs)
        if layout == REAL:
            b_re = 2.0 * b_re
        m_re[s0:s0 + n] = m_re[s0:s0 + n] + b_re
        m_im[s0:s0 + n] = m_im[s0:s0 + n] + b_im
        covered[s0:s0 + n] = True
    y_re, y_im = (m_re, m_im) if mode == "model" else (re - m_re, im - m_im)
    if layout == REAL:
        y_im = np.zeros(ns)
    info = np.iinfo(dtype)
    near = (np.abs(y_re - np.floor(y_re) - 0.5) <= HALF_EPS) | (np.abs(y_im - np.floor(y_im) - 0.5) <= HALF_EPS)
    o_re = np.clip(np.rint(y_re), info.min, info.max)
    o_im = np.clip(np.rint(y_im), info.min, info.max)
    return pack(o_re, o_im, dtype, layout), used, P_all, E_all, sx, near, covered
