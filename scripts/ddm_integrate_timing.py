"""gc_correlate_ddm_integrate against the way a caller gets the same numbers without it: gc_correlate_ddm on the same block list -
every block's map back in the C-ABI's GC_MAX_ARMS layout - followed by the integration in numpy on the host (the rotation of every bin
to the run's first block, the wipe-off weights, the coherent sum in block order, the power over runs).

Shape: 12 GPS L1 C/A channels x 100 epochs of an int8 I/Q record at 18 Msps, 33 taps at j/17 chip x 17 bins spaced 125 Hz; the list
channel by channel, runs of 20 epochs, one power map per channel (5 runs).  Both sides are wall clock around the calls, descriptors in
and results out included; warm-up first, then the two sides alternate and the medians and their spread (min .. max) are reported in one
JSON line, with the bytes each side brings back from the library.  The two sides' results are compared on the way: the host side uses
numpy's cos / sin where the library uses sincospi, so they agree within (16 + L) 2^-52 sum |w| (|D.re| + |D.im|) per coherent cell (the
bound of tests/test_gpu_ddm_integrate.py), not bit for bit.

    python scripts/ddm_integrate_timing.py [--reps 15] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cu_sdr_collection_amd as P  # noqa: E402

FS, RATE, NCH, NEP, RUN = 18e6, 1.023e6, 12, 100, 20
NTAPS, NFREQ = 33, 17


def host_integration(out, s0, w, frq, nruns, per_map):
    """What a caller of gc_correlate_ddm does next: out [nblocks, 3, nfreq, ntaps, 2] -> (coh [nruns, ...] complex, pow [nmaps, ...])."""
    D = out[..., 0] + 1j * out[..., 1]
    coh = np.zeros((nruns,) + D.shape[1:], dtype=np.complex128)
    bound = np.zeros(coh.shape)
    for r in range(nruns):
        re, im, mag = np.zeros(D.shape[1:]), np.zeros(D.shape[1:]), np.zeros(D.shape[1:])
        for b in range(r * RUN, (r + 1) * RUN):
            x = (frq * float(s0[b] - s0[r * RUN])) / FS
            u = x - np.rint(x)
            c, s = np.cos(2.0 * np.pi * u)[None, :, None], np.sin(2.0 * np.pi * u)[None, :, None]
            re = re + w[b] * (c * D[b].real + s * D[b].imag)
            im = im + w[b] * (c * D[b].imag - s * D[b].real)
            mag = mag + abs(w[b]) * (np.abs(D[b].real) + np.abs(D[b].imag))
        coh[r] = re + 1j * im
        bound[r] = (16 + RUN) * 2.0 ** -52 * mag
    pw = np.zeros((nruns // per_map,) + D.shape[1:])
    for q in range(pw.shape[0]):
        for r in range(q * per_map, (q + 1) * per_map):
            pw[q] = pw[q] + (coh[r].real * coh[r].real + coh[r].imag * coh[r].imag)
    return coh, pw, bound


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(20241018)
    nsamp = int(FS * NEP / 1000) + 18000
    iq = rng.integers(-40, 41, size=2 * nsamp, dtype=np.int8)
    eng = P.Engine(0)
    eng.load_if(iq, fs=FS)
    for c in range(NCH):
        eng.set_channel(c, [P.codes.padded_table(P.codes.generateCAcode(c + 1))])
    nb = NCH * NEP
    blocks = eng.make_blocks(nb)
    for c in range(NCH):                             # channel by channel: a run is consecutive epochs of one channel
        for e in range(NEP):
            b = blocks[c * NEP + e]
            step = (RATE + rng.uniform(-3, 3)) / FS
            rem = float(rng.uniform(0, step))
            b.channel, b.rem_code_phase, b.code_phase_step = c, rem, step
            b.blksize = int(np.ceil((1023.0 - rem) / step))
            b.first_sample = min(e * 18000 + int(rng.integers(0, 40)), nsamp - b.blksize)
            b.el_spacing = 0.5
            b.carr_freq = 20e3 + float(rng.uniform(-5e3, 5e3))
            b.rem_carr_phase = float(rng.uniform(-3, 3))
    s0 = np.array([b.first_sample for b in blocks], dtype=np.int64)
    w = rng.choice(np.array([1.0, -1.0]), size=nb)
    off = np.array([j / 17 for j in range(-16, 17)])
    frq = np.array([(m - NFREQ // 2) * 125.0 for m in range(NFREQ)])
    nruns, per_map = nb // RUN, NEP // RUN
    nmaps = nruns // per_map
    run_len = np.full(nruns, RUN, dtype=np.int32)
    map_len = np.full(nmaps, per_map, dtype=np.int32)
    lib, ctx = eng._lib, eng._ctx
    dptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    iptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    out_ddm = np.zeros((nb, 3, NFREQ, NTAPS, 2))
    coh = np.zeros((nruns, 3, NFREQ, NTAPS, 2))
    pw = np.zeros((nmaps, 3, NFREQ, NTAPS))
    host = {}

    def one_call():
        t0 = time.perf_counter()
        P._lib.check(lib.gc_correlate_ddm_integrate(ctx, nb, blocks, dptr(w), NTAPS, dptr(off), NFREQ, dptr(frq), nruns, iptr(run_len), nmaps,
                                                    iptr(map_len), dptr(coh), dptr(pw)))
        return time.perf_counter() - t0

    def ddm_and_host():
        t0 = time.perf_counter()
        P._lib.check(lib.gc_correlate_ddm(ctx, nb, blocks, NTAPS, dptr(off), NFREQ, dptr(frq), dptr(out_ddm)))
        t1 = time.perf_counter()
        host["coh"], host["pow"], host["bound"] = host_integration(out_ddm, s0, w, frq, nruns, per_map)
        t2 = time.perf_counter()
        host["ddm_s"] = t1 - t0
        return t2 - t0

    for _ in range(a.warmup):
        one_call()
        ddm_and_host()
    ta, tb, tddm = [], [], []
    for _ in range(a.reps):
        ta.append(one_call())
        tb.append(ddm_and_host())
        tddm.append(host["ddm_s"])
    got = coh[..., 0] + 1j * coh[..., 1]
    dev = np.maximum(np.abs(got.real - host["coh"].real), np.abs(got.imag - host["coh"].imag))
    live = host["bound"] > 0
    frac = float((dev[live] / host["bound"][live]).max())
    assert frac <= 1.0 and not dev[~live].any(), "the one call and the host integration differ by more than the bound"
    pdev = float((np.abs(pw - host["pow"])[:, 0] / host["pow"][:, 0]).max())
    assert pdev < 1e-12, "the power maps differ"
    ma, mb = float(np.median(ta)), float(np.median(tb))
    spreads = (max(ta) - min(ta)) + (max(tb) - min(tb))
    print(json.dumps({"ntaps": NTAPS, "nfreq": NFREQ, "blocks": nb, "runs": nruns, "maps": nmaps,
                      "integrate_ms": {"median": 1e3 * ma, "min": 1e3 * min(ta), "max": 1e3 * max(ta)},
                      "ddm_plus_host_ms": {"median": 1e3 * mb, "min": 1e3 * min(tb), "max": 1e3 * max(tb)},
                      "of_which_ddm_ms": {"median": 1e3 * float(np.median(tddm)), "min": 1e3 * min(tddm), "max": 1e3 * max(tddm)},
                      "bytes_returned": {"integrate": coh.nbytes + pw.nbytes, "ddm": out_ddm.nbytes},
                      "ratio_ddm_plus_host_over_integrate": mb / ma,
                      "condition_met": ma <= mb + spreads,                # the one call's median not above the other by more than the two spreads
                      "coh_worst_fraction_of_bound": frac, "pow_worst_relative_difference": pdev,
                      "reps": a.reps, "library": os.path.basename(P._lib.LIB_PATH)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
