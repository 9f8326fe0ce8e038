"""gc_correlate_bank against the way a caller gets the same numbers without it: K gc_correlate calls on the same block list with
el_spacing = the K positive offsets (every call reads, converts and carrier-mixes the samples again).

Shape: 12 GPS L1 C/A channels x 1 000 epochs of a 1-s int8 I/Q record at 18 Msps; taps symmetric about zero inside gc_correlate's
domain (|offset| < 1 chip): 33 taps at j/17 chip (16 calls), and the same at 5 and 64 taps for the cost per tap.
Both sides are wall clock around the library call, descriptors in and results out included; warm-up first, then the two sides
alternate and the medians and their spread (min .. max) are reported, one JSON line per tap count.  The two sides' sums are
compared on the way (two float32 paths: 4e-6 of sum |x|).

    python scripts/bank_timing.py [--reps 15] [--warmup 3] [--taps 5,33,64]
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

FS, RATE, NCH, NEP = 18e6, 1.023e6, 12, 1000


def offsets_for(ntaps):
    """(all tap offsets, the positive ones = the el_spacing of the gc_correlate calls)"""
    k = ntaps // 2
    pos = [j / (k + 1) for j in range(1, k + 1)] if ntaps % 2 else [(j + 0.5) / (k + 0.5) for j in range(k)]
    return [-d for d in reversed(pos)] + ([0.0] if ntaps % 2 else []) + pos, pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--taps", default="5,33,64")
    a = ap.parse_args()
    rng = np.random.default_rng(20241018)
    nsamp = int(FS)
    iq = rng.integers(-40, 41, size=2 * nsamp, dtype=np.int8)
    eng = P.Engine(0)
    eng.load_if(iq, fs=FS)
    for c in range(NCH):
        eng.set_channel(c, [P.codes.padded_table(P.codes.generateCAcode(c + 1))])
    blocks = eng.make_blocks(NCH * NEP)
    for e in range(NEP):
        for c in range(NCH):
            b = blocks[e * NCH + c]
            step = (RATE + rng.uniform(-3, 3)) / FS
            rem = float(rng.uniform(0, step))
            b.channel, b.rem_code_phase, b.code_phase_step = c, rem, step
            b.blksize = int(np.ceil((1023.0 - rem) / step))
            b.first_sample = min(e * 18000 + int(rng.integers(0, 40)), nsamp - b.blksize)
            b.el_spacing = 0.5
            b.carr_freq = 20e3 + float(rng.uniform(-5e3, 5e3))
            b.rem_carr_phase = float(rng.uniform(-3, 3))
    nb = len(blocks)
    lib, ctx = eng._lib, eng._ctx
    scale = np.array([np.abs(iq[2 * b.first_sample:2 * (b.first_sample + b.blksize)].astype(np.float64)).sum() for b in blocks[:: nb // 64]])
    for ntaps in [int(x) for x in a.taps.split(",")]:
        offs, pos = offsets_for(ntaps)
        off = np.array(offs)
        out_bank = np.zeros((nb, 3, ntaps, 2))
        out_epl = np.zeros((len(pos), nb, 3, 6))
        lists = []                                   # the caller's K descriptor lists, prepared outside the timed region
        for d in pos:
            lst = eng.make_blocks(nb)
            C.memmove(lst, blocks, C.sizeof(blocks))
            for b in lst:
                b.el_spacing = d
            lists.append(lst)

        def bank():
            t0 = time.perf_counter()
            P._lib.check(lib.gc_correlate_bank(ctx, nb, blocks, ntaps, off.ctypes.data_as(C.POINTER(C.c_double)),
                                               out_bank.ctypes.data_as(C.POINTER(C.c_double))))
            return time.perf_counter() - t0

        def calls():
            t0 = time.perf_counter()
            for k, lst in enumerate(lists):
                P._lib.check(lib.gc_correlate(ctx, nb, lst, out_epl[k].ctypes.data_as(C.POINTER(C.c_double))))
            return time.perf_counter() - t0

        for _ in range(a.warmup):
            bank()
            calls()
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(bank())
            tb.append(calls())
        # the same numbers: tap -d / +d of the bank against I_E,Q_E / I_L,Q_L of call k, the middle tap against I_P,Q_P
        worst = 0.0
        k0 = len(pos)
        for k, d in enumerate(pos):
            lo, hi = k0 - 1 - k, (k0 + 1 + k) if ntaps % 2 else (k0 + k)
            for tap, col in ((lo, 0), (hi, 4)):
                dev = np.abs(out_bank[:: nb // 64, 0, tap, :] - out_epl[k, :: nb // 64, 0, col:col + 2]).max(axis=1) / scale
                worst = max(worst, float(dev.max()))
        if ntaps % 2:
            worst = max(worst, float((np.abs(out_bank[:: nb // 64, 0, k0, :] - out_epl[0, :: nb // 64, 0, 2:4]).max(axis=1) / scale).max()))
        assert worst < 4e-6, worst
        ma, mb = float(np.median(ta)), float(np.median(tb))
        print(json.dumps({"ntaps": ntaps, "blocks": nb, "gc_correlate_calls": len(pos),
                          "bank_ms": {"median": 1e3 * ma, "min": 1e3 * min(ta), "max": 1e3 * max(ta)},
                          "calls_ms": {"median": 1e3 * mb, "min": 1e3 * min(tb), "max": 1e3 * max(tb)},
                          "ratio_calls_over_bank": mb / ma, "bank_us_per_tap": 1e6 * ma / ntaps,
                          "worst_difference_of_sum_abs_x": worst, "reps": a.reps, "kernel_of_calls": eng.last_kernel()}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
