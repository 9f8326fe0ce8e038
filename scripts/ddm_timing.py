"""gc_correlate_ddm against the way a caller gets the same bytes without it: F gc_correlate_bank calls on the same block list with
carr_freq shifted by the F frequency offsets (every call uploads the descriptors, reads and converts the samples and repeats the
float64 boundary search of every tap).

Shape: 12 GPS L1 C/A channels x 100 epochs of an int8 I/Q record at 18 Msps; two grids: 33 taps at j/17 chip with 17 bins spaced
125 Hz, and 5 taps with 64 bins.  Both sides are wall clock around the library calls, descriptors in and results out included;
warm-up first, then the two sides alternate and the medians and their spread (min .. max) are reported, one JSON line per grid.
The two sides' bytes are compared on the way.

    python scripts/ddm_timing.py [--reps 15] [--warmup 3] [--grids 33x17,5x64]

Another group size (bins per work item, csrc/corr_bank.hip) is a throw-away build, never a run-time switch:
    scripts/variants.sh corr_bank "DDM4:-DGC_DDM_GROUP=4" "DDM16:-DGC_DDM_GROUP=16"
    GC_LIB_PATH=cu-sdr-collection_amd/lib/libgnsscorr_DDM4.so python scripts/ddm_timing.py --grids 33x17

--dump-bank FILE writes the bytes gc_correlate_bank returns for the list at the first grid's taps (to compare two builds of the
library: the bank's kernel must not have changed).
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

FS, RATE, NCH, NEP = 18e6, 1.023e6, 12, 100


def grid(ntaps, nfreq):
    """(tap offsets in chips, frequency offsets in Hz), both symmetric about zero"""
    if ntaps == 33:
        offs = [j / 17 for j in range(-16, 17)]
    else:
        k = ntaps // 2
        offs = [j / (k + 1) for j in range(-k, k + 1)][:ntaps]
    spacing = 125.0 if nfreq <= 17 else 31.25
    return np.array(offs), np.array([(m - nfreq // 2) * spacing for m in range(nfreq)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grids", default="33x17,5x64")
    ap.add_argument("--dump-bank", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(20241018)
    nsamp = int(FS * NEP / 1000) + 18000
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
    dptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    grids = [tuple(int(v) for v in g.split("x")) for g in a.grids.split(",")]
    if a.dump_bank:
        off, _ = grid(*grids[0])
        out = np.zeros((nb, 3, off.shape[0], 2))
        P._lib.check(lib.gc_correlate_bank(ctx, nb, blocks, off.shape[0], dptr(off), dptr(out)))
        with open(a.dump_bank, "wb") as f:
            f.write(out.tobytes())
        print(json.dumps({"dump_bank": a.dump_bank, "bytes": out.nbytes, "library": P._lib.LIB_PATH}), flush=True)
        eng.close()
        return
    for ntaps, nfreq in grids:
        off, frq = grid(ntaps, nfreq)
        assert off.shape[0] == ntaps and frq.shape[0] == nfreq
        out_ddm = np.zeros((nb, 3, nfreq, ntaps, 2))
        out_bank = np.zeros((nfreq, nb, 3, ntaps, 2))
        lists = []                                   # the caller's F descriptor lists, prepared outside the timed region
        for f in frq:
            lst = eng.make_blocks(nb)
            C.memmove(lst, blocks, C.sizeof(blocks))
            for b in lst:
                b.carr_freq = float(np.float64(b.carr_freq) + np.float64(f))
            lists.append(lst)

        def ddm():
            t0 = time.perf_counter()
            P._lib.check(lib.gc_correlate_ddm(ctx, nb, blocks, ntaps, dptr(off), nfreq, dptr(frq), dptr(out_ddm)))
            return time.perf_counter() - t0

        def calls():
            t0 = time.perf_counter()
            for m, lst in enumerate(lists):
                P._lib.check(lib.gc_correlate_bank(ctx, nb, lst, ntaps, dptr(off), dptr(out_bank[m])))
            return time.perf_counter() - t0

        for _ in range(a.warmup):
            ddm()
            calls()
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(ddm())
            tb.append(calls())
        same = all(out_ddm[:, :, m].tobytes() == out_bank[m].tobytes() for m in range(nfreq))
        assert same, "gc_correlate_ddm and the gc_correlate_bank calls differ"
        ma, mb = float(np.median(ta)), float(np.median(tb))
        print(json.dumps({"ntaps": ntaps, "nfreq": nfreq, "blocks": nb, "same_bytes": same,
                          "ddm_ms": {"median": 1e3 * ma, "min": 1e3 * min(ta), "max": 1e3 * max(ta)},
                          "bank_calls_ms": {"median": 1e3 * mb, "min": 1e3 * min(tb), "max": 1e3 * max(tb)},
                          "ratio_calls_over_ddm": mb / ma, "ddm_ms_per_bin": 1e3 * ma / nfreq, "bank_ms_per_call": 1e3 * mb / nfreq,
                          "gap_over_spreads": (mb - ma) / ((max(ta) - min(ta)) + (max(tb) - min(tb))),
                          "reps": a.reps, "library": os.path.basename(P._lib.LIB_PATH)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
