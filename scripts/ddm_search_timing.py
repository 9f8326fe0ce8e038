"""gc_correlate_ddm_search against the way a caller gets the same maps without it: one gc_correlate_ddm_integrate call per hypothesis
on the hypothesis's window (the identity of include/gnsscorr.h), each returning its power maps, the peaks picked on the host.

Shape: 12 GPS L1 C/A channels x 100 epochs of an int8 I/Q record at 18 Msps, the list channel by channel, runs of 20 epochs.  Two grids:

    bit edge        17 bins spaced 25 Hz x 33 taps at j/17 chip, 20 shifts of the run grid.  A shifted window may not straddle two
                    channels, so this search is one call per channel (100 blocks, 4 runs common to every shift, one map): 12 search
                    calls against 12 x 20 integrate calls of 80 blocks.
    secondary code  5 bins spaced 25 Hz x 5 taps at j/4 chip, 100 weight rows (the 20 phases of five 20-chip patterns), no shifts, one
                    map of 5 runs per channel: ONE search call on the 1 200 blocks against 100 integrate calls on them.

Both sides are wall clock around the calls, descriptors in and results out included; warm-up first, then the sides alternate and the
medians and their spread (min .. max) are reported in one JSON line per grid, with the bytes each side brings back from the library.
The search is timed as a caller uses it (peaks alone) and once more with the power maps coming back; one integrate call on the same
list is timed too, to show how far above "one map" a search costs.  The power maps of the two sides are compared byte for byte on the way,
the peaks against numpy.argmax of those maps.

    python scripts/ddm_search_timing.py [--reps 15] [--warmup 3]
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
L = P._lib
dptr = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
iptr = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731


def stats(t):
    return {"median": 1e3 * float(np.median(t)), "min": 1e3 * min(t), "max": 1e3 * max(t)}


def first_maxima(pw):
    flat = pw.reshape(pw.shape[:-2] + (-1,))
    idx = np.argmax(flat, axis=-1)
    return np.take_along_axis(flat, idx[..., None], axis=-1)[..., 0], idx // pw.shape[-1], idx % pw.shape[-1]


class Grid:
    """One search: `calls` = [(first block, blocks)] of the list a search call takes each; per call nhyp hypotheses with `shifts` (or
    None) and `weights` [nhyp, blocks of the call] (or None), run_len / map_len of a hypothesis."""

    def __init__(self, eng, blocks, name, off, frq, calls, shifts, weights, run_len, map_len):
        self.eng, self.blocks, self.name, self.off, self.frq, self.calls = eng, blocks, name, off, frq, calls
        self.shifts = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.int32)
        self.weights = weights
        self.run_len, self.map_len = np.ascontiguousarray(run_len, dtype=np.int32), np.ascontiguousarray(map_len, dtype=np.int32)
        self.nhyp = len(shifts) if shifts is not None else weights.shape[0]
        self.nused = int(self.run_len.sum())
        nt, nf, nm = len(off), len(frq), len(map_len)
        self.pk = np.zeros((len(calls), self.nhyp, nm, 3), dtype=L.DDM_PEAK_DTYPE)
        self.pw = np.zeros((len(calls), self.nhyp, nm, 3, nf, nt))
        self.ref = np.zeros((len(calls), self.nhyp, nm, 3, nf, nt))
        self.one = np.zeros((nm, 3, nf, nt))

    def _sub(self, first, n):
        return (L.gc_block * n).from_address(C.addressof(self.blocks) + first * C.sizeof(L.gc_block))

    def search(self, with_pow):
        t0 = time.perf_counter()
        for k, (first, n) in enumerate(self.calls):
            L.check(self.eng._lib.gc_correlate_ddm_search(
                self.eng._ctx, n, self._sub(first, n), self.nhyp, iptr(self.shifts), dptr(self.weights), len(self.off), dptr(self.off),
                len(self.frq), dptr(self.frq), len(self.run_len), iptr(self.run_len), len(self.map_len), iptr(self.map_len), None,
                dptr(self.pw[k]) if with_pow else None, self.pk[k].ctypes.data_as(C.POINTER(L.gc_ddm_peak))))
        return time.perf_counter() - t0

    def integrate(self, one_only=False):
        """The other side: per call and hypothesis the integrate call on the window; one_only: a single such call."""
        t0 = time.perf_counter()
        for k, (first, n) in enumerate(self.calls):
            for h in range(self.nhyp):
                s = 0 if self.shifts is None else int(self.shifts[h])
                w = None if self.weights is None else self.weights[h, s:s + self.nused]
                L.check(self.eng._lib.gc_correlate_ddm_integrate(
                    self.eng._ctx, self.nused, self._sub(first + s, self.nused), dptr(w), len(self.off), dptr(self.off), len(self.frq),
                    dptr(self.frq), len(self.run_len), iptr(self.run_len), len(self.map_len), iptr(self.map_len), None,
                    dptr(self.one if one_only else self.ref[k, h])))
                if one_only:
                    return time.perf_counter() - t0
        self.host_peaks = first_maxima(self.ref)     # what the caller of the integrate function does next
        return time.perf_counter() - t0

    def run(self, reps, warmup):
        for _ in range(warmup):
            self.search(False), self.search(True), self.integrate(), self.integrate(True)
        ts, tp, ti, t1 = [], [], [], []
        for _ in range(reps):
            ts.append(self.search(False))
            ti.append(self.integrate())
            tp.append(self.search(True))
            t1.append(self.integrate(True))
        assert self.pw.tobytes() == self.ref.tobytes(), "the search's power maps are not the integrate calls' bytes"
        val, m, j = first_maxima(self.pw)
        assert self.pk["power"].tobytes() == val.tobytes() and np.array_equal(self.pk["bin"], m) and np.array_equal(self.pk["tap"], j)
        ms, mi = float(np.median(ts)), float(np.median(ti))
        spreads = (max(ts) - min(ts)) + (max(ti) - min(ti))
        return {"grid": self.name, "nfreq": len(self.frq), "ntaps": len(self.off), "hypotheses": self.nhyp, "search_calls": len(self.calls),
                "integrate_calls": len(self.calls) * self.nhyp, "blocks_per_search_call": self.calls[0][1], "runs": len(self.run_len),
                "maps": len(self.map_len), "search_peaks_only_ms": stats(ts), "search_with_pow_ms": stats(tp), "integrate_calls_ms": stats(ti),
                "one_integrate_call_ms": stats(t1), "ratio_integrate_calls_over_search": mi / ms,
                "condition_met": ms < mi - spreads,      # the search's median below the other side's by more than the two spreads together
                "bytes_returned": {"search_peaks_only": self.pk.nbytes, "search_with_pow": self.pk.nbytes + self.pw.nbytes,
                                   "integrate_calls": self.ref.nbytes},
                "reps": reps, "library": os.path.basename(L.LIB_PATH)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(20241019)
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
    edge = Grid(eng, blocks, "bit edge", np.array([j / 17 for j in range(-16, 17)]), np.array([(m - 8) * 25.0 for m in range(17)]),
                [(c * NEP, NEP) for c in range(NCH)], np.arange(RUN), None, [RUN] * ((NEP - RUN + 1) // RUN), [(NEP - RUN + 1) // RUN])
    patterns = rng.choice(np.array([1.0, -1.0]), size=(5, RUN))
    n = np.arange(nb)
    rows = np.concatenate([pat[(n[None, :] + np.arange(RUN)[:, None]) % RUN] for pat in patterns])       # [100, nb]
    sec = Grid(eng, blocks, "secondary code", np.array([j / 4 for j in range(-2, 3)]), np.array([(m - 2) * 25.0 for m in range(5)]),
               [(0, nb)], None, np.ascontiguousarray(rows), [RUN] * (nb // RUN), [NEP // RUN] * NCH)
    for g in (edge, sec):
        print(json.dumps(g.run(a.reps, a.warmup)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
