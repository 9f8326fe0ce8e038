"""gc_excise_pulses and gc_excise_bins against reading the record back, the numpy model of their definitions (tests/excise_model.py)
on one core, and loading it again.

Shape: one second of an int8 I/Q record at 18 Msps (18 000 000 samples, 36 MB): Gaussian noise of sigma 20, a tone, and pulse pairs
that stand over the threshold.  Wall clock around the library call (checks, kernels, synchronise), --warmup calls first, then the
median and spread of --reps calls: gc_excise_pulses with guards of 64 / 256 samples, in place and out of place; gc_excise_bins at
nfft 4096 with a notch, with and without `values`.  Next to each the bytes of the record the call moves at least (what its kernels
read and write, as a multiple of the record's size) and the rate that makes.  Then gc_read_if + the model + gc_load_if once, and
whether the library's record equals the model's (pulses: every byte and statistic).  One JSON line.

    python scripts/excise_timing.py [--reps 15] [--warmup 3] [--no-model]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cu_sdr_collection_amd as P  # noqa: E402
import excise_model as M  # noqa: E402

FS, NS, NFFT = 18e6, 18_000_000, 4096
THRESHOLD2, BEFORE, AFTER = 100 * 100, 64, 256


def record(rng):
    z = 20.0 * (rng.standard_normal(NS) + 1j * rng.standard_normal(NS)) + 30.0 * np.exp(2j * np.pi * 0.123 * np.arange(NS))
    k = np.arange(-60, 61)
    env = 120.0 * np.exp(-0.5 * (k / 27.0) ** 2)
    for c in np.sort(rng.integers(100, NS - 400, 5400)):                             # 2 700 pairs per second and beacon, two beacons
        for off in (0, 216):
            z[c + off + k] += env * np.exp(2j * np.pi * (0.05 * (c + off + k) + rng.uniform()))
    return M.round_clamp(z, np.int8, M.IQ)


def timed(fn, warmup, reps):
    t = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    t = t[warmup:]
    return {"median": float(np.median(t)), "min": min(t), "max": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    iq = record(np.random.default_rng(7))
    gain = np.ones(NFFT, dtype=np.float32)
    gain[(int(round(0.123 * NFFT)) + np.arange(-2, 3)) % NFFT] = 0.0
    rec_bytes = 2 * NS
    with P.Engine(0) as src, P.Engine(0) as dst:
        src.load_if(iq, fs=FS)
        dst.alloc_if(NS)
        res = {"samples": NS, "record_bytes": rec_bytes, "device": src.device_info()[0], "reps": a.reps, "warmup": a.warmup, "nfft": NFFT}
        # bytes of the record per call: the mark kernel reads it, the blank kernel reads and writes it (out of place; in place only the
        # 16 bytes that hold a blanked sample); the spectral excision gathers it, copies it (out of place) and reads and writes the copy
        # (its float2 rows - 16 bytes per sample and pass, six passes - stay in the tile budget and are not counted)
        cases = (("pulses_out_of_place", lambda: src.excise_pulses(0, NS, THRESHOLD2, BEFORE, AFTER, dst=dst), 3.0),
                 ("bins_out_of_place", lambda: src.excise_bins(0, NS, gain, dst=dst), 5.0),
                 ("bins_out_of_place_values", lambda: src.excise_bins(0, NS, gain, dst=dst, values=True), 5.0))
        for label, fn, moved in cases:
            t = timed(fn, a.warmup, a.reps)
            res[label + "_ms"] = t
            res[label + "_record_bytes_moved"] = moved
            res[label + "_gb_per_s"] = moved * rec_bytes / (t["median"] * 1e-3) / 1e9
        st = src.excise_pulses(0, NS, THRESHOLD2, BEFORE, AFTER, dst=dst)
        res["pulse_stats"] = vars(st)

        def in_place():                                                                # every call on a fresh copy of the record
            dst.excise_pulses(0, NS, 1 << 40, 0, 0)
        src.excise_pulses(0, NS, 1 << 40, 0, 0, dst=dst)                               # a plain copy: nothing is hot
        res["pulses_in_place_nothing_hot_ms"] = timed(in_place, a.warmup, a.reps)
        if not a.no_model:
            src.excise_pulses(0, NS, THRESHOLD2, BEFORE, AFTER, dst=dst)
            got = dst.read_if(0, NS)
            t0 = time.perf_counter()
            back = src.read_if(0, NS)
            t1 = time.perf_counter()
            want, want_st = M.excise_pulses(back, M.IQ, 0, NS, THRESHOLD2, BEFORE, AFTER)
            t2 = time.perf_counter()
            dst.load_if(want, fs=FS)
            t3 = time.perf_counter()
            res["pulses_read_model_load_s"] = {"read_if": t1 - t0, "numpy_model": t2 - t1, "load_if": t3 - t2}
            res["pulses_equal_to_the_model"] = bool(np.array_equal(got, want)) and vars(st) == vars(want_st)
            dst.alloc_if(NS)
            vals = src.excise_bins(0, NS, gain, dst=dst, values=True)
            got = dst.read_if(0, NS)
            t0 = time.perf_counter()
            y = M.excise_bins(M.file_order(src.read_if(0, NS), M.IQ), gain)
            want = M.round_clamp(y, np.int8, M.IQ)
            t1 = time.perf_counter()
            res["bins_read_model_s"] = t1 - t0
            res["bins_max_abs_values_minus_y_lsb"] = float(max(np.abs(vals.real - y.real).max(), np.abs(vals.imag - y.imag).max()))
            res["bins_samples_that_differ_from_the_model"] = int(np.any(got.reshape(NS, 2) != want.reshape(NS, 2), axis=1).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
