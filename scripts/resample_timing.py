"""gc_resample against gc_downconvert at the same work per output, and against scipy.signal.upfirdn on one core.

Cases: one second of an 18 Msps int8 I/Q record -> 4 Msps int8 (L / M = 2 / 9, T = 145); one second of a 50 Msps int16 I/Q record
-> 20 Msps int8 (2 / 5, T = 81); the 18 Msps record at 64 / 63 (T = 2 047); and 1 / 3 (T = 25), which is gc_downconvert's call.
The records are Gaussian noise (sigma 20 / 5 000); the prototype is receiver.resample_taps' low-pass moved to a carrier, scaled to
an output rms near 25.
Wall clock around the library call (checks, tap layout and upload, kernel, synchronise), --warmup calls first, then the median and
spread of --reps calls.  Next to each: the tap steps the kernel runs (J = ceil(T / L) per output) and their rate, and two baselines:
gc_downconvert with T' = ceil(T / L) taps at D = ceil(M / L) on the same record for the same number of outputs (the same tap steps,
no phases), and the same filter through scipy.signal.upfirdn in complex128 (--no-upfirdn skips it).  --check compares the library's
record with tests/resample_model.py outside the near-half mask on the first 200 000 outputs.  One JSON line.

    python scripts/resample_timing.py [--reps 15] [--warmup 3] [--no-upfirdn] [--check] [--cases a,b]
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
from cu_sdr_collection_amd import receiver as R  # noqa: E402

# label, fs, samples, src dtype, L, M, T, carrier
CASES = (("18M_i8_2over9_T145", 18e6, 18_000_000, np.int8, 2, 9, 145, 2000137.0),
         ("50M_i16_2over5_T81", 50e6, 50_000_000, np.int16, 2, 5, 81, -4500137.0),
         ("18M_i8_64over63_T2047", 18e6, 18_000_000, np.int8, 64, 63, 2047, 2000137.0),
         ("18M_i8_1over3_T25", 18e6, 18_000_000, np.int8, 1, 3, 25, 2000137.0))


def timed(fn, warmup, reps):
    t = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    t = t[warmup:]
    return {"median": float(np.median(t)), "min": min(t), "max": max(t)}


def record(rng, ns, dtype):
    sigma = 20.0 if dtype == np.int8 else 5000.0
    info = np.iinfo(dtype)
    out = np.empty(2 * ns, dtype=dtype)
    for lo in range(0, 2 * ns, 1 << 24):                                               # in pieces: no float64 copy of the whole record
        hi = min(2 * ns, lo + (1 << 24))
        out[lo:hi] = np.clip(np.rint(rng.standard_normal(hi - lo) * sigma), info.min, info.max)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-upfirdn", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--cases", default="", help="comma-separated labels (default: all)")
    a = ap.parse_args()
    rng = np.random.default_rng(12)
    res = {"reps": a.reps, "warmup": a.warmup}
    records = {}
    with P.Engine(0) as src, P.Engine(0) as dst:
        res["device"] = src.device_info()[0]
        for label, fs, ns, dtype, L, M, T, fc in CASES:
            if a.cases and label not in a.cases.split(","):
                continue
            key = (fs, ns, dtype)
            if key not in records:
                records.clear()
                records[key] = record(rng, ns, dtype)
                src.load_if(records[key], fs=fs)
            raw = records[key]
            sigma = 20.0 if dtype == np.int8 else 5000.0
            J, D = -(-T // L), -(-M // L)
            first = (T - 1) // 2
            nout = min(ns * L // M, ns // D)                 # the same count for both calls: what the baseline's record still covers
            dst.alloc_if(nout, np.int8)
            g, f_used, _ = R.resample_taps(fs, L, M, fc, None, T)
            g = g * (25.0 / (sigma * np.sqrt(np.sum(np.abs(g) ** 2) / L)))   # white noise: sigma^2 sum |g|^2 / L per component, the phases averaged
            call = lambda: src.resample(dst, g, L, M, carr_freq=fc, first_tick=first, noutputs=nout)   # noqa: E731
            t = timed(call, a.warmup, a.reps)
            r = call()
            c = {"fs": fs, "samples": ns, "src": np.dtype(dtype).name, "interp": L, "decim": M, "ntaps": T, "branches": J, "outputs": nout, "ms": t,
                 "out_rate": r.out_rate, "bytes_moved": raw.nbytes + 2 * nout, "tap_steps": J * nout, "tap_steps_per_ns": J * nout / (t["median"] * 1e6),
                 "clipped": r.clipped, "rms": float(np.sqrt(r.sum_sq / (2.0 * nout))), "tile_outputs": P.Engine.debug_rs_tile_outputs(L, M, T)}
            if a.check:
                import resample_model as RM
                n_chk = min(nout, 200000)
                got = dst.read_if(0, n_chk)
                back = src.read_if(0, min(ns, (first + n_chk * M) // L + 2), dtype=dtype)
                want, _, _, near, _ = RM.resample(back, RM.IQ, g, L, M, fs, np.int8, RM.IQ, carr_freq=fc, first_tick=first, noutputs=n_chk)
                c["near_half"] = int(near.sum())
                c["differ_outside_the_mask"] = int(np.sum((got != want) & ~near))
            # the baseline: gc_downconvert, T' = J taps at D = ceil(M / L), the same outputs
            gb, _, _ = R.ddc_band_taps(fs, fc, fs / D / 2.0, J) if J > 1 else (np.ones(1, dtype=complex), 0.0, None)
            gb = gb * (25.0 / (sigma * np.sqrt(np.sum(np.abs(gb) ** 2))))
            base = lambda: src.downconvert(dst, gb, D, carr_freq=fc, first_sample=(J - 1) // 2, noutputs=nout)   # noqa: E731
            tb = timed(base, a.warmup, a.reps)
            c["downconvert"] = {"ntaps": J, "decim": D, "ms": tb, "tap_steps_per_ns": J * nout / (tb["median"] * 1e6)}
            c["rate_against_downconvert"] = tb["median"] / t["median"]
            if not a.no_upfirdn:
                from scipy.signal import upfirdn
                back = src.read_if(0, ns, dtype=dtype)
                t0 = time.perf_counter()
                z = back[0::2].astype(np.float64) + 1j * back[1::2].astype(np.float64)
                y = upfirdn(g, z, L, M)
                c["upfirdn_complex128_s"] = time.perf_counter() - t0
                del z, y, back
            res[label] = c
            print(f"{label}: {t['median']:.3f} ms, gc_downconvert {tb['median']:.3f} ms", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
