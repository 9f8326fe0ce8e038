"""gc_downconvert against reading the record back, the numpy model of its definition (tests/ddc_model.py) on one core, and loading
the result again.

Cases: one second of an 18 Msps int8 I/Q record -> 6 Msps int8 (D = 3, T = 25 and T = 129); one second of a 50 Msps int16 I/Q record
-> 25 Msps int8 (D = 2, T = 65); T = 1, D = 1 on the 18 Msps record, as the floor of the call.  The records are Gaussian noise (sigma
20 / 5 000); the taps a firwin low-pass of half the output rate moved to a carrier, scaled to an output rms near 25.
Wall clock around the library call (checks, tap upload, kernel, synchronise), --warmup calls first, then the median and spread of
--reps calls.  Next to each: the bytes the call moves at least (the record once, the output once), the tap steps (taps x outputs)
and the rates those make.  Then gc_read_if + the model + gc_load_if once per case (--no-model skips it; --upfirdn adds the same
filter through scipy.signal.upfirdn in complex128), and whether the library's record equals the model's outside the near-half mask.
One JSON line.

    python scripts/ddc_timing.py [--reps 15] [--warmup 3] [--no-model] [--upfirdn]
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
import ddc_model as M  # noqa: E402
from cu_sdr_collection_amd import receiver as R  # noqa: E402

# label, fs, samples, src dtype, D, T, carrier
CASES = (("18M_i8_D3_T25", 18e6, 18_000_000, np.int8, 3, 25, 2000137.0),
         ("18M_i8_D3_T129", 18e6, 18_000_000, np.int8, 3, 129, 2000137.0),
         ("50M_i16_D2_T65", 50e6, 50_000_000, np.int16, 2, 65, -4500137.0),
         ("18M_i8_D1_T1", 18e6, 18_000_000, np.int8, 1, 1, 0.0))


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
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--upfirdn", action="store_true")
    ap.add_argument("--cases", default="", help="comma-separated labels (default: all)")
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    res = {"reps": a.reps, "warmup": a.warmup}
    records = {}
    with P.Engine(0) as src, P.Engine(0) as dst:
        res["device"] = src.device_info()[0]
        for label, fs, ns, dtype, D, T, fc in CASES:
            if a.cases and label not in a.cases.split(","):
                continue
            key = (fs, ns, dtype)
            if key not in records:
                records.clear()
                records[key] = record(rng, ns, dtype)
                src.load_if(records[key], fs=fs)
            raw = records[key]
            first = (T - 1) // 2
            nout = ns // D
            dst.alloc_if(nout, np.int8)
            g, f_used, _ = R.ddc_band_taps(fs, fc, fs / D / 2.0, T)
            if T > 1:                                # white noise of sigma per component leaves sigma sqrt(sum |g|^2) per component
                g = g * (25.0 / ((20.0 if dtype == np.int8 else 5000.0) * np.sqrt(np.sum(np.abs(g) ** 2))))
            call = lambda: src.downconvert(dst, g, D, carr_freq=fc, first_sample=first, noutputs=nout)   # noqa: E731
            t = timed(call, a.warmup, a.reps)
            r = call()
            moved = raw.nbytes + 2 * nout
            c = {"fs": fs, "samples": ns, "src": np.dtype(dtype).name, "decim": D, "ntaps": T, "outputs": nout, "ms": t, "bytes_moved": moved,
                 "gb_per_s": moved / (t["median"] * 1e-3) / 1e9, "tap_steps": T * nout, "tap_steps_per_ns": T * nout / (t["median"] * 1e6),
                 "clipped": r.clipped, "rms": float(np.sqrt(r.sum_sq / (2.0 * nout))), "tile_outputs": P.Engine.debug_ddc_tile_outputs(D, T)}
            if not a.no_model:
                got = dst.read_if(0, nout)
                t0 = time.perf_counter()
                back = src.read_if(0, ns, dtype=dtype)
                t1 = time.perf_counter()
                want, clipped, sum_sq, near, _ = M.downconvert(back, M.IQ, g, D, fs, np.int8, M.IQ, carr_freq=fc, first_sample=first, noutputs=nout)
                t2 = time.perf_counter()
                dst.load_if(want, fs=fs / D)
                t3 = time.perf_counter()
                c["read_model_load_s"] = {"read_if": t1 - t0, "numpy_model": t2 - t1, "load_if": t3 - t2}
                c["near_half"] = int(near.sum())
                c["differ_outside_the_mask"] = int(np.sum((got != want) & ~near))
                c["statistics_equal"] = bool((r.clipped, r.sum_sq) == (clipped, sum_sq))
                if a.upfirdn:
                    from scipy.signal import upfirdn
                    t0 = time.perf_counter()
                    z = back[0::2].astype(np.float64) + 1j * back[1::2].astype(np.float64)
                    y = upfirdn(g, z, 1, D)
                    c["upfirdn_complex128_s"] = time.perf_counter() - t0
                    del z, y
            res[label] = c
            print(f"{label}: {t['median']:.3f} ms", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
