"""gc_excise_sweep against gc_excise_bins at the same transform length on the same record, and against the numpy model of its
definition (tests/excise_sweep_model.py) on one core.

Shape: one second of an int8 I/Q record at 18 Msps (18 000 000 samples, 36 MB): Gaussian noise of sigma 8 per component and a chirp
of amplitude 40 from -0.4 fs to +0.4 fs, period 180 samples at nfft 64 and 8 192 at nfft 1024.  The limit is
receiver.excise_sweep_limit(power of the first 4 096 segments, 6).  Wall clock around the library call (checks, kernels,
synchronise), out of place, no optional output, widen = 1; --warmup calls first, then the median and spread of --reps calls; the
static call (a gain of ones) next to it, and their ratio.  Then the mean |z|^2 in front of and behind the call and the mean
|y - jam-free|^2, the share of cells cut, and the model in float64 on the first tenth of the record (its time is given as measured,
for 1 800 000 samples).  One JSON line.

    python scripts/excise_sweep_timing.py [--reps 15] [--warmup 3] [--no-model]
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
import excise_sweep_model as SM  # noqa: E402
from cu_sdr_collection_amd import receiver as R  # noqa: E402

FS, NS = 18e6, 18_000_000
CASES = ((64, 180), (1024, 8192))                                      # nfft, chirp period


def timed(fn, warmup, reps):
    t = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    t = t[warmup:]
    return {"median": float(np.median(t)), "min": min(t), "max": max(t)}


def mean_power(raw):
    x = raw.astype(np.float32)
    return float(np.mean(x * x)) * 2.0                                 # |z|^2 = c0^2 + c1^2: twice the mean square of the components


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(8)
    noise = 8.0 * (rng.standard_normal(NS) + 1j * rng.standard_normal(NS))
    clean = M.round_clamp(noise, np.int8, M.IQ)
    res = {"samples": NS, "record_bytes": 2 * NS, "reps": a.reps, "warmup": a.warmup, "widen": 1, "factor": 6.0}
    with P.Engine(0) as src, P.Engine(0) as dst:
        res["device"] = src.device_info()[0]
        dst.alloc_if(NS)
        for nfft, period in CASES:
            iq = M.round_clamp(noise + SM.chirp(NS, period, 40.0), np.int8, M.IQ)
            src.load_if(iq, fs=FS)
            train = src.excise_sweep(0, 4096 * (nfft // 2), np.full(nfft, np.inf, dtype=np.float32), 0, dst=dst, power=True).power[:4096]
            limit = R.excise_sweep_limit(train, 6.0)
            ones = np.ones(nfft, dtype=np.float32)
            r = {"chirp_period": period}
            r["sweep_ms"] = timed(lambda: src.excise_sweep(0, NS, limit, 1, dst=dst), a.warmup, a.reps)
            r["bins_ms"] = timed(lambda: src.excise_bins(0, NS, ones, dst=dst), a.warmup, a.reps)
            r["sweep_over_bins"] = r["sweep_ms"]["median"] / r["bins_ms"]["median"]
            r["sweep_all_outputs_ms"] = timed(lambda: src.excise_sweep(0, NS, limit, 1, dst=dst, values=True, power=True, masks=True, bin_cut=True), 1, 3)
            out = src.excise_sweep(0, NS, limit, 1, dst=dst)
            got = dst.read_if(0, NS)
            r["stats"] = vars(out.stats)
            r["cells_cut_share"] = out.stats.cut / (out.stats.segments * nfft)
            r["power_before"], r["power_after"], r["power_jam_free"] = mean_power(iq), mean_power(got), mean_power(clean)
            d = got.astype(np.float32) - clean.astype(np.float32)
            r["error_power"] = float(np.mean(d * d)) * 2.0
            if not a.no_model:
                n = NS // 10
                t0 = time.perf_counter()
                want = SM.excise_sweep(M.file_order(iq[:2 * n], M.IQ), limit, 1)
                rec = M.round_clamp(want.y, np.int8, M.IQ)
                r["numpy_model_s_for_a_tenth"] = time.perf_counter() - t0
                dev = src.excise_sweep(0, n, limit, 1, dst=dst, masks=True)
                r["decisions_that_differ_from_the_model"] = int((dev.hot != want.hot).sum())
                r["samples_that_differ_from_the_model"] = int(np.any(dst.read_if(0, n).reshape(n, 2) != rec.reshape(n, 2), axis=1).sum())
            res[f"nfft_{nfft}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
