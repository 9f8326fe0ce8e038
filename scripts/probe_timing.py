"""gc_probe_psd + gc_probe_histogram against the way a caller gets the same arrays without them: gc_read_if of the range, then
scipy.signal.welch and np.bincount on the host.

Shape: one second of an int8 I/Q record at 18 Msps (18 000 000 samples, 36 MB) with probeData.m's call (32768, 2048, Hamming), i.e.
585 segments.  Both sides are wall clock around the calls, results in host arrays; warm-up first, then the sides alternate and the
medians and their spread (min .. max) go into one JSON line, with the largest relative difference of the two spectra (relative to the
largest bin) and whether the histograms agree.  The device side's two calls are also timed one by one.

Then the whole record of --seconds seconds (default 60: 2.16 GB) in one gc_probe_psd call of that many spans plus one histogram
call over all of it, device path alone: a second JSON line.

    python scripts/probe_timing.py [--reps 7] [--warmup 2] [--seconds 60]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cu_sdr_collection_amd as P  # noqa: E402

FS, NFFT, NOVERLAP = 18e6, 32768, 2048
L = P._lib


def stats(t):
    return {"median": 1e3 * float(np.median(t)), "min": 1e3 * min(t), "max": 1e3 * max(t)}


def device_side(eng, first, n, nspans=1):
    t0 = time.perf_counter()
    psd, k = eng.probe_psd(first, n, NFFT, NOVERLAP, "hamming", nspans=nspans)
    t1 = time.perf_counter()
    counts, norm2 = eng.probe_histogram(first, n * nspans)
    t2 = time.perf_counter()
    return (psd, counts, norm2, k), t2 - t0, t1 - t0, t2 - t1


def host_side(eng, first, n):
    from scipy.signal import welch
    t0 = time.perf_counter()
    raw = eng.read_if(first, n)
    t1 = time.perf_counter()
    x = raw[0::2].astype(np.float32) + 1j * raw[1::2].astype(np.float32)
    _, psd = welch(x, FS, window=np.hamming(NFFT), nperseg=NFFT, noverlap=NOVERLAP, nfft=NFFT, detrend=False, return_onesided=False)
    counts = np.stack([np.bincount(raw[c::2].astype(np.int64) + 128, minlength=257) for c in range(2)])
    v = raw.astype(np.int64)
    norm2 = int(np.max(v[0::2] ** 2 + v[1::2] ** 2))
    return (psd, counts, norm2), time.perf_counter() - t0, t1 - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=int, default=60)
    a = ap.parse_args()
    rng = np.random.default_rng(20241020)
    n = int(FS)
    t = np.arange(n)
    z = 25.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 30.0 * np.exp(2j * np.pi * ((0.2113 * t) % 1.0))   # noise and an interferer
    second = np.empty(2 * n, dtype=np.int8)
    second[0::2] = np.clip(np.rint(z.real), -128, 127)
    second[1::2] = np.clip(np.rint(z.imag), -128, 127)
    del z, t
    eng = P.Engine(0)
    t0 = time.perf_counter()
    eng.load_if(np.tile(second, a.seconds), fs=FS)
    load_s = time.perf_counter() - t0
    first = 12345
    for _ in range(a.warmup):
        device_side(eng, first, n), host_side(eng, first, n)
    td, tp, th, thost, tread = [], [], [], [], []
    for _ in range(a.reps):
        dev, all_d, psd_d, hist_d = device_side(eng, first, n)
        host, all_h, read_h = host_side(eng, first, n)
        td.append(all_d), tp.append(psd_d), th.append(hist_d), thost.append(all_h), tread.append(read_h)
    md, mh = float(np.median(td)), float(np.median(thost))
    spreads = (max(td) - min(td)) + (max(thost) - min(thost))
    print(json.dumps({"what": "1 s of record, (32768, 2048, Hamming)", "samples": n, "segments": dev[3], "device_ms": stats(td), "device_psd_ms": stats(tp),
                      "device_histogram_ms": stats(th), "host_ms": stats(thost), "host_read_if_ms": stats(tread), "ratio_host_over_device": mh / md,
                      "condition_met": md < mh - spreads,      # the device path's median below the host path's by more than the two spreads together
                      "psd_max_diff_rel_to_largest_bin": float(np.max(np.abs(dev[0][0] - host[0])) / np.max(host[0])),
                      "histograms_equal": bool(np.array_equal(dev[1], host[1]) and dev[2] == host[2]), "device_msamples_per_s": n / md / 1e6,
                      "reps": a.reps, "library": os.path.basename(L.LIB_PATH)}), flush=True)
    tw = []
    for _ in range(3):
        whole, all_w, psd_w, hist_w = device_side(eng, 0, n, nspans=a.seconds)
        tw.append((all_w, psd_w, hist_w))
    assert whole[0][0].tobytes() == eng.probe_psd(0, n, NFFT, NOVERLAP, "hamming")[0][0].tobytes()      # a span is the single call
    print(json.dumps({"what": f"{a.seconds} s of record in {a.seconds} spans, device path alone", "samples": n * a.seconds, "record_bytes": 2 * n * a.seconds,
                      "load_if_s": load_s, "device_ms": stats([x[0] for x in tw]), "device_psd_ms": stats([x[1] for x in tw]),
                      "device_histogram_ms": stats([x[2] for x in tw]),
                      "device_msamples_per_s": n * a.seconds / float(np.median([x[0] for x in tw])) / 1e6, "reps": 3}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
