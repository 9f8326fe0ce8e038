"""Closed-loop time of the float32 kernels against the float64 correlator (gc_set_precision, csrc/corr_f64.hip), host-closed
(gc_track) and device-closed (gc_track_device), on three shapes: 12 GPS L1 C/A channels (config 2's shape), 8 Galileo E1 B+C
channels (4-ms blocks) and 192 GPS L1 C/A channels.  Prints us per epoch and x real time per row, then the rows as JSON.
    python scripts/closed_loop_precision.py [seconds of the 12- and 8-channel records] [seconds of the 192-channel record]"""
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_workloads as W  # noqa: E402
import cu_sdr_collection_amd as P  # noqa: E402

seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
seconds_many = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
CASES = [("GPS L1 C/A x 12", "GPS_L1CA", 12, 18e6, seconds), ("Galileo E1 B+C x 8", "GAL_E1C", 8, 18e6, seconds),
         ("GPS L1 C/A x 192", "GPS_L1CA", 192, 18e6, seconds_many)]
MODES = {0: "launch per epoch", 1: "persistent host-fed kernel", 2: "device loop"}
rows = []
for label, pkgname, nch, fs, secs in CASES:
    owner = P.Engine(0)
    (pkg, S, scene), = W.make_band(P, owner, [(pkgname, min(nch, 24))], secs, fs, 20e3, 7007)
    n_ep = int((secs - 3 * S.intTime) / S.intTime) - 1
    sats = [scene[i % len(scene)] for i in range(nch)]          # beyond the scene's satellites: the same work per channel
    job = W.prepare_job(P, W.Job(label, pkg, copy.copy(S), sats, owner), n_ep)
    for precision in ("single", "double"):
        for device_loop in (False, True):
            owner.set_precision(precision)
            try:
                W.run_closed_loops(P, [job], device_loop=device_loop)   # first use
                t0 = time.perf_counter()
                W.run_closed_loops(P, [job], device_loop=device_loop)
                t = time.perf_counter() - t0
            finally:
                owner.set_precision("single")
            row = {"workload": label, "precision": precision, "loop": "device-closed" if device_loop else "host-closed",
                   "epochs": n_ep, "us_per_epoch": round(t / n_ep * 1e6, 2), "x_realtime": round(n_ep * S.intTime / t, 1),
                   "launcher": MODES.get(owner.last_track_mode(), "?")}
            rows.append(row)
            print(f"{label:20s} {precision:6s} {row['loop']:13s} {row['us_per_epoch']:9.2f} us/epoch {row['x_realtime']:8.1f} x real time"
                  f"  ({row['launcher']}, {n_ep} epochs)", flush=True)
    owner.close()
print(json.dumps(rows))
