"""Tracking a FILE in windows with the loop closed on the host (gc_track_file) against the loop closed on the device
(gc_track_file_device), next to gc_track_device on the resident record: the configuration-2 shape (12 GPS L1 C/A channels) and
192 channels, float32 and float64, one process, one file, the runs alternating.  Prints us per epoch and wall seconds per row
(median and spread of the repeats), how much of the windows' read + upload was hidden behind tracking, then the rows as JSON.
    python scripts/stream_device_loop.py [seconds of the 12-channel record] [seconds of the 192-channel record] [repeats]

hidden upload: with U the time to read the file and upload it whole (gc_open_if_file) and R the resident device-closed call,
a windowed call that hid nothing takes R + U; hidden = 1 - (windowed - R) / U, cut to [0, 1] (the windowed call also pays one
launch and one state round trip per window, counted against it here)."""
import copy
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_workloads as W  # noqa: E402
import cu_sdr_collection_amd as P  # noqa: E402

seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
seconds_many = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
FS = 18e6
MODES = {0: "launch per epoch", 1: "persistent host-fed kernel", 2: "device loop"}
rows = []
with tempfile.TemporaryDirectory() as td:
    for label, nch, secs in (("GPS L1 C/A x 12", 12, seconds), ("GPS L1 C/A x 192", 192, seconds_many)):
        eng = P.Engine(0)
        (pkg, S, scene), = W.make_band(P, eng, [("GPS_L1CA", min(nch, 24))], secs, FS, 20e3, 7007)
        n_samples = int(round(secs * FS))
        path = os.path.join(td, f"record_{nch}.bin")
        eng.read_if(0, n_samples).tofile(path)
        n_ep = int((secs - 3 * S.intTime) / S.intTime) - 1
        sats = [scene[i % len(scene)] for i in range(nch)]          # beyond the scene's satellites: the same work per channel
        job = W.prepare_job(P, W.Job(label, pkg, copy.copy(S), sats, eng), n_ep)
        window = int(0.5 * FS) if secs >= 4 else int(secs * FS / 8)

        def resident():
            eng.open_if_file(path)
            eng.set_sampling_freq(FS)
            t0 = time.perf_counter()
            _, done, st = eng.track(job.params, job.inits, device_loop=True)
            return time.perf_counter() - t0, done, st

        def upload():
            t0 = time.perf_counter()
            eng.open_if_file(path)
            return time.perf_counter() - t0, None, 0

        def windowed(device_loop):
            def run():
                t0 = time.perf_counter()
                _, done, st = eng.track_file(path, job.params, job.inits, window, device_loop=device_loop)
                return time.perf_counter() - t0, done, st
            return run

        for precision in ("single", "double"):
            eng.set_precision(precision)
            try:
                runs = {"upload alone": upload, "resident, device-closed": resident, "windows, host-closed": windowed(False),
                        "windows, device-closed": windowed(True)}
                times = {k: [] for k in runs}
                launcher = {}
                for rep in range(repeats + 1):                      # the first round is the warm-up; the runs alternate
                    for name, fn in runs.items():
                        t, done, st = fn()
                        if done is not None and (st != 0 or int(done.min()) != n_ep):
                            raise RuntimeError(f"{label} {name}: stopped early (status {st}, epochs {done})")
                        launcher[name] = MODES.get(eng.last_track_mode(), "?")
                        if rep:
                            times[name].append(t)
            finally:
                eng.set_precision("single")
            med = {k: statistics.median(v) for k, v in times.items()}
            for name in list(runs)[1:]:
                row = {"workload": label, "precision": precision, "run": name, "epochs": n_ep, "windows_of_samples": window if "windows" in name else 0,
                       "wall_s": round(med[name], 4), "wall_s_min_max": [round(min(times[name]), 4), round(max(times[name]), 4)],
                       "us_per_epoch": round(med[name] / n_ep * 1e6, 2), "launcher": launcher[name]}
                if "windows" in name:
                    row["upload_hidden"] = round(min(1.0, max(0.0, 1.0 - (med[name] - med["resident, device-closed"]) / med["upload alone"])), 2)
                rows.append(row)
                print(f"{label:18s} {precision:6s} {name:24s} {row['us_per_epoch']:8.2f} us/epoch {row['wall_s']:8.4f} s "
                      f"[{row['wall_s_min_max'][0]:.4f} .. {row['wall_s_min_max'][1]:.4f}]"
                      + (f"  upload hidden {row['upload_hidden']:.2f} (alone {med['upload alone']:.4f} s)" if "windows" in name else "")
                      + f"  ({row['launcher']}, {n_ep} epochs)", flush=True)
        eng.close()
print(json.dumps(rows))
