"""The loop closure (csrc/devloop.h: devloop_cut, devloop_pre, devloop_post - the ONE float64 restatement of tracking.m:219-222,
241-245, 273-283, 302-348 that gc_track's host loop and the device loops share) without a GPU: tests/loop_closure_shim.hip runs
it on the CPU over the correlator sums the REFERENCE'S OWN tracking.m recorded (tests/golden/ref_track_<scene>.npz), from each
scene's initial state, and what it records is compared with what the reference recorded.

Sums: I_E ... Q_L and the Pilot_* sums of the fixture.  The reference drops some pilot sums it computes (the early / late ones, or
all six: tracking.m:47-86 of the package); those - and only those - are taken from the float64 oracle's run of the scene, which
test_ref_vectors.py pins to the fixture at 1e-12.  Scenes that fold two pilot arms (pilot_combine 4 / 5) record the folded pilot,
not the raw arms, and cannot be replayed this way: they are the only ones left out.

Bounds (tests/test_gpu_tracking_f64.py::_against_the_reference): absoluteSample identical; carrFreq, codeFreq, remCodePhase,
remCarrPhase (modulo 2 pi) and the four discriminator fields within 1e-10 of max|want|."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_scenes as RS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
_SUMS = ("I_E", "Q_E", "I_P", "Q_P", "I_L", "Q_L")
_CHECKED = ("carrFreq", "codeFreq", "remCodePhase", "remCarrPhase", "dllDiscr", "dllDiscrFilt", "pllDiscr", "pllDiscrFilt")
TOL = 1e-10


def _shim():
    from cu_sdr_collection_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src, out = os.path.join(HERE, "loop_closure_shim.hip"), os.path.join(HERE, "build", "libloop_closure_shim.so")
    deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = [f for f in B._tu_flags("track.hip") if f != "--offload-compress"]     # -ffp-contract=off among them
        subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.loop_closure_replay.restype = C.c_int
    return lib


def _replay_scene(lib, sc):
    """trackResults of the scene from the closure on the CPU, or None for a scene that folds two pilot arms."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import _lib as L
    from cu_sdr_collection_amd import receiver as R
    from oracle import gnss_oracle as O
    z = np.load(os.path.join(GOLD, f"ref_track_{sc.name}.npz"))
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    assert RS.crc(rec) == int(z["record_crc32"][0])
    chans = {}

    class NoEngine:                                # _tracking_prepare configures the channels: keep arms and index scale
        def set_channel(self, i, tables, index_scale=1.0, arm_mult=None, windows=None):
            chans[i] = (len(tables), float(index_scale))

    job = R._tracking_prepare(NoEngine(), ch, S, sc.signal)
    p = job.p
    if p.pilot_combine in (4, 5):
        return None, z
    n_ep, nch = p.n_epochs, len(job.active)
    out = np.zeros((nch, L.GC_TRK_NFIELDS, n_ep))
    done = np.zeros(nch, dtype=np.int64)
    oracle = None
    for k, i in enumerate(job.active):
        arms, scale = chans[i]
        sums = np.zeros((n_ep, L.GC_OUT_STRIDE))
        for v, f in enumerate(_SUMS):
            sums[:, v] = z["f_" + f][i]
            if arms >= 2:
                if "f_Pilot_" + f in z.files:
                    sums[:, 6 + v] = z["f_Pilot_" + f][i]
                else:                              # computed and dropped by the reference: the float64 oracle's
                    oracle = oracle or sc.oracle(O, rec, ch, S)
                    sums[:, 6 + v] = getattr(oracle[i], "Pilot_" + f)
        status = C.c_int(-1)
        done[k] = lib.loop_closure_replay(C.byref(p), C.byref(job.inits[k]), C.c_int(arms), C.c_double(scale), C.c_ulonglong(1 << 62),
                                          sums.ctypes.data_as(C.POINTER(C.c_double)), out[k].ctypes.data_as(C.POINTER(C.c_double)), C.byref(status))
        assert (done[k], status.value) == (n_ep, 1), (sc.name, i, done[k], status.value)
    fields = {name: out[:, j, :] for j, name in enumerate(L.TRK_FIELDS)}
    tr, _ = R._tracking_finish(job, fields, done, L.GC_OK)
    return tr, z


def test_the_shared_closure_follows_the_references_tracking_m_over_its_own_sums():
    lib = _shim()
    ran, folds = 0, 0
    for sc in RS.TRACK_SCENES:
        tr, z = _replay_scene(lib, sc)
        if tr is None:
            folds += 1
            continue
        worst, compared = {}, 0
        for k, t in enumerate(tr):
            if str(z["status"][k]) != "T":
                continue
            compared += 1
            want, have = z["f_absoluteSample"][k], t.absoluteSample
            assert np.array_equal(have, want), (sc.name, k, np.flatnonzero(have != want)[:5])
            for f in _CHECKED:
                want, have = z["f_" + f][k], getattr(t, f)
                assert np.all(np.isfinite(want)) and have.shape == want.shape, (sc.name, k, f)
                dd = np.abs(have - want)
                if f == "remCarrPhase":
                    dd = np.minimum(dd, np.abs(dd - 2 * np.pi))
                scale = float(np.max(np.abs(want)))
                worst[f] = max(worst.get(f, 0.0), float(np.max(dd)) / scale if scale > 0 else float(np.max(dd)))
        print(f"\n[closure] {sc.name}: " + ", ".join(f"{f} {v:.1e}" for f, v in sorted(worst.items())))
        assert compared >= 1, sc.name
        for f, v in worst.items():
            assert v <= TOL, (sc.name, f, v)
        ran += 1
    print(f"\n[closure] {ran} of {len(RS.TRACK_SCENES)} scenes replayed, {folds} left out (pilot_combine 4 / 5)")
    assert ran >= len(RS.TRACK_SCENES) - folds
