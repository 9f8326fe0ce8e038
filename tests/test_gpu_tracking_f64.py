"""The float64 precision mode (include/gnsscorr.h gc_set_precision, csrc/corr_f64.hip) against what the REFERENCE'S OWN .m files
computed (tests/golden/ref_track_*.npz): with the correlations in float64 the closed loops - host-closed (a launch per epoch) and
device-closed (one workgroup per channel) - follow tracking.m epoch for epoch instead of statistically.

Bounds (tol: relative to max|want| of the field; remCarrPhase modulo 2 pi):
  absoluteSample                           identical, every epoch, every scene (GPS L2C's fractional record included)
  every other field, the 16 short scenes   1e-10;  C/N0 1e-9 dB, VSMIndex identical
  every other field, the 3 long runs       1e-9 (the C float64 oracle's bound);  C/N0 1e-6 dB;  sign(I_P) identical from epoch 0
  per-block sums of gc_correlate           1e-12 of max|want| against the float64 Python oracle (and the C oracle on int8 I/Q)
Every test passes precision= (or sets it and restores it): the session's shared engine must leave each test at float32."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ref_scenes as RS

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_SUMS = ("I_E", "Q_E", "I_P", "Q_P", "I_L", "Q_L")


def _prec(engine) -> int:
    import ctypes as C
    v = C.c_int(-1)
    assert engine._lib.gc_get_precision(engine._ctx, C.byref(v)) == 0
    return v.value


def _against_the_reference(tr, z, ch, tol, cno_tol):
    """trackResults against the reference's; returns the largest relative deviation per field (printed: the measured figures)."""
    ref_fields = [k[2:] for k in z.files if k.startswith("f_") and k != "f_PRN"]
    assert [t.status for t in tr] == [str(s) for s in z["status"]]
    worst = {}
    for k, t in enumerate(tr):
        have_fields = {f for f in vars(t) if isinstance(getattr(t, f), np.ndarray)}
        assert have_fields == set(ref_fields), sorted(have_fields ^ set(ref_fields))
        for f in ref_fields:
            want, have = z["f_" + f][k], getattr(t, f)
            assert have.shape == want.shape, f
            assert np.array_equal(np.isinf(have), np.isinf(want)), (k, f)
            m = np.isfinite(want)
            if not m.any():
                continue
            if f == "absoluteSample":
                assert np.array_equal(have[m], want[m]), (k, f, np.flatnonzero(have[m] != want[m])[:5])
                continue
            dd = np.abs(have[m] - want[m])
            if f == "remCarrPhase":
                dd = np.minimum(dd, np.abs(dd - 2 * np.pi))
            scale = float(np.max(np.abs(want[m])))
            rel = float(np.max(dd)) / scale if scale > 0 else float(np.max(dd))
            worst[f] = max(worst.get(f, 0.0), rel)
            assert rel <= tol, (k, f, rel)
        if "cno_VSMValue" in z.files and t.status == "T":
            d = float(np.max(np.abs(np.asarray(t.CNo.VSMValue, dtype=np.float64) - z["cno_VSMValue"][k]))) if len(z["cno_VSMValue"][k]) else 0.0
            worst["CNo.VSMValue(dB)"] = max(worst.get("CNo.VSMValue(dB)", 0.0), d)
            assert d <= cno_tol, (k, d)
            assert np.array_equal(np.asarray(t.CNo.VSMIndex, dtype=np.float64), z["cno_VSMIndex"][k])
    sat = [getattr(c, "K", getattr(c, "PRN", 0)) for c in ch]
    for k, t in enumerate(tr):
        if bool(z["PRN_set"][k]):
            assert t.PRN == z["PRN"][k] == sat[k]
    return worst


def _run_scene(engine, sc, device_loop):
    import cu_sdr_collection_amd as P
    z = np.load(os.path.join(GOLD, f"ref_track_{sc.name}.npz"))
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    assert RS.crc(rec) == int(z["record_crc32"][0])
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    tr, _ = P.tracking(engine, ch, S, signal=sc.signal, device_loop=device_loop, precision="double")
    assert _prec(engine) == 0                                   # the keyword restored the shared engine's float32
    return tr, z, ch, S


@pytest.mark.parametrize("device_loop", [False, True], ids=["host_loop", "device_loop"])
@pytest.mark.parametrize("sc", RS.TRACK_SCENES, ids=[s.name for s in RS.TRACK_SCENES])
def test_f64_closed_loop_equals_the_references_tracking_m(engine, sc, device_loop):
    tr, z, ch, _ = _run_scene(engine, sc, device_loop)
    assert engine.last_track_mode() == (2 if device_loop else 0)
    if not device_loop:
        assert engine.last_kernel() == 6
    worst = _against_the_reference(tr, z, ch, tol=1e-10, cno_tol=1e-9)
    print(f"\n[f64] {sc.name} {'device' if device_loop else 'host'}: " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("device_loop", [False, True], ids=["host_loop", "device_loop"])
@pytest.mark.parametrize("sc", RS.LONG_TRACK_SCENES, ids=[s.name for s in RS.LONG_TRACK_SCENES])
def test_f64_long_closed_loop_follows_the_references_tracking_m_epoch_for_epoch(engine, sc, device_loop):
    """1 200 / 300 / 800 epochs: the float32 loops leave the reference's trajectory after 261 - 3 666 epochs
    (test_gpu_ref_vectors.py: test_long_closed_loop_stays_with_the_references_tracking_m); the float64 loops do not."""
    tr, z, ch, _ = _run_scene(engine, sc, device_loop)
    assert engine.last_track_mode() == (2 if device_loop else 0)
    for k, t in enumerate(tr):
        if str(z["status"][k]) == "T":
            assert np.array_equal(np.sign(t.I_P), np.sign(z["f_I_P"][k])), k       # the same navigation bits from epoch 0
    worst = _against_the_reference(tr, z, ch, tol=1e-9, cno_tol=1e-6)
    print(f"\n[f64] {sc.name} {'device' if device_loop else 'host'}: " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))


def test_f64_device_loop_is_bitwise_reproducible(engine):
    import cu_sdr_collection_amd as P
    sc = next(s for s in RS.LONG_TRACK_SCENES if s.name == "GAL_E1C_long")
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    runs = [P.tracking(engine, ch, S, signal=sc.signal, device_loop=True, precision="double")[0] for _ in range(2)]
    for a, b in zip(*runs):
        assert a.status == b.status
        for f in vars(a):
            if isinstance(getattr(a, f), np.ndarray):
                assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
        assert np.array_equal(np.asarray(a.CNo.VSMValue), np.asarray(b.CNo.VSMValue))


# per-block sums: blocks rebuilt from the reference's recorded states (as test_gpu_ref_vectors.py's replay test does)
_BLOCK_SCENES = ("GPS_L1CA", "GPS_L5C", "GPS_L1CA_int16_skip", "GPS_L1CA_real", "BDS_B1C_WB", "GPS_L2C")
_EPOCHS = 12


@pytest.mark.parametrize("name", _BLOCK_SCENES)
def test_f64_correlate_equals_the_float64_oracle_per_block(engine, name):
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import signals
    from oracle import c_oracle as CO
    from oracle import gnss_oracle as O
    sc = next(s for s in RS.TRACK_SCENES if s.name == name)
    z = np.load(os.path.join(GOLD, f"ref_track_{sc.name}.npz"))
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    spec = signals.SIGNALS[sc.signal]
    nch, n_ep = 2, min(_EPOCHS, z["f_carrFreq"].shape[1])
    tables = [spec.tables(int(z["PRN"][k]), S) for k in range(nch)]
    for k in range(nch):
        engine.set_channel(k, tables[k], index_scale=spec.index_scale, arm_mult=spec.arm_mult, windows=spec.windows)
    blocks = engine.make_blocks(nch * n_ep)
    fs = S.samplingFreq
    for e in range(n_ep):
        for k in range(nch):
            b = blocks[e * nch + k]
            step = float(z["f_codeFreq"][k][e]) / fs
            rem = float(z["f_remCodePhase"][k][e])
            pos = float(z["f_absoluteSample"][k][e])
            length, spacing = S.codeLength, S.dllCorrelatorSpacing
            if spec.doubled_code:      # GPS L2C: RZ-doubled code, records in single-code units (see the replay test)
                step, rem, length, spacing = 2 * step, 2 * rem, 2 * S.codeLength, 2 * S.dllCorrelatorSpacing
                pos = float(np.rint(pos - 1 + rem / step))
                b.table_offset[1] = int(length) * ((int(ch[k].CLCodePhase) - 1 + e) % 75)
            b.channel = k
            b.first_sample = int(pos)
            b.rem_code_phase = rem
            b.code_phase_step = step
            b.blksize = int(np.ceil((length - rem) / step))
            b.el_spacing = spacing
            b.carr_freq = float(z["f_carrFreq"][k][e])
            b.rem_carr_phase = float(z["f_remCarrPhase"][k][e])
    engine.set_precision("double")
    try:
        got = engine.correlate(blocks).reshape(n_ep, nch, -1, 6)
        assert engine.last_kernel() == 6
    finally:
        engine.set_precision("single")
    file_type = 1 if layout == RS.GC_REAL else 2
    swap = layout == RS.GC_QI
    mult = list(spec.arm_mult) if spec.arm_mult else None
    want = np.zeros_like(got)
    want_c = np.zeros_like(got)
    for e in range(n_ep):
        for k in range(nch):
            b = blocks[e * nch + k]
            raw = O.raw_from_if(rec, int(b.first_sample), int(b.blksize), file_type=file_type, swap_iq=swap)
            arms = len(tables[k])
            s, _, _ = O.correlate_block(raw, [np.asarray(t, dtype=np.float64) for t in tables[k]], b.rem_code_phase, b.code_phase_step,
                                        b.el_spacing, b.carr_freq, b.rem_carr_phase, fs, length, r=float(spec.index_scale),
                                        arm_mult=mult, table_offset=[int(b.table_offset[a]) for a in range(arms)])
            want[e, k, :arms] = s
            same_len = len({len(t) for t in tables[k]}) == 1            # the C oracle takes one table length for all arms
            if rec.dtype == np.int8 and file_type == 2 and not swap and not mult and same_len and not any(b.table_offset[a] for a in range(arms)):
                sc_, _, _ = CO.correlate_block(rec, int(b.first_sample), int(b.blksize), tables[k], b.rem_code_phase, b.code_phase_step,
                                               b.el_spacing, b.carr_freq, b.rem_carr_phase, fs, length, r=float(spec.index_scale))
                want_c[e, k, :arms] = sc_
    scale = float(np.max(np.abs(want)))
    rel = float(np.max(np.abs(got - want))) / scale
    print(f"\n[f64] gc_correlate {name}: {rel:.1e} of max|want| against the Python float64 oracle")
    assert rel <= 1e-12, rel
    if np.any(want_c):
        m = np.any(want_c != 0, axis=(2, 3))
        assert float(np.max(np.abs(got[m] - want_c[m]))) / scale <= 1e-12


def test_f64_windowed_record_equals_the_resident_one(engine, tmp_path):
    import cu_sdr_collection_amd as P
    sc = next(s for s in RS.TRACK_SCENES if s.name == "GPS_L1CA")
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    path = str(tmp_path / "record.bin")
    rec.tofile(path)
    window = int(S.samplingFreq * S.intTime * 14.5)
    assert window < rec.size // 2 / 3                                   # several windows
    tw, _ = P.receiver.tracking_file(engine, path, ch, S, window, signal=sc.signal, precision="double")
    assert _prec(engine) == 0
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    tr, _ = P.tracking(engine, ch, S, signal=sc.signal, precision="double")
    for a, b in zip(tw, tr):
        assert a.status == b.status
        for f in vars(a):
            if isinstance(getattr(a, f), np.ndarray):
                assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f


@pytest.mark.parametrize("device_loop", [False, True], ids=["host_loop", "device_loop"])
def test_f64_concurrent_jobs_equal_their_single_calls(engine, device_loop):
    import cu_sdr_collection_amd as P
    from test_gpu_mix import _l1_band_scene
    iq, (S1, ch1), (S2, ch2), _ = _l1_band_scene()
    engine.load_if(iq, fs=18e6)
    with P.Engine(0) as e2:
        e2.share_if(engine)
        (tr1, _), (tr2, _) = P.receiver.tracking_multi([(engine, ch1, S1, "GPS_L1CA"), (e2, ch2, S2, "GAL_E1C")],
                                                       device_loop=device_loop, precision="double")
        assert _prec(engine) == 0 and _prec(e2) == 0
        seq1, _ = P.tracking(engine, ch1, S1, device_loop=device_loop, precision="double")
        seq2, _ = P.tracking(e2, ch2, S2, signal="GAL_E1C", device_loop=device_loop, precision="double")
    for a, b in ((tr1, seq1), (tr2, seq2)):
        for x, y in zip(a, b):
            assert x.status == y.status and x.PRN == y.PRN
            for f in vars(x):
                if isinstance(getattr(x, f), np.ndarray):
                    assert np.array_equal(getattr(x, f), getattr(y, f), equal_nan=True), f


def _l1ca_params(engine, S, ch):
    """gc_track's arguments for a GPS L1 C/A scene, as receiver.tracking prepares them (the channels set on `engine`)."""
    from cu_sdr_collection_amd import receiver
    job = receiver._tracking_prepare(engine, ch, S, "GPS_L1CA", None)
    return job.p, list(job.inits)


def test_f64_setting_defaults_and_refusals(engine):
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import _lib as L
    sc = next(s for s in RS.TRACK_SCENES if s.name == "GPS_L1CA")
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    with P.Engine(0) as fresh:
        assert _prec(fresh) == 0 and fresh.precision == "single"
        assert fresh._lib.gc_set_precision(fresh._ctx, 2) == L.GC_E_INVALID
        assert fresh._lib.gc_set_precision(fresh._ctx, -1) == L.GC_E_INVALID
        assert _prec(fresh) == 0
        fresh.load_if(rec, layout=layout, fs=S.samplingFreq)
        base, _ = P.tracking(fresh, ch, S, signal=sc.signal)
        fresh.set_precision("double")
        assert fresh.precision == "double"
        blocks = fresh.make_blocks(1)
        blocks[0].blksize, blocks[0].code_phase_step, blocks[0].el_spacing = 1000, 0.0568, 0.5
        assert fresh._lib.gc_replay_prepare(fresh._ctx, 1, blocks) == L.GC_E_UNSUPPORTED   # replay is float32 only
        dbl, _ = P.tracking(fresh, ch, S, signal=sc.signal)                                  # the context's setting
        fresh.set_precision("single")
        again, _ = P.tracking(fresh, ch, S, signal=sc.signal)
    for a, b, c in zip(base, again, dbl):
        for f in vars(a):
            if isinstance(getattr(a, f), np.ndarray):
                assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert any(not np.array_equal(a.I_P, c.I_P) for a, c in zip(base, dbl))                # the setting did reach the kernels
    # the keyword leaves the shared engine as it found it, also when the library call fails
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    P.tracking(engine, ch, S, signal=sc.signal, precision="double", device_loop=True)
    assert _prec(engine) == 0
    params, inits = _l1ca_params(engine, S, ch)
    inits[0].channel = 300                                        # no such channel: GC_E_INVALID / GC_E_STATE from the library
    with pytest.raises(L.GnssCorrError):
        engine.track(params, inits, precision="double")
    assert _prec(engine) == 0


_WRAPPER_DIR = {"GPS_L1CA": "GPS_L1CA", "GPS_L5C": "GPS_L5C"}


@pytest.fixture(scope="module")
def gateway():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexstub"))
    import harness
    g = harness.Gateway()
    plain = g.call
    g.calls = []

    def recorded(cmd, *args, nargout=1):   # the drop-in's gateway commands, in order
        g.calls.append((cmd, args))
        return plain(cmd, *args, nargout=nargout)

    g.call = recorded
    yield g
    g.lib.stub_run_atexit()


@pytest.mark.parametrize("device_loop", [0.0, 1.0], ids=["host_loop", "device_loop"])
@pytest.mark.parametrize("name", ["GPS_L1CA", "GPS_L5C"])
def test_f64_matlab_drop_in_returns_the_references_track_results(gateway, name, device_loop, tmp_path):
    """settings.gnsscorrPrecision = 'double' in the MATLAB drop-in (matlab/gnsscorr_tracking.m -> gnsscorr_mex('set_precision'))."""
    import bridge
    import cu_sdr_collection_amd as P
    from oracle import mlab
    sc = next(s for s in RS.TRACK_SCENES if s.name == name)
    z = np.load(os.path.join(GOLD, f"ref_track_{sc.name}.npz"))
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    S.gnsscorrPrecision = "double"
    S.gnsscorrDeviceLoop = device_loop
    path = str(tmp_path / "record.bin")
    rec.tofile(path)
    I = bridge.install(bridge.interpreter_for(_WRAPPER_DIR[sc.signal]), gateway, P, sc.signal)
    fid = mlab.register_file(I, rec.tobytes(), path)
    mch = mlab.to_matlab([SimpleNamespace(**{k: (v if isinstance(v, str) else float(v)) for k, v in vars(c).items()}) for c in ch])
    n0 = len(gateway.calls)
    try:
        tr, _ = I.call(sc.fn, fid, mch, mlab.to_matlab(S), nargout=2)
    finally:
        I.call("gnsscorr_context", "", "clear")
    tr = mlab.from_matlab(tr)
    calls = [c for c, _ in gateway.calls[n0:]]
    assert "set_precision" in calls and ("track_device" in calls) == bool(device_loop)
    for k in range(2):
        assert tr[k].status == str(z["status"][k])
        for f in ("absoluteSample",) + _SUMS + ("carrFreq", "codeFreq", "remCodePhase", "dllDiscr", "pllDiscr"):
            want = z["f_" + f][k]
            have = np.asarray(getattr(tr[k], f), dtype=np.float64).reshape(-1)
            if f == "absoluteSample":
                assert np.array_equal(have, want), f
            else:
                assert float(np.max(np.abs(have - want))) <= 1e-10 * float(np.max(np.abs(want))), f
