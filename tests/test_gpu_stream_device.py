"""Windowed records with the loop closed on the GPU: gc_track_file_device (two alternating device windows, ONE persistent launch
per window, the kernels' teams pausing channel by channel where the window ends) and gc_track_device_resume (a channel's loop
state handed to the persistent kernels) against gc_track_device on the fully resident record.

Every comparison is against the SAME loop mode on the resident record: window origins are multiples of 256 samples, the kernel
and its teams are chosen from the channels' nominal blocks, and a window's first block is cut from the carried state by the
statements the kernels end every epoch with - so windows must not change a single bit (np.array_equal on every field, on
epochs_done and on the return status).  Across loop modes (a state written by the host-closed loop continued on the device and
the reverse) only the bookkeeping is compared: the float32 sums of the two modes are added in different orders."""
import copy
import dataclasses
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ref_scenes as RS

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _channels(S, sats, nch):
    ch = [SimpleNamespace(PRN=s.prn, acquiredFreq=S.IF + s.doppler + 4.0, codePhase=int(np.ceil(s.code_phase_samples)) + 1, status="T")
          for s in sats]
    while len(ch) < nch:
        ch.append(SimpleNamespace(PRN=0, acquiredFreq=0.0, codePhase=0, status="-"))
    return ch


def _job(engine, S, ch, signal="GPS_L1CA"):
    from cu_sdr_collection_amd import receiver
    return receiver._tracking_prepare(engine, ch, S, signal)


def _same(a, b):
    fa, da, sa = a[:3]
    fb, db, sb = b[:3]
    assert sa == sb and np.array_equal(da, db), (sa, sb, da, db)
    assert set(fa) == set(fb)
    for name in fa:
        if name.startswith("CNo"):       # in-loop estimator (resident) | filled from the records (windows): the receiver test compares them
            continue
        assert np.array_equal(fa[name], fb[name]), (name, float(np.max(np.abs(fa[name] - fb[name]))))


def _windows(p, window_samples, total):
    """The windows gc_track_file cuts (csrc/stream.hip): [(first, last + 1), ...] in record samples."""
    block = p.code_length / p.code_freq_basis * p.sampling_freq
    margin = (int(3.0 * block * 1.01) + 255 + 256) // 256 * 256
    W = window_samples // 256 * 256
    assert 4 * margin <= W < total, (margin, W, total)
    stride = W - margin
    out, k = [], 0
    while True:
        out.append((k * stride, min(k * stride + W, total)))
        if k * stride + W >= total:
            return out
        k += 1


def _blocks(f, p):
    """Block length of every recorded epoch (tracking.m:219-222) from the records themselves."""
    return np.ceil((p.code_length - f["remCodePhase"]) / (f["codeFreq"] / p.sampling_freq))


def _window_changes(f, done, p, windows):
    """Window changes that fall inside the run: window k is left when a recorded block ends beyond it."""
    ends = [f["absoluteSample"][c, :done[c]] + _blocks(f, p)[c, :done[c]] for c in range(len(done)) if done[c]]
    last_end = max(float(e.max()) for e in ends)
    return sum(1 for (_, hi) in windows[:-1] if last_end > hi)


def _every_epoch_accounted_for(f, done, p):
    """absoluteSample advances by the recorded block length from every epoch to the next (window changes included)."""
    n = _blocks(f, p)
    for c in range(len(done)):
        d = int(done[c])
        if d > 1:
            a = f["absoluteSample"][c, :d]
            assert np.array_equal(a[1:] - a[:-1], n[c, :d - 1]), c


# 1 + 8 ---------------------------------------------------------------------------------------------------------------------
def test_windowed_file_device_loop_equals_the_resident_device_loop(engine, l1ca_scene, tmp_path):
    """GPS L1 C/A teams of the transition-mask kernel: 4 channels x 280 epochs in 12 and in 5 windows."""
    S, sats, iq = l1ca_scene                    # 0.3 s at 18 Msps
    S = copy.copy(S)
    S.msToProcess, S.numberOfChannels = 280, 4
    path = os.path.join(tmp_path, "record.bin")
    iq.tofile(path)
    job = _job(engine, S, _channels(S, sats, 4))
    engine.load_if(iq, fs=S.samplingFreq)
    resident = engine.track(job.p, job.inits, device_loop=True)
    assert resident[2] == 0 and all(resident[1] == 280) and engine.last_track_mode() == 2
    _every_epoch_accounted_for(resident[0], resident[1], job.p)
    for window_ms, nwin in ((25, 12), (64.3, 5)):
        window = int(window_ms * 1e-3 * S.samplingFreq)
        wins = _windows(job.p, window, iq.size // 2)
        assert len(wins) >= nwin
        windowed = engine.track_file(path, job.p, job.inits, window, device_loop=True)
        assert engine.last_track_mode() == 2
        _same(resident, windowed)
        _every_epoch_accounted_for(windowed[0], windowed[1], job.p)
        assert _window_changes(windowed[0], windowed[1], job.p, wins) >= nwin - 2
    engine.load_if(iq, fs=S.samplingFreq)       # the context is usable again after the windows are gone
    _same(resident, engine.track(job.p, job.inits, device_loop=True))


# 2 -------------------------------------------------------------------------------------------------------------------------
def test_windowed_int16_lane_kernel_record_device_loop(engine, tmp_path):
    """A 10.23-Mcps data + pilot signal (lane kernel, two arms) on an int16 record with a 512-byte header."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import _lib as L
    sc = next(s for s in RS.TRACK_SCENES if s.name == "GPS_L5C")
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    rec16 = (rec.astype(np.int16) * 5)
    path = os.path.join(tmp_path, "record16.bin")
    with open(path, "wb") as f:
        f.write(b"\0" * 512)                    # a header in front of record sample 0
        rec16.tofile(f)
    job = _job(engine, S, ch, sc.signal)
    engine.load_if(rec16, layout=layout, fs=S.samplingFreq)
    resident = engine.track(job.p, job.inits, device_loop=True)
    assert engine.last_track_mode() == 2 and resident[2] == 0
    n = rec16.size // 2
    windowed = engine.track_file(path, job.p, job.inits, n // 3, dtype=L.GC_I16, layout=layout, skip_bytes=512, device_loop=True)
    assert engine.last_track_mode() == 2
    _same(resident, windowed)
    assert _window_changes(windowed[0], windowed[1], job.p, _windows(job.p, n // 3, n)) >= 2


# 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ms", [("GPS_L2C", 500), ("BDS_B1C_WB", 250)])
def test_windowed_table_and_three_arm_fold_device_loop(engine, name, ms, tmp_path):
    """GPS L2C (the CL code's table_phase carried across windows, its table window restaged from the carried state) and BDS B1C
    wide-band (three arms, the third derived; fold 4).  The scenes' own records hold 6.2 blocks of 20 / 10 ms - shorter than ONE
    window may be (a window is at least four margins of three blocks) -, so the scene's builder makes the same signal longer
    (msToProcess = 25 epochs): the smallest window then leaves at least two window changes inside the run."""
    import cu_sdr_collection_amd as P
    base = next(s for s in RS.TRACK_SCENES if s.name == name)
    sc = dataclasses.replace(base, overrides=dict(base.overrides, msToProcess=ms))
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    path = os.path.join(tmp_path, "record.bin")
    rec.tofile(path)
    job = _job(engine, S, ch, sc.signal)
    assert job.p.n_epochs == 25
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    resident = engine.track(job.p, job.inits, device_loop=True)
    assert engine.last_track_mode() == 2 and resident[2] == 0 and all(resident[1][:2] == 25)
    total = rec.size // 2
    block = job.p.code_length / job.p.code_freq_basis * job.p.sampling_freq
    window = 4 * ((int(3.0 * block * 1.01) + 255 + 256) // 256 * 256) + 1024
    wins = _windows(job.p, window, total)
    windowed = engine.track_file(path, job.p, job.inits, window, layout=layout, device_loop=True)
    assert engine.last_track_mode() == 2
    _same(resident, windowed)
    # the run starts in the first window and its blocks end beyond the second one: two window changes at least
    assert windowed[0]["absoluteSample"][:2, 0].max() < wins[1][0]
    assert _window_changes(windowed[0], windowed[1], job.p, wins) >= 2
    _every_epoch_accounted_for(windowed[0], windowed[1], job.p)


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_windowed_file_device_loop_ends_like_the_resident_record(engine, l1ca_scene, tmp_path):
    """More epochs asked for than the file holds (tracking.m:241-245): GC_E_RANGE, the first channel's records stop at the same
    epoch, the channels after it are zero - windowed and resident alike."""
    from cu_sdr_collection_amd import _lib as L
    S, sats, iq = l1ca_scene
    S = copy.copy(S)
    S.msToProcess, S.numberOfChannels = 400, 3
    path = os.path.join(tmp_path, "record.bin")
    iq.tofile(path)
    job = _job(engine, S, _channels(S, sats, 3))
    engine.load_if(iq, fs=S.samplingFreq)
    resident = engine.track(job.p, job.inits, device_loop=True)
    assert resident[2] == L.GC_E_RANGE and 290 < resident[1][0] < 300 and not resident[1][1:].any()
    windowed = engine.track_file(path, job.p, job.inits, int(0.05 * S.samplingFreq), device_loop=True)
    assert windowed[2] == L.GC_E_RANGE and engine.last_track_mode() == 2
    _same(resident, windowed)
    assert not windowed[0]["I_P"][1:].any()


# 5 -------------------------------------------------------------------------------------------------------------------------
def test_device_resume_continues_a_device_closed_call(engine, l1ca_scene):
    """gc_track_device_resume: 130 epochs, then 150 more from the returned state = one device-closed call of 280 epochs; and the
    state is the one both loop modes understand."""
    S, sats, iq = l1ca_scene
    S = copy.copy(S)
    S.msToProcess, S.numberOfChannels = 280, 4
    job = _job(engine, S, _channels(S, sats, 4))
    engine.load_if(iq, fs=S.samplingFreq)
    pn = copy.copy(job.p)
    pn.cno_interval = 0                         # (a resumed call leaves the in-loop C/N0 to its caller)
    whole = engine.track(pn, job.inits, device_loop=True)
    assert whole[2] == 0 and engine.last_track_mode() == 2
    p1, p2 = copy.copy(pn), copy.copy(pn)
    p1.n_epochs, p2.n_epochs = 130, 150
    f1, d1, s1, state, paused = engine.track_resume(p1, job.inits, device_loop=True)
    assert s1 == 0 and not paused and all(d1 == 130) and engine.last_track_mode() == 2
    assert all(st.status == 0 for st in state)
    f2, d2, s2, state, paused = engine.track_resume(p2, job.inits, state=state, device_loop=True)
    assert s2 == 0 and not paused and all(d2 == 150)
    for name in f1:
        assert np.array_equal(np.concatenate([f1[name], f2[name]], axis=1), whole[0][name]), name
    assert [int(st.next_sample) for st in state] == [int(whole[0]["absoluteSample"][k, -1]) + int(np.ceil(
        (S.codeLength - whole[0]["remCodePhase"][k, -1]) / (whole[0]["codeFreq"][k, -1] / S.samplingFreq))) for k in range(4)]

    # a state written by the host-closed loop continues on the device, and the reverse: status 0, the epochs asked for, and
    # absoluteSample going on without a gap (no bit equality across loop modes: their float32 sums are added in other orders)
    for first_device in (False, True):
        fa, da, sa, st, _ = engine.track_resume(p1, job.inits, device_loop=first_device)
        assert sa == 0 and all(da == 130) and all(x.status == 0 for x in st)
        nxt = [int(x.next_sample) for x in st]
        fb, db, sb, st, paused = engine.track_resume(p2, job.inits, state=st, device_loop=not first_device)
        assert sb == 0 and not paused and all(db == 150) and all(x.status == 0 for x in st)
        assert first_device or engine.last_track_mode() == 2
        assert [int(v) for v in fb["absoluteSample"][:, 0]] == nxt
        both = {k: np.concatenate([fa[k], fb[k]], axis=1) for k in ("absoluteSample", "remCodePhase", "codeFreq")}
        _every_epoch_accounted_for(both, da + db, pn)


def test_device_resume_pauses_each_channel_at_its_own_epoch(engine, l1ca_scene):
    """GC_TRACK_PAUSE_AT_END on a buffer that holds only the record's first 100.3 ms: every channel stops where ITS next block
    does not fit (status 0, paused), and goes on from that state on the rest of the record, bit for bit."""
    S, sats, iq = l1ca_scene
    S = copy.copy(S)
    S.msToProcess, S.numberOfChannels = 280, 4
    job = _job(engine, S, _channels(S, sats, 4))
    pn = copy.copy(job.p)
    pn.cno_interval = 0
    engine.load_if(iq, fs=S.samplingFreq)
    whole = engine.track(pn, job.inits, device_loop=True)
    cut = int(0.1003 * S.samplingFreq)
    engine.load_if(iq[:2 * cut], fs=S.samplingFreq)
    f1, d1, s1, state, paused = engine.track_resume(pn, job.inits, pause_at_end=True, device_loop=True)
    assert s1 == 0 and paused and all(st.status == 0 for st in state) and all((d1 >= 99) & (d1 <= 100))
    for c in range(4):
        nxt = int(state[c].next_sample)
        assert nxt == int(whole[0]["absoluteSample"][c, d1[c]]) and nxt <= cut                 # the block that did not fit
        assert nxt + _blocks(whole[0], pn)[c, d1[c]] > cut
    origin = (min(int(st.next_sample) for st in state) - 1000) // 256 * 256
    engine.load_if(iq[2 * origin:], fs=S.samplingFreq)
    rest = 280 - int(d1.min())
    p2 = copy.copy(pn)
    p2.n_epochs = rest
    f2, d2, s2, state, paused = engine.track_resume(p2, job.inits, state=state, origin=origin, device_loop=True)
    assert s2 == 0 and not paused and all(d2 == rest)
    for c in range(4):
        for name in f1:
            got = np.concatenate([f1[name][c, :d1[c]], f2[name][c, :280 - d1[c]]])
            assert np.array_equal(got, whole[0][name][c]), (c, name)


# 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["GPS_L1CA", "GAL_E1C"])
def test_f64_windowed_device_loop_equals_the_resident_one(engine, name, tmp_path):
    import cu_sdr_collection_amd as P
    sc = next(s for s in RS.TRACK_SCENES if s.name == name)
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    path = str(tmp_path / "record.bin")
    rec.tofile(path)
    job = _job(engine, S, ch, sc.signal)
    total = rec.size // 2
    block = job.p.code_length / job.p.code_freq_basis * job.p.sampling_freq
    window = max(int(block * 14.5), 4 * ((int(3.0 * block * 1.01) + 255 + 256) // 256 * 256) + 512)
    wins = _windows(job.p, window, total)
    tw, _ = P.receiver.tracking_file(engine, path, ch, S, window, signal=sc.signal, precision="double", device_loop=True)
    assert engine.last_track_mode() == 2
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    tr, _ = P.tracking(engine, ch, S, signal=sc.signal, device_loop=True, precision="double")
    assert engine.last_track_mode() == 2 and len(wins) >= 2
    for a, b in zip(tw, tr):
        assert a.status == b.status
        for f in vars(a):
            if isinstance(getattr(a, f), np.ndarray):
                assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f


def test_f64_long_record_in_windows_follows_the_references_tracking_m(engine, tmp_path):
    """GPS_L1CA_long (1 200 epochs of the reference's own tracking.m, tests/golden/ref_track_GPS_L1CA_long.npz) from a file in 9
    windows or more, float64, loop closed on the device: absoluteSample identical to the reference's, every other field within
    the bound tests/test_gpu_tracking_f64.py applies to the resident run of the long scenes (tol 1e-9 of max|want|, C/N0 1e-6 dB:
    test_f64_long_closed_loop_follows_the_references_tracking_m_epoch_for_epoch)."""
    import cu_sdr_collection_amd as P
    from test_gpu_tracking_f64 import _against_the_reference
    sc = next(s for s in RS.LONG_TRACK_SCENES if s.name == "GPS_L1CA_long")
    z = np.load(os.path.join(GOLD, f"ref_track_{sc.name}.npz"))
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    assert RS.crc(rec) == int(z["record_crc32"][0])
    path = str(tmp_path / "record.bin")
    rec.tofile(path)
    total = rec.size // 2
    window = total // 8
    job = _job(engine, S, ch, sc.signal)
    assert len(_windows(job.p, window, total)) >= 8
    tw, _ = P.receiver.tracking_file(engine, path, ch, S, window, signal=sc.signal, precision="double", device_loop=True)
    assert engine.last_track_mode() == 2
    for k, t in enumerate(tw):
        if str(z["status"][k]) == "T":
            assert np.array_equal(t.absoluteSample, z["f_absoluteSample"][k]), k
    worst = _against_the_reference(tw, z, ch, tol=1e-9, cno_tol=1e-6)
    print("\n[f64 windows, device loop] GPS_L1CA_long: " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))


# 7 -------------------------------------------------------------------------------------------------------------------------
# |CNo.VSMValue of the in-kernel estimator (devloop.h: one pass, sums of Z - Z0) - receiver.CNoVSM over the run's own I_P / Q_P|
# on the resident device-closed run of this scene, measured on an MI355X: see the test's docstring.
_CNO_DEVICE_ESTIMATOR_DEVIATION_DB = 3.6e-14   # measured: 3.553e-14 dB (five ulp of a 45-dB value)
_CNO_MARGIN_DB = 1e-12                         # thirty times that: another record's intervals may round a few ulp worse, a wrong
                                               # interval or a float32 estimator is off by 1e-7 dB or more


def test_receiver_tracking_file_device_loop_equals_tracking(engine, l1ca_scene, tmp_path):
    """tracking_file(..., device_loop=True) = tracking(..., device_loop=True): status, PRN, every array field, CNo.VSMIndex.
    CNo.VSMValue: the resident run's values come from the kernel's one-pass estimator, the windowed run's from the complete
    records on the host (gc_fill_cno_host, as gc_track_file) - both are compared with receiver.CNoVSM (Common/CNoVSM.m) over the
    run's own I_P / Q_P.  The device estimator's deviation from it on the resident run is measured first and printed; the
    windowed values must stay within that deviation plus _CNO_MARGIN_DB.
    Measured on an MI355X: resident run (in-kernel estimator) 3.553e-14 dB, windowed run (host fill) 2.132e-14 dB."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import receiver
    S, sats, iq = l1ca_scene
    S = copy.copy(S)
    S.msToProcess, S.numberOfChannels = 250, 5
    ch = _channels(S, sats, 5)
    path = os.path.join(tmp_path, "record.bin")
    iq.tofile(path)
    engine.load_if(iq, fs=S.samplingFreq)
    a, _ = P.tracking(engine, ch, S, device_loop=True)
    assert engine.last_track_mode() == 2
    b, _ = P.tracking_file(engine, path, ch, S, window_samples=int(0.04 * S.samplingFreq), device_loop=True)
    assert engine.last_track_mode() == 2
    K = int(S.CNo.VSMinterval)
    dev_res = dev_win = 0.0
    for x, y in zip(a, b):
        assert x.status == y.status and x.PRN == y.PRN
        for f in vars(x):
            if isinstance(getattr(x, f), np.ndarray):
                assert np.array_equal(getattr(x, f), getattr(y, f)), f
        assert x.CNo.VSMIndex == y.CNo.VSMIndex and len(x.CNo.VSMValue) == len(y.CNo.VSMValue)
        if x.status != "T":
            continue
        assert len(x.CNo.VSMValue) == 250 // K
        for i, loop in enumerate(x.CNo.VSMIndex):
            want = receiver.CNoVSM(x.I_P[loop - K:loop], x.Q_P[loop - K:loop], S.CNo.accTime)
            dev_res = max(dev_res, abs(x.CNo.VSMValue[i] - want))
            dev_win = max(dev_win, abs(y.CNo.VSMValue[i] - want))
    print(f"\n[C/N0] device estimator vs receiver.CNoVSM, resident run: {dev_res:.3e} dB; windowed run (host fill): {dev_win:.3e} dB")
    assert dev_res <= _CNO_DEVICE_ESTIMATOR_DEVIATION_DB + _CNO_MARGIN_DB
    assert dev_win <= _CNO_DEVICE_ESTIMATOR_DEVIATION_DB + _CNO_MARGIN_DB
