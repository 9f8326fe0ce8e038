"""gc_correlate_bank (csrc/corr_bank.hip): a block's correlation function at many code offsets, against a float64 restatement
of its definition (include/gnsscorr.h) written with the oracle's colon() (tests/bank_cases.py).

Tolerance: 2e-6 of sum |x| over the block, the project's correlator-versus-oracle figure (TOL_ORACLE of
tests/test_gpu_full_size.py).  One mis-assigned sample of a 4 097-sample block is 2.4e-4 in those units: the bound hides no
boundary error.  The kernel takes every table boundary from the float64 element rule itself, so ties are exact; what remains is
float32 mixing and float32 prefix sums restarted every 1 024 samples."""
import ctypes as C

import numpy as np
import pytest

from bank_cases import FS, PERIOD_L1, POOL, _blocks, _colon_has_n_elements, _raw, bank_reference, ca_table, noise_record  # noqa: F401  (fixtures)
from oracle import gnss_oracle as O

pytestmark = pytest.mark.gpu
TOL = 2e-6


def _check(engine, rec, descs, offsets, tables, r=1.0, arm_mult=None, layout="IQ", label=""):
    """One call for all of `descs`; every block, arm and tap against the restatement.  Returns (worst error / sum |x|, ties per block)."""
    got = engine.correlate_bank(_blocks(engine, descs), offsets)
    assert got.shape == (len(descs), 3, len(offsets))
    worst, ties = 0.0, []
    for k, d in enumerate(descs):
        raw = _raw(rec, d["s0"], d["n"], layout)
        ref, nt = bank_reference(raw, tables, d["rem"], d["step"], offsets, d["f"], d["phi"], FS, r, arm_mult)
        ties.append(nt)
        scale = float(np.sum(np.abs(raw.real) + np.abs(raw.imag)))
        dev = got[k, :len(tables)] - ref
        err = max(np.abs(dev.real).max(), np.abs(dev.imag).max()) / scale
        worst = max(worst, err)
        assert err < TOL, (label, k, d, err)
        assert not got[k, len(tables):].any(), (label, k)
    print(f"{label}: worst {worst:.3e} of sum |x| (bound {TOL:.1e})")
    return worst, ties


@pytest.mark.parametrize("ntaps", [1, 2, 3, 33, 64])
def test_shapes_around_every_seam(engine, noise_record, ca_table, ntaps):
    """Block sizes around the wavefront (64), the chunk (1 024) and several chunks, at three head alignments; offsets from zero to
    just under a period, negative phases included, in no particular order and with duplicates."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, [ca_table])
    rng = np.random.default_rng(100 + ntaps)
    if ntaps <= 3:
        sets = [POOL[s:s + ntaps] for s in range(0, len(POOL) - ntaps + 1, ntaps)] + [POOL[-ntaps:]]
    else:
        fill = list(rng.uniform(-2.0, 2.0, size=ntaps - len(POOL) - 2)) + [0.5, 0.5]     # duplicates allowed
        sets = [[float(x) for x in rng.permutation(np.array(POOL + fill))]]
    descs = []
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 4097):
        for s0 in (0, 1, 7):
            while True:
                step = (1.023e6 + rng.uniform(-5, 5)) / FS
                d = dict(n=n, s0=s0, rem=float(rng.uniform(-0.9, 1.0)), step=step, f=20e3 + float(rng.uniform(-5e3, 5e3)),
                         phi=float(rng.uniform(-2 * np.pi, 2 * np.pi)))
                if all(_colon_has_n_elements(d, o) for offsets in sets for o in offsets):
                    break
            descs.append(d)
    for offsets in sets:
        assert len(offsets) == ntaps
        _check(engine, noise_record, descs, offsets, [ca_table], label=f"{ntaps} taps {offsets[:3]}")


def test_tie_dense_ramps(engine, noise_record, ca_table):
    """Ramps whose samples sit exactly on table edges: rem = 0 with the nominal L1 C/A step (samples 0 and 3000), rem = 0.1 with
    step 0.2 (tests/test_gpu_correlator.py: the reference's two roundings decide there), integer and half-integer offsets; and a
    negative remainder.  The restatement must itself see samples with an integer t_i in the first two, or the case proves nothing."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, [ca_table])
    offsets = [-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 0.1, -0.1, 0.3, -0.3, 0.4]
    descs = [dict(n=4097, s0=5, rem=0.0, step=1.023e6 / 18e6, f=2.2e4, phi=0.4),
             dict(n=4097, s0=11, rem=0.1, step=0.2, f=2.2e4, phi=0.4),
             dict(n=1000, s0=777, rem=0.1, step=0.2, f=-1.3e4, phi=-1.0),
             dict(n=4097, s0=3, rem=-0.37, step=0.2, f=2.2e4, phi=0.4),
             dict(n=2049, s0=1, rem=-0.37, step=1.023e6 / 18e6, f=2.2e4, phi=0.4)]
    _, ties = _check(engine, noise_record, descs, offsets, [ca_table], label="tie-dense")
    assert ties[0] >= 2 and ties[1] > 100 and ties[2] > 100, ties


def test_channel_kinds(engine, noise_record):
    """Two arms at R = 2 (Galileo E1 B + C), two arms at 10.23 Mcps (GPS L5 I + Q), three arms with ramp multipliers (1, 1, 6)
    (BDS B1C wide-band, 0.68 table entries per sample on the BOC(6,1) arm)."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import codes
    engine.load_if(noise_record, fs=FS)
    offsets = [float(x) for x in np.linspace(-2.0, 2.0, 33)]
    kinds = [("E1", [codes.padded_table(codes.generateE1Bcode(11)), codes.padded_table(codes.generateE1Ccode(11))], 2.0, None, 1.023e6),
             ("L5", [codes.padded_table(codes.generateL5Icode(3)), codes.padded_table(codes.generateL5Qcode(3))], 1.0, None, 10.23e6),
             ("B1C", [codes.padded_table(codes.generateDataBOC11(19)), codes.padded_table(codes.generatePilotBOC11(19)),
                      codes.padded_table(codes.generatePilotBOC61(19))], 2.0, [1.0, 1.0, 6.0], 1.023e6)]
    for ch, (name, tables, r, mult, rate) in enumerate(kinds):
        tables = [np.asarray(t, dtype=np.int8) for t in tables]
        engine.set_channel(ch, tables, index_scale=r, arm_mult=mult)
        descs = [dict(channel=ch, n=4097, s0=9, rem=0.31, step=(rate + 3.0) / FS, f=-3.1e4, phi=2.0),
                 dict(channel=ch, n=4097, s0=50001, rem=0.0, step=rate / FS, f=1.7e4, phi=-0.3)]
        _check(engine, noise_record, descs, offsets, tables, r=r, arm_mult=mult, label=name)


@pytest.mark.parametrize("fmt", ["i8_qi", "i8_real", "i16_iq", "i16_qi", "i16_real"])
def test_record_formats(engine, noise_record, ca_table, fmt):
    import cu_sdr_collection_amd as P
    dt, lay = fmt.split("_")
    rec = noise_record[:2 * 20000] if dt == "i8" else (noise_record[:2 * 20000].astype(np.int16) * 37 + 5)   # the high byte matters
    layout = {"iq": P._lib.GC_IQ, "qi": P._lib.GC_QI, "real": P._lib.GC_REAL}[lay]
    engine.load_if(rec, layout=layout, fs=FS)
    engine.set_channel(0, [ca_table])
    descs = [dict(n=2049, s0=7, rem=0.25, step=(1.023e6 - 2.0) / FS, f=2.5e4, phi=1.1)]
    _check(engine, rec, descs, POOL[:9], [ca_table], layout=lay.upper(), label=fmt)


@pytest.mark.parametrize("d", [0.5, 0.1])
def test_taps_at_the_early_prompt_and_late_offsets_agree_with_gc_correlate(engine, l1ca_scene, d):
    """Two float32 paths, each held to 2e-6 of the oracle: 4e-6 of sum |x| between them."""
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    for i, s in enumerate(sats):
        engine.set_channel(i, [O.pad_code(O.generate_ca_code(s.prn)).astype(np.int8)])
    rng = np.random.default_rng(5)
    descs = []
    for k in range(24):
        step = (1.023e6 + rng.uniform(-5, 5)) / FS
        rem = float(rng.uniform(0, step))
        n = int(np.ceil((1023.0 - rem) / step))
        descs.append(dict(channel=k % len(sats), n=n, s0=int(rng.integers(0, iq.shape[0] // 2 - n)), rem=rem, step=step, d=d,
                          f=20e3 + float(rng.uniform(-5e3, 5e3)), phi=float(rng.uniform(-3, 3))))
    b = _blocks(engine, descs)
    epl = engine.correlate(b)[:, 0]                       # I_E Q_E I_P Q_P I_L Q_L
    bank = engine.correlate_bank(b, [-d, 0.0, d])[:, 0]
    for k, dsc in enumerate(descs):
        scale = float(np.sum(np.abs(iq[2 * dsc["s0"]:2 * (dsc["s0"] + dsc["n"])].astype(np.float64))))
        want = epl[k, 0::2] + 1j * epl[k, 1::2]
        dev = bank[k] - want
        err = max(np.abs(dev.real).max(), np.abs(dev.imag).max()) / scale
        assert err < 4e-6, (k, dsc, err)


def test_many_blocks_in_one_call_equal_the_blocks_one_by_one(engine, l1ca_scene):
    """12 channels x 8 epochs: a block's result does not depend on what else is in the call, nor on the run."""
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    for c in range(12):
        engine.set_channel(c, [O.pad_code(O.generate_ca_code(c + 1)).astype(np.int8)])
    rng = np.random.default_rng(8)
    descs = []
    for e in range(8):
        for c in range(12):
            step = (1.023e6 + rng.uniform(-5, 5)) / FS
            rem = float(rng.uniform(0, step))
            descs.append(dict(channel=c, n=int(np.ceil((1023.0 - rem) / step)), s0=18000 * e + int(rng.integers(0, 9000)), rem=rem, step=step,
                              f=20e3 + float(rng.uniform(-5e3, 5e3)), phi=float(rng.uniform(-3, 3))))
    offsets = [j / 4 for j in range(-8, 9)]
    all_at_once = engine.correlate_bank(_blocks(engine, descs), offsets)
    again = engine.correlate_bank(_blocks(engine, descs), offsets)
    assert all_at_once.tobytes() == again.tobytes()
    assert np.abs(all_at_once[:, 0]).min() > 0 and not all_at_once[:, 1:].any()
    for k, d in enumerate(descs):
        one = engine.correlate_bank(_blocks(engine, [d]), offsets)
        assert one[0].tobytes() == all_at_once[k].tobytes(), k


def test_correlation_function_of_a_tracked_channel_peaks_at_zero_offset(engine, l1ca_scene):
    """receiver.correlation_function on a 40-epoch tracking run: the epoch mean of |R(o)| is largest at o = 0 and falls with |o| over
    0, 1/4, 1/2, 3/4, 1 on both sides - the C/A triangle.  The restatement, on the same recorded state, must show that ordering too
    (the fixture scene has other satellites and noise in it) and agree with the library tap by tap."""
    import cu_sdr_collection_amd as P
    from types import SimpleNamespace
    S, sats, iq = l1ca_scene
    ms, nch = S.msToProcess, S.numberOfChannels
    try:
        S.msToProcess, S.numberOfChannels = 40, 2
        ch = [SimpleNamespace(PRN=s.prn, acquiredFreq=S.IF + s.doppler + 4.0, codePhase=int(np.ceil(s.code_phase_samples)) + 1, status="T")
              for s in sats[:2]]
        engine.load_if(iq, fs=S.samplingFreq)
        tr, _ = P.tracking(engine, ch, S)
        offsets = [j / 4 for j in range(-6, 7)]
        got = P.correlation_function(engine, tr[0], ch[0], S, offsets)
        first = P.correlation_function(engine, tr[0], ch[0], S, offsets, epochs=[0, 39])
    finally:
        S.msToProcess, S.numberOfChannels = ms, nch
    assert got.shape == (40, 1, 13) and got.dtype == np.complex128
    assert first.tobytes() == got[[0, 39]].tobytes()
    tab = O.pad_code(O.generate_ca_code(sats[0].prn))
    ref = np.zeros((40, 13), dtype=np.complex128)
    for e in range(40):
        step = tr[0].codeFreq[e] / S.samplingFreq
        rem = tr[0].remCodePhase[e]
        n = int(np.ceil((S.codeLength - rem) / step))
        s0 = int(tr[0].absoluteSample[e])
        raw = _raw(iq, s0, n)
        r, _ = bank_reference(raw, [tab], rem, step, offsets, tr[0].carrFreq[e], tr[0].remCarrPhase[e], S.samplingFreq)
        ref[e] = r[0]
        dev = got[e, 0] - r[0]
        assert max(np.abs(dev.real).max(), np.abs(dev.imag).max()) < TOL * float(np.sum(np.abs(raw.real) + np.abs(raw.imag))), e
    for name, mean in (("restatement", np.abs(ref).mean(axis=0)), ("library", np.abs(got[:, 0]).mean(axis=0))):
        assert int(np.argmax(mean)) == 6, (name, mean)
        for side in (+1, -1):
            walk = [mean[6 + side * j] for j in range(5)]          # |o| = 0, 1/4, 1/2, 3/4, 1
            assert all(walk[j] > walk[j + 1] for j in range(4)), (name, side, walk)


def test_correlation_function_leaves_out_the_epochs_a_channel_never_reached(engine, l1ca_scene):
    """A channel that stopped early (the short read of tracking.m:241-245) or was never tracked keeps codeFreq = remCodePhase = inf
    and absoluteSample = 0 in the epochs it did not reach (tracking.m:47-86): the default `epochs` takes the completed ones only."""
    import cu_sdr_collection_amd as P
    from types import SimpleNamespace
    S, sats, iq = l1ca_scene
    ms, nch = S.msToProcess, S.numberOfChannels
    try:
        S.msToProcess, S.numberOfChannels = 310, 1                     # the record holds 300 ms
        ch = [SimpleNamespace(PRN=sats[0].prn, acquiredFreq=S.IF + sats[0].doppler + 4.0, codePhase=int(np.ceil(sats[0].code_phase_samples)) + 1,
                              status="T")]
        engine.load_if(iq, fs=S.samplingFreq)
        tr, _ = P.tracking(engine, ch, S)
    finally:
        S.msToProcess, S.numberOfChannels = ms, nch
    n_done = int(np.sum(np.isfinite(tr[0].codeFreq)))
    assert 290 <= n_done < 310 and tr[0].status == "-" and np.isinf(tr[0].codeFreq[-1]) and tr[0].absoluteSample[-1] == 0
    offsets = [-0.5, 0.0, 0.5]
    got = P.correlation_function(engine, tr[0], ch[0], S, offsets)
    assert got.shape == (n_done, 1, 3)
    assert got.tobytes() == P.correlation_function(engine, tr[0], ch[0], S, offsets, epochs=np.arange(n_done)).tobytes()
    mean = np.abs(got[:, 0]).mean(axis=0)                            # the tracked peak, as in the test above: prompt over both half-chip taps
    assert mean[1] > mean[0] and mean[1] > mean[2], mean
    # hand-built: a channel that was never tracked, and one with an inf tail
    never = SimpleNamespace(PRN=sats[0].prn, absoluteSample=np.zeros(5), codeFreq=np.full(5, np.inf), remCodePhase=np.full(5, np.inf),
                            carrFreq=np.full(5, np.inf), remCarrPhase=np.full(5, np.inf))
    assert P.correlation_function(engine, never, ch[0], S, offsets).shape == (0, 1, 3)
    tail = SimpleNamespace(PRN=sats[0].prn, **{f: np.concatenate([getattr(tr[0], f)[:3], getattr(never, f)[:2]])
                                               for f in ("absoluteSample", "codeFreq", "remCodePhase", "carrFreq", "remCarrPhase")})
    assert P.correlation_function(engine, tail, ch[0], S, offsets).tobytes() == got[:3].tobytes()


def test_a_list_walked_in_sub_batches_equals_its_parts(engine, noise_record, ca_table):
    """The library walks a list in sub-batches whose per-chunk partial sums stay under 256 MB.  17 600 blocks of five chunks on a
    three-arm channel at 64 taps need 270 MB (3 072 bytes per chunk): two sub-batches.  The two halves of the list, each one
    sub-batch of its own, must give the same bits, and so must a block called alone."""
    engine.load_if(noise_record, fs=FS)
    tabs = [ca_table, O.pad_code(O.generate_ca_code(8)).astype(np.int8), O.pad_code(O.generate_ca_code(9)).astype(np.int8)]
    engine.set_channel(0, tabs)
    nb, n = 17600, 4097
    assert nb * 5 * 3 * 64 * 16 > 256 << 20 > (nb // 2) * 5 * 3 * 64 * 16
    rng = np.random.default_rng(64)
    rem, s0, f = rng.uniform(0, 1, nb), rng.integers(0, 60000 - n, nb), rng.uniform(-3e4, 3e4, nb)
    descs = [dict(n=n, s0=int(s0[k]), rem=float(rem[k]), step=1.023e6 / FS, f=float(f[k]), phi=0.3) for k in range(nb)]
    offsets = [float(x) for x in np.linspace(-3.0, 3.0, 64)]
    whole = engine.correlate_bank(_blocks(engine, descs), offsets)
    assert np.abs(whole).min() > 0
    for part in (slice(0, nb // 2), slice(nb // 2, nb)):
        assert engine.correlate_bank(_blocks(engine, descs[part]), offsets).tobytes() == whole[part].tobytes()
    for k in (0, nb // 2 - 1, nb // 2, 17475, 17476, nb - 1):                 # 17 476 blocks (87 381 chunks) fill the first sub-batch
        assert engine.correlate_bank(_blocks(engine, [descs[k]]), offsets)[0].tobytes() == whole[k].tobytes(), k
    _check(engine, noise_record, [descs[17475], descs[17476]], offsets, tabs, label="either side of the sub-batch seam")


def test_an_empty_list_is_no_error_even_before_a_record_is_loaded():
    import cu_sdr_collection_amd as P
    with P.Engine(0) as fresh:
        assert fresh.correlate_bank(fresh.make_blocks(0), [0.0, 0.5]).shape == (0, 3, 2)
        with pytest.raises(P.GnssCorrError) as e:
            fresh.correlate_bank(fresh.make_blocks(0), [float("nan")])
        assert e.value.status == P._lib.GC_E_INVALID


def test_correlation_function_refuses_gps_l2c_with_the_librarys_code(engine, l1ca_scene):
    """GPS L2C reads its CL code through a window (gc_set_code_window): the bank reads whole tables periodically and says so."""
    import cu_sdr_collection_amd as P
    from types import SimpleNamespace
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    S2 = SimpleNamespace(samplingFreq=S.samplingFreq, codeLength=10230, CLCodeLength=767250, pilotTRKflag=1)
    tr = SimpleNamespace(PRN=5, absoluteSample=np.array([1000.0]), codeFreq=np.array([511.5e3]), remCodePhase=np.array([0.0]),
                         carrFreq=np.array([2e4]), remCarrPhase=np.array([0.0]))
    with pytest.raises(P.GnssCorrError) as e:
        P.correlation_function(engine, tr, SimpleNamespace(PRN=5), S2, [0.0, 0.5], signal="GPS_L2C")
    assert e.value.status == P._lib.GC_E_UNSUPPORTED


def test_refusals_leave_the_output_untouched(engine, noise_record, ca_table):
    import cu_sdr_collection_amd as P
    L = P._lib
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, [ca_table])
    engine.set_channel(5, [ca_table], windows=[512])
    broken = ca_table.copy()
    broken[0] = -broken[0]                                   # [c(end) c c(1)] with a wrong first pad
    engine.set_channel(6, [broken])
    good = dict(channel=0, n=2049, s0=3, rem=0.2, step=1.023e6 / FS, f=2e4, phi=0.1)

    def call(desc, offsets, ntaps=None):
        off = np.asarray(offsets, dtype=np.float64)
        out = np.full((1, 3, max(len(off), 1), 2), 12345.0)
        rc = engine._lib.gc_correlate_bank(engine._ctx, 1, _blocks(engine, [desc]), len(off) if ntaps is None else ntaps,
                                           off.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
        assert np.all(out == 12345.0), "a refused call must not write its output"
        return rc

    assert call(good, [0.0], ntaps=0) == L.GC_E_INVALID
    assert call(good, np.zeros(65)) == L.GC_E_INVALID
    assert call(good, [0.0, float("nan")]) == L.GC_E_INVALID
    assert call(good, [0.0, float("inf")]) == L.GC_E_INVALID
    assert call(good, [0.0, PERIOD_L1]) == L.GC_E_INVALID                       # a full period
    assert call(good, [0.0, -PERIOD_L1]) == L.GC_E_INVALID
    assert call(dict(good, channel=5), [0.0]) == L.GC_E_UNSUPPORTED             # windowed channel
    assert call(dict(good, channel=6), [0.0]) == L.GC_E_INVALID                 # broken pads
    assert call(dict(good, step=1.5), [0.0]) == L.GC_E_UNSUPPORTED              # more than one table entry per sample
    assert call(dict(good, s0=60000 - 2048), [0.0]) == L.GC_E_RANGE             # one sample past the record
    assert call(dict(good, channel=200), [0.0]) == L.GC_E_STATE
    engine.set_precision("double")
    try:
        assert call(good, [0.0]) == L.GC_E_UNSUPPORTED
    finally:
        engine.set_precision("single")
    ok = engine.correlate_bank(_blocks(engine, [good]), [0.0, 1022.9])
    assert ok.shape == (1, 3, 2) and np.abs(ok[0, 0]).min() > 0
    assert engine.correlate_bank(engine.make_blocks(0), [0.0]).shape == (0, 3, 1)
