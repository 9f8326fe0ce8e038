"""gc_cancel (csrc/cancel.hip) on the GPU: the tracked components of a record rebuilt from their descriptors and subtracted.

1. Sample for sample against the float64 numpy model of the definition (tests/cancel_model.py): array_equal, except samples whose
   model value lies within 1e-9 of a half-integer (one ulp in sin or cos may turn those), at most 10 per 100 000 samples.
2. amp_out against the model's P / E: |dP| <= (N + 8) 2^-52 sum(|re| + |im|) - the order of additions and one ulp in each of sin
   and cos are all that may differ.  E itself does not leave the library; it is checked through A = P / E: an E off by one moves A
   by |A| / E, orders of magnitude more than the bound (the ternary channel has E < N).
3. The projection property: on the residual the prompt sum of the GC_PREC_F64 correlator is what the rounding to integers left,
   |P_res| <= 0.71 N + (N + 8) 2^-52 sum|x| (at most 0.5 per component along the replica), where the source has |A| N.
4. Independence: a block's bytes alone and inside a longer list; the amplitude of a second call on the MODEL output.
5. Refusals: every one leaves dst (a sentinel fill) and amp_out untouched.
6. End to end on the four-satellite scene through receiver.cancel_tracked."""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import cancel_model as M
from oracle import gnss_oracle as O

pytestmark = pytest.mark.gpu
FS = 18e6
NS = 40000
I8, I16 = np.int8, np.int16
REAL, IQ, QI = M.REAL, M.IQ, M.QI
FORMATS = {"i8_iq": (I8, IQ), "i8_qi": (I8, QI), "i8_real": (I8, REAL), "i16_iq": (I16, IQ), "i16_qi": (I16, QI), "i16_real": (I16, REAL)}
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4097]
MAX_LEFT_OUT = NS * 10 // 100000          # 10 per 100 000 samples


def _channels():
    """Engine slot -> channel: one arm R = 1 on the 1 025-entry padded C/A table; two arms R = 2; three arms with multipliers
    (1, 1, 6); one arm on a ternary table with zeros."""
    rng = np.random.default_rng(410)
    pm = lambda n: rng.choice([-1, 1], n).astype(np.int8)                      # noqa: E731
    return {3: {"tables": [O.pad_code(O.generate_ca_code(7)).astype(np.int8)], "r": 1.0, "mult": [1.0]},
            5: {"tables": [pm(2048), pm(2048)], "r": 2.0, "mult": [1.0, 1.0]},
            9: {"tables": [pm(1025), pm(1025), pm(6140)], "r": 1.0, "mult": [1.0, 1.0, 6.0]},
            12: {"tables": [rng.integers(-1, 2, 1025).astype(np.int8)], "r": 1.0, "mult": [1.0]}}


CHANS = _channels()


def _configure(eng):
    for slot, c in CHANS.items():
        eng.set_channel(slot, c["tables"], index_scale=c["r"], arm_mult=c["mult"])
    eng.set_sampling_freq(FS)


def _scene():
    """Per channel the nine block sizes in an order of its own at odd starts, some adjacent, some with gaps; the channels' spans
    overlap each other; channel 3 has a tenth block far behind the others (the mean-length guess misses there); the record's tail
    and the samples in front of the first block are covered by nothing.  Returns the blocks channel by channel."""
    rng = np.random.default_rng(411)
    per = {}
    for slot, start in ((3, 1), (5, 2501), (9, 5003), (12, 333)):
        s0, lst = start, []
        for j, n in enumerate(rng.permutation(SIZES)):
            lst.append({"ch": slot, "s0": int(s0), "n": int(n), "rem": float(rng.uniform(0.0, 0.9)),
                        "step": 1.023e6 / FS * (1.0 + float(rng.uniform(-3e-6, 3e-6))), "f": 20e3 + float(rng.uniform(-5e3, 5e3)),
                        "phi": float(rng.uniform(0.0, 2 * np.pi))})
            s0 += n + (0, 1, 7, 130, 0, 2, 64, 0, 33)[j]
        per[slot] = lst
    per[3].append({"ch": 3, "s0": 35001, "n": 4097, "rem": 0.25, "step": 1.023e6 / FS, "f": 21234.5, "phi": 1.0})
    return per


PER = _scene()


def _order(kind):
    if kind == "epoch_major":
        lst = [PER[s][j] for j in range(10) for s in (3, 5, 9, 12) if j < len(PER[s])]
    else:
        lst = [b for s in (12, 9, 5, 3) for b in PER[s]]
        lst = [lst[i] for i in np.random.default_rng(412).permutation(len(lst))]
    return lst


def _blocks(eng, descs):
    b = eng.make_blocks(len(descs))
    for k, d in enumerate(descs):
        b[k].channel, b[k].blksize, b[k].first_sample = d["ch"], d["n"], d["s0"]
        b[k].rem_code_phase, b[k].code_phase_step, b[k].el_spacing = d["rem"], d["step"], 0.37      # el_spacing is ignored
        b[k].carr_freq, b[k].rem_carr_phase = d["f"], d["phi"]
    return b


def _record(dtype, layout, seed=413):
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(info.min, info.max + 1, NS * (1 if layout == REAL else 2)).astype(dtype)


def _amps(descs, dtype, seed=414):
    rng = np.random.default_rng(seed)
    scale = 40.0 * (256.0 if dtype == I16 else 1.0)                            # large enough to clip now and then
    a = scale * (rng.uniform(-1, 1, (len(descs), 3)) + 1j * rng.uniform(-1, 1, (len(descs), 3)))
    for k, d in enumerate(descs):
        a[k, len(CHANS[d["ch"]]["tables"]):] = 0.0
    return a


@pytest.fixture(scope="module")
def dst_engine():
    import cu_sdr_collection_amd as P
    eng = P.Engine(0)
    yield eng
    eng.close()


def _per_sample(raw, layout):
    return raw.reshape(NS, 1 if layout == REAL else 2)


def _check_amp(tag, descs, got, used, P, E, sx):
    worst = 0.0
    for k, d in enumerate(descs):
        arms = len(CHANS[d["ch"]]["tables"])
        assert not got[k, arms:].any(), (tag, k)
        for a in range(arms):
            bound = (d["n"] + 8) * 2.0 ** -52 * sx[k]
            if E[k, a] == 0:
                assert got[k, a] == 0, (tag, k, a)
                continue
            dP = abs(got[k, a] - used[k, a]) * E[k, a]
            worst = max(worst, dP / bound if bound else 0.0)
            assert dP <= bound, (tag, k, a, dP, bound)
    print(f"CANCEL {tag}: worst |dP| / bound {worst:.3g}")


def _run(eng, dst, raw, dtype, layout, blocks, amp, mode, inplace):
    eng.load_if(raw, layout=layout, fs=FS)
    if inplace:
        used = eng.cancel(blocks, amp=amp, mode=mode)
        return eng.read_if(0, NS, dtype=dtype, layout=layout), used
    dst.load_if(np.full_like(raw, 85), layout=layout)
    used = eng.cancel(blocks, dst=dst, amp=amp, mode=mode)
    assert eng.read_if(0, NS, dtype=dtype, layout=layout).tobytes() == raw.tobytes()              # the source stays as it was
    return dst.read_if(0, NS, dtype=dtype, layout=layout), used


@pytest.mark.parametrize("order", ["epoch_major", "shuffled"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_sample_for_sample_against_the_model(engine, dst_engine, fmt, order):
    dtype, layout = FORMATS[fmt]
    _configure(engine)
    descs = _order(order)
    blocks = _blocks(engine, descs)
    raw = _record(dtype, layout)
    left_out = 0
    for amp in (None, _amps(descs, dtype)):
        for mode in ("subtract", "model"):
            want, used, P, E, sx, near, covered = M.cancel(raw, dtype, layout, descs, CHANS, FS, amp=amp, mode=mode)
            assert int(near.sum()) <= MAX_LEFT_OUT
            left_out = max(left_out, int(near.sum()))
            assert 0 < int(covered.sum()) < NS
            outs = []
            for inplace in (False, True):
                tag = f"{fmt} {order} amp={'given' if amp is not None else 'projected'} {mode} {'in place' if inplace else 'out of place'}"
                got, a_out = _run(engine, dst_engine, raw, dtype, layout, blocks, amp, mode, inplace)
                g, w, x = _per_sample(got, layout), _per_sample(want, layout), _per_sample(raw, layout)
                assert np.array_equal(g[~near], w[~near]), (tag, int(np.sum(np.any(g != w, axis=1) & ~near)))
                assert np.array_equal(g[~covered], x[~covered] if mode == "subtract" else np.zeros_like(x[~covered])), tag
                if amp is None:
                    _check_amp(tag, descs, a_out, used, P, E, sx)
                else:
                    assert np.array_equal(a_out, amp), tag
                outs.append(got.tobytes())
            assert outs[0] == outs[1]                                                              # in place: the same bytes
    print(f"CANCEL {fmt} {order}: at most {left_out} of {NS} samples within 1e-9 of a half-integer")


@pytest.mark.parametrize("fmt", ["i8_iq", "i16_real"])
def test_amplitudes_against_the_models_projection(engine, dst_engine, fmt):
    dtype, layout = FORMATS[fmt]
    _configure(engine)
    descs = _order("epoch_major")
    raw = _record(dtype, layout, seed=415)
    _, used, P, E, sx, _, _ = M.cancel(raw, dtype, layout, descs, CHANS, FS)
    assert any(0 < E[k, 0] < d["n"] for k, d in enumerate(descs) if d["ch"] == 12)                 # the ternary table: E below N
    _, a_out = _run(engine, dst_engine, raw, dtype, layout, _blocks(engine, descs), None, "subtract", False)
    _check_amp(fmt, descs, a_out, used, P, E, sx)
    again = _run(engine, dst_engine, raw, dtype, layout, _blocks(engine, descs), None, "model", True)[1]
    assert again.tobytes() == a_out.tobytes()                                                      # bitwise the same from run to run


@pytest.mark.parametrize("fmt", ["i8_iq", "i8_qi", "i16_iq", "i16_qi"])
def test_the_residual_has_no_component_along_the_replica(engine, dst_engine, fmt):
    dtype, layout = FORMATS[fmt]
    _configure(engine)
    rng = np.random.default_rng(416)
    descs = [{"ch": 3, "s0": 11, "n": 257, "rem": 0.4, "step": 1.023e6 / FS, "f": 19000.0, "phi": 0.3},
             {"ch": 3, "s0": 301, "n": 4097, "rem": 0.1, "step": 1.023e6 / FS * (1 + 2e-6), "f": 21500.0, "phi": 2.0},
             {"ch": 3, "s0": 5001, "n": 18001, "rem": 0.7, "step": 1.023e6 / FS * (1 - 2e-6), "f": 20100.0, "phi": 5.0}]
    planted = 20.0 * np.exp(0.7j)
    re, im = rng.integers(-60, 61, NS).astype(np.float64), rng.integers(-60, 61, NS).astype(np.float64)
    for d in descs:
        sn, cs, c = M.replica(d, CHANS[3], FS)
        z = planted * c[0] * (cs + 1j * sn)
        re[d["s0"]:d["s0"] + d["n"]] += z.real
        im[d["s0"]:d["s0"] + d["n"]] += z.imag
    raw = M.pack(np.rint(re), np.rint(im), dtype, layout)
    assert int(np.abs(raw.astype(np.int64)).max()) <= 100                                          # |x| <= 100: nothing clips
    blocks = _blocks(engine, descs)
    for k in range(len(descs)):
        blocks[k].el_spacing = 0.0
    sx = [M.project(*M.components(raw, layout), d, CHANS[3], FS)[2] for d in descs]
    engine.load_if(raw, layout=layout, fs=FS)
    dst_engine.load_if(np.zeros_like(raw), layout=layout, fs=FS)
    _configure(dst_engine)
    engine.cancel(blocks, dst=dst_engine)
    try:
        engine.set_precision("double")
        dst_engine.set_precision("double")
        p_src = engine.correlate(blocks)[:, 0, 2:4]
        p_res = dst_engine.correlate(blocks)[:, 0, 2:4]
    finally:
        engine.set_precision("single")
        dst_engine.set_precision("single")
    for k, d in enumerate(descs):
        bound = 0.71 * d["n"] + (d["n"] + 8) * 2.0 ** -52 * sx[k]
        src, res = float(np.hypot(*p_src[k])), float(np.hypot(*p_res[k]))
        print(f"CANCEL projection {fmt} N={d['n']}: |P_src| {src:.1f} (|A| N = {20.0 * d['n']:.0f}), |P_res| {res:.2f}, bound {bound:.1f}")
        assert res <= bound, (k, res, bound)
        assert src > 10.0 * bound, (k, src, bound)


def test_a_blocks_bytes_do_not_depend_on_the_rest_of_the_list(engine, dst_engine):
    dtype, layout = I8, IQ
    _configure(engine)
    raw = _record(dtype, layout, seed=417)
    target = next(d for d in PER[3] if d["n"] == 4097 and d["s0"] < 30000)
    lo, hi = target["s0"], target["s0"] + target["n"]
    others = [d for d in _order("shuffled") if d is not target and (d["s0"] + d["n"] <= lo or d["s0"] >= hi)]
    assert len(others) >= 12 and len({d["ch"] for d in others}) == 4
    alone, a_alone = _run(engine, dst_engine, raw, dtype, layout, _blocks(engine, [target]), None, "subtract", False)
    longer = others[:7] + [target] + others[7:]
    inside, a_inside = _run(engine, dst_engine, raw, dtype, layout, _blocks(engine, longer), None, "subtract", False)
    assert _per_sample(alone, layout)[lo:hi].tobytes() == _per_sample(inside, layout)[lo:hi].tobytes()
    assert a_alone[0].tobytes() == a_inside[7].tobytes()
    assert alone.tobytes() != raw.tobytes()


@pytest.mark.parametrize("fmt", ["i8_iq", "i16_qi"])
def test_a_second_call_on_the_model_gives_the_amplitude_back(engine, dst_engine, fmt):
    """dst holds rint(M): its projection is A plus the projection of the rounding, at most 0.5 per component along a +-1 replica,
    so within 0.71 LSB per component of the amplitude the first call used."""
    dtype, layout = FORMATS[fmt]
    _configure(engine)
    _configure(dst_engine)
    descs = [d for d in PER[3] if d["n"] >= 63]
    blocks = _blocks(engine, descs)
    amp = np.zeros((len(descs), 3), dtype=np.complex128)
    amp[:, 0] = 70.0 * np.exp(1j * np.random.default_rng(418).uniform(0, 2 * np.pi, len(descs)))   # |A| <= 100: nothing clips
    raw = _record(dtype, layout, seed=419)
    engine.load_if(raw, layout=layout, fs=FS)
    dst_engine.load_if(np.zeros_like(raw), layout=layout, fs=FS)
    first = engine.cancel(blocks, dst=dst_engine, amp=amp, mode="model")
    assert np.array_equal(first, amp)
    second = dst_engine.cancel(blocks, mode="model")
    dev = second[:, 0] - first[:, 0]
    print(f"CANCEL model again {fmt}: worst component deviation {max(np.abs(dev.real).max(), np.abs(dev.imag).max()):.3f} LSB (bound 0.71)")
    assert np.all(np.abs(dev.real) <= 0.71) and np.all(np.abs(dev.imag) <= 0.71)


def test_refusals_leave_the_destination_untouched(engine, dst_engine):
    from cu_sdr_collection_amd import _lib as L
    dtype, layout = I8, IQ
    _configure(engine)
    raw = _record(dtype, layout, seed=420)
    engine.load_if(raw, layout=layout, fs=FS)
    sentinel = np.full_like(raw, 85)
    dst_engine.load_if(sentinel, layout=layout)
    good = [PER[3][0], PER[5][0]]
    lib = L.load()
    dp = C.POINTER(C.c_double)

    def call(src, dst, n, blocks, amp, mode):
        a_out = np.full((max(n, 1), 3, 2), 7.5)
        a_in = None if amp is None else np.ascontiguousarray(amp, dtype=np.float64)
        rc = lib.gc_cancel(src, dst, n, blocks, None if a_in is None else a_in.ctypes.data_as(dp), a_out.ctypes.data_as(dp), mode)
        assert rc == L.GC_OK or np.all(a_out == 7.5), "amp_out written by a refused call"
        return rc

    def untouched(eng=dst_engine, fill=sentinel, dt=dtype, lay=layout):
        return eng.read_if(0, fill.shape[0] // (1 if lay == REAL else 2), dtype=dt, layout=lay).tobytes() == fill.tobytes()

    src, dst = engine._ctx, dst_engine._ctx
    overlap = [dict(PER[3][0], s0=101, n=64), dict(PER[5][0], s0=7, n=64), dict(PER[3][0], s0=164, n=64)]
    assert call(src, dst, 3, _blocks(engine, overlap), None, 0) == L.GC_E_INVALID and untouched()       # [101, 165) and [164, 228)
    assert call(src, dst, 2, _blocks(engine, good), None, 2) == L.GC_E_INVALID and untouched()           # a bad mode
    assert call(src, dst, 2, _blocks(engine, good), None, -1) == L.GC_E_INVALID and untouched()
    for bad in (np.nan, np.inf):
        amp = np.ones((2, 3, 2))
        amp[1, 0, 1] = bad
        assert call(src, dst, 2, _blocks(engine, good), amp, 0) == L.GC_E_INVALID and untouched()
    assert call(src, dst, 2, None, None, 0) == L.GC_E_INVALID and untouched()                            # null blocks
    assert call(None, dst, 2, _blocks(engine, good), None, 0) == L.GC_E_INVALID and untouched()
    assert call(src, None, 2, _blocks(engine, good), None, 0) == L.GC_E_INVALID
    assert call(src, dst, 1, _blocks(engine, [dict(PER[3][0], s0=NS - 10, n=64)]), None, 0) == L.GC_E_RANGE and untouched()
    assert call(src, dst, 1, _blocks(engine, [dict(PER[3][0], ch=200)]), None, 0) == L.GC_E_STATE and untouched()
    assert call(src, dst, 1, _blocks(engine, [dict(PER[3][0], step=0.0)]), None, 0) == L.GC_E_INVALID and untouched()
    # a destination of another sample count, dtype or layout
    for fill, dt, lay in ((np.full(2 * (NS - 1), 85, dtype=I8), I8, IQ), (np.full(2 * NS, 85, dtype=I16), I16, IQ),
                          (np.full(2 * NS, 85, dtype=I8), I8, QI), (np.full(NS, 85, dtype=I8), I8, REAL)):
        dst_engine.load_if(fill, layout=lay)
        assert call(src, dst, 2, _blocks(engine, good), None, 0) == L.GC_E_INVALID and untouched(fill=fill, dt=dt, lay=lay)
    assert engine.read_if(0, NS, dtype=dtype, layout=layout).tobytes() == raw.tobytes()
    # more than GC_CANCEL_MAX_CHANNELS channels in one call
    dst_engine.load_if(sentinel, layout=layout)
    many = []
    for k in range(L.GC_CANCEL_MAX_CHANNELS + 1):
        engine.set_channel(100 + k, CHANS[3]["tables"])
        many.append(dict(PER[3][0], ch=100 + k))
    assert call(src, dst, len(many), _blocks(engine, many), None, 0) == L.GC_E_INVALID and untouched()
    assert call(src, dst, len(many) - 1, _blocks(engine, many[:-1]), None, 0) == L.GC_OK and not untouched()


def test_an_empty_list_copies_or_clears(engine, dst_engine):
    dtype, layout = I16, REAL
    raw = _record(dtype, layout, seed=421)[:NS - 3]                                                # a record that ends inside 16 bytes
    engine.load_if(raw, layout=layout, fs=FS)
    for mode, want in (("subtract", raw), ("model", np.zeros_like(raw))):
        dst_engine.load_if(np.full_like(raw, 85), layout=layout)
        assert engine.cancel(engine.make_blocks(0), dst=dst_engine, mode=mode).shape == (0, 3)
        assert dst_engine.read_if(0, NS - 3, dtype=dtype, layout=layout).tobytes() == want.tobytes()


def test_end_to_end_on_the_four_satellite_scene(engine, dst_engine, l1ca_scene):
    """Track 250 epochs, cancel the first channel's PRN with receiver.cancel_tracked, look at the residual."""
    import cu_sdr_collection_amd as P
    S0, sats, iq = l1ca_scene
    S = copy.copy(S0)
    S.msToProcess, S.numberOfChannels = 250, 4
    ch = [SimpleNamespace(PRN=s.prn, acquiredFreq=S.IF + s.doppler + 4.0, codePhase=int(np.ceil(s.code_phase_samples)) + 1, status="T")
          for s in sats[:4]]
    engine.load_if(iq, fs=S.samplingFreq)
    tr, _ = P.tracking(engine, ch, S)
    assert all(t.status == "T" for t in tr)
    n = iq.shape[0] // 2
    dst_engine.load_if(np.zeros_like(iq), fs=S.samplingFreq)
    holder, amps = P.cancel_tracked(engine, tr, ch, S, which=[0], dst=dst_engine)
    assert holder is dst_engine and len(amps) == 1 and amps[0].shape == (250, 1)
    res = dst_engine.read_if(0, n)
    first = int(tr[0].absoluteSample[0])
    last = int(tr[0].absoluteSample[249])
    assert res[:2 * first].tobytes() == iq[:2 * first].tobytes() and res[2 * first:2 * last].tobytes() != iq[2 * first:2 * last].tobytes()
    # (3) on every cancelled block, through the bank on the residual
    p_res = P.correlation_function(dst_engine, tr[0], ch[0], S, [0.0])[:, 0, 0]
    p_src = P.correlation_function(engine, tr[0], ch[0], S, [0.0])[:, 0, 0]
    x = iq.astype(np.float64)
    ax = np.concatenate([[0.0], np.cumsum(np.abs(x[0::2]) + np.abs(x[1::2]))])
    worst = 0.0
    for e in range(250):
        step = tr[0].codeFreq[e] / S.samplingFreq
        nb = int(np.ceil((S.codeLength - tr[0].remCodePhase[e]) / step))
        s0 = int(tr[0].absoluteSample[e])
        bound = 0.71 * nb + (nb + 8) * 2.0 ** -52 * (ax[s0 + nb] - ax[s0])
        worst = max(worst, abs(p_res[e]) / bound)
        assert abs(p_res[e]) <= bound, (e, abs(p_res[e]), bound)
    print(f"CANCEL scene: worst |P_res| / bound {worst:.3g}; mean |P_src| {np.abs(p_src).mean():.0f}, mean |P_res| {np.abs(p_res).mean():.1f}")
    # acquisition from the first cancelled block: the other three stay, the cancelled one drops
    S.acqSatelliteList = [s.prn for s in sats[:4]]
    before = P.acquisition(engine, S, first_sample=first)
    after = P.acquisition(dst_engine, S, first_sample=first)
    for s in sats[1:4]:
        k = s.prn - 1
        assert before.carrFreq[k] != 0 and after.carrFreq[k] != 0, s.prn
        assert abs(after.codePhase[k] - before.codePhase[k]) <= 1, (s.prn, before.codePhase[k], after.codePhase[k])
    k = sats[0].prn - 1
    ratio = after.peakMetric[k] / before.peakMetric[k]
    print(f"CANCEL scene: PRN {sats[0].prn} peakMetric {before.peakMetric[k]:.2f} -> {after.peakMetric[k]:.2f} (ratio {ratio:.3f}); "
          f"others {[round(float(after.peakMetric[s.prn - 1] / before.peakMetric[s.prn - 1]), 3) for s in sats[1:4]]}")
    assert ratio < 0.5
