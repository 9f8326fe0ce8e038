"""gc_downconvert (csrc/ddc.hip) on the GPU: a band of a record as a second record at a lower rate, against the float64 numpy model
of the definition (tests/ddc_model.py).

1. Exact class: no NCO, dyadic taps - every product and sum exact, every tie a real tie: all bytes, clipped and sum_sq equal.
2. General class: firwin low-passes moved to a carrier: every component outside the model's near-half mask equal (one ulp in sin or
   cos may turn the others), the mask at most 10 per 100 000 components - asserted before anything is compared.
3. Tile edges, with the input span starting on every residue of 16 bytes.
4. Pieces of a call join to the bytes of the whole; a second run gives the same bytes.
5. The NCO's integers, a tone taken to DC, carr_freq against -carr_freq.
6. Refusals: each next to the accepted call that closes it; dst and a pre-filled result untouched.
7. The probe, the circshift search and the excision return the same bytes around a down-conversion.
8. End to end on the four-satellite scene through receiver.downconvert_band and the library's acquisition."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import ddc_model as M

pytestmark = pytest.mark.gpu
FS = 18e6
NS = 40000
I8, I16 = np.int8, np.int16
REAL, IQ, QI = M.REAL, M.IQ, M.QI
FORMATS = {"i8_iq": (I8, IQ), "i8_qi": (I8, QI), "i8_real": (I8, REAL), "i16_iq": (I16, IQ), "i16_qi": (I16, QI), "i16_real": (I16, REAL)}
PAD_FRONT, PAD_BACK = 7, 9                 # sentinel samples of dst in front of and behind the written range
SENTINEL = 85
F1, F2, F3 = 2000137.0, -4500137.0, 123456.789


def _comps(layout):
    return 1 if layout == REAL else 2


def _full_range(dtype, layout, seed, n=NS):
    """Values over the dtype's whole range, the two ends planted next to each other and at both ends of the record."""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(seed)
    raw = rng.integers(info.min, info.max + 1, n * _comps(layout)).astype(dtype)
    raw[:4] = [info.min, info.min, info.max, info.max]
    raw[-4:] = [info.max, info.min, info.min, info.max]
    raw[1000:1008] = info.min
    raw[2000:2008] = info.max
    return raw


def _noise(dtype, layout, seed, n=NS):
    sigma = 20.0 if dtype == I8 else 5000.0
    info = np.iinfo(dtype)
    return np.clip(np.rint(np.random.default_rng(seed).normal(0.0, sigma, n * _comps(layout))), info.min, info.max).astype(dtype)


@pytest.fixture(scope="module")
def dst_engine():
    import cu_sdr_collection_amd as P
    eng = P.Engine(0)
    yield eng
    eng.close()


def _run(engine, dst, dst_dtype, dst_layout, taps, decim, nout, **kw):
    """One call into a dst record of nout samples between PAD_FRONT and PAD_BACK sentinel samples.  Returns (the written range as
    dst_dtype in file order, result); asserts the sentinels on both sides."""
    c = _comps(dst_layout)
    total = PAD_FRONT + nout + PAD_BACK
    dst.load_if(np.full(total * c, SENTINEL, dtype=dst_dtype), layout=dst_layout)
    res = engine.downconvert(dst, taps, decim, noutputs=nout, dst_first=PAD_FRONT, **kw)
    back = dst.read_if(0, total, dtype=dst_dtype, layout=dst_layout)
    assert np.all(back[:PAD_FRONT * c] == SENTINEL) and np.all(back[(PAD_FRONT + nout) * c:] == SENTINEL), "bytes outside the range were written"
    assert res.noutputs == nout
    return back[PAD_FRONT * c:(PAD_FRONT + nout) * c], res


def _all_outputs(ns, ntaps, decim, first):
    return (ns + ntaps - 2 - first) // decim + 1


# ---- 1. exact class ------------------------------------------------------------------------------------------------------------------
EXACT_TAPS = {"boxcar": [0.25] * 4, "complex": [0.5, -0.25j, 0.125 + 0.375j], "one": [1.0], "three": [3.0]}


@pytest.mark.parametrize("src_fmt", list(FORMATS))
def test_exact_class_every_byte_and_both_statistics(engine, dst_engine, src_fmt):
    """Would catch: a sample left out or taken twice at a tile or record edge, a wrong zero padding in front of sample 0 or behind
    the last sample, a swapped pair, a tie rounded away from even, a clamp at the wrong end, a miscounted clipped or sum_sq - in any
    of the 36 format pairs."""
    sdt, slay = FORMATS[src_fmt]
    raw = _full_range(sdt, slay, 700 + len(src_fmt))
    engine.load_if(raw, layout=slay, fs=FS)
    some_clipped = some_tie = False
    for k, (dst_fmt, (ddt, dlay)) in enumerate(FORMATS.items()):
        for name, taps in EXACT_TAPS.items():
            for decim in (1, 2, 3, 4, 5, 7, 16, 64):
                for first in (0, 1, 5):
                    nout = _all_outputs(NS, len(taps), decim, first)            # the last outputs read beyond the record's end
                    want, clipped, sum_sq, near, _ = M.downconvert(raw, slay, taps, decim, FS, ddt, dlay, first_sample=first, noutputs=nout)
                    got, res = _run(engine, dst_engine, ddt, dlay, taps, decim, nout, first_sample=first)
                    tag = (src_fmt, dst_fmt, name, decim, first)
                    assert got.tobytes() == want.tobytes(), tag
                    assert (res.clipped, res.sum_sq) == (clipped, sum_sq), tag
                    assert (res.phase_step, res.phase0, res.carr_freq) == (0, 0, 0.0)
                    some_clipped |= clipped > 0
                    some_tie |= bool(near.any())
    assert some_clipped and some_tie


@pytest.mark.parametrize("src_fmt", ["i8_iq", "i8_real", "i16_iq", "i16_real"])
def test_exact_class_on_a_record_that_ends_inside_16_bytes(engine, dst_engine, src_fmt):
    """Would catch: the byte path of the record's partial last vector reading too little, too much or the wrong bytes."""
    sdt, slay = FORMATS[src_fmt]
    for ns in (NS - 3, NS - 7, 17, 5):
        raw = _full_range(sdt, slay, 720, NS)[:ns * _comps(slay)]
        engine.load_if(raw, layout=slay, fs=FS)
        for taps in (EXACT_TAPS["boxcar"], EXACT_TAPS["complex"]):
            for decim, first in ((1, 0), (3, 1), (7, 5)):
                nout = _all_outputs(ns, len(taps), decim, first)
                want, clipped, sum_sq, _, _ = M.downconvert(raw, slay, taps, decim, FS, I16, IQ, first_sample=first, noutputs=nout)
                got, res = _run(engine, dst_engine, I16, IQ, taps, decim, nout, first_sample=first)
                assert got.tobytes() == want.tobytes() and (res.clipped, res.sum_sq) == (clipped, sum_sq), (src_fmt, ns, decim, first)


# ---- 2. general class ----------------------------------------------------------------------------------------------------------------
def _lowpass(ntaps, carrier, gain=1.0):
    """A firwin low-pass of 1.2 MHz at FS moved to the frequency the NCO runs at for `carrier`."""
    from scipy.signal import firwin

    from cu_sdr_collection_amd import receiver as R
    h = firwin(ntaps, 1.2e6, fs=FS) if ntaps > 1 else np.ones(1)
    return gain * R.ddc_modulate(h, M.nco_freq(M.phase_step(carrier, FS), FS), FS)


def _hold(got, res, want, clipped, sum_sq, near, dst_layout, tag):
    """The comparison of the general class: the near-half cap first, then every component outside the mask, then the statistics."""
    cap = near.shape[0] * 10 // 100000
    assert int(near.sum()) <= cap, (tag, int(near.sum()), cap)
    differ = got != want
    assert not np.any(differ & ~near), (tag, int(np.sum(differ & ~near)))
    ints = got.astype(np.int64)
    assert res.sum_sq == int(np.sum(ints * ints)), tag                          # what the library says it stored is what it stored
    if not near.any():
        assert (res.clipped, res.sum_sq) == (clipped, sum_sq), tag
    else:
        assert abs(res.clipped - clipped) <= int(near.sum()), tag


# (T, D, carrier, phase, src, dst, gain): each T once, each D once, the corners of the (D, T) domain, complex and real sources
GENERAL = [(1, 1, F1, 0.0, "i8_iq", "i8_iq", 4.0), (2, 3, F2, 100.0, "i16_iq", "i16_iq", 1.0), (33, 4, F3, 0.0, "i8_real", "i8_iq", 2.0),
           (129, 9, F1, 100.0, "i16_real", "i16_qi", 2.0), (700, 64, F2, 0.0, "i8_qi", "i8_real", 2.0), (701, 1, F3, 100.0, "i8_iq", "i16_iq", 64.0),
           (2048, 3, F1, 0.0, "i16_qi", "i8_iq", 1.0 / 64), (2048, 64, F2, 100.0, "i8_iq", "i8_iq", 2.0), (1, 64, F3, 0.0, "i16_iq", "i16_real", 1.0),
           (2048, 1, F2, 0.0, "i8_real", "i16_iq", 64.0)]


@pytest.mark.parametrize("case", GENERAL, ids=[f"T{c[0]}_D{c[1]}_{c[4]}_to_{c[5]}" for c in GENERAL])
def test_general_class_against_the_model(engine, dst_engine, case):
    """Would catch: a tap chain added in another order or with a fused multiply-add, a phase that depends on the call's start or loses
    bits at large indices, a rotation of the wrong sign, a sample offset by one at some (D, T)."""
    T, D, carrier, phase, src_fmt, dst_fmt, gain = case
    (sdt, slay), (ddt, dlay) = FORMATS[src_fmt], FORMATS[dst_fmt]
    raw = _noise(sdt, slay, 730 + T + D)
    engine.load_if(raw, layout=slay, fs=FS)
    taps = _lowpass(T, carrier, gain)
    first = (T - 1) // 2
    nout = _all_outputs(NS, T, D, first)
    want, clipped, sum_sq, near, _ = M.downconvert(raw, slay, taps, D, FS, ddt, dlay, carr_freq=carrier, carr_phase=phase, first_sample=first, noutputs=nout)
    got, res = _run(engine, dst_engine, ddt, dlay, taps, D, nout, carr_freq=carrier, carr_phase=phase, first_sample=first)
    print(f"DDC general T={T} D={D}: {nout} outputs, near-half {int(near.sum())}, differing {int(np.sum(got != want))}, clipped {res.clipped} (model {clipped})")
    _hold(got, res, want, clipped, sum_sq, near, dlay, case)
    assert np.any(want != 0)


# ---- 3. tile edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D,src_fmt", [(25, 3, "i8_real"), (2048, 16, "i8_real"), (25, 3, "i16_iq")])
def test_tile_edges_on_every_residue_of_16_bytes(engine, dst_engine, T, D, src_fmt):
    """Would catch: a tile's last or first output missing or doubled, a staged span one vector short when it starts late in a vector,
    an LDS offset that ignores the span's start inside its first vector."""
    import cu_sdr_collection_amd as P
    sdt, slay = FORMATS[src_fmt]
    bps = _comps(slay) * np.dtype(sdt).itemsize
    tile = P.Engine.debug_ddc_tile_outputs(D, T)
    assert 1 < tile <= 1024 and (T < 2048 or tile < 1024)
    raw = _noise(sdt, slay, 740 + T)
    engine.load_if(raw, layout=slay, fs=FS)
    taps = _lowpass(T, F1, 2.0)
    residues = set()
    info = np.iinfo(I8)
    nmax = 2 * tile + 1
    for first in range(T - 1, T - 1 + 16 // math.gcd(16, bps)):                # the span of tile 0 starts at sample first - (T - 1)
        # one model run per first_sample: an output does not depend on how many follow it
        want, _, _, near, (yr, yi) = M.downconvert(raw, slay, taps, D, FS, I8, IQ, carr_freq=F1, carr_phase=100.0, first_sample=first, noutputs=nmax)
        out_of_range = (np.rint(yr) < info.min) | (np.rint(yr) > info.max), (np.rint(yi) < info.min) | (np.rint(yi) > info.max)
        for nout in (tile - 1, tile, tile + 1, nmax):
            for t in range(-(-nout // tile)):
                residues.add(((first + t * tile * D - (T - 1)) * bps) % 16)
            w = want[:2 * nout]
            clipped = int(out_of_range[0][:nout].sum() + out_of_range[1][:nout].sum())
            sum_sq = int(np.sum(w.astype(np.int64) ** 2))
            got, res = _run(engine, dst_engine, I8, IQ, taps, D, nout, carr_freq=F1, carr_phase=100.0, first_sample=first)
            _hold(got, res, w, clipped, sum_sq, near[:2 * nout], IQ, (T, D, src_fmt, first, nout))
    assert residues == set(range(0, 16, math.gcd(16, bps)))


# ---- 4. pieces join ------------------------------------------------------------------------------------------------------------------
def test_pieces_join_to_the_whole_and_a_second_run_is_the_first(engine, dst_engine):
    """Would catch: an output that depends on the tile or the call it falls in - a phase counted from the call's start, a filter state
    carried between tiles, statistics that are not per output."""
    T, D, n0 = 33, 3, 11
    tile = dst_engine.debug_ddc_tile_outputs(D, T)
    nout, a, b = 3 * tile + 500, 777, 2 * tile
    raw = _noise(I8, IQ, 750)
    engine.load_if(raw, fs=FS)
    taps = _lowpass(T, F2, 2.0)
    kw = dict(carr_freq=F2, carr_phase=100.0)
    whole, res = _run(engine, dst_engine, I8, IQ, taps, D, nout, first_sample=n0, **kw)
    again, res2 = _run(engine, dst_engine, I8, IQ, taps, D, nout, first_sample=n0, **kw)
    assert again.tobytes() == whole.tobytes() and vars(res2) == vars(res)
    dst_engine.load_if(np.full(2 * nout, SENTINEL, dtype=I8))
    parts = [engine.downconvert(dst_engine, taps, D, first_sample=n0 + lo * D, noutputs=hi - lo, dst_first=lo, **kw) for lo, hi in ((0, a), (a, b), (b, nout))]
    assert dst_engine.read_if(0, nout).tobytes() == whole.tobytes()
    assert sum(p.clipped for p in parts) == res.clipped and sum(p.sum_sq for p in parts) == res.sum_sq
    assert res.sum_sq > 0


# ---- 5. the NCO ----------------------------------------------------------------------------------------------------------------------
def test_nco_integers_and_a_tone_taken_to_dc(engine, dst_engine):
    """Would catch: a phase step truncated instead of rounded or of the wrong sign, a phase0 off by a turn, a rotation that moves the
    band up instead of down, taps moved to the wrong side."""
    from cu_sdr_collection_amd import receiver as R
    raw = _noise(I8, IQ, 760)
    engine.load_if(raw, fs=FS)
    for f in (0.0, 1.0, -1.0, FS / 2 - 1.0, -(FS / 2 - 1.0), F1, F2, F3):
        for phi in (0.0, math.pi, -math.pi, 1e-9, -1e-9, 100.0):
            _, res = _run(engine, dst_engine, I8, IQ, [1.0], 1, 16, carr_freq=f, carr_phase=phi)
            assert res.phase_step == M.phase_step(f, FS) and res.phase0 == M.phase0(phi), (f, phi)
            assert res.carr_freq == M.nco_freq(res.phase_step, FS) == R.ddc_nco_freq(R.ddc_nco_step(f, FS), FS)
    # a tone on bin 137 of 1 024 of the output rate, D = 3
    D, nfft, T = 3, 1024, 49
    ft = 137 * (FS / D) / nfft
    n = np.arange(NS)
    z = 100.0 * np.exp(2j * np.pi * ft * n / FS)
    tone = np.empty(2 * NS, dtype=I8)
    tone[0::2], tone[1::2] = np.rint(z.real), np.rint(z.imag)
    engine.load_if(tone, fs=FS)
    g, f_used, h = R.ddc_band_taps(FS, ft, 1.2e6, T)
    nout = 12 * nfft
    dst_engine.load_if(np.zeros(2 * nout, dtype=I8), fs=FS / D)
    res = engine.downconvert(dst_engine, g, D, carr_freq=ft, first_sample=(T - 1) // 2 + 600, noutputs=nout)
    assert res.clipped == 0 and abs(res.carr_freq - ft) < 1e-8
    psd = dst_engine.probe_psd(0, nout, nfft, nfft // 2, "hamming")[0].reshape(-1)
    away = np.concatenate([psd[4:nfft - 3]])
    assert int(np.argmax(psd)) == 0 and psd[0] > 1e5 * away.max(), (psd[0], away.max())
    # the mirrored NCO takes the same tone to 2 ft = 1.6 MHz, past the band of taps moved to -ft: what is left is the stop-band's
    gm, _, _ = R.ddc_band_taps(FS, -ft, 1.2e6, T)
    res_m = engine.downconvert(dst_engine, gm, D, carr_freq=-ft, first_sample=(T - 1) // 2 + 600, noutputs=nout)
    assert res_m.phase_step == (1 << 64) - res.phase_step
    assert res_m.sum_sq < 1e-3 * res.sum_sq                                    # Hamming, 49 taps: below -50 dB out there


@pytest.mark.parametrize("fmt", ["i8_iq", "i16_iq"])
def test_carr_freq_and_its_negative_mirror(engine, dst_engine, fmt):
    """Would catch: a sign convention that differs between the taps, the samples and the NCO: conj(record), conj(taps) and -carr_freq
    must give conj(output)."""
    dtype, layout = FORMATS[fmt]
    raw = _noise(dtype, layout, 770)
    mirrored = raw.copy()
    mirrored[1::2] = -raw[1::2]                                                 # sigma is far from the range's end: no -128 to negate
    T, D = 33, 4
    taps = _lowpass(T, F3, 2.0)
    engine.load_if(raw, layout=layout, fs=FS)
    up, res_up = _run(engine, dst_engine, dtype, layout, taps, D, 9000, carr_freq=F3, first_sample=16)
    _, _, _, near, _ = M.downconvert(raw, layout, taps, D, FS, dtype, layout, carr_freq=F3, first_sample=16, noutputs=9000)
    engine.load_if(mirrored, layout=layout, fs=FS)
    down, res_down = _run(engine, dst_engine, dtype, layout, np.conj(taps), D, 9000, carr_freq=-F3, first_sample=16)
    assert res_down.phase_step == (1 << 64) - res_up.phase_step
    assert int(near.sum()) <= near.shape[0] * 10 // 100000
    ok = ~near
    assert np.array_equal(up[0::2][ok[0::2]], down[0::2][ok[0::2]]) and np.array_equal(up[1::2][ok[1::2]], -down[1::2][ok[1::2]])
    assert np.any(up != 0)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_and_the_result_untouched(engine, dst_engine):
    """Would catch: a check that comes after the first write, a refusal with the wrong status, a result written by a refused call."""
    import cu_sdr_collection_amd as P
    L = P._lib
    lib = L.load()
    raw = _noise(I8, IQ, 780)
    engine.load_if(raw, fs=FS)
    ND = 5000
    sentinel = np.full(2 * ND, SENTINEL, dtype=I8)
    dst_engine.load_if(sentinel)
    ones = np.ones((25, 2))

    def call(src, dst, first=0, nout=1000, dst_first=0, decim=3, ntaps=25, freq=0.0, phase=0.0, taps=ones, null_p=False):
        p = L.gc_ddc_params(first, nout, dst_first, decim, ntaps, freq, phase)
        r = L.gc_ddc_result(7, 7, -7, 7, -7.0)
        t = None if taps is None else np.ascontiguousarray(np.resize(taps, (max(ntaps, 1), 2)), dtype=np.float64)
        rc = lib.gc_downconvert(src, dst, None if null_p else C.byref(p), None if t is None else t.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r))
        assert rc == L.GC_OK or (r.phase_step, r.phase0, r.clipped, r.sum_sq, r.carr_freq) == (7, 7, -7, 7, -7.0), "result written by a refused call"
        return rc

    def untouched():
        return dst_engine.read_if(0, ND).tobytes() == sentinel.tobytes()

    src, dst = engine._ctx, dst_engine._ctx
    bad = np.ones((25, 2))
    bad[7, 1] = float("nan")
    inf = np.ones((25, 2))
    inf[0, 0] = float("inf")
    for kw in (dict(null_p=True), dict(taps=None), dict(first=-1), dict(dst_first=-1), dict(nout=0), dict(nout=-3), dict(decim=0), dict(decim=65),
               dict(ntaps=0), dict(ntaps=2049), dict(taps=bad), dict(taps=inf), dict(freq=float("nan")), dict(freq=float("inf")), dict(phase=float("nan")),
               dict(phase=-float("inf")), dict(freq=FS / 2), dict(freq=-FS / 2), dict(freq=1e9)):
        assert call(src, dst, **kw) == L.GC_E_INVALID and untouched(), kw
    assert call(None, dst) == L.GC_E_INVALID and untouched()
    assert call(src, None) == L.GC_E_INVALID
    assert call(src, src) == L.GC_E_INVALID                                                          # dst == src
    assert engine.read_if(0, NS).tobytes() == raw.tobytes()
    for kw in (dict(nout=ND + 1), dict(dst_first=ND - 999), dict(dst_first=ND, nout=1), dict(dst_first=1 << 62, nout=1), dict(nout=(1 << 63) - 1),
               dict(first=NS + 24, nout=1), dict(first=1 << 62, nout=1), dict(first=24 + 8, decim=8, nout=ND)):
        assert call(src, dst, **kw) == L.GC_E_RANGE and untouched(), kw
    with P.Engine(0) as fresh:                                                                       # no record; no sampling frequency
        assert call(fresh._ctx, dst) == L.GC_E_STATE and untouched()
        assert call(src, fresh._ctx) == L.GC_E_STATE
        assert call(fresh._ctx, dst, decim=0) == L.GC_E_INVALID                                      # arguments before state
        fresh.load_if(raw)                                                                           # a record, no sampling frequency
        assert call(fresh._ctx, dst) == L.GC_E_STATE and untouched()
        fresh.set_sampling_freq(FS)
        assert call(fresh._ctx, dst) == L.GC_OK and not untouched()
    dst_engine.load_if(sentinel)
    # a dst that shares src's record; records that overlap: two attached 32 bytes apart in one allocation
    with P.Engine(0) as other:
        other.share_if(engine)
        assert call(src, other._ctx) == L.GC_E_INVALID and call(other._ctx, src) == L.GC_E_INVALID
        assert engine.read_if(0, NS).tobytes() == raw.tobytes()
        # ... while a src that shares another context's record works, and gives the owner's bytes
        want, _, _, _, _ = M.downconvert(raw, IQ, ones, 3, FS, I8, IQ, noutputs=1000)
        assert call(other._ctx, dst) == L.GC_OK                                                      # (gc_share_if hands the sampling frequency on)
        assert dst_engine.read_if(0, 1000).tobytes() == want.tobytes() and dst_engine.read_if(1000, ND - 1000).tobytes() == sentinel[2000:].tobytes()
        other.load_if(np.zeros(64, dtype=I8))
    dst_engine.load_if(sentinel)
    with P.Engine(0) as big, P.Engine(0) as a, P.Engine(0) as b:
        big.load_if(np.concatenate([raw, raw[:64]]))
        big.synchronize()
        base, _ = big.if_buffer()
        a.attach_if(base, NS, I8, IQ)
        b.attach_if(base + 32, NS, I8, IQ)
        a.set_sampling_freq(FS)
        b.set_sampling_freq(FS)
        assert call(a._ctx, b._ctx) == L.GC_E_INVALID and call(b._ctx, a._ctx) == L.GC_E_INVALID
        assert big.read_if(0, NS + 32).tobytes() == np.concatenate([raw, raw[:64]]).tobytes()
        a.load_if(np.zeros(64, dtype=I8))
        b.load_if(np.zeros(64, dtype=I8))
    # the accepted calls that close the ranges
    assert call(src, dst, nout=ND) == L.GC_OK and not untouched()
    assert call(src, dst, dst_first=ND - 1000) == L.GC_OK and call(src, dst, first=NS + 23, nout=1) == L.GC_OK
    assert call(src, dst, first=24, decim=8, nout=ND) == L.GC_OK and call(src, dst, decim=64, ntaps=2048, nout=10) == L.GC_OK
    assert call(src, dst, freq=math.nextafter(FS / 2, 0.0)) == L.GC_OK and call(src, dst, phase=1e300) == L.GC_OK
    with pytest.raises(P.GnssCorrError) as e:
        engine.downconvert(dst_engine, ones, 3, noutputs=ND + 1)
    assert e.value.status == L.GC_E_RANGE
    # noutputs=None: every output the range rule allows, up to dst's capacity
    assert engine.downconvert(dst_engine, ones, 3).noutputs == ND
    assert engine.downconvert(dst_engine, ones, 64).noutputs == (NS + 25 - 2) // 64 + 1


# ---- 7. neighbours -------------------------------------------------------------------------------------------------------------------
def test_probe_search_and_excision_return_the_same_bytes_around_a_downconversion(engine, dst_engine):
    """Would catch: the unit borrowing a buffer of the probe, the acquisition or the excision, or leaving a stream in another state."""
    import cu_sdr_collection_amd as P
    L = P._lib
    n = 72000
    rng = np.random.default_rng(790)
    iq = rng.integers(-20, 21, 2 * (n + 16)).astype(np.int8)
    codes = rng.choice(np.array([-1, 1], dtype=np.int8), (2, 1, n))
    codes[:, :, n // 2:] = 0
    engine.load_if(iq, fs=FS)
    sp = L.gc_acq_shift_params(sampling_freq=FS, carrier_f0=20e3, carrier_step=125.0, first_sample=0, n=n, n_signals=1, n_carriers=2, n_bins=3,
                               n_arms_max=1, source=0)
    gain = rng.uniform(0.0, 2.0, 1024)
    taps = _lowpass(129, F1, 2.0)

    def everything(between):
        dst_engine.load_if(np.zeros(2 * 30000, dtype=I8), fs=FS)
        engine.acq_shift_prepare(sp)
        spectrum = engine.probe_psd(11, 30000, 4096, 2048, "hamming")[0].tobytes()
        if between:
            assert engine.downconvert(dst_engine, taps, 3, carr_freq=F1, first_sample=64, noutputs=20000).sum_sq > 0
        picks = engine.acq_shift_search_batch(codes, None, L.GC_SHIFT_PICK_GLOBAL)
        assert picks is not None
        again = engine.probe_psd(11, 30000, 4096, 2048, "hamming")[0].tobytes()
        if between:
            engine.downconvert(dst_engine, taps, 3, carr_freq=F1, first_sample=64, noutputs=20000)
        with P.Engine(0) as third:
            third.load_if(np.zeros(2 * (n + 16), dtype=I8), fs=FS)
            engine.excise_bins(11, 30000, gain, dst=third)
            cleaned = third.read_if(0, n + 16).tobytes()
        return bytes(picks), spectrum, again, cleaned
    plain = everything(False)
    assert plain[1] == plain[2]
    assert everything(True) == plain and everything(False) == plain
    assert plain[0] != bytes(len(plain[0]))


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_the_four_satellite_scene(engine, dst_engine, l1ca_scene):
    """The first 50 ms of the scene 18 Msps -> 6 Msps (D = 3, a 2.4 MHz band at the IF, 25 taps, int8 I/Q) through
    receiver.downconvert_band, then the library's acquisition on the 6 Msps record with the returned settings.
    Would catch: a wrong output rate or IF in the returned settings, a delay the wrapper does not account for, a gain that clips.

    The same scene through tests/ddc_model.py and the oracle's acquisition_l1ca on the CPU (target_rms 25: 1.7e-6 of the components
    clip; 20 none, 30 2e-5), peakMetric / codePhase / carrFreq, PRN 1 absent:
        PRN   clean 18 Msps            decimated 6 Msps (carrFreq + f_used)
          2   5.58    740  17425       8.98    248  17425
          5   5.56  10797  15475       8.75   3600  15475
         17   5.59  13258  22825       8.78   4421  22825
          7   5.17  10492  17775       8.19   3499  17775
          1   1.50      -      -       2.44      -      -
    The band keeps the main lobe and drops two thirds of the noise: the metric rises."""
    import cu_sdr_collection_amd as P
    S, sats, iq = l1ca_scene
    fs = S.samplingFreq
    n = int(0.05 * fs)
    D = 3
    rec = iq[:2 * n]
    prns = [s.prn for s in sats]
    absent = next(p for p in range(1, 33) if p not in prns)
    S1 = copy.copy(S)
    S1.acqSatelliteList = prns + [absent]
    engine.load_if(rec, fs=fs)
    clean = P.acquisition(engine, S1, first_sample=0)
    dst_engine.alloc_if(n // D, I8, IQ)
    res, new = P.downconvert_band(engine, dst_engine, S.IF, 2.4e6, D, target_rms=25.0)
    assert res.noutputs == n // D and new.samplingFreq == fs / D and new.decim == D and new.delay == 0.0
    assert new.f_used == res.carr_freq and abs(new.IF) < 1e-6 and new.gain > 1.0
    assert res.clipped < 1e-4 * 2 * res.noutputs
    assert abs(math.sqrt(res.sum_sq / (2 * res.noutputs)) - 25.0) < 1.0
    S2 = copy.copy(S1)
    S2.samplingFreq, S2.IF = new.samplingFreq, new.IF
    got = P.acquisition(dst_engine, S2, first_sample=0)
    fine_step = 25.0
    print("DDC scene: " + "; ".join(f"PRN {p} peakMetric {clean.peakMetric[p - 1]:.2f} -> {got.peakMetric[p - 1]:.2f}, codePhase {clean.codePhase[p - 1]:.0f} -> "
                                    f"{got.codePhase[p - 1]:.0f}, carrFreq {clean.carrFreq[p - 1]:.0f} -> {got.carrFreq[p - 1] + new.f_used:.0f}" for p in prns)
          + f"; absent PRN {absent}: {clean.peakMetric[absent - 1]:.2f} -> {got.peakMetric[absent - 1]:.2f}")
    for p in prns:
        assert clean.peakMetric[p - 1] > S.acqThreshold and got.peakMetric[p - 1] > S.acqThreshold, p
        assert clean.carrFreq[p - 1] != 0 and got.carrFreq[p - 1] != 0, p
        assert abs((got.codePhase[p - 1] - 1) - (clean.codePhase[p - 1] - 1) / D) <= 1.0, (p, clean.codePhase[p - 1], got.codePhase[p - 1])
        assert abs(got.carrFreq[p - 1] + new.f_used - clean.carrFreq[p - 1]) <= fine_step, (p, clean.carrFreq[p - 1], got.carrFreq[p - 1])
    assert got.peakMetric[absent - 1] < S.acqThreshold and got.carrFreq[absent - 1] == 0
