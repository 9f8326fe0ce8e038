"""gc_resample (csrc/resample.hip) on the GPU: a record at the rate L / M of its own as a second record, against the float64 numpy
model of the definition (tests/resample_model.py) and, for L = 1, against gc_downconvert itself.

1. L = 1 is gc_downconvert: bytes and every field of the result.
2. Exact class: no NCO, dyadic taps with another value on every phase - every product and sum exact, every tie a real tie: all
   bytes, clipped and sum_sq equal, over the 36 format pairs.
3. General class: firwin prototypes moved to a carrier: every component outside the model's near-half mask equal (one ulp in sin or
   cos may turn the others), the mask at most 10 per 100 000 components - asserted before anything is compared.
4. Tile edges, with the input span starting on every residue of 16 bytes and the first output on the first and the last phase.
5. Pieces of a call join to the bytes of the whole; a second run gives the same bytes.
6. A tone lands on its bin of the output rate, and on bin 0 when the NCO takes it there.
7. Refusals: each next to the accepted call that closes it; dst and a pre-filled result untouched.
8. The probe, the circshift search and the excision return the same bytes around a resampling.
9. End to end on the four-satellite scene, 18 Msps -> 4 Msps, through receiver.resample_record and the library's acquisition."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import ddc_model as DM
import resample_model as RM

pytestmark = pytest.mark.gpu
FS = 18e6
NS = 40000
I8, I16 = np.int8, np.int16
REAL, IQ, QI = RM.REAL, RM.IQ, RM.QI
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


def _run(engine, dst, dst_dtype, dst_layout, taps, L, M, nout, call="resample", **kw):
    """One call into a dst record of nout samples between PAD_FRONT and PAD_BACK sentinel samples.  Returns (the written range as
    dst_dtype in file order, result); asserts the sentinels on both sides."""
    c = _comps(dst_layout)
    total = PAD_FRONT + nout + PAD_BACK
    dst.load_if(np.full(total * c, SENTINEL, dtype=dst_dtype), layout=dst_layout)
    if call == "resample":
        res = engine.resample(dst, taps, L, M, noutputs=nout, dst_first=PAD_FRONT, **kw)
    else:
        assert L == 1
        res = engine.downconvert(dst, taps, M, noutputs=nout, dst_first=PAD_FRONT, **kw)
    back = dst.read_if(0, total, dtype=dst_dtype, layout=dst_layout)
    assert np.all(back[:PAD_FRONT * c] == SENTINEL) and np.all(back[(PAD_FRONT + nout) * c:] == SENTINEL), "bytes outside the range were written"
    assert res.noutputs == nout
    return back[PAD_FRONT * c:(PAD_FRONT + nout) * c], res


def _prototype(L, M, T, carrier, gain=1.0):
    """gain * L * firwin(T, 0.4 FS min(1, L / M), fs = FS L) moved to the frequency the NCO runs at for `carrier`."""
    from scipy.signal import firwin

    from cu_sdr_collection_amd import receiver as R
    h = firwin(T, 0.4 * FS * min(1.0, L / M), fs=FS * L) if T > 1 else np.ones(1)
    return gain * R.ddc_modulate(L * h, RM.rs_nco_freq(RM.rs_phase_step(carrier, FS, L), FS, L), FS * L)


def _hold(got, res, want, clipped, sum_sq, near, dst_layout, tag):
    """The comparison of the general class (test_gpu_ddc._hold's rule): the near-half cap first, then every component outside the
    mask, then the statistics."""
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


# ---- 1. L = 1 is gc_downconvert --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_fmt", list(FORMATS))
def test_interp_one_is_downconvert(engine, dst_engine, src_fmt):
    """Would catch: any operation of the resampler that differs from the down-converter's - a tap order, a phase, a tile that stages
    another span - on the code that already has its own tests."""
    sdt, slay = FORMATS[src_fmt]
    raw = _noise(sdt, slay, 800 + len(src_fmt))
    engine.load_if(raw, layout=slay, fs=FS)
    rng = np.random.default_rng(801)
    for dst_fmt in ("i8_iq", "i16_qi"):
        ddt, dlay = FORMATS[dst_fmt]
        for M, T in ((1, 1), (3, 25), (64, 2048), (9, 129)):
            assert dst_engine.debug_rs_tile_outputs(1, M, T) == dst_engine.debug_ddc_tile_outputs(M, T)
            scale = (2.0 if sdt == I8 else 1.0 / 64) * (1.0 if ddt == I8 else 64.0) / math.sqrt(T)
            taps = scale * (rng.standard_normal(T) + 1j * rng.standard_normal(T))
            for first in (0, 5):
                nout = RM.full_outputs(NS, T, 1, M, first)
                kw = dict(carr_freq=F1, carr_phase=100.0)
                want, rw = _run(engine, dst_engine, ddt, dlay, taps, 1, M, nout, call="downconvert", first_sample=first, **kw)
                got, rg = _run(engine, dst_engine, ddt, dlay, taps, 1, M, nout, first_tick=first, **kw)
                tag = (src_fmt, dst_fmt, M, T, first)
                assert got.tobytes() == want.tobytes(), tag
                assert (rg.clipped, rg.sum_sq, rg.phase_step, rg.phase0, rg.carr_freq) == (rw.clipped, rw.sum_sq, rw.phase_step, rw.phase0, rw.carr_freq), tag
                assert rg.out_rate == FS / M and rw.sum_sq > 0, tag


# ---- 2. exact class ------------------------------------------------------------------------------------------------------------------
EXACT_LM = [(1, 1), (2, 1), (1, 2), (2, 3), (3, 2), (3, 3), (4, 6), (5, 7), (7, 64), (64, 63), (64, 4096)]


def _exact_taps(L):
    k = np.arange(2 * L)
    return {"ramp": (1 + (k % 7)) / 8.0, "complex": ((k % 5) - 2) / 8.0 + 1j * ((k % 3) - 1) / 8.0, "one": np.ones(1)}


@pytest.mark.parametrize("src_fmt", list(FORMATS))
def test_exact_class_every_byte_and_both_statistics(engine, dst_engine, src_fmt):
    """Would catch: a tap of the wrong phase or branch, a sample left out or taken twice at a tile or record edge, a wrong zero
    padding in front of sample 0 or behind the last sample, a swapped pair, a tie rounded away from even, a clamp at the wrong end, a
    miscounted clipped or sum_sq - in any of the 36 format pairs."""
    sdt, slay = FORMATS[src_fmt]
    raw = _full_range(sdt, slay, 810 + len(src_fmt))
    engine.load_if(raw, layout=slay, fs=FS)
    some_clipped = some_tie = False
    for dst_fmt, (ddt, dlay) in FORMATS.items():
        for L, M in EXACT_LM:
            for name, taps in _exact_taps(L).items():
                for first in sorted({0, 1, L - 1, 5 * L + 3}):
                    nout = RM.full_outputs(NS, len(taps), L, M, first)             # the last outputs read beyond the record's end
                    want, clipped, sum_sq, near, _ = RM.resample(raw, slay, taps, L, M, FS, ddt, dlay, first_tick=first, noutputs=nout)
                    got, res = _run(engine, dst_engine, ddt, dlay, taps, L, M, nout, first_tick=first)
                    tag = (src_fmt, dst_fmt, L, M, name, first)
                    assert got.tobytes() == want.tobytes(), tag
                    assert (res.clipped, res.sum_sq) == (clipped, sum_sq), tag
                    assert (res.phase_step, res.phase0, res.carr_freq) == (0, 0, 0.0) and res.out_rate == (FS * L) / M
                    some_clipped |= clipped > 0
                    some_tie |= bool(near.any())
    assert some_clipped and some_tie


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_three_over_three_with_one_tap_copies_the_record(engine, dst_engine, fmt):
    dtype, layout = FORMATS[fmt]
    raw = _full_range(dtype, layout, 820)
    engine.load_if(raw, layout=layout, fs=FS)
    got, res = _run(engine, dst_engine, dtype, layout, [1.0], 3, 3, NS)
    assert got.tobytes() == raw.tobytes() and res.clipped == 0 and res.out_rate == FS


# ---- 3. general class ----------------------------------------------------------------------------------------------------------------
# (L, M, T, carrier, phase, src, dst, gain)
GENERAL = [(1, 3, 25, F1, 0.0, "i8_iq", "i8_iq", 2.0), (2, 5, 41, F3, 100.0, "i16_iq", "i8_iq", 1.0 / 64), (3, 2, 33, F2, 0.0, "i8_real", "i8_iq", 2.0),
           (64, 63, 2048, F1, 100.0, "i8_iq", "i16_iq", 64.0), (7, 64, 701, F2, 0.0, "i8_qi", "i8_real", 2.0),
           (64, 4096, 2048, F3, 0.0, "i16_qi", "i8_iq", 1.0 / 64), (5, 1, 9, F1, 0.0, "i8_iq", "i16_qi", 64.0),
           (4, 6, 129, F2, 100.0, "i16_real", "i16_iq", 2.0), (1, 1, 1, F3, 0.0, "i8_iq", "i8_iq", 4.0), (64, 1, 64, F1, 100.0, "i8_real", "i8_iq", 2.0),
           (37, 50, 1999, F2, 0.0, "i16_iq", "i16_real", 1.0), (10, 4, 2048, F3, 100.0, "i8_iq", "i8_qi", 8.0)]


@pytest.mark.parametrize("case", GENERAL, ids=[f"L{c[0]}_M{c[1]}_T{c[2]}_{c[5]}_to_{c[6]}" for c in GENERAL])
def test_general_class_against_the_model(engine, dst_engine, case):
    """Would catch: a tap chain added in another order or with a fused multiply-add, a branch that starts at the wrong tap, a phase
    counted in samples instead of ticks or that loses bits at large ticks, a rotation of the wrong sign, a sample offset by one at
    some (L, M, T)."""
    L, M, T, carrier, phase, src_fmt, dst_fmt, gain = case
    (sdt, slay), (ddt, dlay) = FORMATS[src_fmt], FORMATS[dst_fmt]
    raw = _noise(sdt, slay, 830 + T + M + L)
    engine.load_if(raw, layout=slay, fs=FS)
    taps = _prototype(L, M, T, carrier, gain)
    first = (T - 1) // 2
    nout = min(RM.full_outputs(NS, T, L, M, first), 100000)
    want, clipped, sum_sq, near, _ = RM.resample(raw, slay, taps, L, M, FS, ddt, dlay, carr_freq=carrier, carr_phase=phase, first_tick=first, noutputs=nout)
    got, res = _run(engine, dst_engine, ddt, dlay, taps, L, M, nout, carr_freq=carrier, carr_phase=phase, first_tick=first)
    print(f"RS general L={L} M={M} T={T}: {nout} outputs, near-half {int(near.sum())}, differing {int(np.sum(got != want))}, clipped {res.clipped} (model {clipped})")
    _hold(got, res, want, clipped, sum_sq, near, dlay, case)
    assert res.phase_step == RM.rs_phase_step(carrier, FS, L) and res.phase0 == RM.phase0(phase)
    assert res.carr_freq == RM.rs_nco_freq(res.phase_step, FS, L) and res.out_rate == RM.out_rate(FS, L, M)
    assert np.any(want != 0)


# ---- 4. tile edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,T", [(2, 5, 41), (64, 63, 2048), (7, 64, 701)])
def test_tile_edges_on_every_residue_of_16_bytes(engine, dst_engine, L, M, T):
    """Would catch: a tile's last or first output missing or doubled, a staged span one vector short when it starts late in a vector,
    an LDS offset that ignores the span's start inside its first vector, a tile whose first phase is taken for 0."""
    tile = dst_engine.debug_rs_tile_outputs(L, M, T)
    assert 1 < tile <= 1024
    raw = _noise(I8, REAL, 840 + T)                                             # one byte per sample: the span starts on any byte
    engine.load_if(raw, layout=REAL, fs=FS)
    taps = _prototype(L, M, T, F1, 2.0)
    J = -(-T // L)
    residues = set()
    info = np.iinfo(I8)
    nmax = 2 * tile + 1
    for r in range(16):
        for p in sorted({0, L - 1}):
            first = L * (r + J - 1) + p                                         # the span of tile 0 starts at sample r
            # one model run per first_tick: an output does not depend on how many follow it
            want, _, _, near, (yr, yi) = RM.resample(raw, REAL, taps, L, M, FS, I8, IQ, carr_freq=F1, carr_phase=100.0, first_tick=first, noutputs=nmax)
            out_of_range = (np.rint(yr) < info.min) | (np.rint(yr) > info.max), (np.rint(yi) < info.min) | (np.rint(yi) > info.max)
            residues.add(r % 16)
            for nout in (tile - 1, tile, tile + 1, nmax):
                w = want[:2 * nout]
                clipped = int(out_of_range[0][:nout].sum() + out_of_range[1][:nout].sum())
                sum_sq = int(np.sum(w.astype(np.int64) ** 2))
                got, res = _run(engine, dst_engine, I8, IQ, taps, L, M, nout, carr_freq=F1, carr_phase=100.0, first_tick=first)
                _hold(got, res, w, clipped, sum_sq, near[:2 * nout], IQ, (L, M, T, first, nout))
    assert residues == set(range(16))


# ---- 5. pieces join ------------------------------------------------------------------------------------------------------------------
def test_pieces_join_to_the_whole_and_a_second_run_is_the_first(engine, dst_engine):
    """Would catch: an output that depends on the tile or the call it falls in - a phase counted from the call's start, a tick that
    is not carried over the cut, statistics that are not per output."""
    L, M, T, u0 = 3, 2, 33, 11
    tile = dst_engine.debug_rs_tile_outputs(L, M, T)
    nout, a, b = 3 * tile + 500, 777, 2 * tile
    raw = _noise(I8, IQ, 850)
    engine.load_if(raw, fs=FS)
    taps = _prototype(L, M, T, F2, 2.0)
    kw = dict(carr_freq=F2, carr_phase=100.0)
    whole, res = _run(engine, dst_engine, I8, IQ, taps, L, M, nout, first_tick=u0, **kw)
    again, res2 = _run(engine, dst_engine, I8, IQ, taps, L, M, nout, first_tick=u0, **kw)
    assert again.tobytes() == whole.tobytes() and vars(res2) == vars(res)
    dst_engine.load_if(np.full(2 * nout, SENTINEL, dtype=I8))
    parts = [engine.resample(dst_engine, taps, L, M, first_tick=u0 + lo * M, noutputs=hi - lo, dst_first=lo, **kw) for lo, hi in ((0, a), (a, b), (b, nout))]
    assert dst_engine.read_if(0, nout).tobytes() == whole.tobytes()
    assert sum(p.clipped for p in parts) == res.clipped and sum(p.sum_sq for p in parts) == res.sum_sq
    assert res.sum_sq > 0


# ---- 6. a tone -----------------------------------------------------------------------------------------------------------------------
def test_a_tone_lands_on_its_bin_of_the_output_rate(engine, dst_engine):
    """Would catch: an output rate that is not fs L / M, a prototype or an NCO laid out at the wrong rate, a rotation that moves the
    band up instead of down."""
    from cu_sdr_collection_amd import receiver as R
    L, M, nfft, T = 2, 5, 1024, 81
    ft = 137 * (FS * L / M) / nfft
    n = np.arange(NS)
    z = 100.0 * np.exp(2j * np.pi * ft * n / FS)
    tone = np.empty(2 * NS, dtype=I8)
    tone[0::2], tone[1::2] = np.rint(z.real), np.rint(z.imag)
    engine.load_if(tone, fs=FS)
    nout = 12 * nfft
    for carrier, want_bin in ((0.0, 137), (ft, 0)):
        g, f_used, h = R.resample_taps(FS, L, M, carrier, None, T)
        dst_engine.load_if(np.zeros(2 * nout, dtype=I8), fs=FS * L / M)
        res = engine.resample(dst_engine, g, L, M, carr_freq=carrier, first_tick=(T - 1) // 2 + 600 * L, noutputs=nout)
        assert res.out_rate == 7.2e6 and res.clipped == 0 and abs(res.carr_freq - carrier) < 1e-6 and res.carr_freq == f_used
        psd = dst_engine.probe_psd(0, nout, nfft, nfft // 2, "hamming")[0].reshape(-1)
        away = np.roll(psd, -want_bin)[4:nfft - 3]
        assert int(np.argmax(psd)) == want_bin and psd[want_bin] > 1e4 * away.max(), (carrier, int(np.argmax(psd)), psd[want_bin], away.max())


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_and_the_result_untouched(engine, dst_engine):
    """Would catch: a check that comes after the first write, a refusal with the wrong status, a result written by a refused call."""
    import cu_sdr_collection_amd as P
    Lb = P._lib
    lib = Lb.load()
    raw = _noise(I8, IQ, 860)
    engine.load_if(raw, fs=FS)
    ND = 5000
    sentinel = np.full(2 * ND, SENTINEL, dtype=I8)
    dst_engine.load_if(sentinel)
    ones = np.ones((41, 2))

    def call(src, dst, first=0, nout=1000, dst_first=0, interp=2, decim=5, ntaps=41, reserved=0, freq=0.0, phase=0.0, taps=ones, null_p=False):
        p = Lb.gc_rs_params(first, nout, dst_first, interp, decim, ntaps, reserved, freq, phase)
        r = Lb.gc_rs_result(7, 7, -7, 7, -7.0, -7.0)
        t = None if taps is None else np.ascontiguousarray(np.resize(taps, (max(ntaps, 1), 2)), dtype=np.float64)
        rc = lib.gc_resample(src, dst, None if null_p else C.byref(p), None if t is None else t.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r))
        assert rc == Lb.GC_OK or (r.phase_step, r.phase0, r.clipped, r.sum_sq, r.carr_freq, r.out_rate) == (7, 7, -7, 7, -7.0, -7.0), "result written by a refused call"
        return rc

    def untouched():
        return dst_engine.read_if(0, ND).tobytes() == sentinel.tobytes()

    src, dst = engine._ctx, dst_engine._ctx
    bad = np.ones((41, 2))
    bad[7, 1] = float("nan")
    inf = np.ones((41, 2))
    inf[0, 0] = float("inf")
    top = (1 << 63) - 1
    for kw in (dict(null_p=True), dict(taps=None), dict(first=-1), dict(dst_first=-1), dict(nout=0), dict(nout=-3), dict(interp=0), dict(interp=65),
               dict(decim=0), dict(decim=129), dict(interp=1, decim=65), dict(interp=64, decim=4097), dict(ntaps=0), dict(ntaps=2049), dict(reserved=1),
               dict(first=top, nout=2), dict(first=top - 5 * 999 + 1), dict(taps=bad), dict(taps=inf), dict(freq=float("nan")), dict(freq=float("inf")),
               dict(phase=float("nan")), dict(phase=-float("inf")), dict(freq=FS / 2), dict(freq=-FS / 2), dict(freq=1e9)):
        assert call(src, dst, **kw) == Lb.GC_E_INVALID and untouched(), kw
    assert call(None, dst) == Lb.GC_E_INVALID and untouched()
    assert call(src, None) == Lb.GC_E_INVALID
    assert call(src, src) == Lb.GC_E_INVALID                                                         # dst == src
    assert engine.read_if(0, NS).tobytes() == raw.tobytes()
    # J = 21: the last output's oldest sample is (last tick div 2) - 20
    for kw in (dict(nout=ND + 1), dict(dst_first=ND - 999), dict(dst_first=ND, nout=1), dict(dst_first=1 << 62, nout=1), dict(nout=top),
               dict(first=2 * (NS + 20), nout=1), dict(first=1 << 62, nout=1), dict(first=top, nout=1), dict(first=2 * (NS + 20) - 5 * 99, nout=100)):
        assert call(src, dst, **kw) == Lb.GC_E_RANGE and untouched(), kw
    with P.Engine(0) as fresh:                                                                       # no record; no sampling frequency
        assert call(fresh._ctx, dst) == Lb.GC_E_STATE and untouched()
        assert call(src, fresh._ctx) == Lb.GC_E_STATE
        assert call(fresh._ctx, dst, decim=0) == Lb.GC_E_INVALID                                     # arguments before state
        fresh.load_if(raw)                                                                           # a record, no sampling frequency
        assert call(fresh._ctx, dst) == Lb.GC_E_STATE and untouched()
        fresh.set_sampling_freq(FS)
        assert call(fresh._ctx, dst) == Lb.GC_OK and not untouched()
    dst_engine.load_if(sentinel)
    with P.Engine(0) as other:                                                                       # a dst that shares src's record
        other.share_if(engine)
        assert call(src, other._ctx) == Lb.GC_E_INVALID and call(other._ctx, src) == Lb.GC_E_INVALID
        assert engine.read_if(0, NS).tobytes() == raw.tobytes()
        want, _, _, _, _ = RM.resample(raw, IQ, ones, 2, 5, FS, I8, IQ, noutputs=1000)
        assert call(other._ctx, dst) == Lb.GC_OK
        assert dst_engine.read_if(0, 1000).tobytes() == want.tobytes() and dst_engine.read_if(1000, ND - 1000).tobytes() == sentinel[2000:].tobytes()
        other.load_if(np.zeros(64, dtype=I8))
    dst_engine.load_if(sentinel)
    # the accepted calls that close the ranges
    assert call(src, dst, nout=ND) == Lb.GC_OK and not untouched()
    assert call(src, dst, dst_first=ND - 1000) == Lb.GC_OK and call(src, dst, first=2 * (NS + 20) - 1, nout=1) == Lb.GC_OK
    assert call(src, dst, first=2 * (NS + 20) - 1 - 5 * 99, nout=100) == Lb.GC_OK
    assert call(src, dst, interp=64, decim=4096, ntaps=2048, nout=10) == Lb.GC_OK and call(src, dst, interp=64, decim=1, nout=ND) == Lb.GC_OK
    assert call(src, dst, interp=1, decim=64, nout=10) == Lb.GC_OK and call(src, dst, decim=128, nout=10) == Lb.GC_OK
    assert call(src, dst, freq=math.nextafter(FS / 2, 0.0)) == Lb.GC_OK and call(src, dst, phase=1e300) == Lb.GC_OK
    with pytest.raises(P.GnssCorrError) as e:
        engine.resample(dst_engine, ones, 2, 5, noutputs=ND + 1)
    assert e.value.status == Lb.GC_E_RANGE
    # noutputs=None: every output the range rule allows, up to dst's capacity
    assert engine.resample(dst_engine, ones, 2, 5).noutputs == ND
    assert engine.resample(dst_engine, ones, 2, 128).noutputs == RM.full_outputs(NS, 41, 2, 128) == ((NS + 20) * 2 - 1) // 128 + 1


# ---- 8. neighbours -------------------------------------------------------------------------------------------------------------------
def test_probe_search_and_excision_return_the_same_bytes_around_a_resampling(engine, dst_engine):
    """Would catch: the unit borrowing a buffer of the probe, the acquisition or the excision, or leaving a stream in another state."""
    import cu_sdr_collection_amd as P
    Lb = P._lib
    n = 72000
    rng = np.random.default_rng(870)
    iq = rng.integers(-20, 21, 2 * (n + 16)).astype(np.int8)
    codes = rng.choice(np.array([-1, 1], dtype=np.int8), (2, 1, n))
    codes[:, :, n // 2:] = 0
    engine.load_if(iq, fs=FS)
    sp = Lb.gc_acq_shift_params(sampling_freq=FS, carrier_f0=20e3, carrier_step=125.0, first_sample=0, n=n, n_signals=1, n_carriers=2, n_bins=3,
                                n_arms_max=1, source=0)
    gain = rng.uniform(0.0, 2.0, 1024)
    taps = _prototype(2, 5, 129, F1, 2.0)

    def everything(between):
        dst_engine.load_if(np.zeros(2 * 30000, dtype=I8), fs=FS)
        engine.acq_shift_prepare(sp)
        spectrum = engine.probe_psd(11, 30000, 4096, 2048, "hamming")[0].tobytes()
        if between:
            assert engine.resample(dst_engine, taps, 2, 5, carr_freq=F1, first_tick=64, noutputs=20000).sum_sq > 0
        picks = engine.acq_shift_search_batch(codes, None, Lb.GC_SHIFT_PICK_GLOBAL)
        assert picks is not None
        again = engine.probe_psd(11, 30000, 4096, 2048, "hamming")[0].tobytes()
        if between:
            engine.resample(dst_engine, taps, 2, 5, carr_freq=F1, first_tick=64, noutputs=20000)
        with P.Engine(0) as third:
            third.load_if(np.zeros(2 * (n + 16), dtype=I8), fs=FS)
            engine.excise_bins(11, 30000, gain, dst=third)
            cleaned = third.read_if(0, n + 16).tobytes()
        return bytes(picks), spectrum, again, cleaned
    plain = everything(False)
    assert plain[1] == plain[2]
    assert everything(True) == plain and everything(False) == plain
    assert plain[0] != bytes(len(plain[0]))


# ---- 9. end to end -------------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_the_four_satellite_scene(engine, dst_engine, l1ca_scene):
    """The first 50 ms of the scene 18 Msps -> 4 Msps (L / M = 2 / 9, a 2.4 MHz band at the IF, 145 taps, int8 I/Q) through
    receiver.resample_record, then the library's acquisition on the 4 Msps record with the returned settings.
    Would catch: a wrong output rate or IF in the returned settings, a delay the wrapper does not account for, a gain that clips.

    The same scene through tests/resample_model.py and the oracle's acquisition_l1ca on the CPU (gain 3.50, 0 clipped, rms 25.0),
    peakMetric / codePhase / carrFreq + f_used at 4 Msps, threshold 3.5, PRN 1 absent; the clean 18 Msps phases are 740, 10 797,
    13 258 and 10 492:
        PRN 2   6.94   166  17425      PRN 5   6.82  2401  15475      PRN 17  6.76  2948  22825      PRN 7   6.34  2333  17775
        PRN 1   1.88"""
    import cu_sdr_collection_amd as P
    S, sats, iq = l1ca_scene
    fs = S.samplingFreq
    assert fs == 18e6
    n = int(0.05 * fs)
    L, M = 2, 9
    rec = iq[:2 * n]
    prns = [s.prn for s in sats]
    absent = next(p for p in range(1, 33) if p not in prns)
    S1 = copy.copy(S)
    S1.acqSatelliteList = prns + [absent]
    engine.load_if(rec, fs=fs)
    clean = P.acquisition(engine, S1, first_sample=0)
    nout = n * L // M
    dst_engine.alloc_if(nout, I8, IQ)
    res, new = P.resample_record(engine, dst_engine, ratio=(L, M), center_freq=S.IF, bandwidth=2.4e6, ntaps=145, target_rms=25.0)
    assert res.noutputs == nout and new.samplingFreq == 4e6 == res.out_rate and (new.interp, new.decim) == (L, M) and new.delay == 0.0
    assert new.f_used == res.carr_freq and abs(new.IF) < 1e-6 and new.gain > 1.0
    assert res.clipped < 1e-4 * 2 * res.noutputs
    assert abs(math.sqrt(res.sum_sq / (2 * res.noutputs)) - 25.0) < 1.0
    S2 = copy.copy(S1)
    S2.samplingFreq, S2.IF = new.samplingFreq, new.IF
    got = P.acquisition(dst_engine, S2, first_sample=0)
    fine_step = 25.0
    print("RS scene: " + "; ".join(f"PRN {p} peakMetric {clean.peakMetric[p - 1]:.2f} -> {got.peakMetric[p - 1]:.2f}, codePhase {clean.codePhase[p - 1]:.0f} -> "
                                   f"{got.codePhase[p - 1]:.0f}, carrFreq {clean.carrFreq[p - 1]:.0f} -> {got.carrFreq[p - 1] + new.f_used:.0f}" for p in prns)
          + f"; absent PRN {absent}: {clean.peakMetric[absent - 1]:.2f} -> {got.peakMetric[absent - 1]:.2f}; gain {new.gain:.2f}, clipped {res.clipped}")
    for p in prns:
        assert clean.peakMetric[p - 1] > S.acqThreshold and got.peakMetric[p - 1] > S.acqThreshold, p
        assert clean.carrFreq[p - 1] != 0 and got.carrFreq[p - 1] != 0, p
        assert abs((got.codePhase[p - 1] - 1) - (clean.codePhase[p - 1] - 1) * L / M) <= 1.0, (p, clean.codePhase[p - 1], got.codePhase[p - 1])
        assert abs(got.carrFreq[p - 1] + new.f_used - clean.carrFreq[p - 1]) <= fine_step, (p, clean.carrFreq[p - 1], got.carrFreq[p - 1])
    assert got.peakMetric[absent - 1] < S.acqThreshold and got.carrFreq[absent - 1] == 0
