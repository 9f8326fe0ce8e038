"""gc_excise_pulses and gc_excise_bins (csrc/excise.hip) on the GPU.

gc_excise_pulses against the integer numpy model of the definition (tests/excise_model.py): array_equal on every byte of the record
and == on all four statistics; nothing is left out.  Records of 40 000 samples: the kernels' tile is 16 384 samples, so a record
holds two tile boundaries and three workgroups.
1. All six formats x twelve (before, after) pairs - every value of {0, 1, 15, 16, 63, 64, 65, 255, 256, 257, 4095, 4096} once on
   each side - x first_sample in {0, 1, 4097} with a range that ends inside 16 bytes, x four sets of hot samples: one either side
   of every multiple of 64 (and with it of 256 and of the tile); and three sparse ones with the range's first and last sample, one
   inside the guard of each end, and a pair whose guards meet on the first tile boundary - touching (one run), overlapping by one
   sample, missing by one sample (two runs).  Out of place into a sentinel-filled record (outside the range the source's bytes
   arrive, the source stays as it was) and in place (the same bytes).
2. No hot sample; every sample hot; the int16 pair (-32768, -32768), norm 2^31, against 2^31 - 1 and 2^31.
3. A record that ends inside 16 bytes, in all six formats; a record attached inside another allocation (gc_attach_if takes 32-byte
   aligned addresses only: an odd byte offset is refused there, which this test also holds) - there gc_excise_bins and gc_cancel
   in place as well: every call that writes a record 16 bytes at a time leaves the owner's bytes around it alone.
4. Refusals: every one leaves dst (a sentinel fill) and the statistics untouched.
5. Neighbours: a shift search and a spectrum give the same bytes with a gc_excise_pulses between their calls.
6. A call on a context that shares the source's record works in place.

gc_excise_bins: with a gain of ones dst equals src byte for byte at every length and format; out == clamp(rint(values)); in place
equals out of place.  At nfft 16, 1024 and 4096, with the tone's bins zeroed and with a random gain in [0, 2], `values` is held
against the float64 model's unrounded y: r = max|values - y| / (2^-23 A), A the record's largest |component|, may be at most 8 times
the r of the same pipeline in complex64 through scipy.fft on the same case (computed here); dst equals clamp(rint(y)) except where
y lies within that tolerance of a half-integer, where it may differ by one.  The samples that near a half-integer are at most 1 %
of a case (one sample at least) on the int8 records; on the int16 records, where 2 - 16 % of the model's own values lie within the
tolerance whatever computes them, the samples that do differ are held to that 1 % instead.  Run positions (every format, the
three lengths, both gains), a range alone against the same range inside a longer record, one record that the shipping tile budget
cuts, the bin order against gc_probe_psd, refusals, neighbours, and the four-satellite scene with planted interference through receiver.excise_interference.
The short ranges of the run positions (1 to 3 H + 7 samples) are bounded by the complex64 ratio of the whole 40 000-sample record of
the same format, length and gain, not by their own: over one or a few samples the yardstick's largest deviation can be next to
nothing.  A library error confined to those samples is therefore caught only above 8 times the whole record's ratio.
Measured on an MI355X (12 cases per length: six formats x two gains), r of the library / r of the complex64 scipy pipeline:
nfft 16: 0.72 .. 1.46 / 0.82 .. 1.71; nfft 1024: 1.50 .. 3.29 / 1.31 .. 2.78; nfft 4096: 1.47 .. 3.91 / 1.30 .. 2.86; the largest
library / scipy of one case 1.22, 1.27, 1.37 (the bound is 8).  Samples within the tolerance of a half-integer: 11 .. 60 of 40 000 on
the int8 records (at most 1 differs), 970 .. 6 204 on the int16 records (11 .. 75 differ) - DESIGN.md 4.12."""
import ctypes as C

import numpy as np
import pytest

import excise_model as M

pytestmark = pytest.mark.gpu
FS = 18e6
NS = 40000
TILE = 16384
I8, I16 = np.int8, np.int16
REAL, IQ, QI = M.REAL, M.IQ, M.QI
FORMATS = {"i8_iq": (I8, IQ), "i8_qi": (I8, QI), "i8_real": (I8, REAL), "i16_iq": (I16, IQ), "i16_qi": (I16, QI), "i16_real": (I16, REAL)}
GUARDS = [0, 1, 15, 16, 63, 64, 65, 255, 256, 257, 4095, 4096]
PAIRS = list(zip(GUARDS, GUARDS[::-1]))                                # every value once on each side; before + after <= 4096
FIRSTS = [0, 1, 4097]
END = NS - 5                                                           # inside 16 bytes in every format (4, 8 or 16 samples)
QUIET = 10                                                             # |component| of the background: norm <= 200
THRESHOLD2 = 1000


def _quiet(dtype, layout, seed, n=NS):
    return np.random.default_rng(seed).integers(-QUIET, QUIET + 1, n * M.components(layout)).astype(dtype)


def _plant(raw, dtype, layout, hot):
    """Samples `hot` get components far over the threshold, of both signs; the others keep theirs."""
    out = raw.copy()
    per = out.reshape(-1, M.components(layout))
    big = 100 if dtype == I8 else 20000
    hot = np.asarray(sorted(set(int(h) for h in hot)), dtype=np.int64)
    per[hot, 0] = np.where(hot % 2 == 0, big, -big)
    if layout != REAL:
        per[hot, 1] = np.where(hot % 3 == 0, -big + 1, 7)
    return out


def _dense():
    m = np.arange(64, NS, 64)
    return np.concatenate([m - 1, m])


def _sparse(first, before, after, delta):
    """The range's ends, one hot sample inside the guard of each end, and a pair whose guards meet on the first tile boundary: the
    first one's guard ends on sample TILE - 1, the second one's begins on TILE + delta (0 touch, -1 overlap, +1 miss)."""
    h1 = TILE - 1 - after
    h2 = TILE + before + delta
    hot = [first, first + before // 2, END - 1 - after // 2, END - 1, h1, h2]
    assert first + before // 2 + after < h1 - before - 1 and h2 + after + 1 < END - 1 - after // 2 - before    # the pair stands alone
    return hot


@pytest.fixture(scope="module")
def dst_engine():
    import cu_sdr_collection_amd as P
    eng = P.Engine(0)
    yield eng
    eng.close()


def _stats(st):
    return (st.hot, st.blanked, st.runs, st.longest)


def _both_ways(engine, dst, raw, dtype, layout, first, n, threshold2, before, after, tag):
    """Out of place into a sentinel fill, then in place: both against the model, byte for byte and on every statistic."""
    total = raw.shape[0] // M.components(layout)
    want, want_st = M.excise_pulses(raw, layout, first, n, threshold2, before, after)
    engine.load_if(raw, layout=layout, fs=FS)
    dst.load_if(np.full_like(raw, 85), layout=layout)
    st = engine.excise_pulses(first, n, threshold2, before, after, dst=dst)
    got = dst.read_if(0, total, dtype=dtype, layout=layout)
    assert np.array_equal(got, want), (tag, "out of place", int(np.sum(got != want)))
    assert _stats(st) == _stats(want_st), (tag, "out of place")
    assert engine.read_if(0, total, dtype=dtype, layout=layout).tobytes() == raw.tobytes(), (tag, "the source stays as it was")
    st = engine.excise_pulses(first, n, threshold2, before, after)
    got = engine.read_if(0, total, dtype=dtype, layout=layout)
    assert np.array_equal(got, want), (tag, "in place", int(np.sum(got != want)))
    assert _stats(st) == _stats(want_st), (tag, "in place")
    return want, want_st


@pytest.mark.parametrize("before,after", PAIRS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_bytes_and_statistics_against_the_model(engine, dst_engine, fmt, before, after):
    dtype, layout = FORMATS[fmt]
    nc = M.components(layout)
    quiet = _quiet(dtype, layout, 500)
    for first in FIRSTS:
        n = END - first
        raw = _plant(quiet, dtype, layout, _dense())
        want, st = _both_ways(engine, dst_engine, raw, dtype, layout, first, n, THRESHOLD2, before, after, (fmt, before, after, first, "dense"))
        assert st.hot == int(np.sum((_dense() >= first) & (_dense() < END)))
        assert want[:nc * first].tobytes() == raw[:nc * first].tobytes() and want[nc * END:].tobytes() == raw[nc * END:].tobytes()
        seen = {}
        for kind, delta in (("touch", 0), ("overlap", -1), ("miss", 1)):
            hot = _sparse(first, before, after, delta)
            raw = _plant(quiet, dtype, layout, hot)
            _, seen[kind] = _both_ways(engine, dst_engine, raw, dtype, layout, first, n, THRESHOLD2, before, after, (fmt, before, after, first, kind))
            assert seen[kind].hot == len(set(hot))
        # one run against two, and the sample the overlap shares
        assert seen["miss"].runs == seen["touch"].runs + 1 and seen["overlap"].runs == seen["touch"].runs
        assert seen["overlap"].blanked == seen["touch"].blanked - 1 and seen["miss"].blanked == seen["touch"].blanked
        assert seen["touch"].longest == 2 * (before + after + 1) > seen["miss"].longest


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_no_hot_sample_and_every_sample_hot(engine, dst_engine, fmt):
    dtype, layout = FORMATS[fmt]
    raw = _quiet(dtype, layout, 501)
    raw[raw == 0] = 3                                                   # every sample's norm is at least 9
    for first, n in ((0, NS), (1, END - 1), (4097, 20000)):
        _, st = _both_ways(engine, dst_engine, raw, dtype, layout, first, n, 2 * QUIET * QUIET, 4096, 4096, (fmt, first, "none"))
        assert _stats(st) == (0, 0, 0, 0)
        _, st = _both_ways(engine, dst_engine, raw, dtype, layout, first, n, 1 << 40, 0, 0, (fmt, first, "none, a threshold over any norm"))
        assert _stats(st) == (0, 0, 0, 0)
        for guard in (0, 257):
            want, st = _both_ways(engine, dst_engine, raw, dtype, layout, first, n, 0, guard, guard, (fmt, first, "all"))
            assert _stats(st) == (n, n, 1, n)
            assert not want.reshape(-1, M.components(layout))[first:first + n].any()


@pytest.mark.parametrize("fmt", ["i16_iq", "i16_qi"])
def test_the_squares_are_formed_in_64_bits(engine, dst_engine, fmt):
    dtype, layout = FORMATS[fmt]
    raw = _quiet(dtype, layout, 502)
    per = raw.reshape(NS, 2)
    for h in (0, 77, TILE, NS - 1):
        per[h] = (-32768, -32768)                                       # norm 2^31: over 2^31 - 1, not over 2^31
    per[100] = (-32768, 32767)                                          # norm 2^31 - 65535: under both
    _, st = _both_ways(engine, dst_engine, raw, dtype, layout, 0, NS, (1 << 31) - 1, 0, 0, (fmt, "2^31 - 1"))
    assert _stats(st) == (4, 4, 4, 1)
    _, st = _both_ways(engine, dst_engine, raw, dtype, layout, 0, NS, 1 << 31, 0, 0, (fmt, "2^31"))
    assert _stats(st) == (0, 0, 0, 0)
    _, st = _both_ways(engine, dst_engine, raw, dtype, layout, 0, NS, (1 << 31) - 65536, 1, 1, (fmt, "2^31 - 65536"))
    assert st.hot == 5


@pytest.mark.parametrize("fmt", list(FORMATS))                         # int8 real: 13 samples in the last 16 bytes; int16 I/Q: 1
def test_a_record_that_ends_inside_16_bytes(engine, dst_engine, fmt):
    dtype, layout = FORMATS[fmt]
    n = NS - 3
    raw = _plant(_quiet(dtype, layout, 503, n), dtype, layout, [0, 5000, n - 2, n - 1])
    for first, cnt in ((0, n), (n - 1, 1), (n - 40, 40), (4097, n - 4097)):
        _both_ways(engine, dst_engine, raw, dtype, layout, first, cnt, THRESHOLD2, 16, 15, (fmt, first, cnt))


def test_a_record_attached_inside_another_allocation(engine, dst_engine):
    import cu_sdr_collection_amd as P
    dtype, layout = I8, IQ
    n = NS - 3
    whole = _plant(_quiet(dtype, layout, 504, NS + 64), dtype, layout, [16, 17, 16 + 64, 16 + TILE - 1, 16 + n - 1, 16 + n])
    owner = P.Engine(0)
    try:
        owner.load_if(whole, layout=layout, fs=FS)
        owner.synchronize()
        ptr, _ = owner.if_buffer()
        for odd in (1, 2, 16, 31):                                      # gc_attach_if takes 32-byte aligned addresses only
            with pytest.raises(P.GnssCorrError):
                engine.attach_if(ptr + odd, n, dtype, layout)
        engine.attach_if(ptr + 32, n, dtype, layout)                    # sample 16 of the owner's record is its sample 0
        raw = whole[32:32 + 2 * n]
        want, want_st = M.excise_pulses(raw, layout, 1, n - 1, THRESHOLD2, 63, 65)
        dst_engine.load_if(np.full_like(raw, 85), layout=layout)
        st = engine.excise_pulses(1, n - 1, THRESHOLD2, 63, 65, dst=dst_engine)
        assert np.array_equal(dst_engine.read_if(0, n), want) and _stats(st) == _stats(want_st)

        def held(record):
            after = owner.read_if(0, NS + 64)
            assert np.array_equal(after[32:32 + 2 * n], record)
            assert after[:32].tobytes() == whole[:32].tobytes() and after[32 + 2 * n:].tobytes() == whole[32 + 2 * n:].tobytes()   # the owner's bytes around it
        st = engine.excise_pulses(1, n - 1, THRESHOLD2, 63, 65)
        assert _stats(st) == _stats(want_st)
        held(want)
        # the other two calls that write a record 16 bytes at a time, in place on the same record
        engine.excise_bins(0, n, np.ones(8, dtype=np.float32))          # a gain of ones: the identity
        held(want)
        assert engine.cancel(engine.make_blocks(0), mode="model").shape[0] == 0   # an empty list's model: the record cleared (test_gpu_cancel.py)
        held(np.zeros_like(want))
    finally:
        engine.load_if(np.zeros(64, dtype=I8))                         # lets go of the owner's memory before it is freed
        owner.close()


def test_a_context_that_shares_the_record_works_in_place(engine):
    import cu_sdr_collection_amd as P
    dtype, layout = I16, QI
    raw = _plant(_quiet(dtype, layout, 505), dtype, layout, [3, 64, 9000, TILE, NS - 1])
    want, want_st = M.excise_pulses(raw, layout, 2, NS - 2, THRESHOLD2, 255, 1)
    with P.Engine(0) as other:
        engine.load_if(raw, layout=layout, fs=FS)
        other.share_if(engine)
        st = engine.excise_pulses(2, NS - 2, THRESHOLD2, 255, 1, dst=other)
        assert _stats(st) == _stats(want_st)
        assert np.array_equal(engine.read_if(0, NS, dtype=dtype, layout=layout), want)


def test_refusals_leave_the_destination_and_the_statistics_untouched(engine, dst_engine):
    import cu_sdr_collection_amd as P
    L = P._lib
    dtype, layout = I8, IQ
    raw = _plant(_quiet(dtype, layout, 506), dtype, layout, range(0, NS, 50))
    engine.load_if(raw, layout=layout, fs=FS)
    sentinel = np.full_like(raw, 85)
    dst_engine.load_if(sentinel, layout=layout)
    lib = L.load()

    def call(src, dst, first=0, n=NS, threshold2=THRESHOLD2, before=3, after=3, null_p=False):
        p = L.gc_excise_pulse_params(first, n, threshold2, before, after)
        st = L.gc_excise_pulse_stats(-7, -7, -7, -7)
        rc = lib.gc_excise_pulses(src, dst, None if null_p else C.byref(p), C.byref(st))
        assert rc == L.GC_OK or (st.hot, st.blanked, st.runs, st.longest) == (-7, -7, -7, -7), "statistics written by a refused call"
        return rc

    def untouched(eng=dst_engine, fill=sentinel, dt=dtype, lay=layout):
        return eng.read_if(0, fill.shape[0] // M.components(lay), dtype=dt, layout=lay).tobytes() == fill.tobytes()

    src, dst = engine._ctx, dst_engine._ctx
    invalid = [dict(null_p=True), dict(first=-1), dict(n=0), dict(n=-4), dict(threshold2=-1), dict(before=-1), dict(before=4097), dict(after=-1),
               dict(after=4097)]
    for kw in invalid:
        assert call(src, dst, **kw) == L.GC_E_INVALID and untouched(), kw
    assert call(None, dst) == L.GC_E_INVALID and untouched()
    assert call(src, None) == L.GC_E_INVALID
    for kw in (dict(first=NS - 9, n=10), dict(first=NS, n=1), dict(first=1 << 40, n=1), dict(first=1, n=(1 << 63) - 1)):
        assert call(src, dst, **kw) == L.GC_E_RANGE and untouched(), kw
    with P.Engine(0) as fresh:                                                                       # no record on either side
        assert call(fresh._ctx, dst) == L.GC_E_STATE and untouched()
        assert call(src, fresh._ctx) == L.GC_E_STATE
        assert call(fresh._ctx, dst, n=0) == L.GC_E_INVALID                                          # arguments before state
    # a destination of another sample count, dtype or layout
    for fill, dt, lay in ((np.full(2 * (NS - 1), 85, dtype=I8), I8, IQ), (np.full(2 * NS, 85, dtype=I16), I16, IQ),
                          (np.full(2 * NS, 85, dtype=I8), I8, QI), (np.full(NS, 85, dtype=I8), I8, REAL)):
        dst_engine.load_if(fill, layout=lay)
        assert call(src, dst) == L.GC_E_INVALID and untouched(fill=fill, dt=dt, lay=lay)
    # a destination that overlaps the source without being it: two records attached 32 bytes apart in one allocation
    with P.Engine(0) as big, P.Engine(0) as a, P.Engine(0) as b:
        big.load_if(np.concatenate([raw, raw[:64]]), layout=layout)
        big.synchronize()
        base, _ = big.if_buffer()
        a.attach_if(base, NS, dtype, layout)
        b.attach_if(base + 32, NS, dtype, layout)
        assert call(a._ctx, b._ctx) == L.GC_E_INVALID and call(b._ctx, a._ctx) == L.GC_E_INVALID
        assert big.read_if(0, NS + 32).tobytes() == np.concatenate([raw, raw[:64]]).tobytes()
        a.load_if(np.zeros(64, dtype=I8))
        b.load_if(np.zeros(64, dtype=I8))
    assert engine.read_if(0, NS, dtype=dtype, layout=layout).tobytes() == raw.tobytes()
    dst_engine.load_if(sentinel, layout=layout)
    assert call(src, dst, first=NS - 10, n=10) == L.GC_OK and not untouched()                        # the accepted call
    with pytest.raises(P.GnssCorrError) as e:
        engine.excise_pulses(0, NS + 1, THRESHOLD2)
    assert e.value.status == L.GC_E_RANGE


# ---- nothing else moves ------------------------------------------------------------------------------------------------------------
def test_shift_search_returns_the_same_bytes_around_an_excision(engine, dst_engine):
    import cu_sdr_collection_amd as P
    L = P._lib
    n = 72000
    rng = np.random.default_rng(507)
    iq = rng.integers(-20, 21, 2 * (n + 16)).astype(np.int8)
    codes = rng.choice(np.array([-1, 1], dtype=np.int8), (2, 1, n))
    codes[:, :, n // 2:] = 0
    engine.load_if(iq, fs=FS)
    dst_engine.load_if(np.zeros_like(iq), fs=FS)
    sp = L.gc_acq_shift_params(sampling_freq=FS, carrier_f0=20e3, carrier_step=125.0, first_sample=0, n=n, n_signals=1, n_carriers=2, n_bins=3,
                               n_arms_max=1, source=0)

    def search(between):
        engine.acq_shift_prepare(sp)
        if between:
            st = engine.excise_pulses(11, n, 500, 64, 256, dst=dst_engine)
            assert st.hot > 0
        picks = engine.acq_shift_search_batch(codes, None, L.GC_SHIFT_PICK_GLOBAL)
        assert picks is not None
        return bytes(picks)
    plain = search(False)
    assert search(True) == plain and search(False) == plain
    assert plain != bytes(len(plain))


def test_spectrum_returns_the_same_bytes_around_an_excision(engine, dst_engine):
    rng = np.random.default_rng(508)
    iq = rng.integers(-20, 21, 2 * NS).astype(np.int8)
    engine.load_if(iq, fs=FS)
    dst_engine.load_if(np.zeros_like(iq), fs=FS)

    def spectrum(between):
        first = engine.probe_psd(11, 30000, 4096, 2048, "hamming")[0].tobytes()
        if between:
            assert engine.excise_pulses(11, 30000, 500, 64, 256, dst=dst_engine).hot > 0
        counts, norm2 = engine.probe_histogram(11, 30000)
        return first, engine.probe_psd(11, 30000, 4096, 2048, "hamming")[0].tobytes(), counts.tobytes(), norm2
    plain = spectrum(False)
    assert plain[0] == plain[1]
    assert spectrum(True) == plain and spectrum(False) == plain
    # ... and the cleaned record's own histogram has nothing over the level
    assert dst_engine.probe_histogram(11, 30000)[1] <= 500


# ---- gc_excise_bins ------------------------------------------------------------------------------------------------------------------
NFFTS = [4, 16, 60, 64, 1000, 1024, 4096]
MODEL_NFFTS = [16, 1024, 4096]
TONE = 0.123                                                           # of the sampling frequency
MARGIN = 8.0                                                           # the library against the complex64 scipy pipeline on the same case
_REF = {}


def _noise_and_tone(fmt, n=NS, seed=600):
    """Gaussian noise of sigma 25 and a tone of amplitude 60 at 0.123 fs (int16: 2 500 and 6 000), rounded and clamped."""
    key = (fmt, n, seed)
    if key not in _REF:
        dtype, layout = FORMATS[fmt]
        sigma, amp = (2500.0, 6000.0) if dtype == I16 else (25.0, 60.0)
        rng = np.random.default_rng(seed)
        z = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + amp * np.exp(2j * np.pi * TONE * np.arange(n))
        _REF[key] = M.round_clamp(z, dtype, layout)
    return _REF[key]


def _gain(kind, nfft):
    if kind == "ones":
        return np.ones(nfft, dtype=np.float32)
    if kind == "notch":                                                # the tone's bin +- 2
        g = np.ones(nfft, dtype=np.float32)
        g[(int(round(TONE * nfft)) + np.arange(-2, 3)) % nfft] = 0.0
        return g
    return np.random.default_rng(601 + nfft).uniform(0.0, 2.0, nfft).astype(np.float32)


def _reference(fmt, raw, first, n, kind, nfft):
    """(float64 y of the range, ratio of the complex64 scipy pipeline, A) - computed once per case."""
    key = ("y", fmt, raw.shape[0], first, n, kind, nfft)
    if key not in _REF:
        dtype, layout = FORMATS[fmt]
        z = M.file_order(raw, layout)[first:first + n]
        g = _gain(kind, nfft)
        y = M.excise_bins(z, g)
        A = float(np.abs(raw.astype(np.float64)).max())
        y32 = M.excise_bins(z, g, single=True)
        dev = max(np.abs(y32.real - y.real).max(), np.abs(y32.imag - y.imag).max())
        _REF[key] = (y, dev / (2.0 ** -23 * A), A)
    return _REF[key]


def _excise_both_ways(engine, dst, fmt, raw, first, n, gain, tag):
    """Out of place into a sentinel fill and in place: the same bytes and values; out == clamp(rint(values)); the record outside
    the range as it was.  Returns (record after the call, values)."""
    dtype, layout = FORMATS[fmt]
    nc = M.components(layout)
    total = raw.shape[0] // nc
    engine.load_if(raw, layout=layout, fs=FS)
    dst.load_if(np.full_like(raw, 85), layout=layout)
    vals = engine.excise_bins(first, n, gain, dst=dst, values=True)
    got = dst.read_if(0, total, dtype=dtype, layout=layout)
    assert engine.read_if(0, total, dtype=dtype, layout=layout).tobytes() == raw.tobytes(), (tag, "the source stays as it was")
    assert got[:nc * first].tobytes() == raw[:nc * first].tobytes() and got[nc * (first + n):].tobytes() == raw[nc * (first + n):].tobytes(), tag
    assert vals.dtype == np.complex64 and vals.shape == (n,)
    assert np.array_equal(got[nc * first:nc * (first + n)], M.round_clamp(vals, dtype, layout)), (tag, "out == clamp(rint(values))")
    dst.load_if(np.full_like(raw, 85), layout=layout)
    assert engine.excise_bins(first, n, gain, dst=dst) is None                                      # without values: the same bytes
    assert dst.read_if(0, total, dtype=dtype, layout=layout).tobytes() == got.tobytes(), tag
    vals2 = engine.excise_bins(first, n, gain, values=True)
    assert engine.read_if(0, total, dtype=dtype, layout=layout).tobytes() == got.tobytes(), (tag, "in place")
    assert vals2.tobytes() == vals.tobytes(), (tag, "in place")
    return got, vals


def _hold_against_the_model(fmt, raw, first, n, kind, nfft, got, vals, tag, yardstick=None):
    """yardstick: the (first, n) of the case whose complex64 ratio bounds this one (None: this case's own).  The short ranges of the
    run positions take the whole record's: the largest deviation over one or a few samples of the yardstick says nothing about
    the largest over one or a few samples of the library."""
    dtype, layout = FORMATS[fmt]
    nc = M.components(layout)
    y, r_ref, A = _reference(fmt, raw, first, n, kind, nfft)
    if yardstick is not None:
        r_ref = _reference(fmt, raw, yardstick[0], yardstick[1], kind, nfft)[1]
    dev = max(np.abs(vals.real.astype(np.float64) - y.real).max(), np.abs(vals.imag.astype(np.float64) - y.imag).max())
    r = dev / (2.0 ** -23 * A)
    tol = MARGIN * r_ref * 2.0 ** -23 * A
    print(f"EXCISE bins {tag}: r = {r:.3f} (complex64 scipy pipeline {r_ref:.3f}, bound {MARGIN * r_ref:.3f}); |values - y| <= {dev:.3g} LSB")
    assert r <= MARGIN * r_ref, (tag, r, r_ref)
    want = M.round_clamp(y, dtype, layout).reshape(n, nc).astype(np.int64)
    have = got[nc * first:nc * (first + n)].reshape(n, nc).astype(np.int64)
    parts = np.stack([y.real] if layout == REAL else [y.real, y.imag], axis=1)
    near = np.abs(parts - np.floor(parts) - 0.5) <= tol                                             # within the tolerance of a half-integer
    assert np.array_equal(have[~near], want[~near]), (tag, int(np.sum((have != want) & ~near)))
    assert np.all(np.abs(have - want)[near] <= 1), tag
    # The issue caps the samples within the tolerance of a half-integer at 1 % of a case (one sample at least).  On the int8 records
    # that holds and is asserted.  On the int16 records it cannot hold for any implementation: A is 250 times larger, the tolerance
    # 0.01 - 0.03 LSB, and 2 tol of the model's own values per component - 2 to 16 % of a case - lie that near.  There the cap is
    # held on what the library can answer for: the samples that do differ.
    cap = -(-n // 100)
    near_n, differ = int(np.any(near, axis=1).sum()), int(np.any(have != want, axis=1).sum())
    print(f"EXCISE bins {tag}: {near_n} of {n} samples within {tol:.2g} LSB of a half-integer, {differ} differ by one")
    if dtype == I8:
        assert near_n <= cap, (tag, near_n)
    else:
        assert differ <= cap, (tag, differ)


@pytest.mark.parametrize("nfft", NFFTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_a_gain_of_ones_is_the_identity_and_the_model_holds(engine, dst_engine, fmt, nfft):
    raw = _noise_and_tone(fmt)
    got, vals = _excise_both_ways(engine, dst_engine, fmt, raw, 0, NS, _gain("ones", nfft), (fmt, nfft, "ones"))
    assert got.tobytes() == raw.tobytes(), (fmt, nfft, int(np.sum(got != raw)))
    if nfft in MODEL_NFFTS:
        for kind in ("notch", "random"):
            tag = (fmt, nfft, kind)
            got, vals = _excise_both_ways(engine, dst_engine, fmt, raw, 0, NS, _gain(kind, nfft), tag)
            _hold_against_the_model(fmt, raw, 0, NS, kind, nfft, got, vals, tag)
            assert got.tobytes() != raw.tobytes()


@pytest.mark.parametrize("nfft", MODEL_NFFTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_run_positions(engine, dst_engine, fmt, nfft):
    """first_sample in {0, 1, 4097} x nsamples in {1, H - 1, H, H + 1, 3 H + 7} x both gains, held against the model; and the same
    range inside a longer record gives the bytes and values of the call on the range alone: zero padding, not the neighbours."""
    dtype, layout = FORMATS[fmt]
    nc = M.components(layout)
    H = nfft // 2
    raw = _noise_and_tone(fmt)
    for kind in ("notch", "random"):
        for first in FIRSTS:
            for n in (1, H - 1, H, H + 1, 3 * H + 7):
                tag = (fmt, nfft, kind, first, n)
                got, vals = _excise_both_ways(engine, dst_engine, fmt, raw, first, n, _gain(kind, nfft), tag)
                _hold_against_the_model(fmt, raw, first, n, kind, nfft, got, vals, tag, yardstick=(0, NS))
                alone = np.ascontiguousarray(raw[nc * first:nc * (first + n)])
                got1, vals1 = _excise_both_ways(engine, dst_engine, fmt, alone, 0, n, _gain(kind, nfft), tag + ("alone",))
                assert got1.tobytes() == got[nc * first:nc * (first + n)].tobytes() and vals1.tobytes() == vals.tobytes(), tag


def test_a_record_the_shipping_budget_cuts(engine, dst_engine):
    """nfft = 4096 and (tile + 3) * 2048 samples: the segment list is cut once.  Out of place and in place give the same bytes, and
    the 8 192 samples around the cut are the bytes of a call on a sub-range that no cut touches (its ends 2 H or more from them, on
    the same segment grid)."""
    import cu_sdr_collection_amd as P
    nfft, H = 4096, 2048
    tile = P.Engine.debug_excise_tile_segments(nfft)
    n = (tile + 3) * H
    rng = np.random.default_rng(602)
    raw = rng.integers(-90, 91, 2 * n).astype(np.int8)
    g = _gain("random", nfft)
    engine.load_if(raw, fs=FS)
    dst_engine.load_if(np.zeros_like(raw))
    engine.excise_bins(0, n, g, dst=dst_engine)
    out = dst_engine.read_if(0, n)
    cut = (tile - 1) * H                                               # the first tile finishes the samples below this one
    lo, hi = cut - 6 * H, n                                            # 4 H behind the cut: the record's end
    dst_engine.load_if(np.zeros_like(raw))
    engine.excise_bins(lo, hi - lo, g, dst=dst_engine)
    sub = dst_engine.read_if(0, n)
    assert out[2 * (cut - 4096):2 * (cut + 4096)].tobytes() == sub[2 * (cut - 4096):2 * (cut + 4096)].tobytes()
    assert out[2 * (cut - 4096):2 * (cut + 4096)].tobytes() != raw[2 * (cut - 4096):2 * (cut + 4096)].tobytes()
    engine.excise_bins(0, n, g)
    assert engine.read_if(0, n).tobytes() == out.tobytes()


@pytest.mark.parametrize("layout", [IQ, QI])
def test_bin_order_is_the_spectrums(engine, dst_engine, layout):
    """A tone that is exact at bin b0 of nfft = 1024 (amplitude 100 over sigma 10), gain zero at b0 +- 2: the spectrum of the
    source has its maximum at b0, and the cleaned record has less than a hundredth of it there - a mirrored or swapped bin order
    would leave the tone where it was."""
    nfft, b0 = 1024, 137
    rng = np.random.default_rng(603)
    z = 10.0 * (rng.standard_normal(NS) + 1j * rng.standard_normal(NS)) + 100.0 * np.exp(2j * np.pi * b0 * np.arange(NS) / nfft)
    raw = M.round_clamp(z, I16, IQ)                                   # file order: c0 = re, c1 = im, whatever the context calls it
    g = np.ones(nfft, dtype=np.float32)
    g[b0 - 2:b0 + 3] = 0.0
    engine.load_if(raw, layout=layout, fs=FS)
    dst_engine.load_if(np.zeros_like(raw), layout=layout, fs=FS)
    engine.excise_bins(0, NS, g, dst=dst_engine)
    before = engine.probe_psd(0, NS, nfft, nfft // 2, "hamming")[0].reshape(-1)
    after = dst_engine.probe_psd(0, NS, nfft, nfft // 2, "hamming")[0].reshape(-1)
    assert int(np.argmax(before)) == b0
    print(f"EXCISE bin order layout {layout}: psd[b0] {before[b0]:.3g} -> {after[b0]:.3g} (ratio {after[b0] / before[b0]:.2e})")
    assert after[b0] < before[b0] / 100.0
    far = np.r_[300:1024]
    assert 0.5 < after[far].sum() / before[far].sum() < 2.0                                        # the rest of the band stays


def test_bins_refusals_leave_the_destination_and_the_values_untouched(engine, dst_engine):
    import cu_sdr_collection_amd as P
    L = P._lib
    dtype, layout = I8, IQ
    raw = _noise_and_tone("i8_iq")
    engine.load_if(raw, layout=layout, fs=FS)
    sentinel = np.full_like(raw, 85)
    dst_engine.load_if(sentinel, layout=layout)
    lib = L.load()
    fp = C.POINTER(C.c_float)

    def call(src, dst, first=0, n=NS, nfft=64, reserved=0, gain="ones", null_p=False):
        p = L.gc_excise_bins_params(first, n, nfft, reserved)
        g = None if gain is None else np.ones(max(nfft, 1), dtype=np.float32) if isinstance(gain, str) else np.ascontiguousarray(gain, dtype=np.float32)
        vals = np.full((max(min(n, NS), 1), 2), 7.5, dtype=np.float32)
        rc = lib.gc_excise_bins(src, dst, None if null_p else C.byref(p), None if g is None else g.ctypes.data_as(fp), vals.ctypes.data_as(fp))
        assert rc == L.GC_OK or np.all(vals == 7.5), "values written by a refused call"
        return rc

    def untouched(eng=dst_engine, fill=sentinel, dt=dtype, lay=layout):
        return eng.read_if(0, fill.shape[0] // M.components(lay), dtype=dt, layout=lay).tobytes() == fill.tobytes()

    src, dst = engine._ctx, dst_engine._ctx
    nan = np.ones(64)
    nan[63] = np.nan
    inf = np.ones(64)
    inf[0] = -np.inf
    for kw in (dict(null_p=True), dict(gain=None), dict(first=-1), dict(n=0), dict(n=-1), dict(nfft=2), dict(nfft=0), dict(nfft=63), dict(nfft=-4),
               dict(reserved=1), dict(gain=nan), dict(gain=inf)):
        assert call(src, dst, **kw) == L.GC_E_INVALID and untouched(), kw
    assert call(None, dst) == L.GC_E_INVALID and untouched()
    assert call(src, None) == L.GC_E_INVALID
    assert call(src, dst, nfft=14) == L.GC_E_UNSUPPORTED and untouched()                             # a prime factor of 7
    assert b"FFT size 14" in lib.gc_last_error()                                                     # ... with the planner's message
    assert call(src, dst, nfft=32736) == L.GC_E_UNSUPPORTED and untouched()
    for kw in (dict(first=NS - 9, n=10), dict(first=NS, n=1), dict(first=1 << 40, n=1)):
        assert call(src, dst, **kw) == L.GC_E_RANGE and untouched(), kw
    with P.Engine(0) as fresh:
        assert call(fresh._ctx, dst) == L.GC_E_STATE and untouched()
        assert call(src, fresh._ctx) == L.GC_E_STATE
    for fill, dt, lay in ((np.full(2 * (NS - 1), 85, dtype=I8), I8, IQ), (np.full(2 * NS, 85, dtype=I16), I16, IQ),
                          (np.full(2 * NS, 85, dtype=I8), I8, QI), (np.full(NS, 85, dtype=I8), I8, REAL)):
        dst_engine.load_if(fill, layout=lay)
        assert call(src, dst) == L.GC_E_INVALID and untouched(fill=fill, dt=dt, lay=lay)
    assert engine.read_if(0, NS, dtype=dtype, layout=layout).tobytes() == raw.tobytes()
    dst_engine.load_if(sentinel, layout=layout)
    assert call(src, dst, first=NS - 10, n=10) == L.GC_OK and not untouched()                        # the accepted call
    for bad in (np.ones(5), np.ones(2), np.ones((2, 8)), np.ones(8, dtype=complex)):
        with pytest.raises(ValueError):
            engine.excise_bins(0, NS, bad)


def test_searches_and_spectra_return_the_same_bytes_around_a_spectral_excision(engine, dst_engine):
    import cu_sdr_collection_amd as P
    L = P._lib
    n = 72000
    rng = np.random.default_rng(604)
    iq = rng.integers(-20, 21, 2 * (n + 16)).astype(np.int8)
    codes = rng.choice(np.array([-1, 1], dtype=np.int8), (2, 1, n))
    codes[:, :, n // 2:] = 0
    engine.load_if(iq, fs=FS)
    dst_engine.load_if(np.zeros_like(iq), fs=FS)
    sp = L.gc_acq_shift_params(sampling_freq=FS, carrier_f0=20e3, carrier_step=125.0, first_sample=0, n=n, n_signals=1, n_carriers=2, n_bins=3,
                               n_arms_max=1, source=0)

    def run(between):
        engine.acq_shift_prepare(sp)
        psd = engine.probe_psd(11, 36000, 4096, 2048, "hamming")[0].tobytes()
        if between:
            for nfft in (4096, 36000, 64):                             # the spectrum's length, the search's own, a short one
                engine.excise_bins(11, n, _gain("random", nfft), dst=dst_engine)
        picks = engine.acq_shift_search_batch(codes, None, L.GC_SHIFT_PICK_GLOBAL)
        assert picks is not None
        return bytes(picks), psd, engine.probe_psd(11, 36000, 4096, 2048, "hamming")[0].tobytes()
    plain = run(False)
    assert plain[1] == plain[2]
    assert run(True) == plain and run(False) == plain
    assert plain[0] != bytes(len(plain[0]))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
# Interference planted on the four-satellite scene.  The amplitudes were chosen on the CPU with the oracle's acquisition
# (oracle/gnss_oracle.py acquisition_l1ca, threshold 3.5) on the scene's first 50 ms: the clean record gives the peak metrics 5.58,
# 5.56, 5.59, 5.17 for its four PRNs and 1.50 for an absent one; with the tone and the pulses 2.84, 2.75, 2.81, 2.62 (all four lost)
# and 0.91; after the two rules of excise_interference in numpy 5.34, 5.34, 5.31, 4.92 and 1.51, the code phases the clean ones.
CW_AMP, CW_OFFSET = 35.0, 2.345e6            # a carrier 2.345 MHz above the IF
PULSE_AMP, PULSE_OFFSET = 160.0, 1.0e6       # DME-like pairs: Gaussian pulses 3.5 us wide at half amplitude, 12 us apart, 1 MHz above the IF
PAIRS_PER_SECOND = 6000
PULSE_SIGMAS, GUARD_US, BIN_FACTOR = 2.5, (4.0, 4.0), 4.0


def _interfere(iq, fs, f_if):
    n = iq.shape[0] // 2
    z = iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)
    t = np.arange(n)
    z += CW_AMP * np.exp(2j * np.pi * (f_if + CW_OFFSET) / fs * t)
    rng = np.random.default_rng(5)
    starts = np.sort(rng.integers(200, n - 600, int(PAIRS_PER_SECOND * n / fs)))
    k = np.arange(-120, 121)
    env = np.exp(-0.5 * (k / (3.5e-6 / 2.355 * fs)) ** 2)
    centres = []
    for s in starts:
        ph = rng.uniform(0, 2 * np.pi)
        for off in (0, int(round(12e-6 * fs))):
            idx = s + off + k
            z[idx] += PULSE_AMP * env * np.exp(1j * (2 * np.pi * (f_if + PULSE_OFFSET) / fs * idx + ph))
            centres.append(s + off)
    return M.round_clamp(z, I8, IQ), np.array(centres)


def test_end_to_end_on_the_four_satellite_scene(engine, dst_engine, l1ca_scene):
    """A CW tone and DME-like pulse pairs on the scene's first 50 ms: acquisition loses PRNs the clean record has; after
    receiver.excise_interference every one of them is back at the clean code phase, an absent PRN stays undetected, and every
    planted pulse lies under the blanking."""
    import copy

    import cu_sdr_collection_amd as P
    S0, sats, iq = l1ca_scene
    S = copy.copy(S0)
    fs = S.samplingFreq
    n = 50 * 18000
    clean = np.ascontiguousarray(iq[:2 * n])
    bad, centres = _interfere(clean, fs, S.IF)
    prns = [s.prn for s in sats]
    absent = next(p for p in range(1, 33) if p not in prns)
    S.acqSatelliteList = prns + [absent]
    engine.load_if(clean, fs=fs)
    ref = P.acquisition(engine, S, first_sample=0)
    assert all(ref.carrFreq[p - 1] != 0 for p in prns) and ref.carrFreq[absent - 1] == 0
    engine.load_if(bad, fs=fs)
    lost = P.acquisition(engine, S, first_sample=0)
    assert any(lost.carrFreq[p - 1] == 0 for p in prns)
    dst_engine.load_if(np.zeros_like(bad), fs=fs)
    res = P.excise_interference(engine, S, pulse_sigmas=PULSE_SIGMAS, guard_us=GUARD_US, bin_factor=BIN_FACTOR, dst=dst_engine)
    assert res.holder is dst_engine and engine.read_if(0, n).tobytes() == bad.tobytes()
    assert (res.before, res.after) == (72, 72) and res.gain.shape == (4096,) and 0 < int((res.gain == 0).sum()) < 200
    tone_bin = int(round((S.IF + CW_OFFSET) / fs * 4096))
    assert res.gain[tone_bin] == 0 and res.psd_after[tone_bin] < res.psd_before[tone_bin] / 100
    got = P.acquisition(dst_engine, S, first_sample=0)
    print(f"EXCISE scene: peakMetric clean {np.round(ref.peakMetric[[p - 1 for p in prns]], 2)}, interfered "
          f"{np.round(lost.peakMetric[[p - 1 for p in prns]], 2)}, cleaned {np.round(got.peakMetric[[p - 1 for p in prns]], 2)}; absent PRN {absent}: "
          f"{ref.peakMetric[absent - 1]:.2f}, {lost.peakMetric[absent - 1]:.2f}, {got.peakMetric[absent - 1]:.2f}; threshold2 {res.threshold2}, "
          f"stats {vars(res.stats)}, {int((res.gain == 0).sum())} bins zeroed")
    for p in prns:
        assert got.carrFreq[p - 1] != 0 and got.codePhase[p - 1] == ref.codePhase[p - 1], (p, got.codePhase[p - 1], ref.codePhase[p - 1])
    assert got.carrFreq[absent - 1] == 0
    # every planted pulse under the blanking: the pulse stage alone, with what the wrapper used - the samples within one sigma of
    # every pulse centre are zero, and the statistics count them
    dst_engine.load_if(np.zeros_like(bad), fs=fs)
    st = engine.excise_pulses(0, n, res.threshold2, res.before, res.after, dst=dst_engine)
    assert _stats(st) == _stats(res.stats)
    zero = ~dst_engine.read_if(0, n).reshape(n, 2).any(axis=1)
    covered = np.zeros(n, dtype=bool)
    for c in centres:
        covered[c - 27:c + 28] = True
    assert zero[covered].all()
    assert st.blanked >= int(covered.sum())
    assert st.blanked == int(M.blanked_mask(M.norm2(bad, IQ) > res.threshold2, res.before, res.after).sum())
