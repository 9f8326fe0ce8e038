"""gc_probe_psd and gc_probe_histogram (csrc/probe.hip) on the GPU: probeData.m's Welch spectrum and level histograms of the record.

Spectrum: against a float64 restatement written here (_welch: segments, np.hamming, np.fft.fft), which the first test - on the CPU -
shows to agree with scipy.signal.welch given the same symmetric window.  Bound, per bin, from the project's transform bound
(tests/test_gpu_acq_surfaces.py: |got - ref| <= 3e-6 * log2(n) * max|ref| per transform): with X_k the float64 transform of segment
k, m_k = max_b |X_k[b]| and d = 3e-6 * log2(nfft),
    |have - want|[b] <= sum_k (2 |X_k[b]| d m_k + d^2 m_k^2) / (K fs sum w^2);
the float32 rounding of window and product (below 2^-22 of m_k) lies inside it.  Every case prints its worst ratio.
Bit-for-bit identities: repeated calls, spans against single calls, Q/I against I/Q contexts, int16 against int8 records of the
same values, real against I/Q records with zero second components, a span carried across a tile of the library's own budget.
Histogram: exact equality with np.bincount of the clipped components.  Refusals: every status, a sentinel in every output.
Nothing else moves: acquisition and bank calls return the same bytes with a probe call in between."""
import ctypes as C

import numpy as np
import pytest

FS = 18e6
I8, I16 = np.int8, np.int16
REAL, IQ, QI = 0, 1, 2
FORMATS = {"i8_iq": (I8, IQ), "i8_qi": (I8, QI), "i8_real": (I8, REAL), "i16_iq": (I16, IQ), "i16_qi": (I16, QI), "i16_real": (I16, REAL)}
NFFTS = [2, 8, 60, 64, 1000, 1024, 4096, 32768]
FIRSTS = [0, 1, 4097]
gpu = pytest.mark.gpu


# ---- the float64 restatement -------------------------------------------------------------------------------------------------------
def _window(nfft, window):
    return np.hamming(nfft) if window == "hamming" else np.ones(nfft)


def _welch(x, fs, nfft, noverlap, window):
    """(psd, bound, K) of one span x (complex128 or float64): pwelch without detrending, two-sided, density scaling."""
    step = nfft - noverlap
    K = (x.shape[0] - noverlap) // step
    w = _window(nfft, window)
    den = K * fs * np.sum(w * w)
    d = 3e-6 * np.log2(nfft)
    segs = np.lib.stride_tricks.sliding_window_view(x, nfft)[::step][:K]
    psd, bound = np.zeros(nfft), np.zeros(nfft)
    for k0 in range(0, K, 8192):                                       # (in pieces: the tile-cut case has 131 000 segments)
        a = np.abs(np.fft.fft(segs[k0:k0 + 8192] * w, axis=1))
        m = a.max(axis=1)[:, None]
        psd += (a * a).sum(axis=0)
        bound += (2 * a * d * m + d * d * m * m).sum(axis=0)
    return psd / den, bound / den, K


def _complex(raw, layout):
    x = raw.astype(np.float64)
    return x if layout == REAL else x[0::2] + 1j * x[1::2]            # file order, whatever the layout is called


def _components(kind, n, seed):
    """[n, 2] integer components of the three records the spectrum is tried on."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":                                              # uniform full-range int8
        return rng.integers(-128, 128, (n, 2))
    if kind == "tone":                                                 # a strong tone, a DC offset, weak noise: dynamic range, no detrending
        z = 100.0 * np.exp(2j * np.pi * 0.1237 * np.arange(n)) + (9.0 - 6.0j) + 0.7 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        return np.clip(np.rint(np.stack([z.real, z.imag], axis=1)), -128, 127).astype(np.int64)
    assert kind == "full16"                                            # int16 at +-32767
    return rng.choice([-32767, 32767], (n, 2))


def _raw(comps, dtype, layout):
    return np.ascontiguousarray(comps[:, :1 if layout == REAL else 2].astype(dtype).reshape(-1))


def _check(tag, got, want, bound):
    ratio = float(np.max(np.abs(got - want) / bound))
    print(f"PROBE {tag}: worst |have - want| / bound {ratio:.3g}, relative to the largest bin {float(np.max(np.abs(got - want)) / np.max(want)):.2e}")
    assert np.all(np.abs(got - want) <= bound), tag
    return ratio


# ---- the restatement itself, on the CPU --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,noverlap,n,real", [(64, 4, 1000, False), (1000, 62, 5003, False), (60, 59, 300, True), (4096, 256, 20000, False)])
def test_restatement_agrees_with_scipy_welch(nfft, noverlap, n, real):
    from scipy.signal import welch
    comps = _components("tone", n, nfft)
    x = comps[:, 0].astype(np.float64) if real else comps[:, 0] + 1j * comps[:, 1]
    want, _, K = _welch(x, FS, nfft, noverlap, "hamming")
    _, ref = welch(x, FS, window=np.hamming(nfft), nperseg=nfft, noverlap=noverlap, nfft=nfft, detrend=False, return_onesided=False)
    assert K == (n - noverlap) // (nfft - noverlap)
    assert np.max(np.abs(want - ref)) <= 1e-12 * np.max(ref)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nfft", NFFTS)
def test_psd_matches_the_float64_restatement(engine, nfft):
    """Per length: every noverlap of {0, 1, nfft/16, nfft - 1 (short lengths)} x all six formats, and over them in turn the leftovers
    {0, 1, step - 1}, the starts {0, 1, 4097}, both windows and the three records.  Three segments per call."""
    overlaps = sorted({0, 1, nfft // 16} | ({nfft - 1} if nfft <= 64 else set()))
    seen = set()
    for i, noverlap in enumerate(overlaps):
        step = nfft - noverlap
        for j, (fmt, (dtype, layout)) in enumerate(FORMATS.items()):
            c = i * len(FORMATS) + j
            left = [0, 1, step - 1][(i + j) % 3] % step                 # (a step of 1 leaves nothing over)
            first = FIRSTS[(2 * i + j) % 3]
            window = ("hamming", "rect")[(i + j) % 2]
            kinds = ("uniform", "tone", "full16") if dtype == I16 else ("uniform", "tone")
            kind = kinds[(i + j // 2) % len(kinds)]
            nsamples = noverlap + 3 * step + left
            raw = _raw(_components(kind, first + nsamples + 3, 1000 * nfft + c), dtype, layout)
            engine.load_if(raw, layout, fs=FS)
            got, K = engine.probe_psd(first, nsamples, nfft, noverlap, window)
            want, bound, k_ref = _welch(_complex(raw, layout)[first:first + nsamples], FS, nfft, noverlap, window)
            assert K == k_ref == 3 and got.shape == (1, nfft) and got.dtype == np.float64
            _check(f"nfft={nfft} noverlap={noverlap} left={left} first={first} {fmt} {window} {kind}", got[0], want, bound)
            seen |= {("left", (i + j) % 3), ("first", first), ("win", window), ("kind", kind)}
    assert {("first", f) for f in FIRSTS} | {("left", v) for v in range(3)} <= seen and {("win", "hamming"), ("win", "rect"), ("kind", "uniform"), ("kind", "tone"), ("kind", "full16")} <= seen


@gpu
def test_debug_fft_at_32768_holds_the_transform_bound(engine):
    """The length of the reference's call is not in the acquisition's transform sweep: impulses, tones and Gaussian rows, both directions."""
    n = 32768
    rng = np.random.default_rng(32768)
    w = np.exp(2j * np.pi * np.arange(n) / n)
    places = [0, 1, n // 2, n - 1, 12345]
    imp = np.zeros((len(places), n), dtype=np.complex64)
    imp[np.arange(len(places)), places] = 1.0
    tones = np.stack([w[(m * np.arange(n)) % n] for m in places]).astype(np.complex64)
    gauss = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))).astype(np.complex64)
    worst = 0.0
    for name, xs in (("impulse", imp), ("tone", tones), ("gauss", gauss)):
        fwd = np.fft.fft(xs.astype(np.complex128), axis=1)
        bound = 3e-6 * np.max(np.abs(fwd)) * np.log2(n)
        for inverse in (False, True):
            got = engine.debug_fft(xs, inverse=inverse)
            ref = np.roll(fwd[:, ::-1], 1, axis=1) if inverse else fwd
            ratio = float(np.max(np.abs(got - ref))) / bound
            print(f"PROBE fft 32768 {name} {'inverse' if inverse else 'forward'}: worst |got - ref| / bound {ratio:.3g}")
            worst = max(worst, ratio)
    assert worst <= 1.0


# ---- bit-for-bit identities --------------------------------------------------------------------------------------------------------
@gpu
def test_same_call_same_bytes_and_spans_are_single_calls(engine):
    nfft, noverlap, nsamples, first = 1000, 62, 5003, 7
    raw = _raw(_components("uniform", first + 3 * nsamples + 1, 5), I8, IQ)
    engine.load_if(raw, IQ, fs=FS)
    three, K = engine.probe_psd(first, nsamples, nfft, noverlap, "hamming", nspans=3)
    again, _ = engine.probe_psd(first, nsamples, nfft, noverlap, "hamming", nspans=3)
    assert three.tobytes() == again.tobytes() and K == (nsamples - noverlap) // (nfft - noverlap)
    x = _complex(raw, IQ)
    for s in range(3):
        one, k1 = engine.probe_psd(first + s * nsamples, nsamples, nfft, noverlap, "hamming")
        assert k1 == K and one[0].tobytes() == three[s].tobytes(), s
        want, bound, _ = _welch(x[first + s * nsamples:first + (s + 1) * nsamples], FS, nfft, noverlap, "hamming")
        _check(f"span {s} of 3", three[s], want, bound)
    assert three[0].tobytes() != three[1].tobytes()


@gpu
def test_layouts_and_sample_types_that_hold_the_same_values_give_the_same_bytes(engine):
    nfft, noverlap, nsamples, first = 60, 3, 1000, 1
    comps = _components("tone", first + nsamples, 9)
    args = (first, nsamples, nfft, noverlap, "hamming")

    def run(dtype, layout, cc=comps):
        engine.load_if(_raw(cc, dtype, layout), layout, fs=FS)
        return engine.probe_psd(*args)[0].tobytes(), engine.probe_histogram(first, nsamples)
    psd_iq, (h_iq, m_iq) = run(I8, IQ)
    psd_qi, (h_qi, m_qi) = run(I8, QI)                                  # file order: a Q/I context reads the same bytes the same way
    assert psd_qi == psd_iq and h_qi.tobytes() == h_iq.tobytes() and m_qi == m_iq
    psd_16, (h_16, m_16) = run(I16, IQ)                                 # an int16 record holding int8 values
    assert psd_16 == psd_iq and h_16.tobytes() == h_iq.tobytes() and m_16 == m_iq
    zeroed = comps.copy()
    zeroed[:, 1] = 0
    psd_real, (h_real, m_real) = run(I8, REAL)                          # a real record is the I/Q record with zero second components
    psd_zero, (h_zero, m_zero) = run(I8, IQ, zeroed)
    assert psd_real == psd_zero and psd_real != psd_iq and m_real == m_zero
    assert h_real[0].tobytes() == h_zero[0].tobytes() and not h_real[1].any() and h_zero[1, 128] == nsamples
    assert run(I16, REAL)[0] == psd_real


@gpu
def test_more_segments_than_one_tile_of_the_shipping_budget(engine):
    """nfft = 64, noverlap = 63: one segment per sample.  A span of five segments more than the library's tile against the
    restatement, and two spans that share the second tile: the second span's accumulator is carried across the cut, bit for bit."""
    nfft, noverlap = 64, 63
    tile = engine.debug_probe_tile_segments(nfft)
    assert tile == (128 << 20) // (2 * nfft * 8)                        # the planner's own figure: two float2 rows per segment
    K = tile + 5
    nsamples = noverlap + K
    raw = _raw(_components("uniform", nsamples + 100, 64), I8, IQ)
    assert raw.nbytes < 1 << 20 and raw.shape[0] // 2 >= 1 + 2 * (noverlap + tile // 2 + 3)
    engine.load_if(raw, IQ, fs=FS)
    got, k_lib = engine.probe_psd(3, nsamples, nfft, noverlap, "hamming")
    want, bound, k_ref = _welch(_complex(raw, IQ)[3:3 + nsamples], FS, nfft, noverlap, "hamming")
    assert k_lib == k_ref == K > tile
    _check(f"tile cut, K = {K} = tile + 5", got[0], want, bound)
    half = noverlap + tile // 2 + 3                                     # two spans of tile / 2 + 3 segments: tile 1 begins inside span 1
    two, kh = engine.probe_psd(1, half, nfft, noverlap, "rect", nspans=2)
    assert tile // 2 < kh <= tile < 2 * kh
    for s in range(2):
        assert engine.probe_psd(1 + s * half, half, nfft, noverlap, "rect")[0][0].tobytes() == two[s].tobytes(), s


# ---- known answers -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nfft,k0", [(8, 2), (64, 16), (1000, 250), (4096, 1024)])
def test_a_tone_on_a_bin_and_its_conjugate(engine, nfft, k0):
    """A e^{+i 2 pi k0 n / nfft} with k0 = nfft / 4: the samples are A {1, i, -1, -i}, exact in int8.  Rectangular window: bin k0 holds
    A^2 nfft / fs, the conjugate tone's power sits in bin nfft - k0, every other bin holds nothing - all within the bound."""
    A, n = 100, 3 * nfft
    ph = (k0 * np.arange(n)) % nfft * 4 // nfft                         # quarter turns
    re, im = np.array([A, 0, -A, 0])[ph], np.array([0, A, 0, -A])[ph]
    for sign, where in ((1, k0), (-1, nfft - k0)):
        raw = _raw(np.stack([re, sign * im], axis=1), I8, IQ)
        engine.load_if(raw, IQ, fs=FS)
        got, _ = engine.probe_psd(0, n, nfft, 0, "rect")
        _, bound, _ = _welch(_complex(raw, IQ), FS, nfft, 0, "rect")
        want = np.zeros(nfft)
        want[where] = A * A * nfft / FS
        _check(f"tone nfft={nfft} bin {where}", got[0], want, bound)
        assert int(np.argmax(got[0])) == where


@gpu
@pytest.mark.parametrize("window", ["hamming", "rect"])
def test_a_constant_record_has_its_power_at_dc(engine, window):
    nfft, c = 1024, -37 + 12j
    raw = _raw(np.tile([[-37, 12]], (2 * nfft, 1)), I8, IQ)
    engine.load_if(raw, IQ, fs=FS)
    got, _ = engine.probe_psd(0, 2 * nfft, nfft, 0, window)
    w = _window(nfft, window)
    want, bound, _ = _welch(_complex(raw, IQ), FS, nfft, 0, window)
    dc = abs(c) ** 2 * np.sum(w) ** 2 / (FS * np.sum(w * w))           # no detrending: the offset stays
    assert abs(want[0] - dc) <= 1e-12 * dc and abs(got[0, 0] - dc) <= bound[0]
    _check(f"constant {window}", got[0], want, bound)


# ---- the reference's own call ------------------------------------------------------------------------------------------------------
@gpu
def test_probe_data_on_the_l1ca_scene(engine, l1ca_scene):
    import cu_sdr_collection_amd as P
    S, _, iq = l1ca_scene
    first, spc = 0, 18000
    n = 100 * spc
    engine.load_if(iq, fs=S.samplingFreq)
    r = P.probeData(engine, S, first)
    x = _complex(iq, IQ)[first:first + n]
    want, bound, K = _welch(x, S.samplingFreq, 32768, 2048, "hamming")
    assert r.nsegments == K == (n - 2048) // 30720 and r.psd.shape == (32768,)
    _check("probeData (32768, 2048, hamming) on 100 code periods", r.psd, want, bound)
    assert np.array_equal(r.freq, np.arange(32768) * (S.samplingFreq / 32768))
    assert r.timeScale.shape == r.data.shape == (9000,) and np.array_equal(r.data, x[:9000]) and r.timeScale[1] == 1 / S.samplingFreq
    assert np.array_equal(r.histCenters, np.arange(-128, 129))
    for have, v in ((r.histI, x.real), (r.histQ, x.imag)):
        assert have.dtype == np.uint64 and np.array_equal(have, np.bincount(v.astype(np.int64) + 128, minlength=257))
    assert r.dmax == np.sqrt(np.max(x.real ** 2 + x.imag ** 2)) + 1


@gpu
def test_probe_data_folds_a_real_record_to_one_side(engine):
    import cu_sdr_collection_amd as P
    S = P.initSettings()
    S.fileType = 1
    n = 100 * 18000
    raw = _raw(_components("tone", n + 5, 3), I8, REAL)
    engine.load_if(raw, REAL, fs=S.samplingFreq)
    r = P.probeData(engine, S, 5)
    x = raw[5:5 + n].astype(np.float64)
    two, bound, _ = _welch(x, S.samplingFreq, 32768, 2048, "hamming")
    want = two[:16385] * 1e6                                            # pwelch(data, ..., fs / 1e6): density per MHz, one-sided
    want[1:16384] *= 2
    lim = bound[:16385] * 1e6
    lim[1:16384] *= 2
    assert r.psd.shape == (16385,) and np.all(np.abs(r.psd - want) <= lim)
    assert np.array_equal(r.freq, np.arange(16385) * (S.samplingFreq / 1e6 / 32768)) and r.histQ is None
    assert np.array_equal(r.histI, np.bincount(raw[5:5 + n].astype(np.int64) + 128, minlength=257))
    assert r.data.dtype == np.float64 and np.array_equal(r.data, x[:9000]) and r.dmax == np.max(np.abs(x)) + 1


# ---- histogram ---------------------------------------------------------------------------------------------------------------------
N_HIST = 100004


@pytest.fixture(scope="module")
def hist_records():
    """Per sample type [N_HIST, 2] components with the end values in front: int8 -128 and 127; int16 -32768, -129, 128 and 32767."""
    rng = np.random.default_rng(257)
    c8 = rng.integers(-128, 128, (N_HIST, 2))
    c8[:3] = [[5, -7], [-128, 127], [127, -128]]
    c16 = rng.integers(-300, 301, (N_HIST, 2))
    c16[:5] = [[5, -7], [-32768, 32767], [-129, 128], [128, -129], [32767, -32768]]
    return {I8: c8, I16: c16}


@gpu
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_histogram_equals_bincount(engine, hist_records, fmt):
    dtype, layout = FORMATS[fmt]
    comps = hist_records[dtype]
    engine.load_if(_raw(comps, dtype, layout), layout)
    ncomp = 1 if layout == REAL else 2
    for first in (0, 1):
        for n in (1, 255, 256, 257, 100003):
            counts, norm2 = engine.probe_histogram(first, n)
            v = comps[first:first + n]
            assert counts.shape == (2, 257) and counts.dtype == np.uint64
            for c in range(ncomp):
                assert np.array_equal(counts[c], np.bincount(np.clip(v[:, c], -128, 128) + 128, minlength=257)), (fmt, first, n, c)
            if ncomp == 1:
                assert not counts[1].any()
            assert int(counts[0].sum()) == n
            assert norm2 == int(np.max(v[:, 0].astype(np.int64) ** 2 + (v[:, 1].astype(np.int64) ** 2 if ncomp == 2 else 0)))
    if dtype == I16:                                                    # the clamped values sit in the end bins
        counts, norm2 = engine.probe_histogram(0, 5)
        assert counts[0, 0] == 2 and counts[0, 256] == 2 and norm2 == 32768 ** 2 + (32767 ** 2 if ncomp == 2 else 0)
    else:
        counts, _ = engine.probe_histogram(0, 3)
        assert counts[0, 0] == 1 and counts[0, 255] == 1 and counts[0, 256] == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _psd_status(eng, first=0, nsamples=4096, nfft=64, noverlap=4, window=1, nspans=1, null_p=False, null_out=False, ctx=True):
    """(status, outputs untouched) of a raw gc_probe_psd call with a sentinel in every output."""
    from cu_sdr_collection_amd import _lib as L
    p = L.gc_probe_psd_params(first, nsamples, nfft, noverlap, window, nspans)
    out = np.full(max(nspans, 1) * max(nfft, 1), -777.25)
    k = C.c_int64(-777)
    rc = eng._lib.gc_probe_psd(eng._ctx if ctx else None, None if null_p else C.byref(p), None if null_out else out.ctypes.data_as(C.POINTER(C.c_double)),
                               C.byref(k))
    return rc, bool(np.all(out == -777.25)) and k.value == -777


def _hist_status(eng, first=0, n=100, null_out=False, ctx=True):
    counts = np.full((2, 257), 777, dtype=np.uint64)
    m = C.c_int64(-777)
    rc = eng._lib.gc_probe_histogram(eng._ctx if ctx else None, first, n, None if null_out else counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(m))
    return rc, bool(np.all(counts == 777)) and m.value == -777


@gpu
def test_refusals_compute_nothing_and_write_no_output(engine):
    import cu_sdr_collection_amd as P
    L = P._lib
    engine.load_if(_raw(_components("uniform", 40000, 1), I8, IQ), IQ, fs=FS)
    assert _psd_status(engine) == (L.GC_OK, False) and _hist_status(engine) == (L.GC_OK, False)
    invalid = [dict(ctx=False), dict(null_p=True), dict(null_out=True), dict(first=-1), dict(nsamples=0), dict(nspans=0), dict(nspans=-2), dict(nfft=1),
               dict(nfft=0), dict(noverlap=-1), dict(noverlap=64), dict(nsamples=63), dict(window=2), dict(window=-1)]
    for kw in invalid:
        assert _psd_status(engine, **kw) == (L.GC_E_INVALID, True), kw
    assert _psd_status(engine, nfft=7, noverlap=0) == (L.GC_E_UNSUPPORTED, True)                   # a prime factor of 7
    assert b"FFT size 7" in engine._lib.gc_last_error()                                              # ... with the planner's message
    assert _psd_status(engine, nfft=32736, nsamples=32736, noverlap=2048) == (L.GC_E_UNSUPPORTED, True)   # 2^5 3 11 31
    assert _psd_status(engine, first=40000 - 4096) == (L.GC_OK, False)                               # the last span that fits
    assert _psd_status(engine, first=40000 - 4095) == (L.GC_E_RANGE, True)
    assert _psd_status(engine, nsamples=10000, nspans=4) == (L.GC_OK, False)
    assert _psd_status(engine, nsamples=10001, nspans=4) == (L.GC_E_RANGE, True)
    assert _psd_status(engine, first=1 << 40) == (L.GC_E_RANGE, True)
    for kw in (dict(ctx=False), dict(null_out=True), dict(first=-1), dict(n=0), dict(n=-3)):
        assert _hist_status(engine, **kw) == (L.GC_E_INVALID, True), kw
    assert _hist_status(engine, first=39999, n=1) == (L.GC_OK, False)
    assert _hist_status(engine, first=39999, n=2) == (L.GC_E_RANGE, True) and _hist_status(engine, first=40000, n=1) == (L.GC_E_RANGE, True)
    with P.Engine(0) as fresh:                                                                       # no record; then a record without a sampling frequency
        assert _psd_status(fresh) == (L.GC_E_STATE, True) and _hist_status(fresh) == (L.GC_E_STATE, True)
        fresh.load_if(_raw(_components("uniform", 5000, 2), I8, IQ), IQ)
        assert _psd_status(fresh) == (L.GC_E_STATE, True)
        assert _hist_status(fresh) == (L.GC_OK, False)                                               # the histogram needs none
        fresh.set_sampling_freq(FS)
        assert _psd_status(fresh) == (L.GC_OK, False)
    with pytest.raises(ValueError):
        engine.probe_psd(0, 4096, window="hann")
    with pytest.raises(P.GnssCorrError) as e:
        engine.probe_psd(0, 4096, nfft=7, noverlap=0)
    assert e.value.status == L.GC_E_UNSUPPORTED


# ---- nothing else moves ------------------------------------------------------------------------------------------------------------
def _probe_between(engine, n):
    for nfft, noverlap in ((32768, 2048), (36000, 0), (64, 63)):        # the reference's call, the search's own length, a short one
        engine.probe_psd(11, n, nfft, noverlap, "hamming", nspans=2)
    engine.probe_histogram(11, n)


@gpu
def test_acquisition_returns_the_same_bytes_around_a_probe(engine, l1ca_scene):
    import cu_sdr_collection_amd as P
    L = P._lib
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    n = 42 * 18000
    p = P.receiver._acq_params(S, 0)
    p.source = 1
    tables = np.stack([P.codes.makeCaTable(prn, S) for prn in (sats[0].prn, sats[1].prn, 31)])

    def search(between):
        assert engine._lib.gc_acq_signal_from_record(engine._ctx, 1000, n) == L.GC_OK
        if between:
            _probe_between(engine, 200000)
        res = engine.acquire_coarse(p, tables)
        return b"".join(bytes(r) for r in res), engine.acq_conditioned(0, 4096).tobytes()
    plain = search(False)
    assert search(True) == plain and search(False) == plain
    assert plain[0] != bytes(len(plain[0]))


@gpu
def test_shift_search_returns_the_same_bytes_around_a_probe(engine):
    import cu_sdr_collection_amd as P
    L = P._lib
    n = 72000
    rng = np.random.default_rng(72)
    iq = rng.integers(-20, 21, 2 * (n + 16)).astype(np.int8)
    codes = rng.choice(np.array([-1, 1], dtype=np.int8), (2, 1, n))
    codes[:, :, n // 2:] = 0
    engine.load_if(iq, fs=FS)
    sp = L.gc_acq_shift_params(sampling_freq=FS, carrier_f0=20e3, carrier_step=125.0, first_sample=0, n=n, n_signals=1, n_carriers=2, n_bins=3,
                               n_arms_max=1, source=0)

    def search(between):
        engine.acq_shift_prepare(sp)
        if between:
            _probe_between(engine, 36000)
        picks = engine.acq_shift_search_batch(codes, None, L.GC_SHIFT_PICK_GLOBAL)
        assert picks is not None
        return bytes(picks)
    plain = search(False)
    assert search(True) == plain and search(False) == plain
    assert plain != bytes(len(plain))


@gpu
def test_bank_returns_the_same_bytes_around_a_probe(engine, l1ca_scene):
    import cu_sdr_collection_amd as P
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    code = P.codes.generateCAcode(sats[0].prn)
    engine.set_channel(0, [np.concatenate([code[-1:], code, code[:1]]).astype(np.int8)])
    b = engine.make_blocks(2)
    for k, (first, size, rem, step, f, phi) in enumerate([(1234, 17999, 0.25, 1.023e6 / 18e6, 2.1e4, 0.7), (40001, 18001, 0.0, (1.023e6 + 3.0) / 18e6, 1.9e4, -2.0)]):
        b[k].channel, b[k].first_sample, b[k].blksize, b[k].rem_code_phase, b[k].code_phase_step = 0, first, size, rem, step
        b[k].el_spacing, b[k].carr_freq, b[k].rem_carr_phase = 0.5, f, phi
    offsets = np.arange(-12, 13) / 8
    before = engine.correlate_bank(b, offsets).tobytes()
    _probe_between(engine, 100000)
    assert engine.correlate_bank(b, offsets).tobytes() == before
    assert before != bytes(len(before))
