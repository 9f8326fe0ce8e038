"""gc_excise_sweep (csrc/excise.hip) on the GPU: swept interference cut cell by cell.

Records of 40 000 samples unless stated, all six record formats, nfft in {4, 60, 64, 72, 320, 1024} - 60 and 72 have a partial last
mask word, 72 and 320 several words, 4 has 2 * 64 + 1 >= nfft - and widen in {0, 1, 64}.
1. limit = +inf: record and values byte for byte those of gc_excise_bins with the same gain (ones, notch, random; None = ones); masks,
   bin_cut and statistics zero but segments == K; out of place, in place and through a context that shares the record.
2. limit in {0, +inf} on a set Z of bins (0 and nfft - 1 together, a bin next to a word boundary): P > 0 there in every segment (from
   the returned power); record and values byte for byte gc_excise_bins with a gain of zero on the dilation of Z; hot exactly Z, cut
   exactly its dilation, in every row; the statistics and bin_cut follow.  The definition sets Y = (+0, +0) in a cut cell, where
   gc_excise_bins forms 0 * x, a zero of x's sign; an output VALUE that is an exact zero (every one of them where the dilation is
   the whole segment; a rare one at nfft = 4, where a bin's component can vanish) may therefore differ in its sign.  The values
   are held bit for bit except there: where the bits differ both values are zeros, and unless the whole segment is cut such values
   are at most 0.1 % of a case.  The record bytes are equal without exception.
3. Chirp scenes (noise sigma 8, chirp amplitude 40 from -0.4 to +0.4 fs, period 8 nfft, 180 for nfft = 64; int16: 800 and 4 000; real
   records take the real part), the limit from receiver.excise_sweep_limit on the jam-free record's power with factor 6.  Exact:
   hot == (power > limit) in float32, cut == the model's dilation of the device's hot, statistics and bin_cut == the counts of the
   device's masks, record == clamp(rint(values)), the bytes outside the range stay.  Against float64 (tests/excise_sweep_model.py)
   with the device's own cut handed to the model: values and bytes as test_gpu_excise.py holds gc_excise_bins - r = max|values - y| /
   (2^-23 A) at most 8 times the r of the complex64 scipy pipeline on the same case, bytes equal clamp(rint(y)) except within that
   tolerance of a half-integer (by one; such samples at most 1 % of a case on int8 records, the differing ones at most 1 % on int16
   records, where 2 - 16 % of the model's own values lie that near whatever computes them).  power: e = |sqrt(P) - sqrt(P64)| /
   sqrt(max_b P64_k[b]), its largest value at most 8 times the complex64 pipeline's; both printed.  Decisions: a cell where the
   device's hot differs from the float64 model's lies within that tolerance of sqrt(limit[b]), and such cells are at most 0.1 % of a
   case.
4. Run positions: first_sample in {0, 1, 4097} x nsamples in {1, H - 1, H, H + 1, 3 H + 7}; the same range alone in a record gives the
   bytes, values, power and masks of the range inside the longer record.
5. A record the shipping tile budget cuts (int8 real, more than gc_debug_excise_tile_segments(nfft) * H samples): as 3 across the cut,
   in place equals out of place.
6. Every subset of the optional outputs: the same record bytes and the same remaining outputs.
7. Refusals leave dst, out's arrays and stats untouched (sentinels); a shift search, gc_probe_psd and gc_excise_bins return the same
   bytes around a sweep call.
8. End to end on the four-satellite scene with a chirp on its first 50 ms.

Measured on an MI355X (36 chirp cases and the cut record): r of the library 0.18 .. 1.49 next to 0.18 .. 1.40 for the complex64 scipy
pipeline, the largest library / scipy of one case 1.26; the largest e 2.44e-7 next to 2.28e-7, the largest library / scipy 1.30
(both bounds are 8); no decision differs from the float64 model's in any case; samples within the tolerance of a half-integer: 0 ..
40 of 40 000 on the int8 records (at most 14 differ, at nfft 4), 24 .. 1 524 on the int16 records (1 .. 13 differ) - DESIGN.md 4.14."""
import ctypes as C
import itertools

import numpy as np
import pytest

import excise_model as M
import excise_sweep_model as SM

pytestmark = pytest.mark.gpu
FS = 18e6
NS = 40000
I8, I16 = np.int8, np.int16
REAL, IQ, QI = M.REAL, M.IQ, M.QI
FORMATS = {"i8_iq": (I8, IQ), "i8_qi": (I8, QI), "i8_real": (I8, REAL), "i16_iq": (I16, IQ), "i16_qi": (I16, QI), "i16_real": (I16, REAL)}
NFFTS = [4, 60, 64, 72, 320, 1024]
WIDENS = [0, 1, 64]
FIRSTS = [0, 1, 4097]
MARGIN = 8.0                                                           # the library against the complex64 scipy pipeline on the same case
FACTOR = 6.0
_REF = {}


@pytest.fixture(scope="module")
def dst_engine():
    import cu_sdr_collection_amd as P
    eng = P.Engine(0)
    yield eng
    eng.close()


def _period(nfft):
    return 180 if nfft == 64 else 8 * nfft


def _scene(fmt, nfft, n=NS, seed=700):
    """(jammed, jam-free) records: Gaussian noise of sigma 8 per component, and a chirp of amplitude 40 on top (int16: 800, 4 000)."""
    key = ("scene", fmt, nfft, n, seed)
    if key not in _REF:
        dtype, layout = FORMATS[fmt]
        sigma, amp = (800.0, 4000.0) if dtype == I16 else (8.0, 40.0)
        rng = np.random.default_rng(seed)
        z = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        _REF[key] = (M.round_clamp(z + SM.chirp(n, _period(nfft), amp), dtype, layout), M.round_clamp(z, dtype, layout))
    return _REF[key]


def _gain(kind, nfft):
    if kind == "ones":
        return np.ones(nfft, dtype=np.float32)
    if kind == "notch":
        g = np.ones(nfft, dtype=np.float32)
        g[(nfft // 8 + np.arange(-1, 2)) % nfft] = 0.0
        return g
    return np.random.default_rng(701 + nfft).uniform(0.0, 2.0, nfft).astype(np.float32)


def _stats(st):
    return (st.segments, st.hot, st.cut, st.segments_cut, st.most_cut)


def _same(a, b):
    """Two results of Engine.excise_sweep: every output both have, byte for byte, and the statistics."""
    assert _stats(a.stats) == _stats(b.stats)
    for name in ("values", "power", "hot", "cut", "bin_cut"):
        x, y = getattr(a, name), getattr(b, name)
        if x is not None and y is not None:
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), name
    return True


def _sweep_both_ways(engine, dst, fmt, raw, first, n, limit, widen, gain, tag):
    """Out of place into a sentinel fill, with every output, and in place: the same bytes and outputs; out == clamp(rint(values));
    the record outside the range as it was; the shapes.  Returns (record after the call, result)."""
    dtype, layout = FORMATS[fmt]
    nc = M.components(layout)
    total = raw.shape[0] // nc
    nfft = len(limit)
    K = M.segments(n, nfft)
    engine.load_if(raw, layout=layout, fs=FS)
    dst.load_if(np.full_like(raw, 85), layout=layout)
    res = engine.excise_sweep(first, n, limit, widen, gain, dst=dst, values=True, power=True, masks=True, bin_cut=True)
    got = dst.read_if(0, total, dtype=dtype, layout=layout)
    assert engine.read_if(0, total, dtype=dtype, layout=layout).tobytes() == raw.tobytes(), (tag, "the source stays as it was")
    assert got[:nc * first].tobytes() == raw[:nc * first].tobytes() and got[nc * (first + n):].tobytes() == raw[nc * (first + n):].tobytes(), tag
    assert res.values.dtype == np.complex64 and res.values.shape == (n,)
    assert res.power.dtype == np.float32 and res.power.shape == (K, nfft)
    assert res.hot.dtype == bool and res.hot.shape == (K, nfft) == res.cut.shape
    assert res.bin_cut.dtype == np.int64 and res.bin_cut.shape == (nfft,) and res.stats.segments == K
    assert np.array_equal(got[nc * first:nc * (first + n)], M.round_clamp(res.values, dtype, layout)), (tag, "out == clamp(rint(values))")
    dst.load_if(np.full_like(raw, 85), layout=layout)
    bare = engine.excise_sweep(first, n, limit, widen, gain, dst=dst)                               # no optional output: the same bytes
    assert bare.values is None and bare.power is None and bare.hot is None and bare.cut is None and bare.bin_cut is None
    assert dst.read_if(0, total, dtype=dtype, layout=layout).tobytes() == got.tobytes() and _same(bare, res), tag
    res2 = engine.excise_sweep(first, n, limit, widen, gain, values=True, power=True, masks=True, bin_cut=True)
    assert engine.read_if(0, total, dtype=dtype, layout=layout).tobytes() == got.tobytes(), (tag, "in place")
    assert _same(res2, res), (tag, "in place")
    return got, res


def _bins(engine, dst, fmt, raw, first, n, gain):
    """gc_excise_bins out of place: (record, values)."""
    dtype, layout = FORMATS[fmt]
    total = raw.shape[0] // M.components(layout)
    engine.load_if(raw, layout=layout, fs=FS)
    dst.load_if(np.full_like(raw, 85), layout=layout)
    vals = engine.excise_bins(first, n, gain, dst=dst, values=True)
    return dst.read_if(0, total, dtype=dtype, layout=layout), vals


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", NFFTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_an_infinite_limit_is_gc_excise_bins(engine, dst_engine, fmt, nfft):
    import cu_sdr_collection_amd as P
    dtype, layout = FORMATS[fmt]
    raw = _scene(fmt, nfft)[0]
    inf = np.full(nfft, np.inf, dtype=np.float32)
    K = M.segments(NS - 7, nfft)
    for i, kind in enumerate(("ones", "notch", "random")):
        widen = WIDENS[(i + NFFTS.index(nfft)) % 3]
        tag = (fmt, nfft, kind, widen)
        want, want_vals = _bins(engine, dst_engine, fmt, raw, 3, NS - 7, _gain(kind, nfft))
        got, res = _sweep_both_ways(engine, dst_engine, fmt, raw, 3, NS - 7, inf, widen, _gain(kind, nfft), tag)
        assert got.tobytes() == want.tobytes() and res.values.tobytes() == want_vals.tobytes(), tag
        assert not res.hot.any() and not res.cut.any() and not res.bin_cut.any() and _stats(res.stats) == (K, 0, 0, 0, 0), tag
        if kind == "ones":
            assert got.tobytes() == raw.tobytes(), tag
            got, res = _sweep_both_ways(engine, dst_engine, fmt, raw, 3, NS - 7, inf, widen, None, tag + ("no gain",))
            assert got.tobytes() == want.tobytes() and res.values.tobytes() == want_vals.tobytes(), tag
    with P.Engine(0) as other:                                         # a context that shares the record works in place
        engine.load_if(raw, layout=layout, fs=FS)
        other.share_if(engine)
        res = engine.excise_sweep(3, NS - 7, inf, 1, _gain("random", nfft), dst=other, values=True, masks=True)
        assert engine.read_if(0, NS, dtype=dtype, layout=layout).tobytes() == want.tobytes() and res.values.tobytes() == want_vals.tobytes()
        assert not res.hot.any() and not res.cut.any()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def _z_bins(nfft):
    """Bins 0 and nfft - 1 together, and a bin next to a word boundary (63 | 64) where the row has one."""
    return sorted({0, nfft - 1, 64 if nfft > 65 else 63 if nfft > 63 else nfft // 2})


def _power_everywhere(fmt, nfft, first, n, Z):
    """The chirp scene with P > 0 on the bins Z in every segment of the range.  On a real int8 record at nfft = 4 a bin vanishes
    wherever two pairs of samples cancel (x0 = -x3 and x1 = -x2 for bin 0: some twenty segments of 20 000), whatever the seed: a
    segment where the float64 model finds such a bin gets 1 added to the sample in its middle, until none is left."""
    key = ("power everywhere", fmt, nfft, first, n)
    if key not in _REF:
        dtype, layout = FORMATS[fmt]
        nc, H = M.components(layout), nfft // 2
        raw = _scene(fmt, nfft)[0].copy()
        for _ in range(16):
            X = SM.spectra(M.file_order(raw, layout)[first:first + n], nfft)
            empty = np.flatnonzero((SM.power(X)[:, Z] == 0).any(axis=1))
            if empty.size == 0:
                break
            raw[nc * (first + np.minimum(empty * H, n - 1))] += 1       # range sample k H: the middle of segment k (|values| <= 70: no wrap)
        else:
            raise AssertionError((fmt, nfft, "segments without power left"))
        _REF[key] = raw
    return _REF[key]


@pytest.mark.parametrize("widen", WIDENS)
@pytest.mark.parametrize("nfft", NFFTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_a_limit_of_zero_on_a_set_of_bins_cuts_exactly_its_dilation(engine, dst_engine, fmt, nfft, widen):
    Z = _z_bins(nfft)
    raw = _power_everywhere(fmt, nfft, 1, NS - 5, Z)
    hot_row = np.zeros((1, nfft), dtype=bool)
    hot_row[0, Z] = True
    cut_row = SM.dilate(hot_row, widen)[0]
    limit = np.full(nfft, np.inf, dtype=np.float32)
    limit[Z] = 0.0
    gain = np.where(cut_row, 0.0, 1.0).astype(np.float32)
    tag = (fmt, nfft, widen)
    first, n = 1, NS - 5
    K = M.segments(n, nfft)
    got, res = _sweep_both_ways(engine, dst_engine, fmt, raw, first, n, limit, widen, None, tag)
    assert (res.power[:, Z] > 0).all(), (tag, "a bin of Z without power")
    assert np.array_equal(res.hot, np.repeat(hot_row, K, axis=0)) and np.array_equal(res.cut, np.repeat(cut_row[None, :], K, axis=0)), tag
    nz, nd = len(Z), int(cut_row.sum())
    assert _stats(res.stats) == (K, K * nz, K * nd, K, nd), tag
    assert np.array_equal(res.bin_cut, np.where(cut_row, K, 0)), tag
    want, want_vals = _bins(engine, dst_engine, fmt, raw, first, n, gain)
    assert got.tobytes() == want.tobytes(), tag
    a, b = res.values.view(np.float32), want_vals.view(np.float32)
    differ = a.view(np.uint32) != b.view(np.uint32)                      # byte for byte - but for the sign of an exact zero (docstring)
    assert not a[differ].any() and not b[differ].any(), (tag, int(differ.sum()))
    if nd == nfft:
        assert not a.any() and not b.any(), tag
    else:
        print(f"SWEEP {tag}: {int(differ.sum())} of {a.size} values are zeros of the other sign")
        assert int(differ.sum()) <= a.size // 1000, tag


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def _clean_limit(engine, dst, fmt, nfft, clean, first, n):
    """receiver.excise_sweep_limit on the jam-free record's power (a call with limit = +inf)."""
    from cu_sdr_collection_amd import receiver as R
    _, layout = FORMATS[fmt]
    engine.load_if(clean, layout=layout, fs=FS)
    dst.load_if(np.zeros_like(clean), layout=layout)
    power = engine.excise_sweep(first, n, np.full(nfft, np.inf, dtype=np.float32), 0, dst=dst, power=True).power
    limit = R.excise_sweep_limit(power, FACTOR)
    assert limit.dtype == np.float32 and limit.shape == (nfft,) and np.isfinite(limit).all() and (limit > 0).all()
    return limit


def _hold_against_the_model(fmt, raw, first, n, limit, widen, got, res, tag, cells_of=None):
    """The exact checks and the float64 checks of a chirp case (docstring 3).  cells_of: rows to examine (None: all)."""
    dtype, layout = FORMATS[fmt]
    nc = M.components(layout)
    nfft = len(limit)
    # exact, from the device's own outputs
    assert np.array_equal(res.hot, res.power > limit[None, :]), (tag, "hot == (power > limit) in float32")
    assert np.array_equal(res.cut, SM.dilate(res.hot, widen)), (tag, "cut == the dilation of hot")
    want_stats, want_bin_cut = SM.counts(res.hot, res.cut)
    assert _stats(res.stats) == want_stats and np.array_equal(res.bin_cut, want_bin_cut), (tag, _stats(res.stats), want_stats)
    # float64, the device's cut handed to the model: the arithmetic alone
    z = M.file_order(raw, layout)[first:first + n]
    ref = SM.excise_sweep(z, limit, widen, cut=res.cut)
    ref32 = SM.excise_sweep(z, limit, widen, cut=res.cut, single=True)
    A = float(np.abs(raw.astype(np.float64)).max())
    y = ref.y

    def ratio(v):
        return max(np.abs(v.real.astype(np.float64) - y.real).max(), np.abs(v.imag.astype(np.float64) - y.imag).max()) / (2.0 ** -23 * A)
    r, r_ref = ratio(res.values), ratio(ref32.y)
    tol = MARGIN * r_ref * 2.0 ** -23 * A
    print(f"SWEEP {tag}: values r = {r:.3f} (complex64 scipy pipeline {r_ref:.3f}, bound {MARGIN * r_ref:.3f})")
    assert r <= MARGIN * r_ref, (tag, r, r_ref)
    want = M.round_clamp(y, dtype, layout).reshape(n, nc).astype(np.int64)
    have = got[nc * first:nc * (first + n)].reshape(n, nc).astype(np.int64)
    parts = np.stack([y.real] if layout == REAL else [y.real, y.imag], axis=1)
    near = np.abs(parts - np.floor(parts) - 0.5) <= tol                                             # within the tolerance of a half-integer
    assert np.array_equal(have[~near], want[~near]), (tag, int(np.sum((have != want) & ~near)))
    assert np.all(np.abs(have - want)[near] <= 1), tag
    cap = -(-n // 100)
    near_n, differ = int(np.any(near, axis=1).sum()), int(np.any(have != want, axis=1).sum())
    print(f"SWEEP {tag}: {near_n} of {n} samples within {tol:.2g} LSB of a half-integer, {differ} differ by one")
    if dtype == I8:
        assert near_n <= cap, (tag, near_n)
    else:
        assert differ <= cap, (tag, differ)
    # power
    root = np.sqrt(ref.power.max(axis=1, keepdims=True))
    e = (np.abs(np.sqrt(res.power.astype(np.float64)) - np.sqrt(ref.power)) / root).max()
    e_ref = (np.abs(np.sqrt(ref32.power.astype(np.float64)) - np.sqrt(ref.power)) / root).max()
    print(f"SWEEP {tag}: power e = {e:.3g} (complex64 scipy pipeline {e_ref:.3g}, bound {MARGIN * e_ref:.3g})")
    assert e <= MARGIN * e_ref, (tag, e, e_ref)
    # decisions
    differ = res.hot != ref.hot
    dist = np.abs(np.sqrt(ref.power) - np.sqrt(limit.astype(np.float64))[None, :]) / root
    cells = res.hot.size
    print(f"SWEEP {tag}: {int(differ.sum())} of {cells} decisions differ from float64's; {int(res.hot.sum())} hot, {int(res.cut.sum())} cut "
          f"({100.0 * res.cut.mean():.1f} %); complex64 pipeline differs in {int((ref32.hot != ref.hot).sum())}")
    assert (dist[differ] <= MARGIN * e_ref).all(), (tag, float(dist[differ].max()))
    assert int(differ.sum()) <= cells // 1000, (tag, int(differ.sum()))
    return ref


@pytest.mark.parametrize("nfft", NFFTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_chirp_scenes_against_the_model(engine, dst_engine, fmt, nfft):
    dtype, layout = FORMATS[fmt]
    raw, clean = _scene(fmt, nfft)
    first, n, widen = 2, NS - 9, 1
    limit = _clean_limit(engine, dst_engine, fmt, nfft, clean, first, n)
    tag = (fmt, nfft)
    got, res = _sweep_both_ways(engine, dst_engine, fmt, raw, first, n, limit, widen, None, tag)
    _hold_against_the_model(fmt, raw, first, n, limit, widen, got, res, tag)
    if nfft > 4:                                                        # the chirp goes out: a jammer 11 dB over the noise, the noise stays
        z0, z1, zc = (M.file_order(r, layout)[first:first + n] for r in (raw, got, clean))
        p0, p1, pc = (float(np.mean(np.abs(v) ** 2)) for v in (z0, z1, zc))
        print(f"SWEEP {tag}: mean |z|^2 {p0:.4g} -> {p1:.4g} (jam-free {pc:.4g}), |y - jam-free|^2 {float(np.mean(np.abs(z1 - zc) ** 2)):.4g}")
        assert res.stats.cut > 0 and p1 < p0


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", NFFTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_run_positions(engine, dst_engine, fmt, nfft):
    """The same range alone in a record gives the bytes, values, power and masks of the range inside the longer record: zero padding,
    not the neighbours; and the exact checks at every position."""
    from cu_sdr_collection_amd import receiver as R
    dtype, layout = FORMATS[fmt]
    nc = M.components(layout)
    H = nfft // 2
    raw, clean = _scene(fmt, nfft)
    limit = _clean_limit(engine, dst_engine, fmt, nfft, clean, 0, NS)
    widen = WIDENS[NFFTS.index(nfft) % 3]
    cut_cells = 0
    for first in FIRSTS:
        for n in (1, H - 1, H, H + 1, 3 * H + 7):
            tag = (fmt, nfft, first, n)
            got, res = _sweep_both_ways(engine, dst_engine, fmt, raw, first, n, limit, widen, None, tag)
            assert np.array_equal(res.hot, res.power > limit[None, :]) and np.array_equal(res.cut, SM.dilate(res.hot, widen)), tag
            want_stats, want_bin_cut = SM.counts(res.hot, res.cut)
            assert _stats(res.stats) == want_stats and np.array_equal(res.bin_cut, want_bin_cut), tag
            alone = np.ascontiguousarray(raw[nc * first:nc * (first + n)])
            got1, res1 = _sweep_both_ways(engine, dst_engine, fmt, alone, 0, n, limit, widen, None, tag + ("alone",))
            assert got1.tobytes() == got[nc * first:nc * (first + n)].tobytes() and _same(res1, res), tag
            cut_cells += res.stats.cut
    assert cut_cells > 0 or nfft == 4


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_a_record_the_shipping_budget_cuts(engine, dst_engine):
    """nfft = 1024 and (tile + 3) * 512 samples of int8 real data: the segment list is cut once.  Masks, power and bytes are held as
    in the chirp scenes, across the cut; in place equals out of place (_sweep_both_ways); and the rows around the cut are those of
    a call on a sub-range that no cut touches."""
    import cu_sdr_collection_amd as P
    fmt, nfft, H, widen = "i8_real", 1024, 512, 1
    tile = P.Engine.debug_excise_tile_segments(nfft)
    n = (tile + 3) * H
    assert n > tile * H and M.segments(n, nfft) > tile
    raw, clean = _scene(fmt, nfft, n=n, seed=702)
    limit = _clean_limit(engine, dst_engine, fmt, nfft, clean[:NS], 0, NS)
    got, res = _sweep_both_ways(engine, dst_engine, fmt, raw, 0, n, limit, widen, None, ("cut", nfft))
    _hold_against_the_model(fmt, raw, 0, n, limit, widen, got, res, ("cut", nfft))
    assert res.cut[tile - 2:tile + 2].any() and res.stats.segments == tile + 4
    lo = (tile - 7) * H                                                 # a sub-range on the same segment grid, its ends 2 H or more from the rows compared
    engine.load_if(raw, layout=REAL, fs=FS)
    dst_engine.load_if(np.zeros_like(raw), layout=REAL)
    sub = engine.excise_sweep(lo, n - lo, limit, widen, dst=dst_engine, power=True, masks=True)
    k0 = lo // H                                                        # row k of the sub-range is row k0 + k of the whole
    rows = slice(tile - 4, tile + 2)
    sub_rows = slice(tile - 4 - k0, tile + 2 - k0)
    assert res.power[rows].tobytes() == sub.power[sub_rows].tobytes() and np.array_equal(res.hot[rows], sub.hot[sub_rows]) and \
        np.array_equal(res.cut[rows], sub.cut[sub_rows])
    edge = (tile - 1) * H                                               # the first tile finishes the samples below this one
    assert dst_engine.read_if(0, n, dtype=I8, layout=REAL)[edge - 2 * H:edge + 2 * H].tobytes() == got[edge - 2 * H:edge + 2 * H].tobytes()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_every_subset_of_the_optional_outputs(engine, dst_engine):
    fmt, nfft, widen = "i8_iq", 72, 1
    dtype, layout = FORMATS[fmt]
    raw, clean = _scene(fmt, nfft)
    limit = _clean_limit(engine, dst_engine, fmt, nfft, clean, 0, NS)
    got, full = _sweep_both_ways(engine, dst_engine, fmt, raw, 5, NS - 11, limit, widen, _gain("random", nfft), ("subsets",))
    assert full.stats.cut > 0
    names = ("values", "power", "masks", "bin_cut")
    for r in range(len(names) + 1):
        for subset in itertools.combinations(names, r):
            dst_engine.load_if(np.full_like(raw, 85), layout=layout)
            engine.load_if(raw, layout=layout, fs=FS)
            res = engine.excise_sweep(5, NS - 11, limit, widen, _gain("random", nfft), dst=dst_engine, **{k: True for k in subset})
            assert dst_engine.read_if(0, NS, dtype=dtype, layout=layout).tobytes() == got.tobytes(), subset
            assert _same(res, full), subset
            for k in names:
                present = [getattr(res, a) is not None for a in (("hot", "cut") if k == "masks" else (k,))]
                assert all(present) if k in subset else not any(present), (subset, k)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_the_arrays_and_the_statistics_untouched(engine, dst_engine):
    import cu_sdr_collection_amd as P
    L = P._lib
    dtype, layout = I8, IQ
    raw = _scene("i8_iq", 64)[0]
    engine.load_if(raw, layout=layout, fs=FS)
    sentinel = np.full_like(raw, 85)
    dst_engine.load_if(sentinel, layout=layout)
    lib = L.load()
    fp, up, ip = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)

    def call(src, dst, first=0, n=NS, nfft=64, widen=1, limit="ones", gain=None, null_p=False, null_out=False):
        p = L.gc_excise_sweep_params(first, n, nfft, widen)
        lim = None if limit is None else np.full(max(nfft, 1), 100.0, dtype=np.float32) if isinstance(limit, str) else np.ascontiguousarray(limit, dtype=np.float32)
        g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float32)
        rows, cols = max(min(n, NS), 1) // max(nfft // 2, 1) + 3, max(nfft, 1)
        vals = np.full((max(min(n, NS), 1), 2), 7.5, dtype=np.float32)
        power = np.full((rows, cols), 7.5, dtype=np.float32)
        hot, cut = np.full((rows, (cols + 63) // 64), 7, dtype=np.uint64), np.full((rows, (cols + 63) // 64), 7, dtype=np.uint64)
        bin_cut = np.full(cols, -7, dtype=np.int64)
        out = L.gc_excise_sweep_out(vals.ctypes.data_as(fp), power.ctypes.data_as(fp), hot.ctypes.data_as(up), cut.ctypes.data_as(up), bin_cut.ctypes.data_as(ip))
        st = L.gc_excise_sweep_stats(-7, -7, -7, -7, -7)
        rc = lib.gc_excise_sweep(src, dst, None if null_p else C.byref(p), None if lim is None else lim.ctypes.data_as(fp),
                                 None if g is None else g.ctypes.data_as(fp), None if null_out else C.byref(out), C.byref(st))
        if rc != L.GC_OK:
            assert np.all(vals == 7.5) and np.all(power == 7.5) and np.all(hot == 7) and np.all(cut == 7) and np.all(bin_cut == -7), "arrays written by a refused call"
            assert (st.segments, st.hot, st.cut, st.segments_cut, st.most_cut) == (-7,) * 5, "statistics written by a refused call"
        return rc

    def untouched(eng=dst_engine, fill=sentinel, dt=dtype, lay=layout):
        return eng.read_if(0, fill.shape[0] // M.components(lay), dtype=dt, layout=lay).tobytes() == fill.tobytes()

    src, dst = engine._ctx, dst_engine._ctx
    nan, neg, ginf = np.full(64, 100.0), np.full(64, 100.0), np.ones(64)
    nan[63], neg[0], ginf[5] = np.nan, -1.0, np.inf
    for kw in (dict(null_p=True), dict(limit=None), dict(first=-1), dict(n=0), dict(n=-1), dict(nfft=2), dict(nfft=0), dict(nfft=63), dict(nfft=-4),
               dict(widen=-1), dict(widen=65), dict(limit=nan), dict(limit=neg), dict(gain=ginf), dict(gain=np.full(64, np.nan))):
        assert call(src, dst, **kw) == L.GC_E_INVALID and untouched(), kw
    assert call(None, dst) == L.GC_E_INVALID and untouched()
    assert call(src, None) == L.GC_E_INVALID
    assert call(src, dst, nfft=14) == L.GC_E_UNSUPPORTED and untouched()                             # a prime factor of 7
    assert call(src, dst, nfft=32736) == L.GC_E_UNSUPPORTED and untouched()
    for kw in (dict(first=NS - 9, n=10), dict(first=NS, n=1), dict(first=1 << 40, n=1)):
        assert call(src, dst, **kw) == L.GC_E_RANGE and untouched(), kw
    with P.Engine(0) as fresh:
        assert call(fresh._ctx, dst) == L.GC_E_STATE and untouched()
        assert call(src, fresh._ctx) == L.GC_E_STATE
        assert call(fresh._ctx, dst, widen=65) == L.GC_E_INVALID                                     # arguments before state
    for fill, dt, lay in ((np.full(2 * (NS - 1), 85, dtype=I8), I8, IQ), (np.full(2 * NS, 85, dtype=I16), I16, IQ),
                          (np.full(2 * NS, 85, dtype=I8), I8, QI), (np.full(NS, 85, dtype=I8), I8, REAL)):
        dst_engine.load_if(fill, layout=lay)
        assert call(src, dst) == L.GC_E_INVALID and untouched(fill=fill, dt=dt, lay=lay)
    assert engine.read_if(0, NS, dtype=dtype, layout=layout).tobytes() == raw.tobytes()
    dst_engine.load_if(sentinel, layout=layout)
    for kw in (dict(first=NS - 10, n=10), dict(widen=0), dict(widen=64), dict(limit=np.full(64, np.inf)), dict(limit=np.zeros(64)), dict(null_out=True),
               dict(gain=np.full(64, -2.0))):
        dst_engine.load_if(sentinel, layout=layout)
        assert call(src, dst, **kw) == L.GC_OK and not untouched(), kw                               # the accepted calls
    with pytest.raises(P.GnssCorrError) as e:
        engine.excise_sweep(0, NS + 1, np.ones(64))
    assert e.value.status == L.GC_E_RANGE


def test_searches_spectra_and_the_static_excision_return_the_same_bytes_around_a_sweep(engine, dst_engine):
    import cu_sdr_collection_amd as P
    L = P._lib
    n = 72000
    rng = np.random.default_rng(704)
    iq = rng.integers(-20, 21, 2 * (n + 16)).astype(np.int8)
    codes = rng.choice(np.array([-1, 1], dtype=np.int8), (2, 1, n))
    codes[:, :, n // 2:] = 0
    engine.load_if(iq, fs=FS)
    sp = L.gc_acq_shift_params(sampling_freq=FS, carrier_f0=20e3, carrier_step=125.0, first_sample=0, n=n, n_signals=1, n_carriers=2, n_bins=3,
                               n_arms_max=1, source=0)
    g = _gain("random", 4096)

    def run(between):
        dst_engine.load_if(np.zeros_like(iq), fs=FS)
        engine.acq_shift_prepare(sp)
        psd = engine.probe_psd(11, 36000, 4096, 2048, "hamming")[0].tobytes()
        engine.excise_bins(11, n, g, dst=dst_engine)
        static = dst_engine.read_if(0, n + 16).tobytes()
        if between:
            for nfft in (4096, 36000, 64):                             # the spectrum's and the static excision's length, the search's own, a short one
                res = engine.excise_sweep(11, n, np.full(nfft, 4.0 * nfft * 270.0, dtype=np.float32), 1, dst=dst_engine, masks=True, power=True)
                assert res.stats.hot > 0
        picks = engine.acq_shift_search_batch(codes, None, L.GC_SHIFT_PICK_GLOBAL)
        assert picks is not None
        engine.excise_bins(11, n, g, dst=dst_engine)
        return bytes(picks), psd, engine.probe_psd(11, 36000, 4096, 2048, "hamming")[0].tobytes(), static, dst_engine.read_if(0, n + 16).tobytes()
    plain = run(False)
    assert plain[1] == plain[2] and plain[3] == plain[4]
    assert run(True) == plain and run(False) == plain
    assert plain[0] != bytes(len(plain[0]))


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
# A chirp on the four-satellite scene's first 50 ms: -0.4 fs to +0.4 fs in CHIRP_PERIOD samples (0.46 ms at 18 Msps: the lines of its
# spectrum lie closer than the bins of excise_interference's 4 096-point spectrum, which shows a plateau over 80 % of the band and
# no line; at 180 samples the lines are 100 kHz apart and a comb of static notches brings every PRN back).  CHIRP_AMP was chosen on
# an MI355X: the smallest amplitude, in steps of 5, at which acquisition on the interfered record loses at least one of the four
# PRNs (30 keeps all four, 35 loses three).  peakMetric of the four PRNs and of the absent one, measured there:
#   clean                                   5.58  5.56  5.59  5.17   1.50
#   interfered                              3.33  3.68  3.41  3.26   1.58    (three lost)
#   excise_interference(bin_factor=4.0)     3.33  3.68  3.41  3.26   1.58    (no bin over 4 x the median: nothing notched)
#   excise_swept                            5.26  5.22  5.27  4.81   1.44    (126 188 of 1 800 064 cells cut)
# mean |z|^2: clean 805, interfered 2 029, cleaned 730.
CHIRP_AMP, CHIRP_PERIOD = 35.0, 8192


def _chirp_on(iq, amp, period=CHIRP_PERIOD):
    n = iq.shape[0] // 2
    z = iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)
    return M.round_clamp(z + SM.chirp(n, period, amp), I8, IQ)


def test_end_to_end_on_the_four_satellite_scene(engine, dst_engine, l1ca_scene):
    """Acquisition loses PRNs the clean record has; receiver.excise_interference(bin_factor=4.0) alone does not bring every one of
    them back; after receiver.excise_swept every PRN is back at the clean code phase, the absent PRN stays undetected, and the
    cleaned record's mean |z|^2 is below the interfered record's and within 25 % of the clean record's."""
    import copy

    import cu_sdr_collection_amd as P
    S0, sats, iq = l1ca_scene
    S = copy.copy(S0)
    fs = S.samplingFreq
    n = 50 * 18000
    clean = np.ascontiguousarray(iq[:2 * n])
    bad = _chirp_on(clean, CHIRP_AMP)
    prns = [s.prn for s in sats]
    absent = next(p for p in range(1, 33) if p not in prns)
    S.acqSatelliteList = prns + [absent]
    engine.load_if(clean, fs=fs)
    ref = P.acquisition(engine, S, first_sample=0)
    assert all(ref.carrFreq[p - 1] != 0 for p in prns) and ref.carrFreq[absent - 1] == 0
    engine.load_if(bad, fs=fs)
    lost = P.acquisition(engine, S, first_sample=0)
    gone = [p for p in prns if lost.carrFreq[p - 1] == 0]
    assert gone
    dst_engine.load_if(np.zeros_like(bad), fs=fs)
    static = P.excise_interference(engine, S, bin_factor=4.0, dst=dst_engine)
    notch = P.acquisition(static.holder, S, first_sample=0)
    assert any(notch.carrFreq[p - 1] == 0 or notch.codePhase[p - 1] != ref.codePhase[p - 1] for p in gone)
    assert engine.read_if(0, n).tobytes() == bad.tobytes()
    dst_engine.load_if(np.zeros_like(bad), fs=fs)
    holder, limit, stats, bin_cut = P.excise_swept(engine, S, dst=dst_engine)
    assert holder is dst_engine and engine.read_if(0, n).tobytes() == bad.tobytes()
    assert limit.dtype == np.float32 and limit.shape == (64,) and stats.segments == n // 32 + 1 and 0 < stats.cut < stats.segments * 64 // 2
    assert bin_cut.shape == (64,) and int(bin_cut.sum()) == stats.cut
    got = P.acquisition(dst_engine, S, first_sample=0)
    idx = [p - 1 for p in prns]
    print(f"SWEEP scene (amplitude {CHIRP_AMP}, period {CHIRP_PERIOD}): peakMetric clean {np.round(ref.peakMetric[idx], 2)}, interfered "
          f"{np.round(lost.peakMetric[idx], 2)}, static notch {np.round(notch.peakMetric[idx], 2)}, swept {np.round(got.peakMetric[idx], 2)}; absent PRN "
          f"{absent}: {ref.peakMetric[absent - 1]:.2f}, {lost.peakMetric[absent - 1]:.2f}, {got.peakMetric[absent - 1]:.2f}; stats {vars(stats)}")
    for p in prns:
        assert got.carrFreq[p - 1] != 0 and got.codePhase[p - 1] == ref.codePhase[p - 1], (p, got.codePhase[p - 1], ref.codePhase[p - 1])
    assert got.carrFreq[absent - 1] == 0
    power = [float(np.mean(np.abs(M.file_order(r, IQ)) ** 2)) for r in (clean, bad, dst_engine.read_if(0, n))]
    print(f"SWEEP scene: mean |z|^2 clean {power[0]:.4g}, interfered {power[1]:.4g}, cleaned {power[2]:.4g}")
    assert power[2] < power[1] and abs(power[2] - power[0]) <= 0.25 * power[0]
