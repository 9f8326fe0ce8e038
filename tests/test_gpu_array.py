"""gc_array_covariance and gc_array_combine (csrc/array.hip) on the GPU against the numpy model of the definitions
(tests/array_model.py).  The covariance is integers: every returned number equals the model's.  The combine has no sincos: every byte
and both statistics equal the model's, with no near-rounding allowance.

1. Covariance: every number over the six formats, K in {1, 2, 3, 8} and L in {1, 2, 32}; first_sample on every residue of a 16-byte
   vector and below L - 1; ranges of one sample, one tile, one tile +- 1 and a record's end inside a 16-byte vector; the overflow
   corners; additivity, repeatability, lag 0, a repeated context.
2. Combine: six source formats into six destination formats over (K, T) in {(1, 1), (2, 3), (4, 7), (8, 32)} with a gain that clips
   about 1 % of the components; tile edges on every residue; untouched bytes; pieces join; K = 1 against gc_downconvert.
3. Refusals leave cov, dst and res untouched.
4. End to end: a jammed four-element array through receiver.null_steer and the library's acquisition."""
import copy
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import array_model as M

pytestmark = pytest.mark.gpu
NS = 40000
I8, I16 = np.int8, np.int16
REAL, IQ, QI = M.REAL, M.IQ, M.QI
FORMATS = {"i8_iq": (I8, IQ), "i8_qi": (I8, QI), "i8_real": (I8, REAL), "i16_iq": (I16, IQ), "i16_qi": (I16, QI), "i16_real": (I16, REAL)}
PAD_FRONT, PAD_BACK = 7, 9                 # sentinel samples of dst in front of and behind the written range
SENTINEL = 85
KT = [(1, 1), (2, 3), (4, 7), (8, 32)]


def _comps(layout):
    return 1 if layout == REAL else 2


def _bps(dtype, layout):
    return _comps(layout) * np.dtype(dtype).itemsize


def _full_range(dtype, layout, seed, n=NS):
    """Values over the dtype's whole range, the two ends planted next to each other and at both ends of the record."""
    info = np.iinfo(dtype)
    raw = np.random.default_rng(seed).integers(info.min, info.max + 1, n * _comps(layout)).astype(dtype)
    raw[:4] = [info.min, info.min, info.max, info.max]
    raw[-4:] = [info.max, info.min, info.min, info.max]
    raw[1000:1008] = info.min
    raw[2000:2008] = info.max
    return raw


@pytest.fixture(scope="module")
def engines():
    """Eight source engines and a destination on device 0"""
    import cu_sdr_collection_amd as P
    made = [P.Engine(0) for _ in range(9)]
    yield made[:8], made[8]
    for e in made:
        e.close()


def _load(srcs, raws, layout):
    for e, r in zip(srcs, raws):
        e.load_if(r, layout=layout)


@pytest.fixture(scope="module")
def records():
    """Eight full-range records per format, made once and left unchanged"""
    return {name: [_full_range(dt, lay, 900 + 10 * k + len(name)) for k in range(8)] for name, (dt, lay) in FORMATS.items()}


# ---- 1. covariance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_covariance_every_number_of_the_model(engines, records, fmt):
    """Would catch: a sample left out or taken twice at a tile edge, a lagged sample in front of sample 0 that is not zero, a swapped
    pair, a conjugate on the wrong side, an accumulator that wraps, a wave reduction that mixes two outputs, a slot that is not added."""
    import cu_sdr_collection_amd as P
    srcs, _ = engines
    dt, lay = FORMATS[fmt]
    raws = records[fmt]
    _load(srcs, raws, lay)
    for K in (1, 2, 3, 8):
        want = M.covariance(raws[:K], lay, 0, NS, 32)                      # lags 0 .. 31 once: fewer lags are its first rows
        for L in (1, 2, 32):
            got = P.Engine.array_covariance(srcs[:K], 0, NS, L)
            assert got.dtype == np.int64 and got.shape == (L, K, K, 2)
            assert np.array_equal(got, want[:L]), (fmt, K, L)
    assert np.any(want[31, 7, 0] != 0)


@pytest.mark.parametrize("fmt", ["i8_real", "i16_iq", "i8_qi"])
def test_covariance_first_sample_on_every_residue_and_inside_the_zero_history(engines, records, fmt):
    """Would catch: a staged span one vector short when it starts late in a vector, an LDS offset that ignores the span's start
    inside its first vector, a lead-in in front of sample 0 that reads the record."""
    import cu_sdr_collection_amd as P
    srcs, _ = engines
    dt, lay = FORMATS[fmt]
    raws = records[fmt][:2]
    _load(srcs, raws, lay)
    L, n = 4, 3000
    residues = set()
    for first in range(0, 20):                                             # 0, 1, 2 < L - 1: zeros in front of sample 0
        residues.add(((first - (L - 1)) * _bps(dt, lay)) % 16)
        assert np.array_equal(P.Engine.array_covariance(srcs[:2], first, n, L), M.covariance(raws, lay, first, n, L)), (fmt, first)
    assert residues == set(range(0, 16, math.gcd(16, _bps(dt, lay))))


@pytest.mark.parametrize("fmt", ["i8_iq", "i16_real"])
def test_covariance_ranges_of_one_sample_one_tile_and_a_record_that_ends_inside_16_bytes(engines, records, fmt):
    """Would catch: a last tile of one sample that stages nothing, a tile count off by one, the byte path of the record's partial last
    vector reading too little or too much."""
    import cu_sdr_collection_amd as P
    srcs, _ = engines
    dt, lay = FORMATS[fmt]
    K, L = 3, 5
    tile = P.Engine.debug_array_tile_outputs(K, L)
    assert 2 <= tile and 2 * tile + 2 < NS
    ns = NS - 3                                                            # 2 (NS - 3) bytes of int8 pairs or int16: no multiple of 16
    assert (ns * _bps(dt, lay)) % 16 != 0
    raws = [r[:ns * _comps(lay)] for r in records[fmt][:K]]
    _load(srcs, raws, lay)
    for first, n in ((0, 1), (17, 1), (ns - 1, 1), (0, tile), (3, tile - 1), (3, tile), (3, tile + 1), (5, 2 * tile + 1), (ns - tile - 1, tile + 1), (ns - 7, 7),
                     (0, ns)):
        assert np.array_equal(P.Engine.array_covariance(srcs[:K], first, n, L), M.covariance(raws, lay, first, n, L)), (fmt, first, n)


def test_covariance_overflow_corners(engines):
    """Every component at the dtype's most negative value: sums that no int32 accumulator (int16) and no float32 path (both) survives.
    The expected values are Python integers: lag 0 sums n products pairs of 2 v^2, lag 1 one fewer (x[-1] = 0); the imaginary parts
    cancel term by term."""
    import cu_sdr_collection_amd as P
    srcs, _ = engines
    for dtype, v, n in ((I8, -128, NS), (I16, -32768, 1 << 21)):
        for lay in (IQ, REAL):
            raw = np.full(n * _comps(lay), v, dtype=dtype)
            _load(srcs[:2], [raw, raw], lay)
            got = P.Engine.array_covariance(srcs[:2], 0, n, 2)
            per = _comps(lay) * v * v
            for a in range(2):
                for b in range(2):
                    assert [int(x) for x in got[0, a, b]] == [n * per, 0] and [int(x) for x in got[1, a, b]] == [(n - 1) * per, 0], (dtype, lay, a, b)
    assert (1 << 21) * 2 * 32768 ** 2 == 1 << 52 and NS * 2 * 128 ** 2 > 1 << 24      # past int32 and float32's integers; past float32's
    # the most negative against the most positive, int16 I/Q: the most negative sum
    lo, hi = np.full(2 << 21, -32768, dtype=I16), np.full(2 << 21, 32767, dtype=I16)
    _load(srcs[:2], [lo, hi], IQ)
    got = P.Engine.array_covariance(srcs[:2], 0, 1 << 21, 1)
    assert [int(x) for x in got[0, 0, 1]] == [(1 << 21) * 2 * -32768 * 32767, 0] and [int(x) for x in got[0, 1, 1]] == [(1 << 21) * 2 * 32767 ** 2, 0]
    for e in srcs[:2]:
        e.load_if(np.zeros(64, dtype=I8))                                  # give the 8 MB back


def test_covariance_adds_up_repeats_and_lag_zero_is_hermitian(engines, records):
    """Would catch: a range whose first lagged samples are taken as zero instead of the record's own, a result that depends on the
    order the workgroups finish in, a lag-0 matrix that is not Hermitian, a diagonal that is not the record's sum of squares."""
    import cu_sdr_collection_amd as P
    srcs, _ = engines
    raws = records["i8_iq"][:4]
    _load(srcs, raws, IQ)
    K, L = 4, 8
    tile = P.Engine.debug_array_tile_outputs(K, L)
    first, n = 11, 3 * tile + 500
    whole = P.Engine.array_covariance(srcs[:K], first, n, L)
    again = P.Engine.array_covariance(srcs[:K], first, n, L)
    assert np.array_equal(whole, again)
    a, b = 777, 2 * tile
    parts = [P.Engine.array_covariance(srcs[:K], first + lo, hi - lo, L) for lo, hi in ((0, a), (a, b), (b, n))]
    assert np.array_equal(parts[0] + parts[1] + parts[2], whole)
    assert np.array_equal(whole[0, :, :, 0], whole[0, :, :, 0].T) and np.array_equal(whole[0, :, :, 1], -whole[0, :, :, 1].T)
    v2 = np.arange(-128, 129, dtype=np.int64) ** 2
    for k in range(K):
        counts, _ = srcs[k].probe_histogram(first, n)
        assert int(whole[0, k, k, 0]) == int(np.sum(v2 * counts[0].astype(np.int64)) + np.sum(v2 * counts[1].astype(np.int64))) > 0
        assert int(whole[0, k, k, 1]) == 0


def test_covariance_of_a_context_given_twice(engines, records):
    """Would catch: per-record state keyed by the context instead of the position in srcs."""
    import cu_sdr_collection_amd as P
    srcs, _ = engines
    raws = records["i16_qi"][:2]
    _load(srcs, raws, QI)
    got = P.Engine.array_covariance([srcs[0], srcs[1], srcs[0]], 5, 9000, 3)
    assert np.array_equal(got, M.covariance([raws[0], raws[1], raws[0]], QI, 5, 9000, 3))
    assert np.array_equal(got[:, 0], got[:, 2]) and np.array_equal(got[:, :, 0], got[:, :, 2])


# ---- 2. combine ----------------------------------------------------------------------------------------------------------------------
def _weights(K, T, seed):
    """Weights with full mantissas: 1 / 3 and pi / 7 first, the others random multiples of the two."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, (K, T)) / 3.0 + 1j * (rng.uniform(-1.0, 1.0, (K, T)) * (math.pi / 7.0))
    w[0, 0] = 1.0 / 3.0 + 1j * (math.pi / 7.0)
    return w


def _run(srcs, dst, dst_dtype, dst_layout, weights, nout, **kw):
    """One call into a dst record of nout samples between PAD_FRONT and PAD_BACK sentinel samples.  Returns (the written range as
    dst_dtype in file order, result); asserts the sentinels on both sides."""
    import cu_sdr_collection_amd as P
    c = _comps(dst_layout)
    total = PAD_FRONT + nout + PAD_BACK
    dst.load_if(np.full(total * c, SENTINEL, dtype=dst_dtype), layout=dst_layout)
    res = P.Engine.array_combine(srcs, dst, weights, noutputs=nout, dst_first=PAD_FRONT, **kw)
    back = dst.read_if(0, total, dtype=dst_dtype, layout=dst_layout)
    assert np.all(back[:PAD_FRONT * c] == SENTINEL) and np.all(back[(PAD_FRONT + nout) * c:] == SENTINEL), "bytes outside the range were written"
    assert res.noutputs == nout
    return back[PAD_FRONT * c:(PAD_FRONT + nout) * c], res


def _clipping_gain(a_r, a_i, dtype, layout):
    """The gain at which about 1 % of the components that a dst of this dtype and layout stores leave its range"""
    stored = np.abs(a_r) if layout == REAL else np.abs(np.concatenate([a_r, a_i]))
    return np.iinfo(dtype).max / np.quantile(stored, 0.99)


@pytest.mark.parametrize("src_fmt", list(FORMATS))
def test_combine_every_byte_and_both_statistics(engines, records, src_fmt):
    """From first_sample = 0, so that the first T - 1 outputs read in front of sample 0.  Would catch: a tap chain added in another
    order or with a fused multiply-add, records or taps walked in the wrong order, a sample offset by one at some (K, T), a tie rounded
    away from even, a clamp at the wrong end, a miscounted clipped or sum_sq - in any of the 36 format pairs.
    (That the gain clips about 1 % is checked where K T > 1: at K = T = 1 a component takes few distinct values, and the 1 % the gain
    aims at falls between two of them.)"""
    srcs, dst = engines
    sdt, slay = FORMATS[src_fmt]
    raws = records[src_fmt]
    _load(srcs, raws, slay)
    for K, T in KT:
        w = _weights(K, T, 910 + K)
        _, _, _, (a_r, a_i) = M.combine(raws[:K], slay, w, I16, IQ)
        for ddt in (I8, I16):
            model = {}
            for dlay in (IQ, QI, REAL):
                cls = dlay == REAL                                             # I/Q and Q/I store the same components: one model run for both
                if cls not in model:
                    g = _clipping_gain(a_r, a_i, ddt, dlay) * w
                    model[cls] = (g, M.combine(raws[:K], slay, g, ddt, IQ)[3])
                g, (b_r, b_i) = model[cls]
                want, clipped, sum_sq = M.quantise(b_r, b_i, ddt, dlay)
                got, res = _run(srcs[:K], dst, ddt, dlay, g, NS)
                tag = (src_fmt, ddt.__name__, dlay, K, T)
                assert got.tobytes() == want.tobytes(), tag
                assert (res.clipped, res.sum_sq) == (clipped, sum_sq), tag
                assert K * T == 1 or 0.005 * want.shape[0] < clipped < 0.02 * want.shape[0], (tag, clipped)


@pytest.mark.parametrize("src_fmt", ["i8_real", "i16_iq"])
def test_combine_tile_edges_on_every_residue_of_16_bytes(engines, records, src_fmt):
    """Would catch: a tile's last or first output missing or doubled, a span one vector short when it starts late in a vector."""
    import cu_sdr_collection_amd as P
    srcs, dst = engines
    sdt, slay = FORMATS[src_fmt]
    K, T = 2, 3
    bps = _bps(sdt, slay)
    tile = P.Engine.debug_array_tile_outputs(K, T)
    raws = records[src_fmt][:K]
    _load(srcs, raws, slay)
    w = 0.02 * _weights(K, T, 920) if sdt == I8 else 1e-4 * _weights(K, T, 920)
    nmax = 2 * tile + 1
    residues = set()
    for first in range(T - 1, T - 1 + 16 // math.gcd(16, bps)):                # the span of tile 0 starts at sample first - (T - 1)
        # one model run per first_sample: an output does not depend on how many follow it
        _, _, _, (a_r, a_i) = M.combine(raws, slay, w, I8, IQ, first_sample=first, noutputs=nmax)
        for nout in (tile - 1, tile, tile + 1, nmax):
            for t in range(-(-nout // tile)):
                residues.add(((first + t * tile - (T - 1)) * bps) % 16)
            want, clipped, sum_sq = M.quantise(a_r[:nout], a_i[:nout], I8, IQ)
            got, res = _run(srcs[:K], dst, I8, IQ, w, nout, first_sample=first)
            assert got.tobytes() == want.tobytes() and (res.clipped, res.sum_sq) == (clipped, sum_sq), (src_fmt, first, nout)
    assert residues == set(range(0, 16, math.gcd(16, bps)))


def test_combine_pieces_join_to_the_whole_and_a_second_run_is_the_first(engines, records):
    """Would catch: an output that depends on the tile or the call it falls in, statistics that are not per output."""
    import cu_sdr_collection_amd as P
    srcs, dst = engines
    K, T, n0 = 4, 7, 3
    tile = P.Engine.debug_array_tile_outputs(K, T)
    nout, a, b = 3 * tile + 500, 777, 2 * tile
    raws = records["i8_iq"][:K]
    _load(srcs, raws, IQ)
    w = 0.5 * _weights(K, T, 930)                                             # an rms near 60: some components clip
    whole, res = _run(srcs[:K], dst, I8, IQ, w, nout, first_sample=n0)
    again, res2 = _run(srcs[:K], dst, I8, IQ, w, nout, first_sample=n0)
    assert again.tobytes() == whole.tobytes() and vars(res2) == vars(res)
    dst.load_if(np.full(2 * nout, SENTINEL, dtype=I8))
    parts = [P.Engine.array_combine(srcs[:K], dst, w, first_sample=n0 + lo, noutputs=hi - lo, dst_first=lo) for lo, hi in ((0, a), (a, b), (b, nout))]
    assert dst.read_if(0, nout).tobytes() == whole.tobytes()
    assert sum(p.clipped for p in parts) == res.clipped and sum(p.sum_sq for p in parts) == res.sum_sq
    assert res.sum_sq > 0 and res.clipped > 0


@pytest.mark.parametrize("fmt", ["i8_iq", "i16_qi", "i8_real"])
def test_combine_of_one_record_is_the_downconverter_without_nco_and_decimation(engines, records, fmt):
    """Would catch: a finish that differs from gc_downconvert's in rounding, clamping, layout or counting."""
    srcs, dst = engines
    dt, lay = FORMATS[fmt]
    raw = records[fmt][0]
    srcs[0].load_if(raw, layout=lay, fs=18e6)                                  # gc_downconvert asks for a sampling frequency
    T = 32
    w = _weights(1, T, 940) * (0.3 if dt == I8 else 0.003)
    for ddt, dlay in ((I8, IQ), (I16, QI), (I8, REAL)):
        for first in (0, 40):
            nout = NS - first
            c = _comps(dlay)
            dst.load_if(np.full(nout * c, SENTINEL, dtype=ddt), layout=dlay)
            ddc = srcs[0].downconvert(dst, w[0], 1, first_sample=first, noutputs=nout)
            want = dst.read_if(0, nout, dtype=ddt, layout=dlay).tobytes()
            got, res = _run(srcs[:1], dst, ddt, dlay, w, nout, first_sample=first)
            assert got.tobytes() == want and (res.clipped, res.sum_sq) == (ddc.clipped, ddc.sum_sq), (fmt, ddt.__name__, dlay, first)
            assert res.sum_sq > 0


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_cov_dst_and_res_untouched(engines, records):
    """Would catch: a check that comes after the first write, a refusal with the wrong status, a result written by a refused call."""
    import cu_sdr_collection_amd as P
    L = P._lib
    lib = L.load()
    srcs, dst = engines
    raws = records["i8_iq"][:3]
    _load(srcs, raws, IQ)
    srcs[3].load_if(records["i16_iq"][0], layout=IQ)                           # another dtype
    srcs[4].load_if(records["i8_qi"][0], layout=QI)                            # another layout
    srcs[5].load_if(raws[0][:2 * 30000], layout=IQ)                            # a shorter record
    ND = 5000
    sentinel = np.full(2 * ND, SENTINEL, dtype=I8)
    dst.load_if(sentinel)

    def ctxs(engs):
        return (C.c_void_p * len(engs))(*[e._ctx for e in engs])

    def cov(engs, first=0, n=1000, lags=2):
        p = L.gc_array_cov_params(first, n, len(engs), lags)
        out = np.full((lags, len(engs), len(engs), 2), -7, dtype=np.int64)
        rc = lib.gc_array_covariance(ctxs(engs), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == L.GC_OK or np.all(out == -7), "cov written by a refused call"
        return rc

    def comb(engs, d, first=0, nout=1000, dst_first=0, ntaps=3, weights=None):
        p = L.gc_array_combine_params(first, nout, dst_first, len(engs), ntaps)
        r = L.gc_array_combine_result(-7, 7)
        w = np.ones((len(engs), ntaps, 2)) if weights is None else weights
        rc = lib.gc_array_combine(ctxs(engs), d._ctx, C.byref(p), w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r))
        assert rc == L.GC_OK or (r.clipped, r.sum_sq) == (-7, 7), "result written by a refused call"
        return rc

    def untouched():
        return dst.read_if(0, ND).tobytes() == sentinel.tobytes()

    a, b, c = srcs[:3]
    # mixed formats
    assert cov([a, srcs[3]]) == cov([a, srcs[4]]) == L.GC_E_INVALID
    assert comb([a, srcs[3]], dst) == comb([a, srcs[4]], dst) == L.GC_E_INVALID and untouched()
    # dst is a source, shares a source's record, or overlaps one
    assert comb([a, b], a) == comb([a, b], b) == L.GC_E_INVALID
    with P.Engine(0) as other:
        other.share_if(b)
        assert comb([a, b], other) == L.GC_E_INVALID
        assert comb([a, other], dst) == L.GC_OK and not untouched()            # ... while a source that shares a record works
        other.load_if(np.zeros(64, dtype=I8))
    dst.load_if(sentinel)
    with P.Engine(0) as big, P.Engine(0) as lo, P.Engine(0) as hi:
        big.load_if(np.concatenate([raws[0], raws[0][:64]]))
        big.synchronize()
        base, _ = big.if_buffer()
        lo.attach_if(base, NS, I8, IQ)
        hi.attach_if(base + 32, NS, I8, IQ)
        assert comb([a, lo], hi) == comb([hi, a], lo) == L.GC_E_INVALID
        assert big.read_if(0, NS + 32).tobytes() == np.concatenate([raws[0], raws[0][:64]]).tobytes()
        assert cov([lo, hi]) == L.GC_OK                                         # sources may overlap each other
        lo.load_if(np.zeros(64, dtype=I8))
        hi.load_if(np.zeros(64, dtype=I8))
    for e, raw in zip(srcs[:3], raws):
        assert e.read_if(0, NS).tobytes() == raw.tobytes()
    # ranges past a source (the shortest decides) and past dst
    short = srcs[5]
    assert cov([a, short], first=29000, n=1000) == L.GC_OK and cov([a, short], first=29001, n=1000) == cov([short, a], first=29001, n=1000) == L.GC_E_RANGE
    assert cov([a, b], first=NS, n=1) == cov([a, b], first=1 << 62, n=1) == L.GC_E_RANGE
    assert comb([a, short], dst, first=29001) == comb([a, b], dst, first=NS - 999) == L.GC_E_RANGE and untouched()
    assert comb([a, b], dst, nout=ND + 1) == comb([a, b], dst, dst_first=ND - 999) == comb([a, b], dst, dst_first=1 << 62, nout=1) == L.GC_E_RANGE and untouched()
    # arguments and state
    bad = np.ones((2, 3, 2))
    bad[1, 1, 0] = float("nan")
    assert comb([a, b], dst, weights=bad) == comb([a, b], dst, ntaps=0) == comb([a, b], dst, nout=0) == comb([a, b], dst, first=-1) == L.GC_E_INVALID and untouched()
    assert cov([a, b], lags=0) == cov([a, b], lags=33) == cov([a, b], n=0) == cov([a, b], n=(1 << 31) + 1) == cov([a, b], first=-1) == L.GC_E_INVALID
    with P.Engine(0) as fresh:
        assert cov([a, fresh]) == cov([fresh]) == L.GC_E_STATE and comb([a, fresh], dst) == L.GC_E_STATE and untouched()
        assert comb([a, b], fresh) == L.GC_E_STATE
    with pytest.raises(P.GnssCorrError) as e:
        P.Engine.array_combine([a, b], dst, np.ones(2), noutputs=ND + 1)
    assert e.value.status == L.GC_E_RANGE
    with pytest.raises(P.GnssCorrError) as e:
        P.Engine.array_covariance([a, short], 0, NS)
    assert e.value.status == L.GC_E_RANGE
    # the accepted calls that close them; noutputs=None: what both sides hold
    assert comb([a, b], dst, nout=ND) == L.GC_OK and not untouched()
    assert comb([a, b], dst, dst_first=ND - 1000) == comb([a, b], dst, first=NS - 1000) == comb([a] * 8, dst, ntaps=32) == L.GC_OK
    assert cov([a, b], first=NS - 1, n=1) == cov([a] * 8, lags=32) == L.GC_OK
    assert P.Engine.array_combine([a, b], dst, np.ones(2)).noutputs == ND and P.Engine.array_combine([a, short], dst, np.ones(2), first_sample=27000).noutputs == 3000
    assert P.Engine.array_combine([a, b], dst, np.ones(2), dst_first=4000).noutputs == 1000


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
def jammed_array(P, n_antennas=4):
    """The four records of the jammed array of the end-to-end test (int8 I/Q, file order), the settings, the satellites."""
    S = P.initSettings()
    fs = S.samplingFreq
    n = int(0.05 * fs)
    sats = P.synth.scene(4, 20241008 + 2, fs)
    st = np.random.default_rng(16)
    phi = st.uniform(0, 2 * np.pi, (n_antennas, 4))
    phi[0] = 0
    vj = np.exp(1j * st.uniform(0, 2 * np.pi, n_antennas))
    vj[0] = 1
    rj = np.random.default_rng(9)
    jam = 30 * (rj.standard_normal(n) + 1j * rj.standard_normal(n))
    raws = []
    for a in range(n_antennas):
        those = [dataclasses.replace(s, carrier_phase=s.carrier_phase + phi[a, i]) for i, s in enumerate(sats)]
        big = P.synth.generate_if(those, n, fs, S.IF, P.codes.generateCAcode, S.codeFreqBasis, 1023, seed=77, sigma=400.0, noise=False)
        assert np.max(np.abs(big.astype(np.int64))) <= 95
        signal = (big[0::2] + 1j * big[1::2]) * (8 / 400)
        r = np.random.default_rng(100 + a)
        noise = 8 * (r.standard_normal(n) + 1j * r.standard_normal(n))
        z = signal + vj[a] * jam + noise
        rec = np.empty(2 * n, dtype=I8)
        rec[0::2] = np.clip(np.rint(z.real), -128, 127)
        rec[1::2] = np.clip(np.rint(z.imag), -128, 127)
        raws.append(rec)
    return S, sats, raws


def test_end_to_end_on_a_jammed_four_element_array(engines):
    """Four antennas see the four-satellite scene (each with its own carrier phases), a wide-band noise jammer of 30 per component from
    one direction and their own noise of 8 per component, 50 ms at 18 Msps as int8 I/Q (5e-5 of the components clip).
    receiver.null_steer (one tap, reference element 0, target_rms 25) writes a fifth record; the library's acquisition runs on antenna
    0 alone and on the combined record.

    What the numpy model and the oracle's acquisition_l1ca give on the CPU:
        mean |x_0|^2 1930;  mean |w^H x|^2 171.8;  noise floor 2 * 8^2 * sum |w|^2 = 168.7 (the output stands 1.9 % over it: the
        satellites and the rounding);  acqThreshold 3.5
        PRN   antenna 0 alone   combined: peakMetric  codePhase  carrFreq
          2        1.54                      6.45         740      17425
          5        1.77                      6.31       10797      15475
         17        1.65                      6.78       13258      22825
          7        1.57                      5.87       10492      17775
          1        (absent)                  1.66
    codePhase and carrFreq are the clean scene's (tests/test_gpu_ddc.py).
    Would catch: weights applied without the conjugate (the jammer doubles instead of vanishing), a covariance with the wrong sign of
    its imaginary parts, a reference element that is not kept, a delay the wrapper does not account for."""
    import cu_sdr_collection_amd as P
    srcs, dst = engines
    S, sats, raws = jammed_array(P)
    n = raws[0].shape[0] // 2
    prns = [s.prn for s in sats]
    assert prns == [2, 5, 17, 7]
    absent = 1
    expect = {2: (740, 17425), 5: (10797, 15475), 17: (13258, 22825), 7: (10492, 17775)}
    S1 = copy.copy(S)
    S1.acqSatelliteList = prns + [absent]
    for e, r in zip(srcs, raws):
        e.load_if(r, fs=S.samplingFreq)
    jammed = P.acquisition(srcs[0], S1, first_sample=0)
    dst.alloc_if(n, I8, IQ)
    res, w, gain, cov = P.null_steer(srcs[:4], dst, S, ntaps=1, ref=0, target_rms=25.0)
    assert res.noutputs == n and w.shape == (4, 1) and abs(w[0, 0] - 1.0) < 1e-12 and gain > 0
    assert np.array_equal(cov, M.covariance(raws, IQ, 0, n, 1))
    assert abs(math.sqrt(res.sum_sq / (2 * n)) - 25.0) < 1.0 and res.clipped < 1e-4 * 2 * n
    got = P.acquisition(dst, S1, first_sample=0)
    print("array scene: " + "; ".join(f"PRN {p} peakMetric {jammed.peakMetric[p - 1]:.2f} -> {got.peakMetric[p - 1]:.2f}, codePhase {got.codePhase[p - 1]:.0f}, "
                                      f"carrFreq {got.carrFreq[p - 1]:.0f}" for p in prns)
          + f"; absent PRN {absent}: {jammed.peakMetric[absent - 1]:.2f} -> {got.peakMetric[absent - 1]:.2f}; mean |x_0|^2 {cov[0, 0, 0, 0] / n:.1f}")
    for p in prns:
        assert jammed.peakMetric[p - 1] < S.acqThreshold and jammed.carrFreq[p - 1] == 0, p
        assert got.peakMetric[p - 1] > S.acqThreshold, (p, got.peakMetric[p - 1])
        assert abs(got.codePhase[p - 1] - expect[p][0]) <= 1 and abs(got.carrFreq[p - 1] - expect[p][1]) <= 25.0, (p, got.codePhase[p - 1], got.carrFreq[p - 1])
    assert got.peakMetric[absent - 1] < S.acqThreshold and got.carrFreq[absent - 1] == 0
    # unscaled into int16 I/Q: the output power is the noise the weights let through
    dst.alloc_if(n, I16, IQ)
    plain = P.Engine.array_combine(srcs[:4], dst, np.conj(w))
    power = plain.sum_sq / n
    floor = 2 * 8.0 ** 2 * float(np.sum(np.abs(w) ** 2))
    print(f"array scene: mean |w^H x|^2 {power:.1f}, noise floor {floor:.1f} ({100 * (power / floor - 1):+.1f} %)")
    assert plain.clipped == 0 and abs(power - floor) <= 0.05 * floor
