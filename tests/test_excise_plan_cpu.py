"""The host plan of the excision (csrc/excise_plan.h: the argument checks of gc_excise_pulses and gc_excise_bins, the blanker's range
laid over its bitmap and cut into tiles, the spectral excision's segment count and tile walk) without a GPU:
tests/excise_plan_shim.hip runs it on the CPU, the tile walk under budgets of a few segments.

Refusals: every status of gc_excise_pulses that needs no device, each next to the accepted call that closes it; a refused call
leaves the plan unwritten.  Layout: what the kernels rely on to stay inside the record and the bitmap - bit 0 on a multiple of 64 at
or below the range, every sample of the range, and every 16 bytes of record that hold one, inside a tile,
the bitmap long enough for the last tile's halo and the word the last prefix count names.

Spectral excision: K for nsamples in {1, H - 1, H, H + 1, 2 H, 2 H + 1}; every segment 0 .. K - 1 once and in order, the carried
segment named at every cut, every range sample written once by a tile that holds both its segments.  The transform planner's
refusal (GC_E_UNSUPPORTED) is make_plan's, asked through gc_debug_fft_plan.

The last test follows the numpy model of the blanker (tests/excise_model.py) by hand on cases small enough for that.  It holds the
reference the GPU tests compare against, not the library: it is the one test here that passes without the feature."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OK, INVALID, RANGE, STATE = 0, -1, -2, -5
I8, I16 = 0, 1
REAL, IQ, QI = 0, 1, 2
I64P = C.POINTER(C.c_longlong)
A0 = 1 << 20                                                            # an address; never read
_LIB = []


def _shim():
    if not _LIB:
        from cu_sdr_collection_amd import build as B
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not found")
        src, out = os.path.join(HERE, "excise_plan_shim.hip"), os.path.join(HERE, "build", "libexcise_plan_shim.so")
        deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = [f for f in B._tu_flags("excise.hip") if f != "--offload-compress"]
            subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
        lib = C.CDLL(out)
        lib.excise_shim_create.restype = C.c_void_p
        lib.excise_shim_create.argtypes = [C.c_longlong, C.c_int, C.c_ulonglong, C.c_int, C.c_int]
        lib.excise_shim_destroy.argtypes = [C.c_void_p]
        lib.excise_shim_check_pulses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, I64P]
        lib.excise_shim_constants.argtypes = [I64P]
        lib.excise_shim_check_bins.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, I64P]
        lib.excise_shim_segments.restype = lib.excise_shim_tile_segments.restype = lib.excise_shim_walk.restype = C.c_longlong
        lib.excise_shim_segments.argtypes = [C.c_longlong, C.c_int]
        lib.excise_shim_tile_segments.argtypes = [C.c_int, C.c_longlong]
        lib.excise_shim_walk.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, I64P, C.c_longlong]
        _LIB.append(lib)
    return _LIB[0]


class Ctx:
    def __init__(self, address=A0, device=0, nsamples=100000, dtype=I8, layout=IQ):
        self.args = (address, device, nsamples, dtype, layout)

    def __enter__(self):
        self.p = _shim().excise_shim_create(*self.args)
        return self.p

    def __exit__(self, *exc):
        _shim().excise_shim_destroy(self.p)


def _check(src, dst, first=0, nsamples=1000, threshold2=100, before=0, after=0, have_p=True):
    from cu_sdr_collection_amd import _lib as L
    p = L.gc_excise_pulse_params(first, nsamples, threshold2, before, after)
    out = (C.c_longlong * 4)(*[-7] * 4)
    rc = _shim().excise_shim_check_pulses(src, dst, C.addressof(p) if have_p else None, out)
    return rc, list(out)


def _constants():
    out = (C.c_longlong * 4)()
    _shim().excise_shim_constants(out)
    return list(out)


def test_constants():
    from cu_sdr_collection_amd import _lib as L
    tile, tile_words, halo, guard = _constants()
    assert guard == L.GC_EXCISE_MAX_GUARD == 4096
    assert tile == 64 * tile_words and halo * 64 == guard               # the halo holds the longest guard
    assert tile % (16 * 256) == 0                                       # whole 16-byte vectors per thread in every format


def test_pulse_refusals_that_need_no_device():
    with Ctx() as src, Ctx(address=A0 + (1 << 22)) as dst:
        assert _check(src, dst)[0] == OK and _check(src, src)[0] == OK
        bad = [dict(have_p=False), dict(first=-1), dict(nsamples=0), dict(nsamples=-3), dict(threshold2=-1), dict(before=-1), dict(before=4097),
               dict(after=-1), dict(after=4097), dict(before=1 << 30), dict(after=-(1 << 31))]
        for kw in bad:
            rc, out = _check(src, dst, **kw)
            assert rc == INVALID and out == [-7] * 4, kw
        for kw in (dict(first=0), dict(nsamples=1), dict(threshold2=0), dict(threshold2=(1 << 63) - 1), dict(before=0, after=0), dict(before=4096, after=4096)):
            assert _check(src, dst, **kw)[0] == OK, kw                  # the accepted calls that close them
        assert _shim().excise_shim_check_pulses(None, dst, None, (C.c_longlong * 4)()) == INVALID
        assert _check(None, dst)[0] == INVALID and _check(src, None)[0] == INVALID
        # the record's end: the range may end ON it
        assert _check(src, dst, first=99000, nsamples=1000)[0] == OK
        assert _check(src, dst, first=99001, nsamples=1000)[0] == RANGE
        assert _check(src, dst, first=99999, nsamples=1)[0] == OK
        assert _check(src, dst, first=100000, nsamples=1)[0] == RANGE
        assert _check(src, dst, first=100001, nsamples=1)[0] == RANGE
        assert _check(src, dst, first=5, nsamples=(1 << 63) - 1)[0] == RANGE                      # no sum that leaves int64
        assert _check(src, dst, first=(1 << 63) - 1, nsamples=(1 << 63) - 1)[0] == RANGE
    with Ctx(address=0) as none, Ctx() as rec:
        assert _check(none, rec)[0] == STATE and _check(rec, none)[0] == STATE and _check(none, none)[0] == STATE
        assert _check(none, rec, nsamples=0)[0] == INVALID                                          # arguments before state
        assert _check(rec, rec)[0] == OK


def test_a_destination_that_differs_or_overlaps_is_refused():
    far = A0 + (1 << 22)
    with Ctx() as src:
        for kw in (dict(device=1), dict(nsamples=99999), dict(nsamples=100001), dict(dtype=I16), dict(layout=QI), dict(layout=REAL)):
            with Ctx(address=far, **kw) as dst:
                rc, out = _check(src, dst)
                assert rc == INVALID and out == [-7] * 4, kw
        # 100 000 int8 pairs are 200 000 bytes: a record that begins inside them overlaps, one that begins behind them does not
        for off, want in ((1, INVALID), (199999, INVALID), (200000, OK), (-1, INVALID), (-199999, INVALID), (-200000, OK), (0, OK)):
            with Ctx(address=far + off) as dst, Ctx(address=far) as s2:
                assert _check(s2, dst)[0] == want, off
        with Ctx(address=A0) as shared:                                                           # another context on the same record: in place
            assert _check(src, shared)[0] == OK
    with Ctx(dtype=I16, layout=REAL, nsamples=1000) as src, Ctx(address=A0 + 1999, dtype=I16, layout=REAL, nsamples=1000) as dst:
        assert _check(src, dst)[0] == INVALID                                                      # 2 bytes per sample: 2 000 bytes
    with Ctx(dtype=I16, layout=REAL, nsamples=1000) as src, Ctx(address=A0 + 2000, dtype=I16, layout=REAL, nsamples=1000) as dst:
        assert _check(src, dst)[0] == OK


@pytest.mark.parametrize("dtype,layout,bps", [(I8, IQ, 2), (I8, QI, 2), (I8, REAL, 1), (I16, IQ, 4), (I16, QI, 4), (I16, REAL, 2)])
def test_the_range_over_the_bitmap_and_the_tiles(dtype, layout, bps):
    tile, tile_words, halo, _ = _constants()
    per16 = 16 // bps
    rec = 5 * tile + 77
    with Ctx(nsamples=rec, dtype=dtype, layout=layout) as ctx:
        firsts = [0, 1, 63, 64, 65, 4097, tile - 1, tile, tile + 1, 2 * tile + 63]
        counts = [1, 2, per16 - 1, per16, per16 + 1, 63, 64, 65, tile - 64, tile - 1, tile, tile + 1, 2 * tile + 5]
        for first in firsts:
            for n in [c for c in counts if c >= 1] + [rec - first]:
                if first + n > rec:
                    continue
                rc, (base, ntiles, words, got_bps) = _check(ctx, ctx, first=first, nsamples=n)
                assert rc == OK and got_bps == bps
                end = first + n
                assert base % 64 == 0 and base <= first < base + 64                             # bit 0: the word the range begins in
                assert base % per16 == 0                                                         # ... which is a 16-byte boundary of the record
                assert base + (ntiles - 1) * tile < end <= base + ntiles * tile                  # every sample in a tile, no idle tile
                assert words == ntiles * tile_words + 2 * halo + 1
                # every 16 bytes of record that hold a sample of the range belong to a tile's thread
                assert first // per16 * per16 >= base and -(-end // per16) * per16 <= base + ntiles * tile


# ---- gc_excise_bins ----------------------------------------------------------------------------------------------------------------
UNSUPPORTED = -6


def _check_bins(src, dst, first=0, nsamples=1000, nfft=64, reserved=0, gain="ones", have_p=True, tile_bytes=0):
    from cu_sdr_collection_amd import _lib as L
    p = L.gc_excise_bins_params(first, nsamples, nfft, reserved)
    g = None if gain is None else np.ones(max(nfft, 1), dtype=np.float32) if isinstance(gain, str) else np.ascontiguousarray(gain, dtype=np.float32)
    out = (C.c_longlong * 3)(-7, -7, -7)
    rc = _shim().excise_shim_check_bins(src, dst, C.addressof(p) if have_p else None, None if g is None else g.ctypes.data, tile_bytes, out)
    return rc, list(out)


def test_bins_refusals_that_need_no_device():
    with Ctx() as src, Ctx(address=A0 + (1 << 22)) as dst:
        assert _check_bins(src, dst) == (OK, [32, 1000 // 32 + 2, (128 << 20) // (2 * 64 * 8)])
        assert _check_bins(src, src)[0] == OK
        bad = [dict(have_p=False), dict(gain=None), dict(first=-1), dict(nsamples=0), dict(nsamples=-2), dict(nfft=2), dict(nfft=0), dict(nfft=-64),
               dict(nfft=5), dict(nfft=63), dict(reserved=1), dict(reserved=-1)]
        for kw in bad:
            rc, out = _check_bins(src, dst, **kw)
            assert rc == INVALID and out == [-7] * 3, kw
        for kw in (dict(nfft=4), dict(nfft=6), dict(nsamples=1), dict(first=99999, nsamples=1)):
            assert _check_bins(src, dst, **kw)[0] == OK, kw
        for v in (np.nan, np.inf, -np.inf):
            for where in (0, 17, 63):
                g = np.ones(64)
                g[where] = v
                assert _check_bins(src, dst, gain=g) == (INVALID, [-7] * 3), (v, where)
        assert _check_bins(src, dst, gain=np.full(64, -3.0e38))[0] == OK                              # any finite value, of either sign
        assert _check_bins(None, dst)[0] == INVALID and _check_bins(src, None)[0] == INVALID
        assert _check_bins(src, dst, first=99000, nsamples=1000)[0] == OK
        assert _check_bins(src, dst, first=99001, nsamples=1000)[0] == RANGE
        assert _check_bins(src, dst, first=100000, nsamples=1)[0] == RANGE
        assert _check_bins(src, dst, first=7, nsamples=(1 << 63) - 1)[0] == RANGE
        with Ctx(address=A0 + (1 << 22), layout=QI) as other:
            assert _check_bins(src, other)[0] == INVALID
        with Ctx(address=A0 + 2) as lap:
            assert _check_bins(src, lap)[0] == INVALID
    with Ctx(address=0) as none, Ctx() as rec:
        assert _check_bins(none, rec)[0] == STATE and _check_bins(rec, none)[0] == STATE
        assert _check_bins(none, rec, nfft=5)[0] == INVALID                                           # arguments before state


def test_planner_refuses_the_lengths_the_excision_refuses_and_the_tile_of_the_budget():
    from cu_sdr_collection_amd import _lib as L
    lib = L.load()
    ints = [C.c_int(0) for _ in range(6)]
    r1, r2 = (C.c_int * 12)(), (C.c_int * 12)()

    def plan(n):
        return lib.gc_debug_fft_plan(n, C.byref(ints[0]), C.byref(ints[1]), r1, C.byref(ints[2]), r2, C.byref(ints[3]), C.byref(ints[4]), C.byref(ints[5]))
    assert plan(14) == UNSUPPORTED and plan(32736) == UNSUPPORTED
    for n in (4, 16, 60, 64, 1000, 1024, 4096):
        assert plan(n) == OK and ints[0].value * ints[1].value == n
    assert lib.gc_debug_excise_tile_segments(4096) == 2048 and lib.gc_debug_excise_tile_segments(64) == 131072
    assert lib.gc_debug_excise_tile_segments(3) == 0 and lib.gc_debug_excise_tile_segments(4) == (128 << 20) // 64
    for nseg in (1, 2, 3, 5):
        assert _shim().excise_shim_tile_segments(64, nseg * 2 * 64 * 8) == nseg
    assert _shim().excise_shim_tile_segments(64, 1) == 1                                               # never less than one segment


@pytest.mark.parametrize("nfft", [4, 16, 60, 1024])
def test_segment_count(nfft):
    H = nfft // 2
    for n, want in ((1, 2), (H - 1, 2), (H, 2), (H + 1, 3), (2 * H, 3), (2 * H + 1, 4)):
        if n >= 1:
            assert _shim().excise_shim_segments(n, nfft) == want, n
            # the last segment [(K - 2) H, K H) holds the range's last sample; the one before it does not end the range alone
            assert (want - 2) * H < n <= (want - 1) * H


@pytest.mark.parametrize("tile", [1, 2, 3, 5])
@pytest.mark.parametrize("H,nsamples", [(2, 1), (2, 2), (2, 3), (8, 7), (8, 8), (8, 9), (8, 16), (8, 17), (8, 100), (32, 1000), (30, 333)])
def test_every_segment_once_in_order_and_the_carried_segment_named_at_every_cut(tile, H, nsamples):
    K = _shim().excise_shim_segments(nsamples, 2 * H)
    cap = 5 * (K + 2)
    buf = (C.c_longlong * cap)()
    n = _shim().excise_shim_walk(nsamples, H, K, tile, buf, cap)
    assert 0 < n <= cap and n % 5 == 0
    next_g, next_m, tiles = 0, 0, 0
    for i in range(0, n, 5):
        g0, cnt, carried, m0, m1 = buf[i:i + 5]
        assert g0 == next_g and 1 <= cnt <= tile and (cnt == tile or g0 + cnt == K)     # consecutive runs of the list, only the last short
        assert carried == (g0 - 1 if g0 > 0 else -1)                                      # the cut names the segment it carries
        assert m0 == next_m                                                               # every range sample written once, in order
        for m in range(m0, m1):                                                           # ... by a tile that holds both its segments
            k0 = m // H
            assert (k0 >= g0 or k0 == carried) and g0 <= k0 + 1 < g0 + cnt
        if m1 < nsamples:
            assert m1 == (g0 + cnt - 1) * H                                               # up to the last segment's first half, no further
        next_g, next_m, tiles = g0 + cnt, max(m1, m0), tiles + 1
    assert next_g == K and next_m == nsamples and tiles == -(-K // tile)


def test_the_model_on_cases_small_enough_to_follow():
    import excise_model as M
    raw = np.zeros(40, dtype=np.int8)                                   # 20 I/Q samples
    raw[2 * 5], raw[2 * 5 + 1] = 3, 4                                   # sample 5: norm 25
    raw[2 * 12] = -6                                                    # sample 12: norm 36
    raw[2 * 19 + 1] = 5                                                 # sample 19: norm 25
    raw[1::2] += 1                                                      # every second value 1: something to keep
    raw[2 * 5 + 1], raw[2 * 19 + 1] = 4, 5
    out, st = M.excise_pulses(raw, M.IQ, 0, 20, 24)
    assert (st.hot, st.blanked, st.runs, st.longest) == (3, 3, 3, 1)
    assert np.flatnonzero(~out.reshape(20, 2).any(axis=1)).tolist() == [5, 12, 19]
    out, st = M.excise_pulses(raw, M.IQ, 0, 20, 25)                     # > threshold2, not >=: only sample 12 (norm 37 with its 1)
    assert (st.hot, st.blanked, st.runs, st.longest) == (1, 1, 1, 1)
    out, st = M.excise_pulses(raw, M.IQ, 0, 20, 24, before=2, after=3)  # [3, 8], [10, 15], [17, 19] cut at the end
    assert (st.hot, st.blanked, st.runs, st.longest) == (3, 15, 3, 6)
    assert np.flatnonzero(~out.reshape(20, 2).any(axis=1)).tolist() == [3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 17, 18, 19]
    out, st = M.excise_pulses(raw, M.IQ, 0, 20, 24, before=3, after=3)  # [2, 8], [9, 15] and [16, 19] touch: one run
    assert (st.hot, st.blanked, st.runs, st.longest) == (3, 18, 1, 18)
    out, st = M.excise_pulses(raw, M.IQ, 6, 10, 24, before=4, after=1)  # the range [6, 16): sample 5 is not examined
    assert (st.hot, st.blanked, st.runs, st.longest) == (1, 6, 1, 6)
    assert out[:2 * 8].tobytes() == raw[:2 * 8].tobytes() and out[2 * 14:].tobytes() == raw[2 * 14:].tobytes()
    assert not out[2 * 8:2 * 14].any()
    # file order: a Q/I context gives the bytes of an I/Q context; a real record has c0 only
    assert M.excise_pulses(raw, M.QI, 0, 20, 24, 2, 3)[0].tobytes() == M.excise_pulses(raw, M.IQ, 0, 20, 24, 2, 3)[0].tobytes()
    out, st = M.excise_pulses(raw, M.REAL, 0, 40, 24)                   # values -6 and 5 (norms 36, 25)
    assert (st.hot, np.flatnonzero(out != raw).tolist()) == (2, [24, 39])
    # the squares in 64 bits
    big = np.full(2, -32768, dtype=np.int16)
    assert M.excise_pulses(big, M.IQ, 0, 1, (1 << 31) - 1)[1].hot == 1 and M.excise_pulses(big, M.IQ, 0, 1, 1 << 31)[1].hot == 0
