"""The host plan of the swept excision (csrc/excise_plan.h: gc_excise_sweep's argument checks, the words of a mask row, the rows a
tile of the segment list names in the caller's [K] arrays) without a GPU: tests/excise_sweep_shim.hip runs it on the CPU, the tile
walk under budgets of a few segments.

Refusals: every status of gc_excise_sweep that needs no device, each next to the accepted call that closes it; a refused call leaves
the plan unwritten.  W for nfft in {4, 6, 60, 64, 72, 128, 320}.  The tile walk: every segment's mask row and power row named once
and in order, inside the tile buffers.

The last test follows the dilation rule of the numpy model (tests/excise_sweep_model.py) by hand: the wrap at both ends, an nfft
that is no multiple of 64, and 2 widen + 1 >= nfft.  It holds the reference the GPU tests compare against, not the library: it is the
one test here that passes without the feature."""
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
        src, out = os.path.join(HERE, "excise_sweep_shim.hip"), os.path.join(HERE, "build", "libexcise_sweep_shim.so")
        deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = [f for f in B._tu_flags("excise.hip") if f != "--offload-compress"]
            subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
        lib = C.CDLL(out)
        lib.sweep_shim_create.restype = C.c_void_p
        lib.sweep_shim_create.argtypes = [C.c_longlong, C.c_int, C.c_ulonglong, C.c_int, C.c_int]
        lib.sweep_shim_destroy.argtypes = [C.c_void_p]
        lib.sweep_shim_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, I64P]
        lib.sweep_shim_mask_words.restype = lib.sweep_shim_walk.restype = C.c_longlong
        lib.sweep_shim_mask_words.argtypes = [C.c_int]
        lib.sweep_shim_walk.argtypes = [C.c_longlong, C.c_int, C.c_longlong, I64P, C.c_longlong]
        _LIB.append(lib)
    return _LIB[0]


class Ctx:
    def __init__(self, address=A0, device=0, nsamples=100000, dtype=I8, layout=IQ):
        self.args = (address, device, nsamples, dtype, layout)

    def __enter__(self):
        self.p = _shim().sweep_shim_create(*self.args)
        return self.p

    def __exit__(self, *exc):
        _shim().sweep_shim_destroy(self.p)


def _check(src, dst, first=0, nsamples=1000, nfft=64, widen=1, limit="ones", gain=None, have_p=True, tile_bytes=0):
    from cu_sdr_collection_amd import _lib as L
    p = L.gc_excise_sweep_params(first, nsamples, nfft, widen)
    lim = None if limit is None else np.ones(max(nfft, 1), dtype=np.float32) if isinstance(limit, str) else np.ascontiguousarray(limit, dtype=np.float32)
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float32)
    out = (C.c_longlong * 5)(*[-7] * 5)
    rc = _shim().sweep_shim_check(src, dst, C.addressof(p) if have_p else None, None if lim is None else lim.ctypes.data,
                                  None if g is None else g.ctypes.data, tile_bytes, out)
    return rc, list(out)


def test_refusals_that_need_no_device():
    from cu_sdr_collection_amd import _lib as L
    assert _shim().sweep_shim_max_widen() == L.GC_EXCISE_MAX_WIDEN == 64
    with Ctx() as src, Ctx(address=A0 + (1 << 22)) as dst:
        K = 1000 // 32 + 2
        assert _check(src, dst) == (OK, [32, K, (128 << 20) // (2 * 64 * 8), 1, K])
        assert _check(src, src)[0] == OK
        bad = [dict(have_p=False), dict(limit=None), dict(first=-1), dict(nsamples=0), dict(nsamples=-2), dict(nfft=2), dict(nfft=0), dict(nfft=-64),
               dict(nfft=5), dict(nfft=63), dict(widen=-1), dict(widen=65), dict(widen=1 << 30), dict(widen=-(1 << 31))]
        for kw in bad:
            rc, out = _check(src, dst, **kw)
            assert rc == INVALID and out == [-7] * 5, kw
        for kw in (dict(nfft=4), dict(nfft=6), dict(nsamples=1), dict(first=99999, nsamples=1), dict(widen=0), dict(widen=64), dict(gain=None),
                   dict(gain=np.ones(64)), dict(nfft=4, widen=64)):
            assert _check(src, dst, **kw)[0] == OK, kw                  # the accepted calls that close them
        for where in (0, 17, 63):
            for v in (np.nan, -1.0, -np.inf, -1e-45):                   # NaN or negative (the smallest subnormal too)
                lim = np.ones(64)
                lim[where] = v
                assert _check(src, dst, limit=lim) == (INVALID, [-7] * 5), (v, where)
            for v in (np.inf, 0.0, -0.0, 3.4e38, 1e-45):                # +INF protects a bin; 0 makes it hot wherever P > 0
                lim = np.ones(64)
                lim[where] = v
                assert _check(src, dst, limit=lim)[0] == OK, (v, where)
            for v in (np.nan, np.inf, -np.inf):
                g = np.ones(64)
                g[where] = v
                assert _check(src, dst, gain=g) == (INVALID, [-7] * 5), (v, where)
        assert _check(src, dst, limit=np.full(64, np.inf), gain=np.full(64, -3.0e38))[0] == OK         # any finite gain, of either sign
        assert _check(None, dst)[0] == INVALID and _check(src, None)[0] == INVALID
        # the record's end: the range may end ON it
        assert _check(src, dst, first=99000, nsamples=1000)[0] == OK
        assert _check(src, dst, first=99001, nsamples=1000)[0] == RANGE
        assert _check(src, dst, first=100000, nsamples=1)[0] == RANGE
        assert _check(src, dst, first=7, nsamples=(1 << 63) - 1)[0] == RANGE
        for kw in (dict(device=1), dict(nsamples=99999), dict(dtype=I16), dict(layout=QI), dict(layout=REAL)):
            with Ctx(address=A0 + (1 << 22), **kw) as other:
                assert _check(src, other) == (INVALID, [-7] * 5), kw
        with Ctx(address=A0 + 2) as lap:                                # overlaps the source without being it
            assert _check(src, lap)[0] == INVALID
        with Ctx(address=A0) as shared:                                 # another context on the same record: in place
            assert _check(src, shared)[0] == OK
    with Ctx(address=0) as none, Ctx() as rec:
        assert _check(none, rec)[0] == STATE and _check(rec, none)[0] == STATE
        assert _check(none, rec, widen=65)[0] == INVALID and _check(none, rec, limit=np.full(64, -1.0))[0] == INVALID   # arguments before state


@pytest.mark.parametrize("nfft,W", [(4, 1), (6, 1), (60, 1), (64, 1), (72, 2), (128, 2), (320, 5)])
def test_words_of_a_mask_row(nfft, W):
    assert _shim().sweep_shim_mask_words(nfft) == W
    import excise_sweep_model as SM
    assert SM.mask_words(nfft) == W
    with Ctx() as ctx:
        rc, out = _check(ctx, ctx, nfft=nfft, nsamples=5000)
        assert rc == OK and out[3] == W and out[0] == nfft // 2 and out[1] == -(-5000 // (nfft // 2)) + 1
        # under a budget of three segments the tile buffers hold three rows; under the library's, the whole list
        rc, small = _check(ctx, ctx, nfft=nfft, nsamples=5000, tile_bytes=3 * 2 * nfft * 8)
        assert rc == OK and small[2] == 3 and small[4] == 3 and out[4] == min(out[1], out[2])


@pytest.mark.parametrize("tile", [1, 2, 3, 5])
@pytest.mark.parametrize("nfft,nsamples", [(4, 1), (4, 3), (60, 29), (60, 333), (64, 1000), (72, 100), (320, 2000)])
def test_every_segments_mask_row_is_named_once_and_in_order(tile, nfft, nsamples):
    W, K = (nfft + 63) // 64, -(-nsamples // (nfft // 2)) + 1
    cap = 4 * (K + 2)
    buf = (C.c_longlong * cap)()
    n = _shim().sweep_shim_walk(nsamples, nfft, tile, buf, cap)
    assert 0 < n <= cap and n % 4 == 0
    rows = []
    for i in range(0, n, 4):
        g0, cnt, mask_off, power_off = buf[i:i + 4]
        assert 1 <= cnt <= tile                                          # the tile's rows fit buffers of `tile` rows
        assert mask_off == g0 * W and power_off == g0 * nfft            # row g0 of the [K][W] masks and of the [K][nfft] power
        assert mask_off + cnt * W <= K * W and power_off + cnt * nfft <= K * nfft
        rows += list(range(g0, g0 + cnt))
    assert rows == list(range(K))


def test_the_models_dilation_on_rows_small_enough_to_follow():
    import excise_sweep_model as SM

    def cut(nfft, hot_bins, widen):
        hot = np.zeros((1, nfft), dtype=bool)
        hot[0, list(hot_bins)] = True
        return np.flatnonzero(SM.dilate(hot, widen)[0]).tolist()
    assert cut(16, [], 3) == []
    assert cut(16, [5], 0) == [5]
    assert cut(16, [5], 2) == [3, 4, 5, 6, 7]
    assert cut(16, [0], 2) == [0, 1, 2, 14, 15]                         # the wrap at the low end
    assert cut(16, [15], 1) == [0, 14, 15]                              # ... and at the high end: bin nfft - 1 is next to bin 0
    assert cut(16, [0, 15], 1) == [0, 1, 14, 15]
    assert cut(16, [3, 6], 1) == [2, 3, 4, 5, 6, 7]                     # two neighbourhoods that touch
    assert cut(60, [59], 2) == [0, 1, 57, 58, 59]                       # an nfft that is no multiple of 64
    assert cut(72, [0], 3) == [0, 1, 2, 3, 69, 70, 71]
    assert cut(72, [63], 1) == [62, 63, 64] and cut(72, [64], 1) == [63, 64, 65]   # across the word boundary
    assert cut(320, [1], 64) == list(range(0, 66)) + list(range(257, 320))
    assert cut(6, [2], 2) == [0, 1, 2, 3, 4]                            # 2 widen + 1 = 5 < 6: bin 5 is three away
    assert cut(4, [2], 1) == [1, 2, 3]
    assert cut(4, [2], 2) == [0, 1, 2, 3] and cut(4, [], 2) == []       # 2 widen + 1 >= nfft: one hot bin cuts the segment
    assert cut(4, [0], 64) == [0, 1, 2, 3] and cut(128, [77], 64) == list(range(128)) and len(cut(130, [0], 64)) == 129
    # rows are decided one by one
    hot = np.zeros((3, 8), dtype=bool)
    hot[0, 7] = hot[2, 3] = True
    assert SM.dilate(hot, 1).astype(int).tolist() == [[1, 0, 0, 0, 0, 0, 1, 1], [0] * 8, [0, 0, 1, 1, 1, 0, 0, 0]]
    (segments, nhot, ncut, segments_cut, most), bin_cut = SM.counts(hot, SM.dilate(hot, 1))
    assert (segments, nhot, ncut, segments_cut, most) == (3, 2, 6, 2, 3) and bin_cut.tolist() == [1, 0, 1, 1, 1, 0, 1, 1]
    # the model on a record small enough to follow: one strong cell, and the mask handed in from outside decides alone
    z = np.zeros(16, dtype=complex)
    z[:] = 10.0 * np.exp(2j * np.pi * 2 * np.arange(16) / 8)            # a tone on bin 2 of nfft = 8
    res = SM.excise_sweep(z, np.full(8, 100.0), widen=0)
    assert res.hot.shape == (5, 8) and res.hot[:, 2].all() and not np.delete(res.hot, [1, 2, 3], axis=1).any()
    quiet = SM.excise_sweep(z, np.full(8, np.inf))
    assert not quiet.hot.any() and np.allclose(quiet.y, z)              # nothing cut: the identity
    forced = SM.excise_sweep(z, np.full(8, np.inf), cut=np.ones((5, 8), dtype=bool))
    assert not forced.hot.any() and forced.cut.all() and not forced.y.any()
