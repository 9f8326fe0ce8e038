"""The host plan of the record probe (csrc/probe_plan.h: the argument checks, the segment count, the tile walk) without a GPU:
tests/probe_plan_shim.hip runs it on the CPU under budgets of a few segments, so that short lists are cut where the tests choose.

The power kernel is modelled symbolically: a span's accumulator is the list of segments added to it; a tile appends its segments
[k0, k1) of the span, starting from the list the earlier tiles left when k0 > 0 (the carry) and from nothing when k0 == 0.  What
stands there after the last tile must be every span's segments 0 .. K - 1, in order, once - wherever the cuts fall.

Refusals: every status of gc_probe_psd / gc_probe_histogram that needs no device, with the accepted calls that close them.  The
transform planner's refusal (GC_E_UNSUPPORTED) is make_plan's, asked through gc_debug_fft_plan on the lengths the GPU test refuses."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FS = 18e6
OK, INVALID, RANGE, STATE, UNSUPPORTED = 0, -1, -2, -5, -6
I64P = C.POINTER(C.c_longlong)
_LIB = []


def _shim():
    if not _LIB:
        from cu_sdr_collection_amd import build as B
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not found")
        src, out = os.path.join(HERE, "probe_plan_shim.hip"), os.path.join(HERE, "build", "libprobe_plan_shim.so")
        deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = [f for f in B._tu_flags("probe.hip") if f != "--offload-compress"]
            subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
        lib = C.CDLL(out)
        lib.probe_shim_create.restype = C.c_void_p
        lib.probe_shim_create.argtypes = [C.c_int, C.c_ulonglong, C.c_double]
        lib.probe_shim_destroy.argtypes = [C.c_void_p]
        lib.probe_shim_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, I64P]
        lib.probe_shim_check_histogram.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_int]
        lib.probe_shim_segments.restype = lib.probe_shim_tile_segments.restype = lib.probe_shim_walk.restype = C.c_longlong
        lib.probe_shim_segments.argtypes = [C.c_longlong, C.c_int, C.c_int]
        lib.probe_shim_tile_segments.argtypes = [C.c_int, C.c_longlong]
        lib.probe_shim_walk.argtypes = [C.c_longlong, C.c_int, C.c_longlong, I64P, C.c_longlong]
        lib.probe_shim_hist_grid.argtypes = [C.c_longlong, I64P]
        _LIB.append(lib)
    return _LIB[0]


class Ctx:
    def __init__(self, have_record=True, nsamples=1 << 20, fs=FS):
        self.args = (int(have_record), nsamples, fs)

    def __enter__(self):
        self.p = _shim().probe_shim_create(*self.args)
        return self.p

    def __exit__(self, *exc):
        _shim().probe_shim_destroy(self.p)


def _check(ctx, first=0, nsamples=4096, nfft=64, noverlap=4, window=1, nspans=1, have_p=True, have_psd=True, tile_bytes=0):
    from cu_sdr_collection_amd import _lib as L
    p = L.gc_probe_psd_params(first, nsamples, nfft, noverlap, window, nspans)
    out = (C.c_longlong * 4)(-7, -7, -7, -7)
    rc = _shim().probe_shim_check(ctx, C.addressof(p) if have_p else None, int(have_psd), tile_bytes, out)
    return rc, list(out)


# ---- K -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,noverlap", [(2, 0), (2, 1), (8, 1), (60, 3), (64, 63), (1000, 62), (32768, 2048)])
def test_segment_count_for_leftovers_of_none_one_and_a_step_less_one(nfft, noverlap):
    step = nfft - noverlap
    for k in (1, 2, 7):
        exact = noverlap + k * step                                    # k segments and nothing left over
        for left in sorted({0, 1, step - 1} & set(range(step))):      # (a step of 1 has no leftover of 1)
            assert _shim().probe_shim_segments(exact + left, nfft, noverlap) == k, (k, left)
            # the last segment ends inside the span: (K - 1) * step + nfft <= nsamples
            assert (k - 1) * step + nfft <= exact + left < k * step + nfft
    assert _shim().probe_shim_segments(nfft, nfft, noverlap) == 1      # the shortest span the call accepts


def test_accepted_call_returns_step_segments_and_the_tile_of_the_budget():
    with Ctx() as ctx:
        rc, (step, K, total, tile) = _check(ctx, first=5, nsamples=4096 + 59, nfft=64, noverlap=4, nspans=3)
        assert (rc, step, K, total) == (OK, 60, (4096 + 59 - 4) // 60, 3 * ((4096 + 59 - 4) // 60))
        assert tile == (128 << 20) // (2 * 64 * 8)                      # two float2 rows per segment in 128 MB
        for nseg in (1, 2, 3, 5):
            assert _check(ctx, tile_bytes=nseg * 2 * 64 * 8)[1][3] == nseg
        assert _check(ctx, tile_bytes=1)[1][3] == 1                     # never less than one segment
    assert _shim().probe_shim_tile_segments(32768, 0) == 256            # the reference's call: 256 rows of 256 KB, twice, in 128 MB


# ---- the tile walk -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 2, 3, 5])
@pytest.mark.parametrize("K,nspans", [(1, 1), (1, 4), (2, 3), (3, 1), (4, 5), (7, 3), (10, 2), (11, 4)])
def test_every_segment_is_added_once_in_order_and_a_straddled_span_is_carried(tile, K, nspans):
    cap = 8 * (K * nspans + 4) + 64
    buf = (C.c_longlong * cap)()
    n = _shim().probe_shim_walk(K, nspans, tile, buf, cap)
    assert 0 < n <= cap
    v, i = list(buf[:n]), 0
    acc, next_g, tiles = {}, 0, 0
    while i < n:
        g0, cnt, s0, s1 = v[i:i + 4]
        i += 4
        assert g0 == next_g and 1 <= cnt <= tile                        # consecutive runs of the whole list, none empty
        assert cnt == tile or g0 + cnt == K * nspans                    # only the last one is short
        assert (s0, s1) == (g0 // K, (g0 + cnt - 1) // K)
        rows = []                                                       # the tile's rows in the order the gather kernel writes them
        for s in range(s0, s1 + 1):
            span, k0, k1 = v[i:i + 3]
            i += 3
            assert span == s and 0 <= k0 < k1 <= K                      # every span the launch covers has work in this tile
            if k0 > 0:
                assert acc[s] == list(range(k0)), "a span that began in an earlier tile is carried, not restarted"
            else:
                assert s not in acc
                acc[s] = []
            acc[s] += list(range(k0, k1))
            rows += [s * K + k for k in range(k0, k1)]
        assert rows == list(range(g0, g0 + cnt))                        # ... and they are exactly the tile's segments
        next_g += cnt
        tiles += 1
    assert next_g == K * nspans and tiles == -(-K * nspans // tile)
    assert acc == {s: list(range(K)) for s in range(nspans)}


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_psd_refusals_that_need_no_device():
    with Ctx(nsamples=10000) as ctx:
        assert _check(ctx)[0] == OK
        bad = [dict(have_p=False), dict(have_psd=False), dict(first=-1), dict(nsamples=0), dict(nsamples=-5), dict(nspans=0), dict(nspans=-1),
               dict(nfft=1), dict(nfft=0), dict(nfft=-64), dict(noverlap=-1), dict(noverlap=64), dict(noverlap=65), dict(nsamples=63),
               dict(window=2), dict(window=-1)]
        for kw in bad:
            rc, out = _check(ctx, **kw)
            assert rc == INVALID and out == [-7] * 4, kw
        assert _shim().probe_shim_check(None, None, 1, 0, (C.c_longlong * 4)()) == INVALID          # null ctx
        # the record's end: the last span may end ON it
        assert _check(ctx, first=10000 - 4096)[0] == OK
        assert _check(ctx, first=10000 - 4095)[0] == RANGE
        assert _check(ctx, first=0, nsamples=5000, nspans=2)[0] == OK
        assert _check(ctx, first=1, nsamples=5000, nspans=2)[0] == RANGE
        assert _check(ctx, first=10001, nsamples=64)[0] == RANGE
        assert _check(ctx, first=0, nsamples=1 << 62, nspans=1 << 30)[0] == RANGE                    # no product that leaves int64
        assert _check(ctx, nsamples=64, nfft=64, noverlap=63)[0] == OK                               # nsamples == nfft: one segment
    with Ctx(have_record=False) as ctx:
        assert _check(ctx)[0] == STATE
    with Ctx(fs=0.0) as ctx:
        assert _check(ctx)[0] == STATE
    with Ctx(have_record=False) as ctx:
        assert _check(ctx, nfft=1)[0] == INVALID                                                    # arguments before state


def test_histogram_refusals_that_need_no_device():
    h = _shim().probe_shim_check_histogram
    with Ctx(nsamples=1000, fs=0.0) as ctx:                                                        # the histogram needs no sampling frequency
        assert h(ctx, 0, 1000, 1) == OK and h(ctx, 999, 1, 1) == OK
        assert h(ctx, 0, 1001, 1) == RANGE and h(ctx, 1000, 1, 1) == RANGE and h(ctx, 5, 1 << 62, 1) == RANGE
        assert h(ctx, -1, 10, 1) == INVALID and h(ctx, 0, 0, 1) == INVALID and h(ctx, 0, 10, 0) == INVALID
        assert h(None, 0, 10, 1) == INVALID
    with Ctx(have_record=False) as ctx:
        assert h(ctx, 0, 10, 1) == STATE


def test_planner_refuses_the_lengths_the_probe_refuses():
    from cu_sdr_collection_amd import _lib as L
    lib = L.load()
    ints = [C.c_int(0) for _ in range(6)]
    r1, r2 = (C.c_int * 12)(), (C.c_int * 12)()

    def plan(n):
        return lib.gc_debug_fft_plan(n, C.byref(ints[0]), C.byref(ints[1]), r1, C.byref(ints[2]), r2, C.byref(ints[3]), C.byref(ints[4]), C.byref(ints[5]))
    assert plan(7) == UNSUPPORTED and plan(32736) == UNSUPPORTED and plan(1 << 23) == UNSUPPORTED
    for n in (2, 8, 60, 64, 1000, 1024, 4096, 32768):
        assert plan(n) == OK and ints[0].value * ints[1].value == n
    assert lib.gc_debug_probe_tile_segments(32768) == 256 and lib.gc_debug_probe_tile_segments(64) == 131072
    assert lib.gc_debug_probe_tile_segments(1) == 0


# ---- the histogram's grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096, 4097, 100003, 18_000_000, 1_080_000_000, (1 << 42) + 1, 1 << 50])
def test_histogram_grid_covers_the_range_with_32_bit_partial_counts(n):
    out = (C.c_longlong * 2)()
    _shim().probe_shim_hist_grid(n, out)
    per, grid = out[0], out[1]
    assert per % 256 == 0 and 4096 <= per <= 1 << 31                   # a workgroup's 32-bit counts cannot overflow
    assert (grid - 1) * per < n <= grid * per                          # every sample in exactly one workgroup, none of them idle
    assert grid <= 2048 or per == 1 << 31
