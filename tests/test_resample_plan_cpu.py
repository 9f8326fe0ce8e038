"""The host plan of the resampler (csrc/resample_plan.h: gc_resample's argument checks, the NCO's two integers, the branches of the
polyphase filter, the tile of outputs a workgroup takes with its input span and LDS bytes, the tile walk) without a GPU:
tests/resample_plan_shim.hip runs it on the CPU.

Refusals: every status of gc_resample that needs no device, each next to the accepted call that closes it; a refused call leaves the
plan unwritten.  NCO: phase_step (per tick) and out_rate against Python integers and Fraction.  Tile: every output in exactly one
tile, in order; each output's samples inside its tile's span, the span inside what the kernel stages (the arithmetic is the kernel's
own, shared through the header), the staged bytes inside the plan's LDS bytes, those inside 60 KB - over the corners and a sweep of
(L, M, T).  With L = 1 the tile is the down-converter's.

The last test follows the numpy model (tests/resample_model.py) by hand on cases small enough for that.  It holds the reference the
GPU tests compare against, not the library: it is the one test here that passes without the feature."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OK, INVALID, RANGE, STATE = 0, -1, -2, -5
I8, I16 = 0, 1
REAL, IQ, QI = 0, 1, 2
I64P = C.POINTER(C.c_longlong)
U64P = C.POINTER(C.c_ulonglong)
A0, A1 = 1 << 20, 1 << 24                                               # two addresses; never read
MASK = (1 << 64) - 1
_LIB = []


def _shim():
    if not _LIB:
        from cu_sdr_collection_amd import build as B
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not found")
        assert "resample.hip" in B.NO_CONTRACT and "resample_plan.h" in B.HEADERS and "resample.hip" in B.LIBS["libgnsscorr.so"]
        src, out = os.path.join(HERE, "resample_plan_shim.hip"), os.path.join(HERE, "build", "libresample_plan_shim.so")
        deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = [f for f in B._tu_flags("resample.hip") if f != "--offload-compress"]
            subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
        lib = C.CDLL(out)
        lib.rs_shim_create.restype = C.c_void_p
        lib.rs_shim_create.argtypes = [C.c_longlong, C.c_int, C.c_ulonglong, C.c_int, C.c_int, C.c_double]
        lib.rs_shim_destroy.argtypes = [C.c_void_p]
        lib.rs_shim_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, U64P, C.POINTER(C.c_double)]
        lib.rs_shim_tile_outputs.restype = lib.rs_shim_ddc_tile_outputs.restype = lib.rs_shim_lds_bytes.restype = lib.rs_shim_walk.restype = C.c_longlong
        lib.rs_shim_tile_outputs.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.rs_shim_ddc_tile_outputs.argtypes = [C.c_int, C.c_int]
        lib.rs_shim_lds_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.rs_shim_geometry.argtypes = [C.c_int, C.c_int, C.c_int, I64P]
        lib.rs_shim_walk.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, I64P, C.c_longlong]
        lib.rs_shim_output.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, I64P]
        lib.rs_shim_stage.argtypes = [C.c_longlong, C.c_longlong, C.c_int, I64P]
        lib.rs_shim_constants.argtypes = [I64P]
        _LIB.append(lib)
    return _LIB[0]


class Ctx:
    def __init__(self, address=A0, device=0, nsamples=40000, dtype=I8, layout=IQ, fs=18e6):
        self.args = (address, device, nsamples, dtype, layout, fs)

    def __enter__(self):
        self.p = _shim().rs_shim_create(*self.args)
        return self.p

    def __exit__(self, *exc):
        _shim().rs_shim_destroy(self.p)


PLAN = ["phase_step", "phase0", "tile", "ntiles", "span", "lds_bytes", "lds_budget", "src_bps", "dst_bps", "branches", "row", "stride"]
UNWRITTEN = 0xDEADBEEF


def _check(src, dst, first_tick=0, noutputs=1000, dst_first=0, interp=2, decim=5, ntaps=41, reserved=0, carr_freq=0.0, carr_phase=0.0,
           taps="ones", have_p=True):
    from cu_sdr_collection_amd import _lib as L
    p = L.gc_rs_params(first_tick, noutputs, dst_first, interp, decim, ntaps, reserved, carr_freq, carr_phase)
    out = (C.c_ulonglong * len(PLAN))(*[UNWRITTEN] * len(PLAN))
    dbl = (C.c_double * 2)(-7.0, -7.0)
    if isinstance(taps, str):
        taps = np.ones((max(ntaps, 1), 2))
    t = None if taps is None else np.ascontiguousarray(taps, dtype=np.float64)
    rc = _shim().rs_shim_check(src, dst, C.addressof(p) if have_p else None, None if t is None else t.ctypes.data_as(C.c_void_p), out, dbl)
    return rc, dict(zip(PLAN, out)), list(dbl)


def _accepted(r):
    rc, plan, dbl = r
    return rc == OK and all(v != UNWRITTEN for v in plan.values()) and all(v != -7.0 for v in dbl)


def _refused(r, status):
    rc, plan, dbl = r
    return rc == status and all(v == UNWRITTEN for v in plan.values()) and all(v == -7.0 for v in dbl)


def _constants():
    out = (C.c_longlong * 8)()
    _shim().rs_shim_constants(out)
    return list(out)


def _geometry(L, M, T):
    out = (C.c_longlong * 5)()
    _shim().rs_shim_geometry(L, M, T, out)
    return list(out)


def test_constants():
    from cu_sdr_collection_amd import _lib as L
    wg, chains, max_tile, budget, max_taps, max_interp, slack, max_decim = _constants()
    assert max_taps == L.GC_RS_MAX_TAPS == 2048 and max_interp == L.GC_RS_MAX_INTERP == 64 and max_decim == L.GC_DDC_MAX_DECIM == 64
    assert max_tile == wg * chains == 1024 and wg % 64 == 0
    assert budget == 60 * 1024
    assert slack >= 30                                                  # up to 15 bytes in front of the span and 15 behind


def test_every_refusal_next_to_the_call_that_closes_it():
    with Ctx() as src, Ctx(address=A1, nsamples=5000) as dst, Ctx(address=0) as empty, Ctx(address=A1, device=1) as other, \
            Ctx(address=A1, fs=0.0) as nofs:
        assert _accepted(_check(src, dst))
        # null arguments
        assert _refused(_check(None, dst), INVALID) and _refused(_check(src, None), INVALID)
        assert _refused(_check(src, dst, have_p=False), INVALID) and _refused(_check(src, dst, taps=None), INVALID)
        # the integers
        assert _refused(_check(src, dst, first_tick=-1), INVALID) and _accepted(_check(src, dst, first_tick=0))
        assert _refused(_check(src, dst, dst_first=-1), INVALID) and _accepted(_check(src, dst, dst_first=0))
        assert _refused(_check(src, dst, noutputs=0), INVALID) and _accepted(_check(src, dst, noutputs=1))
        assert _refused(_check(src, dst, interp=0), INVALID) and _accepted(_check(src, dst, interp=1))
        assert _refused(_check(src, dst, interp=65), INVALID) and _accepted(_check(src, dst, interp=64))
        assert _refused(_check(src, dst, decim=0), INVALID) and _accepted(_check(src, dst, decim=1))
        assert _refused(_check(src, dst, interp=1, decim=65, noutputs=10), INVALID) and _accepted(_check(src, dst, interp=1, decim=64, noutputs=10))
        assert _refused(_check(src, dst, interp=2, decim=129, noutputs=10), INVALID) and _accepted(_check(src, dst, interp=2, decim=128, noutputs=10))
        assert _refused(_check(src, dst, interp=64, decim=4097, noutputs=10), INVALID) and _accepted(_check(src, dst, interp=64, decim=4096, noutputs=10))
        assert _refused(_check(src, dst, ntaps=0), INVALID) and _accepted(_check(src, dst, ntaps=1))
        assert _refused(_check(src, dst, ntaps=2049), INVALID) and _accepted(_check(src, dst, ntaps=2048))
        assert _refused(_check(src, dst, reserved=1), INVALID) and _refused(_check(src, dst, reserved=-1), INVALID)
        # the last tick in 63 bits: first_tick + (noutputs - 1) M <= 2^63 - 1 (and then no record sample under it: range, not arguments)
        top = (1 << 63) - 1
        assert _refused(_check(src, dst, first_tick=top - 5 * 999 + 1, noutputs=1000), INVALID)
        assert _refused(_check(src, dst, first_tick=top - 5 * 999, noutputs=1000), RANGE)
        assert _refused(_check(src, dst, first_tick=top, noutputs=2), INVALID) and _refused(_check(src, dst, first_tick=top, noutputs=1), RANGE)
        # what is not finite
        for bad in (float("nan"), float("inf"), -float("inf")):
            t = np.ones((41, 2))
            t[40, 1] = bad
            assert _refused(_check(src, dst, taps=t), INVALID)
            assert _refused(_check(src, dst, carr_freq=bad), INVALID) and _refused(_check(src, dst, carr_phase=bad), INVALID)
        t = np.ones((41, 2))
        t[40, 1] = 1e308
        assert _accepted(_check(src, dst, taps=t)) and _accepted(_check(src, dst, carr_phase=1e300))
        # the carrier against the INPUT's sampling frequency, whatever L
        for L in (1, 3, 64):
            assert _refused(_check(src, dst, interp=L, carr_freq=9e6), INVALID) and _refused(_check(src, dst, interp=L, carr_freq=-9e6), INVALID)
            assert _accepted(_check(src, dst, interp=L, carr_freq=math.nextafter(9e6, 0.0)))
            assert _accepted(_check(src, dst, interp=L, carr_freq=-math.nextafter(9e6, 0.0)))
        # state
        assert _refused(_check(empty, dst), STATE) and _refused(_check(src, empty), STATE)
        assert _refused(_check(nofs, src), STATE) and _accepted(_check(src, nofs))     # dst needs no sampling frequency
        # device
        assert _refused(_check(src, other), INVALID)
        # dst's record is src's, or overlaps it: src holds 80000 bytes from A0
        assert _refused(_check(src, src), INVALID)
        with Ctx(address=A0) as same, Ctx(address=A0 + 79999) as last_byte, Ctx(address=A0 + 80000) as behind, \
                Ctx(address=A0 - 10000, nsamples=5000) as in_front, Ctx(address=A0 - 10000, nsamples=5001) as into:
            assert _refused(_check(src, same), INVALID) and _refused(_check(src, last_byte), INVALID)
            assert _accepted(_check(src, behind)) and _accepted(_check(src, in_front)) and _refused(_check(src, into), INVALID)
        # dst's range
        assert _refused(_check(src, dst, noutputs=5001), RANGE) and _accepted(_check(src, dst, noutputs=5000))
        assert _refused(_check(src, dst, dst_first=4001), RANGE) and _accepted(_check(src, dst, dst_first=4000))
        assert _refused(_check(src, dst, dst_first=5001, noutputs=1), RANGE) and _accepted(_check(src, dst, dst_first=4999, noutputs=1))
        # the last output's oldest sample must be a record sample: (last tick div L) - (J - 1) <= 39999; L = 2, T = 41: J = 21
        assert _accepted(_check(src, dst, first_tick=2 * 40020 - 1, noutputs=1)) and _refused(_check(src, dst, first_tick=2 * 40020, noutputs=1), RANGE)
        assert _accepted(_check(src, dst, first_tick=2 * 40019 + 1 - 5 * 99, noutputs=100)) and _refused(_check(src, dst, first_tick=2 * 40020 - 5 * 99, noutputs=100), RANGE)
        # L = 1 is the down-converter's bound: first + (nout - 1) D - (T - 1) <= 39999
        assert _accepted(_check(src, dst, interp=1, decim=8, ntaps=25, first_tick=24, noutputs=5000))
        assert _refused(_check(src, dst, interp=1, decim=8, ntaps=25, first_tick=32, noutputs=5000), RANGE)
        # arguments come before state, state before range
        assert _refused(_check(empty, dst, decim=0), INVALID) and _refused(_check(empty, dst, reserved=3), INVALID)
        assert _refused(_check(empty, dst, noutputs=5001), STATE)


def _py_step(f, rate):
    return int(round(Fraction(math.ldexp(f / rate, 64))))                # to nearest, ties to even: llrint


@pytest.mark.parametrize("L", [1, 3, 64])
@pytest.mark.parametrize("fs", [18e6, 50e6])
def test_nco_integers_and_the_output_rate_are_pythons(fs, L):
    """phase_step per tick against Python integers, out_rate against Fraction: (fs L) / M with each operation rounded by itself."""
    import resample_model as RM
    rate = fs * float(L)
    assert Fraction(rate) == Fraction(fs) * L                            # fs L is exact for these rates: one rounding, in the division
    with Ctx(fs=fs) as src, Ctx(address=A1) as dst:
        for f in (0.0, 1.0, -1.0, fs / 2 - 1.0, -(fs / 2 - 1.0), 2000137.0, -4500137.0, 123456.789):
            for M in (1, 5, 63 * L):
                rc, plan, (freq, out_rate) = _check(src, dst, interp=L, decim=M, noutputs=10, carr_freq=f, carr_phase=100.0)
                want = _py_step(f, rate)
                assert rc == OK and plan["phase_step"] == want & MASK == RM.rs_phase_step(f, fs, L), (f, fs, L)
                assert plan["phase0"] == RM.phase0(100.0)
                signed = want
                assert freq == math.ldexp(float(signed), -64) * rate == RM.rs_nco_freq(want & MASK, fs, L)
                assert abs(freq - f) <= 1e-6                             # half a step of fs L 2^-64, and the product's rounding
                assert out_rate == rate / M == RM.out_rate(fs, L, M)
                assert abs(Fraction(out_rate) - Fraction(rate) / M) <= Fraction(math.ulp(out_rate)) / 2
    with Ctx(fs=18e6) as src, Ctx(address=A1) as dst:
        assert _check(src, dst, interp=2, decim=9)[2][1] == 4e6 and _check(src, dst, interp=2, decim=5)[2][1] == 7.2e6


CORNERS = [(1, 1, 1), (1, 64, 2048), (64, 1, 64), (64, 4096, 2048), (64, 63, 2048), (7, 64, 701), (4, 6, 129)]
SWEEP = [(L, M, T) for L in (1, 2, 3, 5, 16, 37, 63, 64) for M in (1, 2, 3, 50, 64 * L - 1, 64 * L) for T in (1, 2, L, 700, 2047, 2048)]


@pytest.mark.parametrize("L,M,T", CORNERS + [c for c in SWEEP if c not in CORNERS])
def test_tiles_cover_every_output_once_and_stage_what_they_read(L, M, T):
    lib = _shim()
    wg, chains, max_tile, budget, *_ = _constants()
    lp, stride, J, row, taps_bytes = _geometry(L, M, T)
    assert lp == L // math.gcd(L, M) and J == -(-T // L)
    assert stride % lp == 0 and stride <= wg < stride + lp               # the largest multiple of Lp in the workgroup
    assert (stride * M) % L == 0                                         # a lane's chains share its phase
    assert row >= J and (L == 1 or row % 2 == 1) and taps_bytes == 16 * L * row >= 16 * T
    tile = lib.rs_shim_tile_outputs(L, M, T)
    assert 1 <= tile <= chains * stride <= max_tile
    assert lib.rs_shim_lds_bytes(tile, L, M, T, 4) <= budget == 60 * 1024
    assert tile == chains * stride or lib.rs_shim_lds_bytes(tile + 1, L, M, T, 4) + 16 > budget  # as many as fit (to a vector)
    if L == 1:
        assert tile == lib.rs_shim_ddc_tile_outputs(M, T) and taps_bytes == 16 * T
    for noutputs in sorted({1, max(tile - 1, 1), tile, tile + 1, 3 * tile + 1}):
        for first in (0, 1, L - 1, 5 * L + 3, 12345):
            cap = 7 * (noutputs // tile + 2)
            out = (C.c_longlong * cap)()
            n = lib.rs_shim_walk(first, noutputs, L, M, T, out, cap)
            assert n % 7 == 0 and n <= cap
            tiles = [tuple(out[i:i + 7]) for i in range(0, n, 7)]
            assert len(tiles) == -(-noutputs // tile)
            nxt = 0
            for m0, cnt, u0, n0, p0, n_lo, n_hi in tiles:
                assert m0 == nxt and 1 <= cnt <= tile                                        # in order, no gap, no overlap
                nxt = m0 + cnt
                assert u0 == first + m0 * M and (n0, p0) == divmod(u0, L)
                assert n_lo == n0 - (J - 1) and n_hi == (u0 + (cnt - 1) * M) // L
                for q in sorted({0, 1 % cnt, cnt // 2, cnt - 1}):                             # an output's samples lie inside the span
                    o = (C.c_longlong * 2)()
                    lib.rs_shim_output(p0, q, L, M, o)
                    assert (n0 + o[0], o[1]) == divmod(u0 + q * M, L)
                    assert n_lo <= n0 + o[0] - (J - 1) and n0 + o[0] <= n_hi
                    assert 0 <= o[1] * row and (o[1] + 1) * row <= L * row                  # its tap row inside the staged taps
                assert n_hi - n_lo + 1 <= (( tile - 1) * M + L - 1) // L + J
                for bps in (1, 2, 4):
                    st = (C.c_longlong * 2)()
                    lib.rs_shim_stage(n_lo, n_hi, bps, st)
                    base, vecs = st
                    assert base % 16 == 0 and base <= n_lo * bps < base + 16                 # the first sample's vector
                    assert base + 16 * (vecs - 1) < (n_hi + 1) * bps <= base + 16 * vecs     # the last sample's vector, and no more
                    assert taps_bytes + 16 * vecs <= lib.rs_shim_lds_bytes(tile, L, M, T, bps) <= budget
            assert nxt == noutputs


def test_every_output_of_a_tile_has_one_lane_and_the_lane_one_phase():
    lib = _shim()
    wg, chains, *_ = _constants()
    for L, M, T in CORNERS + [(37, 50, 1999), (10, 4, 2048), (43, 1, 64), (51, 7, 100), (52, 3, 100)]:
        _, stride, _, _, _ = _geometry(L, M, T)
        tile = lib.rs_shim_tile_outputs(L, M, T)
        owner = {}
        for lane in range(min(stride, wg)):
            phases = set()
            for c in range(chains):
                q = lane + c * stride
                if q < tile:
                    assert q not in owner
                    owner[q] = lane
                    o = (C.c_longlong * 2)()
                    lib.rs_shim_output(L - 1, q, L, M, o)
                    phases.add(o[1])
            assert len(phases) <= 1
        assert sorted(owner) == list(range(tile))


def test_debug_hook_and_the_plan_agree():
    lib = _shim()
    for bad in ((0, 1, 5), (65, 1, 5), (1, 0, 5), (1, 65, 5), (2, 129, 5), (2, 5, 0), (2, 5, 2049)):
        assert lib.rs_shim_tile_outputs(*bad) == 0
    with Ctx(dtype=I16) as src, Ctx(address=A1) as dst:
        for L, M, T in ((2, 5, 41), (64, 63, 2048), (1, 1, 1), (1, 3, 25)):
            rc, plan, _ = _check(src, dst, interp=L, decim=M, ntaps=T, noutputs=50)
            tile = lib.rs_shim_tile_outputs(L, M, T)
            lp, stride, J, row, _ = _geometry(L, M, T)
            assert rc == OK and plan["tile"] == tile and plan["ntiles"] == -(-50 // tile)
            assert plan["span"] == ((tile - 1) * M + L - 1) // L + J and plan["src_bps"] == 4 and plan["dst_bps"] == 2
            assert plan["lds_bytes"] == lib.rs_shim_lds_bytes(tile, L, M, T, 4) <= plan["lds_budget"]
            assert (plan["branches"], plan["row"], plan["stride"]) == (J, row, stride)


def test_the_model_by_hand():
    import ddc_model as DM
    import resample_model as RM
    # L / M = 2 / 3 on the ramp 1 .. 6, real: ticks u = 0, 3, 6, 9, 12 -> (n, p) = (0,0) (1,1) (3,0) (4,1) (6,0); J = 2.
    # p = 0 meets g[0], g[2]; p = 1 meets g[1], g[3].
    x = np.arange(1, 7, dtype=np.int8)
    g = [1.0, 0.5, 0.25, 0.125]
    out, clipped, sum_sq, near, (yr, _) = RM.resample(x, RM.REAL, g, 2, 3, 18e6, np.int8, RM.REAL)
    # 1*x0 = 1;  .5*x1 + .125*x0 = 1.125;  1*x3 + .25*x2 = 4.75;  .5*x4 + .125*x3 = 3;  1*x6 (= 0) + .25*x5 = 1.5 -> 2 (tie to even);
    # u = 15: n = 7, its oldest sample 6 is no record sample: not an output
    assert yr.tolist() == [1.0, 1.125, 4.75, 3.0, 1.5] and out.tolist() == [1, 1, 5, 3, 2]
    assert clipped == 0 and sum_sq == 1 + 1 + 25 + 9 + 4 and near.tolist() == [False] * 4 + [True]
    assert RM.full_outputs(6, 4, 2, 3) == 5
    # T = 3: the phase-1 branch has one tap (k = 3 is skipped): .5*x1 = 1, .5*x4 = 2.5 -> 2 (tie to even)
    out, _, _, near, (yr, _) = RM.resample(x, RM.REAL, g[:3], 2, 3, 18e6, np.int8, RM.REAL)
    assert yr.tolist() == [1.0, 1.0, 4.75, 2.5, 1.5] and out.tolist() == [1, 1, 5, 2, 2] and near.tolist() == [False] * 3 + [True] * 2
    # first_tick moves the phase: u = 1, 4, 7 -> (0,1) (2,0) (3,1): .5*x0 = .5 -> 0; x2 + .25*x1 = 3.5 -> 4; .5*x3 + .125*x2 = 2.375
    out, _, _, _, (yr, _) = RM.resample(x, RM.REAL, g, 2, 3, 18e6, np.int8, RM.REAL, first_tick=1, noutputs=3)
    assert yr.tolist() == [0.5, 3.5, 2.375] and out.tolist() == [0, 4, 2]
    # a hold: L = 2, M = 1, taps (1, 1): every sample twice, and once more behind the record? no: J = 1, the last output sits on sample 5
    out, _, _, _, _ = RM.resample(x, RM.REAL, [1.0, 1.0], 2, 1, 18e6, np.int8, RM.REAL)
    assert out.tolist() == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    # L = M = 3 with the tap (1) copies the record
    iq = np.array([1, -2, 3, -4, 127, -128], dtype=np.int8)
    out, _, _, _, _ = RM.resample(iq, RM.IQ, [1.0], 3, 3, 18e6, np.int8, RM.IQ)
    assert out.tolist() == iq.tolist()
    # the NCO counts ticks: fs = 4, L = 2: 1 Hz is an eighth of a turn per tick, M = 2 a quarter turn per output
    c = np.tile(np.array([7, 0], dtype=np.int8), 8)
    out, _, sum_sq, near, _ = RM.resample(c, RM.IQ, [1.0, 1.0], 2, 2, 4.0, np.int8, RM.IQ, carr_freq=1.0)
    assert RM.rs_phase_step(1.0, 4.0, 2) == 1 << 61
    assert out.tolist() == [7, 0, 0, -7, -7, 0, 0, 7] * 2 and sum_sq == 8 * 49 and not near.any()
    # the same from tick 1 (phase 1 of the hold, an eighth of a turn on): 7 (cos 45, -sin 45) = (4.95, -4.95) -> (5, -5)
    out, _, _, _, _ = RM.resample(c, RM.IQ, [1.0, 1.0], 2, 2, 4.0, np.int8, RM.IQ, carr_freq=1.0, first_tick=1, noutputs=2)
    assert out.tolist() == [5, -5, -5, -5]
    # a complex tap on a Q/I source, gain 3 clipping, counted per stored component: ddc_model's cases through L = 2, M = 2 (p = 0 only)
    q = np.tile(np.array([2, 1], dtype=np.int16), 3)
    out, _, _, _, (yr, yi) = RM.resample(q, RM.QI, [0.5 - 0.25j, 99.0], 2, 2, 18e6, np.int16, RM.IQ)
    assert yr.tolist() == [1.0] * 3 and yi.tolist() == [0.75] * 3 and out.tolist() == [1, 1] * 3
    f = np.array([127, -128, 100, 1], dtype=np.int8)
    out, clipped, sum_sq, _, _ = RM.resample(f, RM.IQ, [3.0], 1, 1, 18e6, np.int8, RM.IQ)
    assert out.tolist() == [127, -128, 127, 3] and clipped == 3 and sum_sq == 127 * 127 * 2 + 128 * 128 + 9
    # L = 1 is ddc_model.downconvert, value for value
    rng = np.random.default_rng(7)
    raw = rng.integers(-128, 128, 2 * 300).astype(np.int8)
    taps = rng.standard_normal(25) + 1j * rng.standard_normal(25)
    a = RM.resample(raw, RM.IQ, taps / 8, 1, 3, 18e6, np.int8, RM.QI, carr_freq=2000137.0, carr_phase=100.0, first_tick=5)
    b = DM.downconvert(raw, DM.IQ, taps / 8, 3, 18e6, np.int8, DM.QI, carr_freq=2000137.0, carr_phase=100.0, first_sample=5)
    assert a[0].tolist() == b[0].tolist() and a[1:3] == b[1:3] and a[3].tolist() == b[3].tolist()
    assert a[4][0].tolist() == b[4][0].tolist() and a[4][1].tolist() == b[4][1].tolist()
