"""mask_words of csrc/corr_common.h (the edge masks of every chunked correlator kernel) without a GPU.

Since round 9 mask_words derives the chunk's valid sample range [max(0, -i0), min(SPL, N - i0)) once and takes every word's mask
from it; before, it tested sample by sample.  tests/mask_words_shim.hip runs it on the CPU next to a reference that tests every
sample on its own and clears its bits one by one.  The sweep is exhaustive over the six record modes with the chunk lengths the
kernels instantiate (16 and 8 samples for int8 I/Q and Q/I, 8 for the others), i0 in [-SPL - 1, SPL + 1] and N in [0, 3 SPL + 1]:
chunks that start before the block, end behind it, do both, lie outside it altogether, and blocks of no sample at all.  The words
must be equal in every case, on all-ones words and on a random pattern (a mask may only clear bits).  The shim's reference is itself
checked against a restatement in numpy, so that the two C++ functions cannot be wrong in the same way unnoticed.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = {"i8_iq": (0, 2), "i8_qi": (1, 2), "i16_iq": (2, 4), "i16_qi": (3, 4), "i8_real": (4, 1), "i16_real": (5, 2)}   # (Mode, bytes per sample)
CASES = [("i8_iq", 16), ("i8_qi", 16), ("i8_iq", 8), ("i8_qi", 8), ("i16_iq", 8), ("i16_qi", 8), ("i8_real", 8), ("i16_real", 8)]
_LIB = []


def _shim():
    if _LIB:
        return _LIB[0]
    from cu_sdr_collection_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(HERE, "mask_words_shim.hip")
    out = os.path.join(HERE, "build", "libmask_words_shim.so")
    deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = [f for f in B._tu_flags("corr_fast.hip") if f != "--offload-compress"]
        subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
    lib = C.CDLL(out)
    words = C.POINTER(C.c_uint)
    lib.mask_shim_run.argtypes = [C.c_int, C.c_int, words, C.c_int, C.c_int, words, words]
    lib.mask_shim_sweep.argtypes = [C.c_int, C.c_int, words, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    _LIB.append(lib)
    return lib


def _pattern(mode, spl):
    rng = np.random.default_rng(1000 * MODES[mode][0] + spl)
    w = rng.integers(0, 1 << 32, size=8, dtype=np.uint64).astype(np.uint32)
    return w | np.uint32(0x01010101)            # no sample of the pattern is zero: a sample left unmasked by mistake shows


def _numpy_reference(words, bps, spl, i0, n):
    """The chunk's bytes with every sample outside [0, n) cleared."""
    by = words[:spl * bps // 4].copy().view(np.uint8).reshape(spl, bps)          # little-endian words: sample j = bytes j*bps ..
    i = i0 + np.arange(spl)
    by[(i < 0) | (i >= n)] = 0
    return by.reshape(-1).view(np.uint32)


@pytest.mark.parametrize("mode,spl", CASES)
def test_range_masks_equal_the_per_sample_reference(mode, spl):
    lib = _shim()
    pat = _pattern(mode, spl)
    bad, first = C.c_int(0), (C.c_int * 2)()
    cases = lib.mask_shim_sweep(MODES[mode][0], spl, pat.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(bad), first)
    assert cases == (2 * spl + 3) * (3 * spl + 2) * 2, cases                    # every (i0, N) of the sweep, two word patterns
    assert bad.value == 0, (mode, spl, bad.value, "first at i0, N =", first[0], first[1])


@pytest.mark.parametrize("mode,spl", CASES)
def test_the_shims_reference_is_the_rule(mode, spl):
    lib = _shim()
    m, bps = MODES[mode]
    pat = _pattern(mode, spl)
    got, want = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))
    seen = set()
    for i0 in range(-spl - 1, spl + 2):
        for n in range(0, 3 * spl + 2):
            nw = lib.mask_shim_run(m, spl, ptr(pat), i0, n, ptr(got), ptr(want))
            assert nw == spl * bps // 4
            ref = _numpy_reference(pat, bps, spl, i0, n)
            assert np.array_equal(want[:nw], ref), (mode, spl, i0, n)
            assert np.array_equal(got[:nw], ref), (mode, spl, i0, n)
            valid = np.flatnonzero((i0 + np.arange(spl) >= 0) & (i0 + np.arange(spl) < n))
            seen.add((int(valid[0]), int(valid[-1]) + 1) if valid.size else None)
    # the sweep reaches every range a chunk can have: empty, and every [lo, hi) with 0 <= lo < hi <= SPL
    assert seen == {None} | {(lo, hi) for lo in range(spl) for hi in range(lo + 1, spl + 1)}


def test_a_mode_the_kernels_do_not_instantiate_is_refused():
    lib = _shim()
    z = np.zeros(8, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))
    assert lib.mask_shim_run(MODES["i16_iq"][0], 16, ptr(z), 0, 16, ptr(z.copy()), ptr(z.copy())) == 0
