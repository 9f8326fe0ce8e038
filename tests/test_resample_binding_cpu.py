"""gc_resample at the boundary, without a GPU: declared in include/gnsscorr.h, exported by the library, bound by _lib.py with the
declared argument types; the two structs field by field, with the sizes (56, 48) and offsets the C compiler gives them; the two
constants the same on both sides; the API version unchanged (new entry points are detected by symbol); Engine.resample refuses taps
of another shape, values that are no whole numbers and an L or M out of range before any library call; the MEX gateway lists and
handles the command; receiver.resample_record's L / M and tap design against direct Fraction and firwin."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnsscorr.h")
STRUCTS = {"gc_rs_params": ["first_tick", "noutputs", "dst_first", "interp", "decim", "ntaps", "reserved", "carr_freq", "carr_phase"],
           "gc_rs_result": ["phase_step", "phase0", "clipped", "sum_sq", "carr_freq", "out_rate"]}
SIZES = {"gc_rs_params": 56, "gc_rs_result": 48}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"include/gnsscorr.h does not declare {name}"
    return [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_gc_resample_and_the_binding_has_its_argument_types():
    from cu_sdr_collection_amd import _lib as L
    ctypes_of = {"gc_context*": C.c_void_p, "const gc_rs_params*": C.POINTER(L.gc_rs_params), "const double*": C.POINTER(C.c_double),
                 "gc_rs_result*": C.POINTER(L.gc_rs_result)}
    params = ["gc_context*", "gc_context*", "const gc_rs_params*", "const double*", "gc_rs_result*"]
    assert _params("gc_resample") == params
    res, args = L.SYMBOLS["gc_resample"]
    assert res is C.c_int and args == [ctypes_of[p] for p in params]
    lib = L.load()
    assert hasattr(lib, "gc_resample") and lib.gc_resample.argtypes == args
    assert lib.gc_api_version() == 4                      # an addition, not a break
    assert re.search(r"\blong long\s+gc_debug_rs_tile_outputs\s*\(\s*int\s+interp\s*,\s*int\s+decim\s*,\s*int\s+ntaps\s*\)\s*;", _header())
    assert L.SYMBOLS["gc_debug_rs_tile_outputs"] == (C.c_longlong, [C.c_int, C.c_int, C.c_int])
    assert lib.gc_debug_rs_tile_outputs(1, 3, 25) == lib.gc_debug_ddc_tile_outputs(3, 25) == 1024
    assert lib.gc_debug_rs_tile_outputs(1, 64, 2048) == lib.gc_debug_ddc_tile_outputs(64, 2048)
    assert lib.gc_debug_rs_tile_outputs(2, 5, 41) == 1024 and lib.gc_debug_rs_tile_outputs(3, 2, 33) == 4 * 255
    assert 1 <= lib.gc_debug_rs_tile_outputs(64, 4096, 2048) < 256
    for bad in ((0, 1, 25), (65, 1, 25), (1, 0, 25), (1, 65, 25), (64, 4097, 25), (2, 5, 0), (2, 5, 2049)):
        assert lib.gc_debug_rs_tile_outputs(*bad) == 0, bad
    # a null argument is refused before any device is looked for
    assert lib.gc_resample(None, None, None, None, None) == L.GC_E_INVALID
    p = L.gc_rs_params(0, 1, 0, 1, 1, 1, 0, 0.0, 0.0)
    one = (C.c_double * 2)(1.0, 0.0)
    assert lib.gc_resample(None, None, C.byref(p), one, None) == L.GC_E_INVALID


def test_structs_and_the_constants_are_the_same_on_both_sides_and_as_the_c_compiler_sees_them():
    from cu_sdr_collection_amd import _lib as L
    h = _header()
    m = re.search(r"#define\s+GC_RS_MAX_TAPS\s+(\d+)", h)
    assert m and int(m.group(1)) == L.GC_RS_MAX_TAPS == 2048
    m = re.search(r"#define\s+GC_RS_MAX_INTERP\s+(\d+)", h)
    assert m and int(m.group(1)) == L.GC_RS_MAX_INTERP == 64
    assert re.search(r"#define\s+GC_API_VERSION\s+4\b", h)
    for name, fields in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), h, flags=re.S)
        assert body, name
        declared = [f for decl in body.group(1).split(";") if decl.strip() for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
        assert declared == fields == [f for f, _ in getattr(L, name)._fields_], name
    lines = ['printf("%d %d %d\\n", GC_RS_MAX_TAPS, GC_RS_MAX_INTERP, GC_API_VERSION);']
    for name, fields in STRUCTS.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % name)
        lines += ['printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f) for f in fields]
    prog = "#include <stddef.h>\n#include <stdio.h>\n#include \"gnsscorr.h\"\nint main(void) {\n  %s\n  return 0;\n}\n" % "\n  ".join(lines)
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert got.pop(0) == [L.GC_RS_MAX_TAPS, L.GC_RS_MAX_INTERP, 4]
    for name, fields in STRUCTS.items():
        cls = getattr(L, name)
        assert got.pop(0) == [C.sizeof(cls)] == [SIZES[name]], name
        for f in fields:
            d = getattr(cls, f)
            assert got.pop(0) == [d.offset, d.size], (name, f)
    assert not got


class _NoLibrary:
    """Stands where an Engine would: any use is a library call that came too early."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was used ({name}) before the arguments were checked")


def test_engine_resample_refuses_taps_and_numbers_that_do_not_fit_before_any_library_call():
    import cu_sdr_collection_amd as P
    eng = object.__new__(P.Engine)                        # no context, no library: a call that got past the checks would fail otherwise
    eng._lib = eng._ctx = _NoLibrary()
    dst = _NoLibrary()
    for bad in (np.ones((4, 3)), np.ones((2, 2, 2)), np.ones((4, 2), dtype=complex), np.array(["a"] * 4), 1.0, np.ones(0), np.ones(2049),
                np.ones((2049, 2))):
        with pytest.raises(ValueError, match=r"resample\(\): .*taps"):
            P.Engine.resample(eng, dst, bad, 2, 5)
    good = dict(interp=2, decim=5, first_tick=0, noutputs=10, dst_first=0)
    for name, bad in (("interp", 2.5), ("interp", None), ("interp", 0), ("interp", 65), ("interp", -1), ("decim", 2.5), ("decim", None), ("decim", 1 << 31),
                      ("decim", 0), ("decim", 129), ("first_tick", 0.5), ("first_tick", "3"), ("noutputs", 1 << 63), ("noutputs", True),
                      ("dst_first", 1.25), ("dst_first", -(1 << 63) - 1)):
        with pytest.raises(ValueError, match=r"resample\(\): .*" + name):
            P.Engine.resample(eng, dst, np.ones(4), **dict(good, **{name: bad}))
    with pytest.raises(ValueError, match="decim"):
        P.Engine.resample(eng, dst, np.ones(4), 64, 4097, noutputs=10)
    eng._ctx = None                                       # (close() in __del__ then has nothing to do)


def test_mex_gateway_lists_and_handles_the_command():
    text = open(os.path.join(ROOT, "matlab", "gnsscorr_mex.c")).read()
    head = text[:text.index("#include")]
    assert "gnsscorr_mex('resample'" in head              # the usage line in the file's head
    assert 'strcmp(cmd, "resample")' in text and "gc_resample(" in text
    wrapper = open(os.path.join(ROOT, "matlab", "gnsscorr_resample.m")).read()
    assert "gnsscorr_mex('resample'" in wrapper


def test_the_receivers_ratio_is_the_fraction_in_lowest_terms():
    from cu_sdr_collection_amd import receiver as R
    for fs, fs_out in ((18e6, 4e6), (18e6, 8e6), (50e6, 20e6), (16.368e6, 4.092e6), (53e6, 26e6), (26e6, 25e6), (18e6, 18e6), (4e6, 18e6)):
        want = Fraction(fs_out / fs).limit_denominator(4096)
        assert R.resample_ratio(fs, fs_out) == (want.numerator, want.denominator), (fs, fs_out)
        L, M = R.resample_ratio(fs, fs_out)
        assert math.gcd(L, M) == 1 and 1 <= L <= 64 and 1 <= M <= 64 * L and abs(fs * L / M - fs_out) <= 1e-9 * fs_out
    assert R.resample_ratio(18e6, 4e6) == (2, 9) and R.resample_ratio(50e6, 20e6) == (2, 5)
    for fs, fs_out, word in ((16.368e6, 18e6, "L = 375"), (18e6, 18e6 / 65, "lowers the rate"), (18e6, 18e6 * 65, "L = 65"), (18e6, 18e6 / math.pi, "no fraction"),
                             (18e6, 0.0, "positive"), (0.0, 4e6, "positive")):
        with pytest.raises(ValueError, match=word):
            R.resample_ratio(fs, fs_out)


def test_the_receivers_tap_design_is_firwin_at_the_tick_rate_moved_to_the_nco_frequency():
    from scipy.signal import firwin

    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import receiver as R
    assert P.resample_record is R.resample_record and "resample_record" in P.__all__
    fs, fc, bw, L, M, T = 18e6, 4500137.0, 2.4e6, 2, 9, 145
    rate = fs * L
    g, f_used, h = R.resample_taps(fs, L, M, fc, bw, T)
    step = int(round(Fraction(math.ldexp(fc / rate, 64))))
    assert R.ddc_nco_step(fc, rate) == step
    assert f_used == math.ldexp(float(step), -64) * rate and abs(f_used - fc) < 1e-8
    want_h = L * firwin(T, bw / 2, fs=rate)
    assert np.array_equal(h, want_h) and abs(h.sum() - L) < 1e-12         # gain L at DC: 1 after the zeros between the samples
    want = want_h * np.exp(2j * np.pi * f_used * np.arange(T) / rate)
    assert np.max(np.abs(g - want)) < 1e-15 * L
    # every branch of the prototype has gain 1 at the band's centre: the L phases of an output agree
    for p in range(L):
        k = np.arange(p, T, L)
        assert abs(abs(np.sum(g[k] * np.exp(-2j * np.pi * fc * k / rate))) - 1.0) < 0.02
    # the defaults: cut = 0.4 fs min(1, L / M), T odd, 16 max(L, M) + 1, at most 2047
    for L, M, T in ((2, 9, 145), (2, 5, 81), (1, 3, 49), (5, 1, 81), (64, 63, 1025), (64, 4096, 2047), (37, 200, 2047)):
        g, _, h = R.resample_taps(fs, L, M)
        assert h.shape == (T,) and T % 2 == 1
        assert np.array_equal(h, L * firwin(T, 0.4 * fs * min(1.0, L / M), fs=fs * L)) and np.array_equal(g.real, h) and not g.imag.any()
    # resample_record's own refusals come before any library call
    with pytest.raises(ValueError, match="sampling frequency"):
        R.resample_record(type("E", (), {})(), _NoLibrary(), fs_out=4e6)
    e = type("E", (), {"sampling_freq": fs})()
    with pytest.raises(ValueError, match="one of the two"):
        R.resample_record(e, _NoLibrary())
    with pytest.raises(ValueError, match="one of the two"):
        R.resample_record(e, _NoLibrary(), fs_out=4e6, ratio=(2, 9))
    for bad, word in (((65, 1), "L = 65"), ((0, 1), "L = 0"), ((2, 129), "lowers the rate"), ((2, 0), "lowers the rate"), ((2.5, 3), "whole numbers"), (7, "whole numbers"),
                      ((1, 2, 3), "whole numbers")):
        with pytest.raises(ValueError, match=word):
            R.resample_record(e, _NoLibrary(), ratio=bad)
    with pytest.raises(ValueError, match="L = 375"):
        R.resample_record(type("E", (), {"sampling_freq": 16.368e6})(), _NoLibrary(), fs_out=18e6)
