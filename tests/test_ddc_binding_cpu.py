"""gc_downconvert at the boundary, without a GPU: declared in include/gnsscorr.h, exported by the library, bound by _lib.py with the
declared argument types; the two structs field by field, with the sizes (48, 40) and offsets the C compiler gives them; the two
constants the same on both sides; the API version unchanged (new entry points are detected by symbol); Engine.downconvert refuses
taps of another shape and values that are no whole numbers before any library call; the MEX gateway lists and handles the command;
receiver.downconvert_band's tap design against a direct firwin plus modulation."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnsscorr.h")
STRUCTS = {"gc_ddc_params": ["first_sample", "noutputs", "dst_first", "decim", "ntaps", "carr_freq", "carr_phase"],
           "gc_ddc_result": ["phase_step", "phase0", "clipped", "sum_sq", "carr_freq"]}
SIZES = {"gc_ddc_params": 48, "gc_ddc_result": 40}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"include/gnsscorr.h does not declare {name}"
    return [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_gc_downconvert_and_the_binding_has_its_argument_types():
    from cu_sdr_collection_amd import _lib as L
    ctypes_of = {"gc_context*": C.c_void_p, "const gc_ddc_params*": C.POINTER(L.gc_ddc_params), "const double*": C.POINTER(C.c_double),
                 "gc_ddc_result*": C.POINTER(L.gc_ddc_result)}
    params = ["gc_context*", "gc_context*", "const gc_ddc_params*", "const double*", "gc_ddc_result*"]
    assert _params("gc_downconvert") == params
    res, args = L.SYMBOLS["gc_downconvert"]
    assert res is C.c_int and args == [ctypes_of[p] for p in params]
    lib = L.load()
    assert hasattr(lib, "gc_downconvert") and lib.gc_downconvert.argtypes == args
    assert lib.gc_api_version() == 4                      # an addition, not a break
    assert re.search(r"\blong long\s+gc_debug_ddc_tile_outputs\s*\(\s*int\s+decim\s*,\s*int\s+ntaps\s*\)\s*;", _header())
    assert L.SYMBOLS["gc_debug_ddc_tile_outputs"] == (C.c_longlong, [C.c_int, C.c_int])
    assert lib.gc_debug_ddc_tile_outputs(3, 25) == 1024 and 1 <= lib.gc_debug_ddc_tile_outputs(64, 2048) < 1024
    assert lib.gc_debug_ddc_tile_outputs(0, 25) == lib.gc_debug_ddc_tile_outputs(65, 25) == lib.gc_debug_ddc_tile_outputs(3, 0) == 0
    assert lib.gc_debug_ddc_tile_outputs(3, 2049) == 0
    # a null argument is refused before any device is looked for
    assert lib.gc_downconvert(None, None, None, None, None) == L.GC_E_INVALID


def test_structs_and_the_constants_are_the_same_on_both_sides_and_as_the_c_compiler_sees_them():
    from cu_sdr_collection_amd import _lib as L
    h = _header()
    m = re.search(r"#define\s+GC_DDC_MAX_TAPS\s+(\d+)", h)
    assert m and int(m.group(1)) == L.GC_DDC_MAX_TAPS == 2048
    m = re.search(r"#define\s+GC_DDC_MAX_DECIM\s+(\d+)", h)
    assert m and int(m.group(1)) == L.GC_DDC_MAX_DECIM == 64
    assert re.search(r"#define\s+GC_API_VERSION\s+4\b", h)
    for name, fields in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), h, flags=re.S)
        assert body, name
        declared = [f for decl in body.group(1).split(";") if decl.strip() for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
        assert declared == fields == [f for f, _ in getattr(L, name)._fields_], name
    lines = ['printf("%d %d %d\\n", GC_DDC_MAX_TAPS, GC_DDC_MAX_DECIM, GC_API_VERSION);']
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
    assert got.pop(0) == [L.GC_DDC_MAX_TAPS, L.GC_DDC_MAX_DECIM, 4]
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


def test_engine_downconvert_refuses_taps_and_numbers_that_do_not_fit_before_any_library_call():
    import cu_sdr_collection_amd as P
    eng = object.__new__(P.Engine)                        # no context, no library: a call that got past the checks would fail otherwise
    eng._lib = eng._ctx = _NoLibrary()
    dst = _NoLibrary()
    for bad in (np.ones((4, 3)), np.ones((2, 2, 2)), np.ones((4, 2), dtype=complex), np.array(["a"] * 4), 1.0, np.ones(0), np.ones(2049),
                np.ones((2049, 2))):
        with pytest.raises(ValueError, match="taps"):
            P.Engine.downconvert(eng, dst, bad, 3)
    good = dict(decim=3, first_sample=0, noutputs=10, dst_first=0)
    for name, bad in (("decim", 2.5), ("decim", None), ("decim", 1 << 31), ("first_sample", 0.5), ("first_sample", "3"), ("noutputs", 1 << 63),
                      ("noutputs", True), ("dst_first", 1.25), ("dst_first", -(1 << 63) - 1)):
        with pytest.raises(ValueError, match=name):
            P.Engine.downconvert(eng, dst, np.ones(4), **dict(good, **{name: bad}))
    eng._ctx = None                                       # (close() in __del__ then has nothing to do)
    g = P.Engine._ddc_taps([1, 2j, 0.5 - 0.25j])
    assert g.dtype == np.float64 and g.flags.c_contiguous and g.tolist() == [[1.0, 0.0], [0.0, 2.0], [0.5, -0.25]]
    assert P.Engine._ddc_taps([[1, 2], [3, 4]]).tolist() == [[1.0, 2.0], [3.0, 4.0]]          # [T][2] real
    assert P.Engine._ddc_taps(np.ones(2048)).shape == (2048, 2)
    assert P.Engine._whole("downconvert()", "decim", 7.0, 32) == 7 and P.Engine._whole("downconvert()", "decim", -1, 32) == -1   # the library's to refuse


def test_mex_gateway_lists_and_handles_the_command():
    text = open(os.path.join(ROOT, "matlab", "gnsscorr_mex.c")).read()
    head = text[:text.index("#include")]
    assert "gnsscorr_mex('downconvert'" in head           # the usage line in the file's head
    assert 'strcmp(cmd, "downconvert")' in text and "gc_downconvert(" in text
    wrapper = open(os.path.join(ROOT, "matlab", "gnsscorr_downconvert.m")).read()
    assert "gnsscorr_mex('downconvert'" in wrapper


def test_the_receivers_tap_design_is_firwin_moved_to_the_nco_frequency():
    from scipy.signal import firwin

    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import receiver as R
    assert P.downconvert_band is R.downconvert_band and "downconvert_band" in P.__all__
    fs, fc, bw, T = 18e6, 4500137.0, 2.4e6, 25
    g, f_used, h = R.ddc_band_taps(fs, fc, bw, T)
    step = int(math.ldexp(fc / fs, 64))                                   # a whole number already
    assert R.ddc_nco_step(fc, fs) == step and R.ddc_nco_step(-fc, fs) == -step
    assert f_used == math.ldexp(float(step), -64) * fs and abs(f_used - fc) < 1e-8
    want_h = firwin(T, bw / 2, fs=fs)
    assert np.array_equal(h, want_h) and abs(h.sum() - 1.0) < 1e-12       # gain 1 at DC
    want = want_h * np.exp(2j * np.pi * f_used * np.arange(T) / fs)
    assert np.max(np.abs(g - want)) < 1e-15
    # the filter passes its centre and stops what lies a band away
    H = lambda f: abs(np.sum(g * np.exp(-2j * np.pi * f * np.arange(T) / fs)))     # noqa: E731
    assert abs(H(fc) - 1.0) < 1e-9 and H(fc + 3 * bw) < 0.01 and H(-fc) < 0.01
    # 1 Hz: ldexp(f / fs, 64) has a fraction; the step is the nearest integer, as the library's llrint gives it
    assert abs(R.ddc_nco_step(1.0, fs) - math.ldexp(1.0 / fs, 64)) <= 0.5
    # the default length is odd, 8 D + 1, and stays inside the limit
    with pytest.raises(ValueError, match="sampling frequency"):
        R.downconvert_band(type("E", (), {})(), _NoLibrary(), fc, bw, 3)
    e = type("E", (), {"sampling_freq": fs})()
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="decim"):
            R.downconvert_band(e, _NoLibrary(), fc, bw, bad)
