"""gc_excise_pulses and gc_excise_bins at the boundary, without a GPU: declared in include/gnsscorr.h, exported by the library, bound
by _lib.py with the declared argument types; the three structs field by field, with the sizes and offsets the C compiler gives them; the constant the
same on both sides; the API version unchanged (new entry points are detected by symbol); Engine.excise_pulses refuses values that are
no whole numbers of their fields' widths, Engine.excise_bins a gain of another shape, before any library call; the MEX gateway lists
and handles the commands."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnsscorr.h")
STRUCTS = {"gc_excise_pulse_params": ["first_sample", "nsamples", "threshold2", "before", "after"],
           "gc_excise_pulse_stats": ["hot", "blanked", "runs", "longest"],
           "gc_excise_bins_params": ["first_sample", "nsamples", "nfft", "reserved"]}
SIZES = {"gc_excise_pulse_params": 32, "gc_excise_pulse_stats": 32, "gc_excise_bins_params": 24}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"include/gnsscorr.h does not declare {name}"
    return [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_gc_excise_pulses_and_the_binding_has_its_argument_types():
    from cu_sdr_collection_amd import _lib as L
    ctypes_of = {"gc_context*": C.c_void_p, "const gc_excise_pulse_params*": C.POINTER(L.gc_excise_pulse_params),
                 "gc_excise_pulse_stats*": C.POINTER(L.gc_excise_pulse_stats)}
    params = ["gc_context*", "gc_context*", "const gc_excise_pulse_params*", "gc_excise_pulse_stats*"]
    assert _params("gc_excise_pulses") == params
    res, args = L.SYMBOLS["gc_excise_pulses"]
    assert res is C.c_int and args == [ctypes_of[p] for p in params]
    lib = L.load()
    assert hasattr(lib, "gc_excise_pulses") and lib.gc_excise_pulses.argtypes == args
    assert lib.gc_api_version() == 4                      # an addition, not a break
    ctypes_of.update({"const gc_excise_bins_params*": C.POINTER(L.gc_excise_bins_params), "const float*": C.POINTER(C.c_float),
                      "float*": C.POINTER(C.c_float)})
    params = ["gc_context*", "gc_context*", "const gc_excise_bins_params*", "const float*", "float*"]
    assert _params("gc_excise_bins") == params
    res, args = L.SYMBOLS["gc_excise_bins"]
    assert res is C.c_int and args == [ctypes_of[p] for p in params] and lib.gc_excise_bins.argtypes == args
    assert re.search(r"\blong long\s+gc_debug_excise_tile_segments\s*\(\s*int\s+nfft\s*\)\s*;", _header())
    assert L.SYMBOLS["gc_debug_excise_tile_segments"] == (C.c_longlong, [C.c_int]) and lib.gc_debug_excise_tile_segments(4096) == 2048


def test_structs_and_the_constant_are_the_same_on_both_sides_and_as_the_c_compiler_sees_them():
    from cu_sdr_collection_amd import _lib as L
    h = _header()
    m = re.search(r"#define\s+GC_EXCISE_MAX_GUARD\s+(\d+)", h)
    assert m and int(m.group(1)) == L.GC_EXCISE_MAX_GUARD == 4096
    assert re.search(r"#define\s+GC_API_VERSION\s+4\b", h)
    for name, fields in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), h, flags=re.S)
        assert body, name
        declared = [f for decl in body.group(1).split(";") if decl.strip() for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
        assert declared == fields == [f for f, _ in getattr(L, name)._fields_], name
    lines = ['printf("%d %d\\n", GC_EXCISE_MAX_GUARD, GC_API_VERSION);']
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
    assert got.pop(0) == [L.GC_EXCISE_MAX_GUARD, 4]
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


def test_engine_excise_pulses_refuses_values_that_do_not_fit_before_any_library_call():
    import cu_sdr_collection_amd as P
    eng = object.__new__(P.Engine)                        # no context, no library: a call that got past the checks would fail otherwise
    eng._lib = eng._ctx = _NoLibrary()
    good = dict(first_sample=0, nsamples=10, threshold2=100, before=1, after=2)
    for name, bad in (("first_sample", 1.5), ("nsamples", None), ("nsamples", 1 << 63), ("threshold2", "9"), ("threshold2", -(1 << 63) - 1),
                      ("before", 1 << 31), ("after", 2.25), ("after", True)):
        with pytest.raises(ValueError, match=name):
            P.Engine.excise_pulses(eng, **dict(good, **{name: bad}))
    eng._ctx = None                                       # (close() in __del__ then has nothing to do)
    p = P.Engine._excise_pulse_args(5, 7.0, (1 << 31) - 1, 4096, 0)     # a whole float is a whole number
    assert (p.first_sample, p.nsamples, p.threshold2, p.before, p.after) == (5, 7, (1 << 31) - 1, 4096, 0)
    p = P.Engine._excise_pulse_args(-1, 0, -1, -1, 4097)                # what the library refuses is the library's to refuse
    assert (p.first_sample, p.nsamples, p.threshold2, p.before, p.after) == (-1, 0, -1, -1, 4097)


def test_engine_excise_bins_refuses_a_gain_of_another_shape_before_any_library_call():
    import numpy as np

    import cu_sdr_collection_amd as P
    eng = object.__new__(P.Engine)
    eng._lib = eng._ctx = _NoLibrary()
    for bad in (np.ones(2), np.ones(5), np.ones((4, 4)), np.ones(8, dtype=complex), np.array(["a"] * 8), 1.0):
        with pytest.raises(ValueError, match="gain"):
            P.Engine.excise_bins(eng, 0, 100, bad)
    eng._ctx = None
    g = P.Engine._excise_gain([1, 0, 2, 1])
    assert g.dtype == np.float32 and g.flags.c_contiguous and g.tolist() == [1.0, 0.0, 2.0, 1.0]


def test_mex_gateway_lists_and_handles_the_commands():
    text = open(os.path.join(ROOT, "matlab", "gnsscorr_mex.c")).read()
    head = text[:text.index("#include")]
    for cmd, fn in (("excise_pulses", "gc_excise_pulses("), ("excise_bins", "gc_excise_bins(")):
        assert "gnsscorr_mex('%s'" % cmd in head          # the usage line in the file's head
        assert 'strcmp(cmd, "%s")' % cmd in text and fn in text


def test_the_wrappers_two_rules():
    import numpy as np

    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import receiver as R
    assert P.excise_interference is R.excise_interference and "excise_interference" in P.__all__
    counts = np.zeros((2, 257), dtype=np.uint64)
    counts[0, 128 + 3], counts[0, 128 - 4], counts[0, 128 + 30] = 5, 5, 1     # |c0|: five 3s, five 4s, one 30 - the median is 4
    counts[1, 0] = 11                                                         # row 1 is not looked at
    t2, sigma = R.excise_pulse_threshold(counts, 2.5, 2)
    assert sigma == 1.4826 * 4 and t2 == int((2.5 * sigma) ** 2 * 2)
    assert R.excise_pulse_threshold(counts, 2.5, 1)[0] == int((2.5 * sigma) ** 2)
    counts[0, 128 + 30] = 0                                                   # ten samples: the middle two are 3 and 4
    assert R.excise_pulse_threshold(counts, 1.0, 1)[1] == 1.4826 * 3.5
    end = np.zeros((2, 257), dtype=np.uint64)
    end[0, 0], end[0, 256], end[0, 128] = 3, 3, 5                             # six of eleven at |c0| >= 128
    with pytest.raises(ValueError, match="end bin"):
        R.excise_pulse_threshold(end, 3.0, 2)
    end[0, 128] = 7                                                           # seven of thirteen at 0
    assert R.excise_pulse_threshold(end, 3.0, 2) == (0, 0.0)
    g = R.excise_bin_gain([1, 1, 1, 9, 1, 1, 1, 1], 4.0, 1)
    assert g.dtype == np.float32 and g.tolist() == [1, 1, 0, 0, 0, 1, 1, 1]
    assert R.excise_bin_gain([9, 1, 1, 1, 1, 1, 1, 1], 4.0, 2).tolist() == [0, 0, 0, 1, 1, 1, 0, 0]      # around the ends
    assert R.excise_bin_gain([1, 1, 1, 4, 1, 1, 1, 1], 4.0, 1).tolist() == [1] * 8                      # above, not at, the factor
    assert R.excise_bin_gain([1, 1, 1, 9, 1, 1, 1, 1], 4.0, 0).tolist() == [1, 1, 1, 0, 1, 1, 1, 1]
    with pytest.raises(ValueError, match="pulse_sigmas"):
        R.excise_interference(_NoLibrary(), type("S", (), {"samplingFreq": 18e6})())
