"""gc_probe_psd and gc_probe_histogram at the boundary, without a GPU: declared in include/gnsscorr.h, exported by the library, bound
by _lib.py with the declared argument types; gc_probe_psd_params laid out as the C compiler lays it out; the constants the same on
both sides; the API version unchanged (new entry points are detected by symbol)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnsscorr.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"include/gnsscorr.h does not declare {name}"
    return [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_both_functions_and_the_binding_has_their_argument_types():
    from cu_sdr_collection_amd import _lib as L
    ctypes_of = {"gc_context*": C.c_void_p, "const gc_probe_psd_params*": C.POINTER(L.gc_probe_psd_params), "double*": C.POINTER(C.c_double),
                 "int64_t*": C.POINTER(C.c_int64), "int64_t": C.c_int64, "uint64_t*": C.POINTER(C.c_uint64)}
    want = {"gc_probe_psd": ["gc_context*", "const gc_probe_psd_params*", "double*", "int64_t*"],
            "gc_probe_histogram": ["gc_context*", "int64_t", "int64_t", "uint64_t*", "int64_t*"]}
    lib = L.load()
    for name, params in want.items():
        assert _params(name) == params
        assert name in L.SYMBOLS
        res, args = L.SYMBOLS[name]
        assert res is C.c_int and args == [ctypes_of[p] for p in params]
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args
    assert lib.gc_api_version() == 4                      # an addition, not a break


def test_constants_are_the_same_on_both_sides():
    from cu_sdr_collection_amd import _lib as L
    h = _header()
    m = re.search(r"#define\s+GC_PROBE_HIST_BINS\s+(\d+)", h)
    assert m and int(m.group(1)) == L.GC_PROBE_HIST_BINS == 257
    m = re.search(r"enum\s+gc_probe_window\s*\{\s*GC_WIN_RECT\s*=\s*(\d+)\s*,\s*GC_WIN_HAMMING\s*=\s*(\d+)\s*\}", h)
    assert m and (int(m.group(1)), int(m.group(2))) == (L.GC_WIN_RECT, L.GC_WIN_HAMMING) == (0, 1)
    assert re.search(r"#define\s+GC_API_VERSION\s+4\b", h)


def test_params_layout_matches_the_c_compiler():
    from cu_sdr_collection_amd import _lib as L
    fields = ["first_sample", "nsamples", "nfft", "noverlap", "window", "nspans"]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "gnsscorr.h"
int main(void) {
  printf("%zu", sizeof(gc_probe_psd_params));
''' + "".join(f'  printf(" %zu", offsetof(gc_probe_psd_params, {f}));\n' for f in fields) + r'''  printf(" %d %d %d\n", GC_PROBE_HIST_BINS, (int)GC_WIN_RECT, (int)GC_WIN_HAMMING);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(L.gc_probe_psd_params)] + [getattr(L.gc_probe_psd_params, f).offset for f in fields] + [L.GC_PROBE_HIST_BINS, L.GC_WIN_RECT,
                                                                                                             L.GC_WIN_HAMMING]
    assert got == want and got[0] == 32
    assert [name for name, _ in L.gc_probe_psd_params._fields_] == fields


def test_engine_and_receiver_expose_the_probe():
    import cu_sdr_collection_amd as P
    assert callable(P.Engine.probe_psd) and callable(P.Engine.probe_histogram) and callable(P.probeData)
    assert "probeData" in P.__all__
    assert P.receiver.probeData is P.probeData


def test_mex_gateway_lists_and_handles_both_commands():
    text = open(os.path.join(ROOT, "matlab", "gnsscorr_mex.c")).read()
    head = text[:text.index("#include")]
    for cmd in ("probe_psd", "probe_histogram"):
        assert f"gnsscorr_mex('{cmd}'" in head                     # the usage line in the file's head
        assert f'strcmp(cmd, "{cmd}")' in text
