"""The C-ABI library loads on a CPU-only box and exports every symbol include/gnsscorr.h declares;
struct layouts seen by ctypes equal the C compiler's."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnsscorr.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gc_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    from cu_sdr_collection_amd import _lib as L
    lib = L.load()
    names = _declared_functions()
    assert len(names) >= 25 and {"gc_debug_last_kernel", "gc_debug_last_track_mode", "gc_debug_last_track_team"} <= set(names)
    for n in names:
        assert hasattr(lib, n), f"libgnsscorr.so does not export {n}"
        assert n in L.SYMBOLS, f"_lib.py has no binding for {n}"
    assert lib.gc_api_version() == 4


def test_struct_layouts_match_the_c_compiler():
    from cu_sdr_collection_amd import _lib as L
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "gnsscorr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(gc_block), offsetof(gc_block, table_offset),
         sizeof(gc_track_params), offsetof(gc_track_params, n_epochs), sizeof(gc_channel_init),
         sizeof(gc_acq_params), sizeof(gc_acq_result), offsetof(gc_acq_result, coarse_freq), GC_OUT_STRIDE, GC_TRK_NFIELDS);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    got = [int(x) for x in out]
    want = [C.sizeof(L.gc_block), L.gc_block.table_offset.offset, C.sizeof(L.gc_track_params),
            L.gc_track_params.n_epochs.offset, C.sizeof(L.gc_channel_init), C.sizeof(L.gc_acq_params),
            C.sizeof(L.gc_acq_result), L.gc_acq_result.coarse_freq.offset, L.GC_OUT_STRIDE, L.GC_TRK_NFIELDS]
    assert got == want


def test_no_cpu_fallback_without_a_gpu():
    """Without a visible MI355X the product must fail loudly, not fall back to anything."""
    import cu_sdr_collection_amd as P
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present on this box")
    with pytest.raises(P.GnssCorrError) as e:
        P.Engine(0)
    assert e.value.status == P._lib.GC_E_HIP


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "cu-sdr-collection_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "liboracle" not in text, f
