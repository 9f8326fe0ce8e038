"""gc_correlate_ddm_integrate at the boundary, without a GPU: declared in include/gnsscorr.h with the agreed parameter list, exported by
the library, bound by _lib.py with the declared argument types, the API version unchanged, and the Python entry points exposed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnsscorr.h")

# C parameter type -> ctypes type, for the types this declaration uses
CTYPES = {"gc_context*": C.c_void_p, "int": C.c_int, "const gc_block*": "gc_block*", "const double*": C.POINTER(C.c_double),
          "double*": C.POINTER(C.c_double), "const int32_t*": C.POINTER(C.c_int32)}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_function_and_the_binding_has_its_argument_types():
    from cu_sdr_collection_amd import _lib as L
    m = re.search(r"\bint\s+gc_correlate_ddm_integrate\s*\(([^)]*)\)\s*;", _header())
    assert m, "include/gnsscorr.h does not declare gc_correlate_ddm_integrate"
    params = [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", p.strip()).group(1) for p in m.group(1).split(",")]
    assert params == ["gc_context*", "int", "const gc_block*", "const double*", "int", "const double*", "int", "const double*",
                      "int", "const int32_t*", "int", "const int32_t*", "double*", "double*"]
    assert names == ["ctx", "nblocks", "blocks", "block_weights", "ntaps", "tap_offsets", "nfreq", "freq_offsets", "nruns", "run_len",
                     "nmaps", "map_len", "coh", "pow"]
    assert "gc_correlate_ddm_integrate" in L.SYMBOLS
    res, args = L.SYMBOLS["gc_correlate_ddm_integrate"]
    want = [C.POINTER(L.gc_block) if CTYPES[p] == "gc_block*" else CTYPES[p] for p in params]
    assert res is C.c_int and args == want
    lib = L.load()
    assert hasattr(lib, "gc_correlate_ddm_integrate")
    assert lib.gc_correlate_ddm_integrate.argtypes == want
    assert lib.gc_api_version() == 4                      # an addition, not a break


def test_the_header_states_the_definition():
    """The coherent sum is defined in the header's comment, operation by operation: the GPU tests restate it from there."""
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    for line in ("dn = first_sample[b] - first_sample[b0]", "x  = (freq_offsets[m] * (double)dn) / fs", "u  = x - rint(x)",
                 "c  = cospi(2u),  s = sinpi(2u)", "re += w * (c * D.re + s * D.im)", "im += w * (c * D.im - s * D.re)",
                 "p += (re * re + im * im)"):
        assert line in text, line


def test_engine_and_receiver_expose_the_integrated_map():
    import inspect

    import cu_sdr_collection_amd as P
    import cu_sdr_collection_amd.receiver as R
    assert callable(P.Engine.correlate_ddm_integrate) and callable(P.integrated_delay_doppler_map)
    assert P.integrated_delay_doppler_map is R.integrated_delay_doppler_map
    assert "integrated_delay_doppler_map" in P.__all__
    assert list(inspect.signature(P.Engine.correlate_ddm_integrate).parameters) == [
        "self", "blocks", "offsets", "freqs", "run_len", "weights", "map_len", "coherent"]
    sig = inspect.signature(P.integrated_delay_doppler_map)
    assert list(sig.parameters) == ["fid", "trackResults_k", "channel_k", "settings", "offsets", "freqs", "coherent", "noncoherent", "wipe",
                                    "signal", "epochs"]
    assert sig.parameters["wipe"].default == "prompt" and sig.parameters["noncoherent"].default is None
