"""The precision= keyword and the float64 mode's C-ABI entries, without a GPU (include/gnsscorr.h gc_set_precision)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoLibrary:
    """Stands in for the engine: any attribute access means the library would have been reached."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the precision was checked")


@pytest.mark.parametrize("bad", ["quad", "Double", 1, 64, ""])
def test_unknown_precision_raises_before_any_library_call(bad):
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd.engine import precision_code
    with pytest.raises(ValueError):
        precision_code(bad)
    S = P.initSettings()
    with pytest.raises(ValueError):
        P.receiver.tracking(_NoLibrary(), [], S, precision=bad)
    with pytest.raises(ValueError):
        P.receiver.tracking_file(_NoLibrary(), "no-such-file", [], S, 1000, precision=bad)
    with pytest.raises(ValueError):
        P.receiver.tracking_multi([(_NoLibrary(), [], S, "GPS_L1CA")], precision=bad)
    with pytest.raises(ValueError):
        P.Engine.track(_NoLibrary(), None, [], precision=bad)
    with pytest.raises(ValueError):
        P.Engine.track_file(_NoLibrary(), "no-such-file", None, [], 1000, precision=bad)
    with pytest.raises(ValueError):
        P.Engine.track_multi([], precision=bad)


def test_known_precisions_map_to_the_header_values():
    from cu_sdr_collection_amd import _lib as L
    from cu_sdr_collection_amd.engine import precision_code
    assert precision_code(None) is None
    assert (precision_code("single"), precision_code("double")) == (L.GC_PREC_F32, L.GC_PREC_F64) == (0, 1)
    header = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    assert re.search(r"enum gc_precision \{ GC_PREC_F32 = 0, GC_PREC_F64 = 1 \};", header)


def test_precision_entry_points_are_declared_exported_and_bound():
    from cu_sdr_collection_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    assert re.search(r"^int gc_set_precision\(gc_context\* ctx, int precision\);", header, re.M)
    assert re.search(r"^int gc_get_precision\(const gc_context\* ctx, int\* precision\);", header, re.M)
    assert L.SYMBOLS["gc_set_precision"][1][1] is L.C.c_int
    assert "gc_get_precision" in L.SYMBOLS
    lib = L.load()                       # built by build(): the symbols resolve in libgnsscorr.so
    assert hasattr(lib, "gc_set_precision") and hasattr(lib, "gc_get_precision")
