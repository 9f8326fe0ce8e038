"""gc_cancel at the boundary, without a GPU: declared in include/gnsscorr.h, exported by the library, bound by _lib.py with the
declared argument types; the constants the same on both sides and as the C compiler sees them; the API version unchanged (new entry
points are detected by symbol); Engine.cancel and receiver.cancel_tracked refuse a bad mode and amplitudes of a wrong shape before
any library call; the numpy model of the definition (tests/cancel_model.py) on two cases small enough to follow by hand."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnsscorr.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"include/gnsscorr.h does not declare {name}"
    return [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_gc_cancel_and_the_binding_has_its_argument_types():
    from cu_sdr_collection_amd import _lib as L
    ctypes_of = {"gc_context*": C.c_void_p, "int": C.c_int, "const gc_block*": C.POINTER(L.gc_block), "const double*": C.POINTER(C.c_double),
                 "double*": C.POINTER(C.c_double)}
    params = ["gc_context*", "gc_context*", "int", "const gc_block*", "const double*", "double*", "int"]
    assert _params("gc_cancel") == params
    res, args = L.SYMBOLS["gc_cancel"]
    assert res is C.c_int and args == [ctypes_of[p] for p in params]
    lib = L.load()
    assert hasattr(lib, "gc_cancel") and lib.gc_cancel.argtypes == args
    assert lib.gc_api_version() == 4                      # an addition, not a break


def test_constants_are_the_same_on_both_sides():
    from cu_sdr_collection_amd import _lib as L
    h = _header()
    m = re.search(r"#define\s+GC_CANCEL_MAX_CHANNELS\s+(\d+)", h)
    assert m and int(m.group(1)) == L.GC_CANCEL_MAX_CHANNELS == 64
    m = re.search(r"enum\s+gc_cancel_mode\s*\{\s*GC_CANCEL_SUBTRACT\s*=\s*(\d+)\s*,\s*GC_CANCEL_MODEL\s*=\s*(\d+)\s*\}", h)
    assert m and (int(m.group(1)), int(m.group(2))) == (L.GC_CANCEL_SUBTRACT, L.GC_CANCEL_MODEL) == (0, 1)
    assert re.search(r"#define\s+GC_API_VERSION\s+4\b", h)
    prog = r'''
#include <stdio.h>
#include "gnsscorr.h"
int main(void) {
  printf("%d %d %d %d %d\n", GC_CANCEL_MAX_CHANNELS, (int)GC_CANCEL_SUBTRACT, (int)GC_CANCEL_MODEL, GC_MAX_ARMS, GC_API_VERSION);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [L.GC_CANCEL_MAX_CHANNELS, L.GC_CANCEL_SUBTRACT, L.GC_CANCEL_MODEL, L.GC_MAX_ARMS, 4]


class _NoLibrary:
    """Stands where an Engine would: any use is a library call that came too early."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was used ({name}) before the arguments were checked")


def test_engine_cancel_refuses_a_bad_mode_and_a_bad_amp_shape_before_any_library_call():
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import _lib as L
    blocks = (L.gc_block * 4)()
    eng = object.__new__(P.Engine)                        # no context, no library: a call that got past the checks would fail otherwise
    eng._lib = eng._ctx = _NoLibrary()
    for mode in ("both", "", None, 0, "SUBTRACT"):
        with pytest.raises(ValueError, match="mode"):
            P.Engine.cancel(eng, blocks, mode=mode)
    for amp in (np.zeros(4), np.zeros((4, 2)), np.zeros((3, 3)), np.zeros((4, 3, 2))):
        with pytest.raises(ValueError, match="amp"):
            P.Engine.cancel(eng, blocks, amp=amp)
    eng._ctx = None                                       # (close() in __del__ then has nothing to do)
    code, a_in = P.Engine._cancel_args(4, np.full((4, 3), 1 - 2j), "model")
    assert code == L.GC_CANCEL_MODEL and a_in.shape == (4, 3, 2) and a_in.flags.c_contiguous and a_in.dtype == np.float64
    assert np.all(a_in[..., 0] == 1.0) and np.all(a_in[..., 1] == -2.0)
    assert P.Engine._cancel_args(4, None, "subtract") == (L.GC_CANCEL_SUBTRACT, None)


def test_cancel_tracked_refuses_a_bad_mode_and_bad_amplitudes_before_any_library_call():
    import cu_sdr_collection_amd as P
    assert P.receiver.cancel_tracked is P.cancel_tracked and "cancel_tracked" in P.__all__
    fid = _NoLibrary()
    tr = [type("T", (), {"PRN": 5})(), type("T", (), {"PRN": 0})()]
    with pytest.raises(ValueError, match="mode"):
        P.cancel_tracked(fid, tr, [None, None], None, mode="remove")
    with pytest.raises(ValueError, match="amp"):
        P.cancel_tracked(fid, tr, [None, None], None, amp=[np.zeros((3, 1)), np.zeros((3, 1))])         # one tracked channel, two arrays
    with pytest.raises(ValueError, match="amp"):
        P.cancel_tracked(fid, tr, [None, None], None, which=[0], amp=[np.zeros(3)])
    with pytest.raises(ValueError, match="amp"):
        P.cancel_tracked(fid, tr, [None, None], None, which=[0], amp=[np.zeros((3, 4))])
    with pytest.raises(ValueError, match="channels"):
        P.cancel_tracked(fid, tr * 40, [None] * 80, None, which=list(range(0, 80, 2)) + list(range(0, 80, 2)))


def test_mex_gateway_lists_and_handles_the_command():
    text = open(os.path.join(ROOT, "matlab", "gnsscorr_mex.c")).read()
    head = text[:text.index("#include")]
    assert "gnsscorr_mex('cancel'" in head                # the usage line in the file's head
    assert 'strcmp(cmd, "cancel")' in text and "gc_cancel(" in text


def test_the_model_on_cases_small_enough_to_follow():
    import cancel_model as M
    tab = np.array([1, 1, -1, 1, -1, -1, 1], dtype=np.int8)
    chans = {0: {"tables": [tab], "r": 1.0, "mult": [1.0]}}
    # zero carrier: a block of x = 3 c(i) projects to A = 3 exactly, the residual is zero, the model is the block itself
    blk = {"ch": 0, "s0": 2, "n": 8, "rem": 0.5, "step": 0.5, "f": 0.0, "phi": 0.0}
    sn, cs, c = M.replica(blk, chans[0], 1e6)
    assert np.all(sn == 0) and np.all(cs == 1)
    assert c[0].tolist() == [float(tab[k]) for k in (1, 1, 2, 2, 3, 3, 4, 4)]                           # ceil(0.5 + 0.5 i)
    raw = np.zeros(24, dtype=np.int8)
    raw[4:20:2] = (3 * c[0]).astype(np.int8)
    raw[0], raw[23] = 9, -7
    out, used, P, E, sx, near, covered = M.cancel(raw, np.int8, M.IQ, [blk], chans, 1e6)
    assert used[0, 0] == 3.0 and E[0, 0] == 8 and sx[0] == 24.0 and not near.any() and covered.tolist() == [False] * 2 + [True] * 8 + [False] * 2
    assert out.tolist() == [9] + [0] * 22 + [-7]
    model = M.cancel(raw, np.int8, M.IQ, [blk], chans, 1e6, mode="model")[0]
    assert model.tolist() == [0] * 4 + raw[4:20].tolist() + [0] * 4
    # a given amplitude on a Q/I record: re is the second value of each pair
    big = M.cancel(raw, np.int8, M.QI, [blk], chans, 1e6, amp=np.array([[100j, 0, 0]]), mode="model")[0]
    assert big[4:20:2].tolist() == (100 * c[0]).astype(int).tolist() and not big[5:20:2].any()            # j 100 c: all in im, stored first
    sub = M.cancel(raw, np.int8, M.IQ, [blk], chans, 1e6, amp=np.array([[200.0, 0, 0]]))[0]               # 3 c - 200 c clips
    assert sub[4:20:2].tolist() == np.clip(-197 * c[0], -128, 127).astype(int).tolist()
    # a real record: the model is 2 Re(.).  At f = 0 the carrier has no second half, the projection of x = 6 c is A = 6 and the
    # model 12 c - the definition is for carriers whose image the block averages out
    real = np.zeros(12, dtype=np.int16)
    real[2:10] = (6 * c[0]).astype(np.int16)
    out, used, *_ = M.cancel(real, np.int16, M.REAL, [blk], chans, 1e6)
    assert used[0, 0] == 6.0 and out[2:10].tolist() == (-6 * c[0]).astype(int).tolist()
