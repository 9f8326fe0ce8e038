"""The MEX gateway's 'excise_pulses' and 'excise_bins' commands (matlab/gnsscorr_mex.c) through the test-only mex.h: the bytes,
statistics and values of Engine.excise_pulses / Engine.excise_bins on the same record - out of place and in place, with and without
the optional arguments - and the library's refusals as errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexstub"))
pytestmark = pytest.mark.gpu
FS = 18e6
NS = 40000


def test_excise_pulses_command_returns_the_librarys_bytes_and_statistics(engine):
    import cu_sdr_collection_amd as P
    import harness
    rng = np.random.default_rng(4200)
    iq = rng.integers(-10, 11, 2 * NS).astype(np.int8)
    hot = np.concatenate([[0, 63, 64, 16383, 16384 + 70, NS - 1], rng.integers(0, NS, 40)])
    iq[2 * hot] = 100
    dst = P.Engine(0)
    gateway = harness.Gateway()
    try:
        hs, hd = gateway.call("create", 0), gateway.call("create", 0)
        for first, n, extra in ((0, NS, ()), (1, NS - 6, (64,)), (4097, 30000, (64, 256)), (5, 1000, (0, 4096))):
            before, after = (list(extra) + [0, 0])[:2]
            for inplace in (False, True):
                engine.load_if(iq, fs=FS)
                dst.load_if(np.full_like(iq, 85), fs=FS)
                want_st = engine.excise_pulses(first, n, 1000, before, after, dst=None if inplace else dst)
                want = (engine if inplace else dst).read_if(0, NS)
                gateway.call("load_if", hs, iq, 2, FS, nargout=0)
                gateway.call("load_if", hd, np.full_like(iq, 85), 2, FS, nargout=0)
                st = gateway.call("excise_pulses", hs, hs if inplace else hd, first, n, 1000, *extra)
                got = gateway.call("read_if", hs if inplace else hd, 0, NS, "int8", 2)
                assert np.ravel(got).astype(np.int8).tobytes() == want.tobytes(), (first, n, extra, inplace)
                assert st.dtype == np.float64 and np.ravel(st).tolist() == [want_st.hot, want_st.blanked, want_st.runs, want_st.longest]
                assert want_st.hot > 0
                if not inplace:
                    assert np.ravel(gateway.call("read_if", hs, 0, NS, "int8", 2)).astype(np.int8).tobytes() == iq.tobytes()
        with pytest.raises(harness.MexError):
            gateway.call("excise_pulses", hs, 9, 0, NS, 1000)                         # no such context
        with pytest.raises(harness.MexError):
            gateway.call("excise_pulses", hs, hd, 0, NS)                              # too few arguments
        with pytest.raises(harness.MexError):
            gateway.call("excise_pulses", hs, hd, 0, NS, 1000.5)                      # no whole number
        with pytest.raises(harness.MexError):
            gateway.call("excise_pulses", hs, hd, 0, NS, 1000, 4097)                  # a guard the library refuses
        with pytest.raises(harness.MexError):
            gateway.call("excise_pulses", hs, hd, 1, NS, 1000)                        # beyond the record
        gateway.call("destroy", hs, nargout=0)
        gateway.call("destroy", hd, nargout=0)
    finally:
        gateway.lib.stub_run_atexit()
        dst.close()


def test_excise_bins_command_returns_the_librarys_bytes_and_values(engine):
    import cu_sdr_collection_amd as P
    import harness
    rng = np.random.default_rng(4201)
    iq = rng.integers(-100, 101, 2 * NS).astype(np.int8)
    dst = P.Engine(0)
    gateway = harness.Gateway()
    try:
        hs, hd = gateway.call("create", 0), gateway.call("create", 0)
        for first, n, nfft, as_single in ((0, NS, 64, False), (1, NS - 6, 1000, True), (4097, 3 * 512 + 7, 1024, False)):
            gain = rng.uniform(0.0, 2.0, nfft)
            gain_mx = gain.astype(np.float32) if as_single else gain
            for inplace in (False, True):
                for want_values in (True, False):
                    engine.load_if(iq, fs=FS)
                    dst.load_if(np.full_like(iq, 85), fs=FS)
                    want_v = engine.excise_bins(first, n, gain, dst=None if inplace else dst, values=want_values)
                    want = (engine if inplace else dst).read_if(0, NS)
                    gateway.call("load_if", hs, iq, 2, FS, nargout=0)
                    gateway.call("load_if", hd, np.full_like(iq, 85), 2, FS, nargout=0)
                    got_v = gateway.call("excise_bins", hs, hs if inplace else hd, first, n, gain_mx, nargout=1 if want_values else 0)
                    got = gateway.call("read_if", hs if inplace else hd, 0, NS, "int8", 2)
                    assert np.ravel(got).astype(np.int8).tobytes() == want.tobytes(), (first, n, nfft, inplace, want_values)
                    if want_values:
                        assert got_v.dtype == np.float32 and got_v.shape == (2, n)
                        assert np.array_equal(got_v[0] + 1j * got_v[1], want_v)
        with pytest.raises(harness.MexError):
            gateway.call("excise_bins", hs, 9, 0, NS, np.ones(64), nargout=0)         # no such context
        with pytest.raises(harness.MexError):
            gateway.call("excise_bins", hs, hd, 0, NS, nargout=0)                      # too few arguments
        with pytest.raises(harness.MexError):
            gateway.call("excise_bins", hs, hd, 0, NS, np.ones(2), nargout=0)          # too short a transform
        with pytest.raises(harness.MexError):
            gateway.call("excise_bins", hs, hd, 0, NS, np.ones(14), nargout=0)         # no plan for this length
        with pytest.raises(harness.MexError):
            gateway.call("excise_bins", hs, hd, 1, NS, np.ones(64), nargout=0)         # beyond the record
        gateway.call("destroy", hs, nargout=0)
        gateway.call("destroy", hd, nargout=0)
    finally:
        gateway.lib.stub_run_atexit()
        dst.close()
