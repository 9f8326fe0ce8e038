"""The MEX gateway's 'probe_psd' and 'probe_histogram' commands (matlab/gnsscorr_mex.c) through the test-only mex.h: the same bytes
as Engine.probe_psd / Engine.probe_histogram on the same record, and the library's refusals as errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexstub"))
pytestmark = pytest.mark.gpu
FS = 18e6


def test_probe_commands_return_the_librarys_bytes(engine):
    import harness
    rng = np.random.default_rng(2048)
    iq = rng.integers(-128, 128, 2 * 40011).astype(np.int8)
    iq[2:4] = [-128, 127]
    engine.load_if(iq, fs=FS)
    gateway = harness.Gateway()
    try:
        h = gateway.call("create", 0)
        gateway.call("load_if", h, iq, 2, FS, nargout=0)
        want, k_want = engine.probe_psd(7, 10000, 1000, 62, "hamming", nspans=3)
        got, k = gateway.call("probe_psd", h, 7, 10000, 1000, 62, "hamming", 3, nargout=2)
        assert got.shape == (1000, 3) and got.dtype == np.float64 and float(np.ravel(k)[0]) == k_want == 10
        assert got.tobytes(order="F") == want.tobytes()                                # one column per span: gc_probe_psd's rows as they lie
        rect = gateway.call("probe_psd", h, 0, 4096, 64, 4, "rect")
        assert rect.tobytes(order="F") == engine.probe_psd(0, 4096, 64, 4, "rect")[0].tobytes()
        dflt = gateway.call("probe_psd", h, 3, 40000)                                  # the reference's call: 32768, 2048, Hamming
        assert dflt.shape == (32768, 1) and dflt.tobytes(order="F") == engine.probe_psd(3, 40000)[0].tobytes()
        counts, norm2 = gateway.call("probe_histogram", h, 1, 30000, nargout=2)
        c_want, m_want = engine.probe_histogram(1, 30000)
        assert counts.shape == (257, 2) and counts.dtype == np.uint64 and float(np.ravel(norm2)[0]) == m_want == 128 ** 2 + 127 ** 2
        assert counts.tobytes(order="F") == c_want.tobytes() and int(counts[:, 0].sum()) == 30000
        with pytest.raises(harness.MexError):
            gateway.call("probe_psd", 9, 0, 4096, 64, 4)                               # no such context
        with pytest.raises(harness.MexError):
            gateway.call("probe_psd", h, 0, 4096, 7, 0)                                # the planner's refusal comes through as an error
        with pytest.raises(harness.MexError):
            gateway.call("probe_psd", h, 0, 4096, 64, 4, "hann")
        with pytest.raises(harness.MexError):
            gateway.call("probe_psd", h, 36000, 4096, 64, 4)                           # beyond the record
        with pytest.raises(harness.MexError):
            gateway.call("probe_histogram", h, 40011, 1)
        gateway.call("destroy", h, nargout=0)
    finally:
        gateway.lib.stub_run_atexit()
