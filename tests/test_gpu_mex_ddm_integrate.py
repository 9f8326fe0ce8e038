"""The MEX gateway's 'correlate_ddm_integrate' command (matlab/gnsscorr_mex.c) through the test-only mex.h: the same bits as
Engine.correlate_ddm_integrate on the same blocks, in the documented layouts 2 x ntaps x (nfreq*3*nruns) and ntaps x (nfreq*3*nmaps),
for a coherent call, a power-only call and both."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexstub"))
pytestmark = pytest.mark.gpu


def test_correlate_ddm_integrate_command_returns_the_librarys_bits(engine, l1ca_scene):
    import cu_sdr_collection_amd as P
    import harness
    S, sats, iq = l1ca_scene
    gateway = harness.Gateway()
    try:
        code = P.codes.generateCAcode(sats[0].prn)
        table = np.concatenate([code[-1:], code, code[:1]]).astype(np.int8)
        offsets = np.array([j / 8 for j in range(-6, 7)])
        freqs = np.array([-500.0, -250.0, 0.0, 0.37, 250.0, 500.0, 1e4, -1e4, 0.0])
        # rows as for 'correlate': channel, first_sample, blksize, remCodePhase, codePhaseStep, earlyLateSpc, carrFreq, remCarrPhase
        rows = np.array([[0, 1234 + 18000 * k, 17999 + k % 3, 0.25 * (k % 4), (1.023e6 + k) / 18e6, 0.5, 2.1e4 - 10.0 * k, 0.7 - k]
                         for k in range(6)], dtype=np.float64).T
        run_len, map_len = np.array([3.0, 1.0, 2.0]), np.array([1.0, 2.0])
        weights = np.array([1.0, -1.0, 1.0, 0.5, -1.0, 0.0])
        engine.load_if(iq, fs=S.samplingFreq)
        engine.set_channel(0, [table])
        b = engine.make_blocks(6)
        for k in range(6):
            (b[k].channel, b[k].first_sample, b[k].blksize, b[k].rem_code_phase, b[k].code_phase_step, b[k].el_spacing, b[k].carr_freq,
             b[k].rem_carr_phase) = (int(rows[0, k]), int(rows[1, k]), int(rows[2, k]), *[float(x) for x in rows[3:, k]])
        nt, nf = offsets.shape[0], freqs.shape[0]
        want_coh, want_pow = engine.correlate_ddm_integrate(b, offsets, freqs, [3, 1, 2], weights=weights, map_len=[1, 2])
        plain_coh, _ = engine.correlate_ddm_integrate(b, offsets, freqs, [3, 1, 2])
        h = gateway.call("create", 0)
        gateway.call("load_if", h, iq, 2, S.samplingFreq, nargout=0)
        gateway.call("set_channel", h, 0, [table.astype(np.float64)], 1, nargout=0)

        def coh_bits(got, want):
            assert got.shape == (2, nt, nf * 3 * 3) and got.dtype == np.float64
            r = got.reshape(2, nt, nf, 3, 3, order="F")                           # (re|im, tap, bin, arm, run)
            for k in range(3):
                for arm in range(3):
                    for m in range(nf):
                        assert r[0, :, m, arm, k].tobytes() == np.ascontiguousarray(want[k, arm, m].real).tobytes(), (k, arm, m)
                        assert r[1, :, m, arm, k].tobytes() == np.ascontiguousarray(want[k, arm, m].imag).tobytes(), (k, arm, m)
            assert np.abs(r[:, :, :, 0, :]).max() > 0

        def pow_bits(got):
            assert got.shape == (nt, nf * 3 * 2) and got.dtype == np.float64
            r = got.reshape(nt, nf, 3, 2, order="F")                              # (tap, bin, arm, map)
            for q in range(2):
                for arm in range(3):
                    for m in range(nf):
                        assert r[:, m, arm, q].tobytes() == np.ascontiguousarray(want_pow[q, arm, m]).tobytes(), (q, arm, m)

        coh_bits(gateway.call("correlate_ddm_integrate", h, rows, offsets, freqs, run_len), plain_coh)               # coherent, no weights
        coh_bits(gateway.call("correlate_ddm_integrate", h, rows, offsets, freqs, run_len, weights), want_coh)
        c, p = gateway.call("correlate_ddm_integrate", h, rows, offsets, freqs, run_len, weights, map_len, nargout=2)     # both
        coh_bits(c, want_coh)
        pow_bits(p)
        c, p = gateway.call("correlate_ddm_integrate", h, rows, offsets, freqs, run_len, weights, map_len, 0, nargout=2)  # power only
        assert c.size == 0
        pow_bits(p)
        with pytest.raises(harness.MexError):
            gateway.call("correlate_ddm_integrate", 9, rows, offsets, freqs, run_len)                 # no such context
        with pytest.raises(harness.MexError, match="usage|correlate_ddm_integrate"):
            gateway.call("correlate_ddm_integrate", h, rows, offsets, freqs)                          # no run lengths
        with pytest.raises(harness.MexError, match="weights"):
            gateway.call("correlate_ddm_integrate", h, rows, offsets, freqs, run_len, weights[:5])    # not one weight per block
        with pytest.raises(harness.MexError, match="mapLen"):
            gateway.call("correlate_ddm_integrate", h, rows, offsets, freqs, run_len, weights, map_len)   # maps without an output for them
        with pytest.raises(harness.MexError):
            gateway.call("correlate_ddm_integrate", h, rows, offsets, freqs, np.array([3.0, 1.0, 1.0]))   # the library's refusal comes through
        with pytest.raises(harness.MexError):
            gateway.call("correlate_ddm_integrate", h, rows, offsets, np.zeros(65), run_len)
        gateway.call("destroy", h, nargout=0)
    finally:
        gateway.lib.stub_run_atexit()
