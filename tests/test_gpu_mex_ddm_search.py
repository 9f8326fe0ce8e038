"""The MEX gateway's 'correlate_ddm_search' command (matlab/gnsscorr_mex.c) through the test-only mex.h: the same bits as
Engine.correlate_ddm_search on the same blocks - the peaks as three arrays 3 x (nmaps*nhyp), the power maps ntaps x
(nfreq*3*nmaps*nhyp) and the coherent sums 2 x ntaps x (nfreq*3*nruns*nhyp) - with peaks alone, with maps and with everything."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexstub"))
pytestmark = pytest.mark.gpu


def test_correlate_ddm_search_command_returns_the_librarys_bits(engine, l1ca_scene):
    import cu_sdr_collection_amd as P
    import harness
    S, sats, iq = l1ca_scene
    gateway = harness.Gateway()
    try:
        code = P.codes.generateCAcode(sats[0].prn)
        table = np.concatenate([code[-1:], code, code[:1]]).astype(np.int8)
        offsets = np.array([j / 4 for j in range(-3, 4)])
        freqs = np.array([-250.0, 0.0, 0.37, 250.0, 0.0])
        # rows as for 'correlate': channel, first_sample, blksize, remCodePhase, codePhaseStep, earlyLateSpc, carrFreq, remCarrPhase
        rows = np.array([[0, 1234 + 18000 * k, 17999 + k % 3, 0.25 * (k % 4), (1.023e6 + k) / 18e6, 0.5, 2.1e4 - 10.0 * k, 0.7 - k]
                         for k in range(8)], dtype=np.float64).T
        run_len, map_len, shifts = np.array([3.0, 1.0, 2.0]), np.array([1.0, 2.0]), np.array([2.0, 0.0, 1.0])
        weights = np.random.default_rng(5).choice(np.array([1.0, -1.0, 0.5, 0.0]), size=(3, 8))      # [nhyp, nblocks]
        engine.load_if(iq, fs=S.samplingFreq)
        engine.set_channel(0, [table])
        b = engine.make_blocks(8)
        for k in range(8):
            (b[k].channel, b[k].first_sample, b[k].blksize, b[k].rem_code_phase, b[k].code_phase_step, b[k].el_spacing, b[k].carr_freq,
             b[k].rem_carr_phase) = (int(rows[0, k]), int(rows[1, k]), int(rows[2, k]), *[float(x) for x in rows[3:, k]])
        nt, nf = offsets.shape[0], freqs.shape[0]
        want_coh, want_pow, want_pk = engine.correlate_ddm_search(b, offsets, freqs, [3, 1, 2], map_len=[1, 2], shifts=[2, 0, 1], weights=weights,
                                                                  coherent=True)
        _, _, plain_pk = engine.correlate_ddm_search(b, offsets, freqs, [3, 1, 2], map_len=[1, 2], power=False)
        assert want_pk["power"][:, :, 0].min() > 0
        h = gateway.call("create", 0)
        gateway.call("load_if", h, iq, 2, S.samplingFreq, nargout=0)
        gateway.call("set_channel", h, 0, [table.astype(np.float64)], 1, nargout=0)

        def peak_bits(got, want):
            nhyp = want.shape[0]
            for arr, name in zip(got, ("power", "bin", "tap")):
                assert arr.shape == (3, 2 * nhyp) and arr.dtype == np.float64
                r = arr.reshape(3, 2, nhyp, order="F")                                # (arm, map, hypothesis)
                assert np.ascontiguousarray(r.transpose(2, 1, 0)).tobytes() == want[name].astype(np.float64).tobytes(), name

        peak_bits(gateway.call("correlate_ddm_search", h, rows, offsets, freqs, run_len, map_len, nargout=3), plain_pk)   # one hypothesis
        w_mx = np.ascontiguousarray(weights.T)                                        # nblocks x nhyp
        peak_bits(gateway.call("correlate_ddm_search", h, rows, offsets, freqs, run_len, map_len, shifts, w_mx, nargout=3), want_pk)
        pk, bn, tp, p, c = gateway.call("correlate_ddm_search", h, rows, offsets, freqs, run_len, map_len, shifts, w_mx, nargout=5)
        peak_bits((pk, bn, tp), want_pk)
        assert p.shape == (nt, nf * 3 * 2 * 3) and c.shape == (2, nt, nf * 3 * 3 * 3)
        pr = p.reshape(nt, nf, 3, 2, 3, order="F")                                    # (tap, bin, arm, map, hypothesis)
        assert np.ascontiguousarray(pr.transpose(4, 3, 2, 1, 0)).tobytes() == want_pow.tobytes()
        cr = c.reshape(2, nt, nf, 3, 3, 3, order="F")                                 # (re|im, tap, bin, arm, run, hypothesis)
        assert np.ascontiguousarray(cr[0].transpose(4, 3, 2, 1, 0)).tobytes() == np.ascontiguousarray(want_coh.real).tobytes()
        assert np.ascontiguousarray(cr[1].transpose(4, 3, 2, 1, 0)).tobytes() == np.ascontiguousarray(want_coh.imag).tobytes()
        with pytest.raises(harness.MexError):
            gateway.call("correlate_ddm_search", 9, rows, offsets, freqs, run_len, map_len, nargout=3)                   # no such context
        with pytest.raises(harness.MexError, match="usage|correlate_ddm_search"):
            gateway.call("correlate_ddm_search", h, rows, offsets, freqs, run_len, nargout=3)                            # no map lengths
        with pytest.raises(harness.MexError, match="PK"):
            gateway.call("correlate_ddm_search", h, rows, offsets, freqs, run_len, map_len)                              # nowhere to put the peaks
        with pytest.raises(harness.MexError, match="weights"):
            gateway.call("correlate_ddm_search", h, rows, offsets, freqs, run_len, map_len, shifts, w_mx[:7], nargout=3)
        with pytest.raises(harness.MexError):
            gateway.call("correlate_ddm_search", h, rows, offsets, freqs, run_len, map_len, np.array([0.0, 3.0]), nargout=3)   # 3 + 6 > 8
        with pytest.raises(harness.MexError):
            gateway.call("correlate_ddm_search", h, rows, offsets, freqs, run_len, np.array([1.0, 1.0]), nargout=3)      # the maps do not sum
        gateway.call("destroy", h, nargout=0)
    finally:
        gateway.lib.stub_run_atexit()
