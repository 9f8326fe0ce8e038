"""The MEX gateway's 'correlate_ddm' command (matlab/gnsscorr_mex.c) through the test-only mex.h: the same bits as
Engine.correlate_ddm on the same blocks, in the documented layout 2 x ntaps x (nfreq*3*nblocks)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexstub"))
pytestmark = pytest.mark.gpu


def test_correlate_ddm_command_returns_the_librarys_bits(engine, l1ca_scene):
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
        rows = np.array([[0, 1234, 17999, 0.25, 1.023e6 / 18e6, 0.5, 2.1e4, 0.7],
                         [0, 40001, 18001, 0.0, (1.023e6 + 3.0) / 18e6, 0.5, 1.9e4, -2.0]], dtype=np.float64).T
        engine.load_if(iq, fs=S.samplingFreq)
        engine.set_channel(0, [table])
        b = engine.make_blocks(2)
        for k in range(2):
            (b[k].channel, b[k].first_sample, b[k].blksize, b[k].rem_code_phase, b[k].code_phase_step, b[k].el_spacing, b[k].carr_freq,
             b[k].rem_carr_phase) = (int(rows[0, k]), int(rows[1, k]), int(rows[2, k]), *[float(x) for x in rows[3:, k]])
        want = engine.correlate_ddm(b, offsets, freqs)                            # [block, arm, bin, tap]
        nt, nf = offsets.shape[0], freqs.shape[0]
        h = gateway.call("create", 0)
        gateway.call("load_if", h, iq, 2, S.samplingFreq, nargout=0)
        gateway.call("set_channel", h, 0, [table.astype(np.float64)], 1, nargout=0)
        got = gateway.call("correlate_ddm", h, rows, offsets, freqs)
        assert got.shape == (2, nt, nf * 3 * 2) and got.dtype == np.float64
        r = got.reshape(2, nt, nf, 3, 2, order="F")                               # (I|Q, tap, bin, arm, block)
        for k in range(2):
            for arm in range(3):
                for m in range(nf):
                    assert r[0, :, m, arm, k].tobytes() == np.ascontiguousarray(want[k, arm, m].real).tobytes(), (k, arm, m)
                    assert r[1, :, m, arm, k].tobytes() == np.ascontiguousarray(want[k, arm, m].imag).tobytes(), (k, arm, m)
        assert np.abs(r[:, :, :, 0, :]).min() > 0
        with pytest.raises(harness.MexError):
            gateway.call("correlate_ddm", 9, rows, offsets, freqs)                # no such context
        with pytest.raises(harness.MexError):
            gateway.call("correlate_ddm", h, rows, offsets, np.zeros(65))         # the library's refusal comes through as an error
        gateway.call("destroy", h, nargout=0)
    finally:
        gateway.lib.stub_run_atexit()
