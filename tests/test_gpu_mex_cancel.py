"""The MEX gateway's 'cancel' command (matlab/gnsscorr_mex.c) through the test-only mex.h: the bytes and amplitudes of Engine.cancel
on the same record - out of place and in place, projected and given amplitudes, both modes - and the library's refusals as errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexstub"))
pytestmark = pytest.mark.gpu
FS = 18e6
NS = 40000


def test_cancel_command_returns_the_librarys_bytes_and_amplitudes(engine):
    import cu_sdr_collection_amd as P
    import harness
    from oracle import gnss_oracle as O
    rng = np.random.default_rng(4100)
    iq = rng.integers(-128, 128, 2 * NS).astype(np.int8)
    tabs = {2: [O.pad_code(O.generate_ca_code(3)).astype(np.int8)], 6: [rng.choice([-1, 1], 2048).astype(np.int8), rng.choice([-1, 1], 2048).astype(np.int8)]}
    # rows: channel, first_sample, blksize, remCodePhase, codePhaseStep, earlyLateSpc, carrFreq, remCarrPhase
    rows = np.array([[6, 4001, 4097, 0.25, 1.023e6 / FS, 0.5, 20500.0, 1.0], [2, 17, 18001, 0.5, 1.023e6 / FS, 0.5, 19000.0, 0.1],
                     [2, 18018, 257, 0.1, 1.023e6 / FS, 0.5, 19001.0, 2.0], [6, 3, 65, 0.7, 1.023e6 / FS, 0.5, 20499.0, 4.0]])
    blocks = engine.make_blocks(len(rows))
    for k, r in enumerate(rows):
        blocks[k].channel, blocks[k].first_sample, blocks[k].blksize = int(r[0]), int(r[1]), int(r[2])
        blocks[k].rem_code_phase, blocks[k].code_phase_step, blocks[k].el_spacing, blocks[k].carr_freq, blocks[k].rem_carr_phase = r[3:]
    for ch, t in tabs.items():
        engine.set_channel(ch, t, index_scale=float(len(t)))
    amp = 30.0 * (rng.uniform(-1, 1, (4, 3)) + 1j * rng.uniform(-1, 1, (4, 3)))
    amp[[1, 2], 1:] = 0
    amp[:, 2] = 0
    amp_mx = np.stack([amp.real, amp.imag], axis=0)                                   # 2 x nblocks x 3 -> (re|im, arm, block)
    amp_mx = np.ascontiguousarray(np.transpose(amp_mx, (0, 2, 1)))
    dst = P.Engine(0)
    gateway = harness.Gateway()
    try:
        hs, hd = gateway.call("create", 0), gateway.call("create", 0)
        for h in (hs, hd):
            for ch, t in tabs.items():
                gateway.call("set_channel", h, ch, list(t), float(len(t)), nargout=0)
        for a_py, a_mx in ((None, None), (amp, amp_mx)):
            for model_only in (0, 1):
                for inplace in (False, True):
                    engine.load_if(iq, fs=FS)
                    dst.load_if(np.zeros_like(iq), fs=FS)
                    want_amp = engine.cancel(blocks, dst=None if inplace else dst, amp=a_py, mode="model" if model_only else "subtract")
                    want = (engine if inplace else dst).read_if(0, NS)
                    gateway.call("load_if", hs, iq, 2, FS, nargout=0)
                    gateway.call("load_if", hd, np.zeros_like(iq), 2, FS, nargout=0)
                    args = [hs, hs if inplace else hd, rows.T] + ([[] if a_mx is None else a_mx, model_only] if (a_mx is not None or model_only) else [])
                    got_amp = gateway.call("cancel", *args)
                    got = gateway.call("read_if", hs if inplace else hd, 0, NS, "int8", 2)
                    assert got_amp.shape == (2, 3, 4) and got_amp.dtype == np.float64
                    assert np.ravel(got).astype(np.int8).tobytes() == want.tobytes(), (a_py is None, model_only, inplace)
                    assert np.array_equal(got_amp[0].T + 1j * got_amp[1].T, want_amp)
                    if not inplace:
                        assert np.ravel(gateway.call("read_if", hs, 0, NS, "int8", 2)).astype(np.int8).tobytes() == iq.tobytes()
        with pytest.raises(harness.MexError):
            gateway.call("cancel", hs, 9, rows.T)                                      # no such context
        with pytest.raises(harness.MexError):
            gateway.call("cancel", hs, hd, rows.T, amp_mx[:, :, :3])                   # amplitudes of another size
        bad = rows.copy()
        bad[2, 1] = 18017                                                              # overlaps the block before it
        with pytest.raises(harness.MexError):
            gateway.call("cancel", hs, hd, bad.T)
        bad = rows.copy()
        bad[1, 2] = NS                                                                 # beyond the record
        with pytest.raises(harness.MexError):
            gateway.call("cancel", hs, hd, bad.T)
        gateway.call("destroy", hs, nargout=0)
        gateway.call("destroy", hd, nargout=0)
    finally:
        gateway.lib.stub_run_atexit()
        dst.close()
