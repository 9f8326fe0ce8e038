"""The MATLAB drop-in with settings.gnsscorrWindowSamples AND settings.gnsscorrDeviceLoop: matlab/gnsscorr_tracking.m sends the file
through gnsscorr_mex('track_file_device') -> gc_track_file_device (compiled gateway, oracle/mlab interpreter, as
tests/test_gpu_mex_gateway.py) and returns the trackResults of the drop-in with gnsscorrDeviceLoop alone (resident record)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ref_scenes as RS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexstub"))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gateway():
    import harness
    g = harness.Gateway()
    plain = g.call
    g.calls = []

    def recorded(cmd, *args, nargout=1):   # the drop-in's gateway commands, in order
        g.calls.append(cmd)
        return plain(cmd, *args, nargout=nargout)

    g.call = recorded
    yield g
    g.lib.stub_run_atexit()          # mexAtExit: destroys whatever contexts are left


def test_matlab_drop_in_tracks_windows_with_the_loop_closed_on_the_gpu(gateway, tmp_path):
    import bridge
    import cu_sdr_collection_amd as P
    from oracle import mlab
    sc = next(s for s in RS.TRACK_SCENES if s.name == "GPS_L1CA")
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    S.gnsscorrDeviceLoop = 1.0
    path = str(tmp_path / "record.bin")
    rec.tofile(path)
    mch = mlab.to_matlab([SimpleNamespace(**{k: (v if isinstance(v, str) else float(v)) for k, v in vars(c).items()}) for c in ch])
    out, cmds = [], []
    for window in (0, int(S.samplingFreq * S.intTime * 14.5)):
        I = bridge.install(bridge.interpreter_for("GPS_L1CA"), gateway, P, sc.signal)
        fid = mlab.register_file(I, rec.tobytes(), path)
        if window:
            S.gnsscorrWindowSamples = float(window)
        n0 = len(gateway.calls)
        try:
            tr, _ = I.call("tracking", fid, mch, mlab.to_matlab(S), nargout=2)
        finally:
            I.call("gnsscorr_context", "", "clear")
        cmds.append(gateway.calls[n0:])
        out.append(mlab.from_matlab(tr))
    assert "track_device" in cmds[0] and "track_file_device" not in cmds[0]
    assert "track_file_device" in cmds[1] and "track_file" not in cmds[1] and "track_device" not in cmds[1]
    for a, b in zip(*out):
        assert a.status == b.status
        for f in vars(a):
            if isinstance(getattr(a, f), np.ndarray):
                assert np.array_equal(getattr(a, f), getattr(b, f)), f
