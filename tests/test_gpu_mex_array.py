"""The MEX gateway's 'array_covariance' and 'array_combine' commands (matlab/gnsscorr_mex.c) through the test-only mex.h, and
matlab/gnsscorr_null_steer.m through the interpreter of oracle/mlab: the numbers and bytes of Engine.array_covariance /
Engine.array_combine / receiver.null_steer on the same records, with and without the optional arguments - and the library's refusals
as errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexstub"))
pytestmark = pytest.mark.gpu
FS = 18e6
NS = 40000
K = 3


def _records():
    rng = np.random.default_rng(4500)
    common = rng.normal(0.0, 25.0, 2 * NS)                                       # something the three records share: a covariance with structure
    return [np.clip(np.rint(0.8 * np.roll(common, 2 * k) + rng.normal(0.0, 10.0, 2 * NS)), -128, 127).astype(np.int8) for k in range(K)]


def test_array_commands_return_the_librarys_numbers_and_bytes():
    import cu_sdr_collection_amd as P
    import harness
    raws = _records()
    dt = np.int16
    ND = 30000
    fill = np.full(2 * ND, 85, dtype=dt)
    rng = np.random.default_rng(4501)
    T = 5
    w = rng.uniform(-1, 1, (K, T)) / 3 + 1j * rng.uniform(-1, 1, (K, T))
    weights = np.ascontiguousarray(np.stack([w.real, w.imag], axis=-1)).reshape(K, T, 2)        # C order [K][T][2] ...
    weights_mx = np.asfortranarray(np.transpose(weights, (2, 1, 0)))                             # ... is MATLAB's 2 x T x K
    engines = [P.Engine(0) for _ in range(K + 1)]
    srcs, dst = engines[:K], engines[K]
    gateway = harness.Gateway()
    try:
        hs = [gateway.call("create", 0) for _ in range(K)]
        hd = gateway.call("create", 0)
        hlist = np.array([float(np.ravel(h)[0]) for h in hs])
        for h, e, r in zip(hs, srcs, raws):
            gateway.call("load_if", h, r, 2, FS, nargout=0)
            e.load_if(r, fs=FS)
        for first, n, lags in ((0, NS, 1), (11, 9000, 4), (NS - 1, 1, 32)):
            want = P.Engine.array_covariance(srcs, first, n, lags)
            got = gateway.call("array_covariance", hlist, first, n, lags)
            assert got.dtype == np.int64 and got.shape == (2, K, K * lags)            # the test-only mex.h holds three dimensions: 2 x K x (K L)
            assert np.array_equal(np.ravel(got, order="F"), np.ravel(want)), (first, n, lags)       # cov(:, b, a, l) = C[l][a][b]
        # (optional arguments after weights), the keywords of Engine.array_combine they stand for
        for extra, kw in (((), {}), ((13, 5000, 9), dict(first_sample=13, noutputs=5000, dst_first=9)),
                          ((20000, np.zeros((0, 0)), 77), dict(first_sample=20000, dst_first=77))):
            dst.load_if(fill, fs=FS)
            want_res = P.Engine.array_combine(srcs, dst, w, **kw)
            want = dst.read_if(0, ND, dtype=dt)
            gateway.call("load_if", hd, fill, 2, FS, nargout=0)
            r = gateway.call("array_combine", hlist, hd, weights_mx, *extra)
            got = gateway.call("read_if", hd, 0, ND, "int16", 2)
            assert np.ravel(got).astype(dt).tobytes() == want.tobytes(), extra
            assert r.dtype == np.float64 and np.ravel(r).tolist() == [want_res.clipped, want_res.sum_sq, want_res.noutputs]
            assert want_res.sum_sq > 0
        with pytest.raises(harness.MexError):
            gateway.call("array_covariance", hlist, 0, NS)                          # too few arguments
        with pytest.raises(harness.MexError):
            gateway.call("array_covariance", hlist, 0, NS, 33)                      # more lags than the library takes
        with pytest.raises(harness.MexError):
            gateway.call("array_covariance", hlist, 0.5, NS, 1)                     # no whole number
        with pytest.raises(harness.MexError):
            gateway.call("array_covariance", hlist, 1, NS, 1)                       # beyond the records
        with pytest.raises(harness.MexError):
            gateway.call("array_covariance", np.zeros(9), 0, NS, 1)                 # nine handles
        with pytest.raises(harness.MexError):
            gateway.call("array_combine", hlist, hd, np.ones((3, T * K)))            # weights that are not 2 x T x K
        with pytest.raises(harness.MexError):
            gateway.call("array_combine", hlist, hd, np.ones((2, K * T + 1)))        # ... or no whole number of taps per record
        with pytest.raises(harness.MexError):
            gateway.call("array_combine", hlist, float(hlist[1]), weights_mx)        # dst is a source
        with pytest.raises(harness.MexError):
            gateway.call("array_combine", hlist, hd, weights_mx, 0, ND + 1)          # beyond dst's record
        for h in hs + [hd]:
            gateway.call("destroy", h, nargout=0)
    finally:
        gateway.lib.stub_run_atexit()
        for e in engines:
            e.close()


def test_the_matlab_wrapper_maps_its_arguments_as_the_python_one():
    import bridge
    import cu_sdr_collection_amd as P
    import harness
    from oracle import mlab
    raws = _records()
    dt, target_rms = np.int8, 30.0
    engines = [P.Engine(0) for _ in range(K + 1)]
    srcs, dst = engines[:K], engines[K]
    gateway = harness.Gateway()
    try:
        hs = [gateway.call("create", 0) for _ in range(K)]
        hd = gateway.call("create", 0)
        hlist = np.array([[float(np.ravel(h)[0]) for h in hs]])
        for h, e, r in zip(hs, srcs, raws):
            gateway.call("load_if", h, r, 2, FS, nargout=0)
            e.load_if(r, fs=FS)
        S = P.initSettings()
        S.samplingFreq, S.fileType = FS, 2
        I = bridge.install(bridge.interpreter_for("GPS_L1CA"), gateway, P, "GPS_L1CA")
        mex = I.extra_builtins["gnsscorr_mex"]

        def mex_2d(_I, args, nargout):
            """The interpreter holds matrices only: the 2 x K x K x L covariance goes in as 2 x (K K L), the same numbers in the same
            (column-major) order, which is all gnsscorr_null_steer.m relies on (it indexes cov(:))."""
            if args[0].s != "array_covariance":
                return mex(_I, args, nargout)
            cov = gateway.call("array_covariance", *[bridge._to_py(a) for a in args[1:]])
            return np.ravel(cov, order="F").reshape(2, -1, order="F").astype(np.float64)
        I.extra_builtins["gnsscorr_mex"] = mex_2d
        for ntaps, ref, first, n, loading in ((1, 0, 0, NS, 0.0), (3, 1, 7, 20000, 1e4)):
            ND = n + 5
            dst.load_if(np.full(2 * ND, 85, dtype=dt), fs=FS)
            want_res, want_w, want_gain, want_cov = P.null_steer(srcs, dst, S, ntaps=ntaps, ref=ref, first_sample=first, nsamples=n, loading=loading,
                                                                 target_rms=target_rms)
            want = dst.read_if(0, ND, dtype=dt)
            gateway.call("load_if", hd, np.full(2 * ND, 85, dtype=dt), 2, FS, nargout=0)
            args = [mlab.to_matlab(hlist), mlab.to_matlab(float(np.ravel(hd)[0])), mlab.to_matlab(S), mlab.to_matlab(float(ntaps)), mlab.to_matlab(float(ref + 1)),
                    mlab.to_matlab(float(first)), mlab.to_matlab(float(n)), mlab.to_matlab(float(loading)), mlab.to_matlab(float(target_rms))]
            res, w, gain, cov = I.call("gnsscorr_null_steer", *args, nargout=4)
            res, w, gain, cov = mlab.from_matlab(res), np.ravel(mlab.from_matlab(w)), float(np.ravel(mlab.from_matlab(gain))[0]), mlab.from_matlab(cov)
            got = gateway.call("read_if", hd, 0, ND, "int8", 2)
            assert np.ravel(got).astype(dt).tobytes() == want.tobytes(), ntaps
            assert (res.clipped, res.sumSq, res.nOutputs) == (want_res.clipped, want_res.sum_sq, want_res.noutputs) and want_res.noutputs == n
            assert np.array_equal(w, np.ravel(want_w)) and gain == want_gain and want_gain != 1.0
            assert np.array_equal(np.ravel(cov, order="F"), np.ravel(want_cov).astype(np.float64))
            assert abs(want_w[ref, 0] - 1.0) < 1e-12 and abs(np.sqrt(want_res.sum_sq / (2 * n)) - target_rms) < 1.5
            assert np.all(want[2 * n:] == 85)
        for h in hs + [hd]:
            gateway.call("destroy", h, nargout=0)
    finally:
        gateway.lib.stub_run_atexit()
        for e in engines:
            e.close()
