"""HIP correlator (gc_correlate / replay, through the C-ABI) vs the CPU oracle — the parity
gate for tracking.m:247-300.

Tolerance.  The reference computes in float64; the kernel keeps code/carrier *phase* in float64 /
64-bit fixed point (so chip-edge decisions are exact) but mixes and accumulates in float32.
Bound used: |delta| <= TOL * sum_n(|I_n| + |Q_n|) per output, TOL = 2e-6; measured margin is
reported by test_tolerance_margin (typically < 2e-7).  A single wrong chip decision or a one-sample
misalignment changes an output by ~1e-4 * sum, i.e. 50x the bound.
"""
import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import gnss_oracle as O

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TOL = 2e-6


def _blocks(engine, descs):
    b = engine.make_blocks(len(descs))
    for k, d in enumerate(descs):
        b[k].channel = d["channel"]
        b[k].blksize = d["n"]
        b[k].first_sample = d["s0"]
        b[k].rem_code_phase = d["rem"]
        b[k].code_phase_step = d["step"]
        b[k].el_spacing = d["d"]
        b[k].carr_freq = d["f"]
        b[k].rem_carr_phase = d["phi"]
    return b


def _oracle(iq, d, table, code_length=1023.0, fs=18e6):
    s, _, _ = CO.correlate_block(iq, d["s0"], d["n"], [table], d["rem"], d["step"], d["d"], d["f"], d["phi"],
                                 fs, code_length)
    return s[0]


def _scale(iq, d):
    seg = iq[2 * d["s0"]:2 * (d["s0"] + d["n"])].astype(np.float64)
    return np.sum(np.abs(seg))


def _random_descs(rng, n, nsamp, nch, fs=18e6, fc=1.023e6, L=1023.0):
    out = []
    for _ in range(n):
        step = (fc + rng.uniform(-5, 5)) / fs
        rem = rng.uniform(0, step)
        N = int(np.ceil((L - rem) / step))
        out.append(dict(channel=int(rng.integers(0, nch)), n=N, s0=int(rng.integers(0, nsamp - N)),
                        rem=rem, step=step, d=0.5, f=20e3 + rng.uniform(-5e3, 5e3),
                        phi=rng.uniform(-2 * np.pi, 2 * np.pi)))
    return out


def test_correlate_matches_oracle(engine, l1ca_scene):
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    tables = []
    for i, s in enumerate(sats):
        t = O.pad_code(O.generate_ca_code(s.prn))
        tables.append(t)
        engine.set_channel(i, [t.astype(np.int8)])
    rng = np.random.default_rng(1)
    descs = _random_descs(rng, 64, iq.shape[0] // 2, len(sats))
    # edge cases the reference hits: rem = 0 at the first block (tracking.m:165; ceil(0)+1 -> the
    # wrapped last chip, :266-270), block starting at sample 0 and ending at the last sample
    descs[0].update(rem=0.0, s0=0, phi=0.0)
    descs[1].update(s0=iq.shape[0] // 2 - descs[1]["n"])
    descs[2].update(s0=7)  # unaligned head
    got = engine.correlate(_blocks(engine, descs))
    worst = 0.0
    for k, d in enumerate(descs):
        ref = _oracle(iq, d, tables[d["channel"]])
        err = np.abs(got[k, 0] - ref).max() / _scale(iq, d)
        worst = max(worst, err)
        assert err < TOL, (k, d, got[k, 0], ref)
        assert np.all(got[k, 1:] == 0)
    print(f"worst relative error {worst:.3e} (bound {TOL:.1e})")


def test_replay_matches_correlate_and_is_deterministic(engine, l1ca_scene):
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    for i, s in enumerate(sats):
        engine.set_channel(i, [O.pad_code(O.generate_ca_code(s.prn)).astype(np.int8)])
    rng = np.random.default_rng(2)
    descs = _random_descs(rng, 1024, iq.shape[0] // 2, len(sats))
    b = _blocks(engine, descs)
    a = engine.correlate(b)
    engine.replay_prepare(b)
    engine.replay_launch()
    r1 = engine.replay_fetch()
    engine.replay_launch()
    r2 = engine.replay_fetch()
    assert np.array_equal(r1, r2), "replay must be bit-reproducible (no atomics in the reduction)"
    # correlate() may split blocks over several workgroups; the sums then differ by rounding only
    scale = np.array([_scale(iq, d) for d in descs])[:, None]
    assert np.max(np.abs(a[:, 0] - r1[:, 0]) / scale) < 5e-7


def test_noise_free_identities(engine):
    """Analytic identities: a noise-free block correlated against its own replica
    gives I_P = A*N, Q_P ~ 0 and E = L = A*N*(1 - d) for spacing d."""
    import cu_sdr_collection_amd as P
    S = P.initSettings()
    fs, fc = S.samplingFreq, S.codeFreqBasis
    sat = P.synth.SatSpec(prn=7, doppler=1234.0, code_phase_samples=0.0, carrier_phase=0.0, cn0_dbhz=0.0)
    n = int(0.004 * fs)
    A = 100.0
    # amplitude override: build the IF by hand (no noise, no data bits)
    code = P.codes.generateCAcode(7).astype(np.float64)
    t = np.arange(n) / fs
    chip = np.floor(np.arange(n) * (fc / fs)).astype(np.int64) % 1023
    x = A * code[chip] * np.exp(1j * 2 * np.pi * (S.IF + sat.doppler) * t)
    iq = np.empty(2 * n, dtype=np.int8)
    iq[0::2] = np.rint(x.real)
    iq[1::2] = np.rint(x.imag)
    engine.load_if(iq, fs=fs)
    engine.set_channel(0, [P.codes.padded_table(P.codes.generateCAcode(7))])
    step = fc / fs
    N = int(np.ceil(1023 / step))
    # rem = 0: replica index ceil(n*step) picks chip floor(n*step) for every n > 0, i.e. exactly the
    # chip the synthetic signal carries; only sample 0 reads the wrapped last chip (tracking.m:266-270)
    d = dict(channel=0, n=N, s0=0, rem=0.0, step=step, d=0.5, f=S.IF + sat.doppler, phi=0.0)
    got = engine.correlate(_blocks(engine, [d]))[0, 0]
    ref = _oracle(iq, d, O.pad_code(O.generate_ca_code(7)))
    assert np.abs(got - ref).max() < TOL * _scale(iq, d)
    i_e, q_e, i_p, q_p, i_l, q_l = got
    assert abs(i_p - A * N) < 0.01 * A * N
    assert abs(q_p) < 0.01 * A * N
    assert abs(np.hypot(i_e, q_e) - 0.5 * A * N) < 0.05 * A * N
    assert abs(np.hypot(i_l, q_l) - 0.5 * A * N) < 0.05 * A * N


def test_range_error_and_argument_checks(engine, l1ca_scene):
    import cu_sdr_collection_amd as P
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    engine.set_channel(0, [O.pad_code(O.generate_ca_code(1)).astype(np.int8)])
    d = dict(channel=0, n=18000, s0=iq.shape[0] // 2 - 17999, rem=0.0, step=1.023e6 / 18e6, d=0.5, f=2e4, phi=0.0)
    with pytest.raises(P.GnssCorrError) as e:
        engine.correlate(_blocks(engine, [d]))
    assert e.value.status == P._lib.GC_E_RANGE  # short read, tracking.m:241-245
    d.update(s0=0, channel=200)
    with pytest.raises(P.GnssCorrError) as e:
        engine.correlate(_blocks(engine, [d]))
    assert e.value.status == P._lib.GC_E_STATE
    assert engine.correlate(engine.make_blocks(0)).shape[0] == 0  # empty input


def test_int16_and_qi_layouts(engine, l1ca_scene):
    """int16 samples (tracking.m:145-148,212-213) and the GLONASS Q,I order
    (GLO_GL1/include/tracking.m:227) go through the same kernel template."""
    import cu_sdr_collection_amd as P
    S, sats, iq = l1ca_scene
    iq = iq[:2 * 400000]
    rng = np.random.default_rng(5)
    descs = _random_descs(rng, 16, iq.shape[0] // 2, 1)
    tab = O.pad_code(O.generate_ca_code(sats[0].prn))
    engine.set_channel(0, [tab.astype(np.int8)])
    # int16: scale by 37 so the high byte matters
    iq16 = iq.astype(np.int16) * 37
    engine.load_if(iq16, fs=S.samplingFreq)
    got16 = engine.correlate(_blocks(engine, descs))[:, 0]
    engine.load_if(iq, layout=P._lib.GC_QI, fs=S.samplingFreq)
    gotqi = engine.correlate(_blocks(engine, descs))[:, 0]
    for k, d in enumerate(descs):
        ref = _oracle(iq, d, tab)
        assert np.abs(got16[k] - 37 * ref).max() < TOL * 37 * _scale(iq, d)
        sw, _, _ = CO.correlate_block(iq, d["s0"], d["n"], [tab], d["rem"], d["step"], d["d"], d["f"], d["phi"],
                                      18e6, 1023.0, swap_iq=True)
        assert np.abs(gotqi[k] - sw[0]).max() < TOL * _scale(iq, d)


def test_fast_and_generic_kernels_agree_with_oracle(engine, l1ca_scene):
    """GPS L1 C/A qualifies for the fast single-transition kernel (corr_fast.hip); the generic
    per-sample-lookup kernel (corr_kernel.hip) must give the same sums.  Both vs the oracle,
    including first-block ties (rem = 0 with the rational nominal step: samples 3000k sit exactly
    on chip edges) at every head alignment."""
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    tab = O.pad_code(O.generate_ca_code(sats[0].prn))
    engine.set_channel(0, [tab.astype(np.int8)])
    rng = np.random.default_rng(11)
    descs = _random_descs(rng, 40, iq.shape[0] // 2, 1)
    step0 = 1.023e6 / 18e6
    for k in range(16):  # tie blocks
        descs[k].update(rem=0.0, step=step0, n=18000, s0=1000 + k, phi=0.0)
    b = _blocks(engine, descs)
    try:
        engine.force_generic_kernel(False)
        fast = engine.correlate(b)[:, 0]
        engine.force_generic_kernel(True)
        gen = engine.correlate(b)[:, 0]
    finally:
        engine.force_generic_kernel(False)
    for k, d in enumerate(descs):
        ref = _oracle(iq, d, tab)
        sc = _scale(iq, d)
        assert np.abs(fast[k] - ref).max() < TOL * sc, ("fast", k, d)
        assert np.abs(gen[k] - ref).max() < TOL * sc, ("generic", k, d)


def test_tie_dense_blocks_use_the_references_two_roundings(engine, l1ca_scene):
    """Rational code steps (0.05, 0.1, 0.2 chip per sample) with rem = 0.1 and early-late spacing 0.3 put a
    sample of the early or late ramp within 1e-16 chip of a table edge every few samples.  There the reference's
    fl(a + fl(i*d)) (and the backwards half of MATLAB's colon, tracking.m:252-270) decides the index, and a fused
    multiply-add gives a DIFFERENT answer (one rounding instead of two) — the regression this test pins: the
    exact paths must not be compiled with floating-point contraction.  All three kernels: 16- and 8-sample
    transition-mask kernels and the lane kernel."""
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    tab = O.pad_code(O.generate_ca_code(sats[0].prn))
    engine.set_channel(0, [tab.astype(np.int8)])
    descs = []
    for step in (0.05, 0.1, 0.2):
        for d in (0.3, 0.5, 0.25):
            for n in (64, 1000, 5000):
                descs.append(dict(channel=0, n=n, s0=777 + 13 * len(descs), rem=0.1, step=step, d=d, f=2.2e4, phi=0.4))
    for generic in (False, True):
        engine.force_generic_kernel(generic)
        try:
            for d in descs:      # one launch per block: the step decides which kernel a launch takes
                got = engine.correlate(_blocks(engine, [d]))[0, 0]
                ref = _oracle(iq, d, tab)
                assert np.abs(got - ref).max() < TOL * _scale(iq, d), (generic, d, got, ref)
        finally:
            engine.force_generic_kernel(False)


def test_two_bit_packed_record_is_expanded_on_the_gpu(engine):
    """gc_load_if_packed2: the packed bytes of unpack_cplx.m's input format cross PCIe and become the int8
    I/Q record in HBM; bit-exact against the oracle's restatement of the reference's lookup tables, odd lengths included."""
    rng = np.random.default_rng(5)
    for n in (1, 3, 4, 1021, 200001):
        packed = rng.integers(0, 256, size=n, dtype=np.uint8)
        engine.load_if_packed2(packed, fs=18e6)
        _, ns = engine.if_buffer()
        assert ns == 2 * n
        got = engine.read_if(0, 2 * n)
        assert np.array_equal(got, O.unpack_cplx(packed))


def test_preamble_cross_correlation_and_subframe_start(engine):
    """gc_preamble_xcorr against numpy and the oracle's NAVdecoding restatement."""
    import cu_sdr_collection_amd as P
    from tests.test_host_logic import _nav_stream
    rng = np.random.default_rng(4)
    x = _nav_stream(rng, 1234, 3)
    want_start, want_corr = O.find_subframe_start(x, x.shape[0])
    got_corr = engine.preamble_xcorr(x, np.kron(P.nav_sync.PREAMBLE_BITS, np.ones(20, dtype=np.int8)))
    assert np.array_equal(got_corr, want_corr.astype(np.float32))
    assert P.nav_sync.find_subframe_start(engine, x, x.shape[0]) == want_start == 1234
    assert P.nav_sync.find_subframe_start(engine, -x, x.shape[0]) == 1234


def test_big_periodic_replay_lists_take_the_four_wave_kernels_and_match_the_oracle(engine, monkeypatch):
    """BASELINE-size replay lists (>= 64 blocks per channel and CU, periodic channel pattern) run the four-wave
    instantiations of the fast kernel, which no small list reaches: float tables (GPS L1 C/A, shared early/late ramp),
    int8-pair tables, and the unshared-ramp variant (spacing != 1/2 chip).  Sampled blocks against the C oracle,
    2000 blocks against gc_correlate (one-wave kernel) on the same descriptors."""
    rng = np.random.default_rng(77)
    nsamp = 2_000_000
    iq = rng.integers(-40, 41, size=2 * nsamp, dtype=np.int8)
    engine.load_if(iq, fs=18e6)
    tables = [O.pad_code(O.generate_ca_code(p)) for p in (5, 19)]
    for k, t in enumerate(tables):
        engine.set_channel(k, [t])
    _, cus = engine.device_info()
    nb = 64 * 2 * cus + 2 * 37                      # just over the launcher's big-list threshold, not a multiple of 8 epochs
    from cu_sdr_collection_amd import _lib as L
    for spacing, env, want in ((0.5, {}, 3), (0.5, {"GC_NO_TABF": "1"}, 2), (0.3, {}, 3)):
        if env and not L.is_tuning_build():          # the switch back to the int8-pair tables exists in libgnsscorr_tuning.so only
            continue
        descs = _random_descs(rng, nb, nsamp, 2)
        for i, d in enumerate(descs):
            d["channel"] = i % 2
            d["d"] = spacing
        descs[0]["rem"] = 0.0                        # exact ties at samples 3000 k with the nominal step
        descs[0]["step"] = 1.023e6 / 18e6
        descs[0]["n"] = 18000
        b = _blocks(engine, descs)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        engine.replay_prepare(b)
        engine.replay_launch()
        got = engine.replay_fetch()[:, 0]
        assert engine.last_kernel() == want
        for k in env:
            monkeypatch.delenv(k)
        for i in list(range(0, 8)) + [int(x) for x in rng.integers(0, nb, 40)] + [nb - 1]:
            d = descs[i]
            assert np.abs(got[i] - _oracle(iq, d, tables[d["channel"]])).max() < TOL * _scale(iq, d), (spacing, env, i)
        sub = list(range(0, nb, nb // 2000))
        small = engine.correlate(_blocks(engine, [descs[i] for i in sub]))[:, 0]
        assert engine.last_kernel() == 1
        scale = 18000 * 2 * 20.0
        assert np.abs(got[sub] - small).max() < 2e-7 * scale


def test_replay_launch_does_not_depend_on_what_ran_in_between(engine, l1ca_scene):
    """gc_replay_launch plans from the scope gc_replay_prepare kept with the list (LaunchScope, gc_internal.h), not from whatever the
    context's last launch left behind: a prepared list of 2 one-arm channels x 4 epochs of 2 048 samples, then - on the same context -
    gc_correlate on a three-arm channel with tables more than ten times longer and a 4-epoch gc_track of a two-arm channel, then gc_replay_launch
    again without a second prepare.  Same kernel, bit-identical sums."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import _lib as L
    from cu_sdr_collection_amd.receiver import track_params
    S, sats, iq = l1ca_scene
    engine.load_if(iq, fs=S.samplingFreq)
    rng = np.random.default_rng(91)
    ca = [P.codes.padded_table(P.codes.generateCAcode(s.prn)) for s in sats[:2]]
    for k, t in enumerate(ca):
        engine.set_channel(k, [t])
    step = 1.023e6 / 18e6
    descs = [dict(channel=i % 2, n=2048, s0=int(rng.integers(0, 10 ** 6)), rem=float(rng.uniform(0, step)), step=step, d=0.5,
                  f=20e3 + float(rng.uniform(-5e3, 5e3)), phi=float(rng.uniform(-3, 3))) for i in range(8)]
    engine.replay_prepare(_blocks(engine, descs))
    engine.replay_launch()
    first, kernel = engine.replay_fetch().copy(), engine.last_kernel()
    for i, d in enumerate(descs):
        assert np.abs(first[i, 0] - _oracle(iq, d, O.pad_code(O.generate_ca_code(sats[d["channel"]].prn)))).max() < TOL * _scale(iq, d), i
    # another scope: three arms of 10 402 entries (the replay list's tables have 1 025) at ten times the rate (the lane kernel, other LDS needs, other splits)
    engine.set_channel(2, [O.pad_code(rng.choice([-1.0, 1.0], size=10400)).astype(np.int8) for _ in range(3)])
    other = engine.correlate(_blocks(engine, [dict(channel=2, n=9000, s0=4321, rem=0.1, step=10.23e6 / 18e6, d=0.3, f=20e3, phi=0.5)]))
    assert other[0, :3].any() and engine.last_kernel() == 0 != kernel
    # ... and a closed loop over a two-arm channel: its scope comes from the channel set and changes with every epoch
    engine.set_channel(3, [ca[0], ca[1]])
    ms = S.msToProcess
    try:
        S.msToProcess = 4
        init = L.gc_channel_init(channel=3, prn=sats[0].prn, acquired_freq=S.IF + sats[0].doppler, code_freq=S.codeFreqBasis,
                                 code_phase=int(np.ceil(sats[0].code_phase_samples)) + 1)
        _, done, st = engine.track(track_params(S), [init])
    finally:
        S.msToProcess = ms
    assert st == 0 and list(done) == [4]
    engine.replay_launch()
    again = engine.replay_fetch()
    assert engine.last_kernel() == kernel
    assert first.tobytes() == again.tobytes()


def test_big_periodic_replay_with_eight_sample_chunks(engine, monkeypatch):
    """The same for a B1I-rate replica (2.046 Mcps at 18 Msps: 8.8 samples per chip -> 8-sample lane-chunks): four-wave
    kernels with float tables and with int8-pair tables."""
    rng = np.random.default_rng(78)
    nsamp = 2_000_000
    iq = rng.integers(-40, 41, size=2 * nsamp, dtype=np.int8)
    engine.load_if(iq, fs=18e6)
    tables = [O.pad_code(rng.choice(np.array([-1, 1], dtype=np.int8), size=2046)) for _ in range(2)]
    for k, t in enumerate(tables):
        engine.set_channel(k, [t])
    _, cus = engine.device_info()
    nb = 64 * 2 * cus + 2 * 11
    # (GC_NO_MULTI: without it such a list goes to corr_multi.hip - 16-sample chunks with two transitions, kernel 4, third pass)
    from cu_sdr_collection_amd import _lib as L
    for env, want in (({"GC_NO_MULTI": "1"}, 3), ({"GC_NO_MULTI": "1", "GC_NO_TABF": "1"}, 2), ({}, 4)):
        if env and not L.is_tuning_build():          # the 8-sample kernels behind their switches: libgnsscorr_tuning.so only
            continue
        descs = _random_descs(rng, nb, nsamp, 2, fc=2.046e6, L=2046.0)
        for i, d in enumerate(descs):
            d["channel"] = i % 2
        b = _blocks(engine, descs)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        engine.replay_prepare(b)
        engine.replay_launch()
        got = engine.replay_fetch()[:, 0]
        assert engine.last_kernel() == want
        for k in env:
            monkeypatch.delenv(k)
        for i in list(range(0, 4)) + [int(x) for x in rng.integers(0, nb, 30)] + [nb - 1]:
            d = descs[i]
            ref = _oracle(iq, d, tables[d["channel"]], code_length=2046.0)
            assert np.abs(got[i] - ref).max() < TOL * _scale(iq, d), (env, i)


def test_broadcast_record_is_adopted_without_a_copy():
    """sharding.broadcast_record on the GPU (backend nccl = RCCL; world size 1 here, the eight-GPU run is the driver's) and
    gc_attach_if: the engine correlates straight out of the torch tensor that received the broadcast.  In its own process,
    torch first: torch brings its own copy of the HIP runtime, and whichever copy is loaded first serves the process."""
    import subprocess
    import sys
    code = r"""
import socket, sys
import numpy as np
import torch, torch.distributed as dist
assert torch.cuda.is_available()
torch.cuda.set_device(0)
sys.path.insert(0, %r)
import cu_sdr_collection_amd as P
from cu_sdr_collection_amd.sharding import broadcast_record
from oracle import gnss_oracle as O
S = P.initSettings()
sats = P.synth.scene(2, 5, S.samplingFreq)
iq = P.synth.generate_if(sats, int(0.05 * S.samplingFreq), S.samplingFreq, S.IF, P.codes.generateCAcode, S.codeFreqBasis, 1023, seed=9)
with socket.socket() as s:
    s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda:0"))
t = broadcast_record(torch.from_numpy(iq.copy()), src=0, device="cuda:0")
torch.cuda.synchronize()
assert t.is_cuda and t.dtype == torch.int8 and t.numel() == iq.size
eng = P.Engine(0)
eng.set_channel(0, [O.pad_code(O.generate_ca_code(sats[0].prn))])
b = eng.make_blocks(3)
for k in range(3):
    b[k].channel = 0; b[k].first_sample = 1000 + 20000 * k; b[k].blksize = 18000; b[k].rem_code_phase = 0.25 * k
    b[k].code_phase_step = 1.023e6 / 18e6; b[k].el_spacing = 0.5; b[k].carr_freq = 20e3 + 100 * k; b[k].rem_carr_phase = 0.3
eng.load_if(iq, fs=S.samplingFreq)
want = eng.correlate(b).copy()
eng.attach_if(t.data_ptr(), iq.size // 2)
eng.set_sampling_freq(S.samplingFreq)
got = eng.correlate(b)
assert np.array_equal(got, want) and np.abs(got).max() > 0
eng.close()
dist.destroy_process_group()
print("BROADCAST_ATTACH_OK")
""" % (ROOT,)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "BROADCAST_ATTACH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_wave_transpose_sum_adds_every_component_over_the_wave(engine):
    """The lane kernel empties its 6 x ARMS per-lane sums through ONE transposing reduction (corr_common.h: wave_transpose_sum).
    Integer-valued floats add exactly in any order: every component's total must be the exact sum of its 64 lanes, for the three
    sizes the kernel instantiates (6, 12, 18) and for odd, small and full ones (1, 2, 7, 31, 32); general values within float32
    rounding of a 64-term sum."""
    rng = np.random.default_rng(91)
    for k in (1, 2, 6, 7, 12, 18, 31, 32):
        v = rng.integers(-1000, 1001, size=(k, 64)).astype(np.float32)
        got = engine.debug_wave_transpose_sum(v)
        assert np.array_equal(got, v.sum(axis=1, dtype=np.float64).astype(np.float32)), k
        one = np.zeros((k, 64), np.float32)          # a single non-zero lane per component: nothing lost, nothing doubled
        one[np.arange(k), rng.integers(0, 64, size=k)] = np.arange(1, k + 1)
        assert np.array_equal(engine.debug_wave_transpose_sum(one), np.arange(1, k + 1, dtype=np.float32)), k
        w = rng.standard_normal((k, 64)).astype(np.float32) * 1e3
        ref = w.astype(np.float64).sum(axis=1)
        assert np.max(np.abs(engine.debug_wave_transpose_sum(w) - ref)) <= 64 * 2.0 ** -24 * np.abs(w).sum(axis=1).max(), k
    with pytest.raises(Exception):
        engine.debug_wave_transpose_sum(np.zeros((33, 64), np.float32))
