"""The float64 synthesiser model (tests/synth_model.py) on its own and against the NumPy generators.

The model is what tests/test_gpu_synth.py holds the HIP kernels to, so it is pinned here from the other side: its hash to the
published splitmix64 vector, its noise to the moments of N(0, sigma^2), and its signal part to synth.generate_if /
generate_if_mix (float64 as well, written independently, bits drawn from default_rng and handed to the model through bits=)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_model as M  # noqa: E402

FS = 18e6
SIGMA = 20.0


def test_splitmix64_is_the_published_function():
    assert int(M.splitmix64(0)[0]) == 0xE220A8397B1DCDAF
    # the next outputs of the published generator seeded with 0 (state advances by the golden-ratio constant)
    assert int(M.splitmix64(0x9E3779B97F4A7C15)[0]) == 0x6E789E6AA1B965F4
    assert int(M.splitmix64(np.uint64((2 * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)))[0]) == 0x06C45D188009454F


def test_noise_moments_over_four_million_samples():
    """Measured on the model: means 0.008 / -0.019, variance ratio 0.99975, corr(I,Q) -5e-4, lag-1 6e-4, fourth moment 0.9988,
    largest |value| 100.3: sigma = 20 never clips on noise alone.  The bounds are several times those values."""
    z = M.noise(np.arange(1 << 22, dtype=np.uint64), SIGMA, 4243)
    i, q = z.real, z.imag
    assert abs(i.mean()) < 0.05 and abs(q.mean()) < 0.05, (i.mean(), q.mean())
    var = 0.5 * (i.var() + q.var())
    assert abs(var / SIGMA ** 2 - 1.0) < 1e-3, var / SIGMA ** 2
    assert abs(np.mean(i * q) / SIGMA ** 2) < 2e-3
    both = np.concatenate([i, q])
    lag1 = 0.5 * (np.mean(i[1:] * i[:-1]) + np.mean(q[1:] * q[:-1])) / SIGMA ** 2
    assert abs(lag1) < 2e-3, lag1
    assert abs(np.mean(both ** 4) / (3 * SIGMA ** 4) - 1.0) < 5e-3, np.mean(both ** 4) / (3 * SIGMA ** 4)
    assert np.abs(both).max() < 127, np.abs(both).max()


def test_data_bits_differ_by_version_position_and_prn():
    b = np.arange(-64, 64)
    v1 = M.data_bits(9, 5, 0, b, 1)
    assert set(np.unique(v1)) == {-1.0, 1.0}
    assert np.array_equal(v1, M.data_bits(9, 5, 3, b, 1))            # version 1 does not see the position
    assert np.array_equal(v1, M.data_bits(9, 5, 0, b, 2))            # position 0 xors nothing
    assert not np.array_equal(M.data_bits(9, 5, 0, b, 2), M.data_bits(9, 5, 1, b, 2))
    assert not np.array_equal(v1, M.data_bits(9, 6, 0, b, 1))


def _amp(cn0):
    return SIGMA * np.sqrt(2.0 * 10 ** (cn0 / 10.0) / FS)


def _rng_bits(rng, n_samples, code_rate, code_len, bit_periods):
    return rng.integers(0, 2, size=int(n_samples / FS * code_rate / code_len / bit_periods) + 8) * 2.0 - 1.0


def _exact_outside_half_band(rec, m):
    """Both sides are float64: nothing but a value within 1e-9 of a half-integer may round differently."""
    mism, _, _ = M.compare(rec, m, chip_band=False, cap_share=False)
    assert np.count_nonzero(m.near_half) <= 2 and mism <= 2
    return mism


def _l1_sats(P):
    S = P.synth.SatSpec
    # the last one starts its reference code period beyond the record: negative chips, periods and bit indices throughout
    return [S(3, 1234.5, 777.25, 0.3, 68.0), S(11, -3210.0, 17999.75, -1.1, 64.0), S(22, 402.0, 25000.5, 7.0, 70.0)]


def _model_sats(P, sats, code_fn, code_rate, code_len, bit_periods, f_if, pilot_fn=None, pilot_phase=0.0, carrier_ratio=1540.0):
    return [M.ModelSat(prn=s.prn, code=code_fn(s.prn), doppler=s.doppler, code_phase_samples=s.code_phase_samples,
                       carrier_phase=s.carrier_phase, amplitude=_amp(s.cn0_dbhz),
                       code_rate=code_rate + s.doppler / carrier_ratio * (code_rate / 1.023e6), intermediate_freq=f_if,
                       bit_periods=bit_periods, pilot=pilot_fn(s.prn) if pilot_fn else None, pilot_phase=pilot_phase) for s in sats]


@pytest.mark.parametrize("bit_periods", [20, 1])
def test_generate_if_l1ca_with_a_code_start_beyond_the_record(bit_periods):
    import cu_sdr_collection_amd as P
    n, seed = 20000, 31
    sats = _l1_sats(P)
    rec = P.synth.generate_if(sats, n, FS, 20e3, P.codes.generateCAcode, 1.023e6, 1023, seed=seed, sigma=SIGMA,
                              bit_periods=bit_periods, chunk=6000, noise=False)
    rng = np.random.default_rng(seed)
    tables = [_rng_bits(rng, n, 1.023e6, 1023, bit_periods) for _ in sats]
    ms = _model_sats(P, sats, P.codes.generateCAcode, 1.023e6, 1023, bit_periods, 20e3)
    m = M.evaluate(ms, np.arange(n), FS, SIGMA, seed, version=1, bits=lambda s, b: tables[s][np.mod(b, tables[s].shape[0])],
                   delta=1e-9, with_noise=False)
    _exact_outside_half_band(rec, m)
    assert np.abs(rec).max() > 30                                   # three strong satellites, not a record of zeros
    cp = (np.arange(n) - sats[2].code_phase_samples) * (ms[2].code_rate / FS)
    assert cp.max() < 0 and np.floor(cp.min() / 1023) < -1          # the third satellite lives in negative periods only


def test_generate_if_e1_with_its_pilot_in_phase():
    import cu_sdr_collection_amd as P
    n, seed = 12000, 32
    S = P.synth.SatSpec
    sats = [S(4, 900.0, 100.5, 1.0, 66.0), S(19, -2500.0, 15000.25, 4.0, 69.0)]
    rec = P.synth.generate_if(sats, n, FS, 20e3, P.codes.generateE1Bcode, 2.046e6, 8184, seed=seed, sigma=SIGMA, bit_periods=1,
                              chunk=5000, noise=False, pilot_fn=P.codes.generateE1Ccode)
    rng = np.random.default_rng(seed)
    tables = [_rng_bits(rng, n, 2.046e6, 8184, 1) for _ in sats]
    ms = _model_sats(P, sats, P.codes.generateE1Bcode, 2.046e6, 8184, 1, 20e3, pilot_fn=P.codes.generateE1Ccode)
    m = M.evaluate(ms, np.arange(n), FS, SIGMA, seed, version=1, bits=lambda s, b: tables[s][np.mod(b, tables[s].shape[0])],
                   delta=1e-9, with_noise=False)
    _exact_outside_half_band(rec, m)


def test_generate_if_mix_three_families_one_with_its_own_if():
    """L1 C/A, E1 (pilot at 0) and L5 (pilot at +pi/2, its own intermediate frequency and carrier ratio) in one record."""
    import cu_sdr_collection_amd as P
    n, seed = 16000, 33
    S, G = P.synth.SatSpec, P.synth.SignalGroup
    e1 = [S(4, 900.0, 100.5, 1.0, 66.0), S(19, -2500.0, 15000.25, 4.0, 69.0)]
    l5 = [S(7, -1800.0, 9000.75, 2.5, 67.0), S(3, 2600.0, 16500.5, -0.4, 65.0)]
    groups = [G(_l1_sats(P), P.codes.generateCAcode, 1.023e6, 1023),
              G(e1, P.codes.generateE1Bcode, 2.046e6, 8184, bit_periods=1, pilot_fn=P.codes.generateE1Ccode),
              G(l5, P.codes.generateL5Icode, 10.23e6, 10230, bit_periods=10, pilot_fn=P.codes.generateL5Qcode,
                pilot_phase=np.pi / 2, carrier_ratio=115.0, intermediate_freq=-1.5e6)]
    rec = P.synth.generate_if_mix(groups, n, FS, 20e3, seed=seed, sigma=SIGMA, chunk=7000, noise=False)
    rng = np.random.default_rng(seed)
    ms, tables = [], []
    for g in groups:                                                # bits are drawn group by group, satellite by satellite
        f_if = 20e3 if g.intermediate_freq is None else g.intermediate_freq
        ms += _model_sats(P, g.sats, g.code_fn, g.code_rate, g.code_len, g.bit_periods, f_if, g.pilot_fn, g.pilot_phase, g.carrier_ratio)
        tables += [_rng_bits(rng, n, g.code_rate, g.code_len, g.bit_periods) for _ in g.sats]
    m = M.evaluate(ms, np.arange(n), FS, SIGMA, seed, version=2, bits=lambda s, b: tables[s][np.mod(b, tables[s].shape[0])],
                   delta=1e-9, with_noise=False)
    _exact_outside_half_band(rec, m)
    # the pilot at +90 degrees is visible: with it at -90 the record differs in thousands of samples
    flipped = [M.ModelSat(**{**s.__dict__, "pilot_phase": -s.pilot_phase}) for s in ms]
    other = M.evaluate(flipped, np.arange(n), FS, SIGMA, seed, version=2, bits=lambda s, b: tables[s][np.mod(b, tables[s].shape[0])],
                       delta=1e-9, with_noise=False)
    assert np.count_nonzero(other.rounded != rec) > n // 10


def test_masks_and_neighbouring_chips():
    """near_chip marks exactly the samples within the band of a chip edge and offers the neighbouring chip there."""
    code = np.array([1, -1, -1, 1, 1, 1, -1], dtype=np.int8)
    # one chip per 4 samples, code start on sample 0: every fourth sample sits exactly on an edge
    st = M.ModelSat(prn=1, code=code, doppler=0.0, code_phase_samples=0.0, carrier_phase=0.0, amplitude=10.3, code_rate=FS / 4,
                    bit_periods=1000000)
    m = M.evaluate([st], np.arange(64), FS, 0.0, 1, version=1)
    assert np.array_equal(np.nonzero(m.near_chip)[0], np.arange(0, 64, 4))
    lo, base = m.alts[0], m.rounded
    d = M.data_bits(1, 1, 0, np.array([0]), 1)[0]
    for p in range(4, 64, 4):
        assert lo[2 * p] == base[2 * (p - 1)] and base[2 * p] == int(np.rint(d * 10.3 * code[(p // 4) % 7]))
    assert np.array_equal(m.alts[1], base)                          # floor(cp + band) is the chip the model chose
    # near_half: 10.3 is not near a half-integer, 10.5 is, and a clipped value never is
    assert not m.near_half.any()
    st.amplitude = 10.5
    assert M.evaluate([st], np.arange(8), FS, 0.0, 1, version=1).near_half.all()
    st.amplitude = 200.5
    assert not M.evaluate([st], np.arange(8), FS, 0.0, 1, version=1).near_half.any()
    assert M.evaluate([st], np.arange(8), FS, 0.0, 1, version=2, limit=32767).near_half.all()
