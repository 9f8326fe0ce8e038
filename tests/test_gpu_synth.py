"""The GPU record synthesiser (csrc/synth.hip: synth_kernel behind gs_generate, synth2_kernel behind gs_generate2) sample for sample
against the float64 model of tests/synth_model.py.

A record is a pure function of (seed, sample index), so the model predicts every int8 / int16 value the kernels write, except
where float32 arithmetic may land on the other side of a rounding or chip edge.  Those places are bounded in advance
(synth_model.DELTA_F32 = 2^-8 around half-integers, synth_model.CHIP_BAND around chip edges) and may cover 2.5 % of a case at
most; everywhere else the record equals the model, and nowhere is it more than 1 LSB away (synth_model.compare).

The C entry points are called through ctypes with struct declarations of this file's own (from the comments in synth.hip), on
the session engine's buffer; the wrappers synth.generate_if_gpu / generate_if_mix_gpu where they are what is under test.  Every
comparison prints one line `synth-band <case>: ...` with the number of samples that differ from the model's first choice, their
largest distance from a half-integer and the banded share (pytest -s shows them).

Measured on an MI355X when these tests were written: banded share 1.1 - 1.9 % in every case; samples inside the half-integer
band that rounded the other way: 2 and 1 (int8 clipping, versions 1 and 2), 1 (generate_if_gpu), 1 and 1 (generate_if_mix_gpu,
int8 and int16), 0 in every other case, the windows of the 2.16 GB record included; none further than 4.3e-6 from a half-integer,
three orders of magnitude inside the band.  Mutants of synth.hip that these tests catch: the pilot's imaginary part negated, the
floor of the bit index for negative periods removed, the Q,I flag ignored for int16."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth_model as M  # noqa: E402

FS = 18e6
PAD = 64                      # samples behind the record that must keep their sentinel


class gs_sat(C.Structure):
    _fields_ = [("prn", C.c_int32), ("code_index", C.c_int32), ("doppler", C.c_double), ("code_phase_samples", C.c_double),
                ("carrier_phase", C.c_double), ("amplitude", C.c_double), ("code_rate", C.c_double)]


class gs_sat2(C.Structure):
    _fields_ = [("prn", C.c_int32), ("code_len", C.c_int32), ("code_offset", C.c_int32), ("pilot_offset", C.c_int32),
                ("bit_periods", C.c_int32), ("reserved", C.c_int32), ("doppler", C.c_double), ("code_phase_samples", C.c_double),
                ("carrier_phase", C.c_double), ("amplitude", C.c_double), ("code_rate", C.c_double), ("pilot_phase", C.c_double),
                ("intermediate_freq", C.c_double)]


@pytest.fixture(scope="module")
def lib():
    import cu_sdr_collection_amd as P
    path = os.path.join(os.path.dirname(os.path.abspath(P.synth.__file__)), "lib", "libgnsssynth.so")
    so = C.CDLL(path)
    so.gs_generate.restype = C.c_int
    so.gs_generate.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_int,
                               C.c_void_p, C.c_int, C.c_double, C.c_uint64]
    so.gs_generate2.restype = C.c_int
    so.gs_generate2.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int,
                                C.c_double, C.c_uint64, C.c_int]
    assert so.gs_version() == 2
    return so


def _sentinel(count, dt):
    k = np.arange(count, dtype=np.int64)
    if dt == np.int8:
        return ((k * 37 + 11) % 251 - 125).astype(np.int8)
    return ((k * 9973 + 5) % 60001 - 30000).astype(np.int16)


def _args1(sats, nsat=None):
    """gs_generate's arguments for ModelSats that share code length, bit length and intermediate frequency."""
    code_len = sats[0].code.shape[0] if sats else 1
    assert all(s.code.shape[0] == code_len and s.bit_periods == sats[0].bit_periods and
               s.intermediate_freq == sats[0].intermediate_freq and s.pilot is None for s in sats)
    codes = np.ascontiguousarray(np.stack([np.asarray(s.code, dtype=np.int8) for s in sats])) if sats else np.ones((1, 1), np.int8)
    arr = (gs_sat * max(1, len(sats)))()
    for i, s in enumerate(sats):
        arr[i] = gs_sat(s.prn, i, s.doppler, s.code_phase_samples, s.carrier_phase, s.amplitude, s.code_rate)
    return dict(f_if=sats[0].intermediate_freq if sats else 0.0, codes=codes, ncodes=codes.shape[0], code_len=code_len,
                bit_periods=sats[0].bit_periods if sats else 1, arr=arr, nsat=len(sats) if nsat is None else nsat)


def _args2(sats):
    flat, off = [], 0
    arr = (gs_sat2 * max(1, len(sats)))()
    for i, s in enumerate(sats):
        n = s.code.shape[0]
        e = gs_sat2(prn=s.prn, code_len=n, code_offset=off, pilot_offset=-1, bit_periods=s.bit_periods, reserved=0,
                    doppler=s.doppler, code_phase_samples=s.code_phase_samples, carrier_phase=s.carrier_phase,
                    amplitude=s.amplitude, code_rate=s.code_rate, pilot_phase=s.pilot_phase, intermediate_freq=s.intermediate_freq)
        flat.append(np.asarray(s.code, dtype=np.int8))
        off += n
        if s.pilot is not None:
            flat.append(np.asarray(s.pilot, dtype=np.int8))
            e.pilot_offset = off
            off += n
        arr[i] = e
    codes = np.ascontiguousarray(np.concatenate(flat)) if flat else np.ones(1, np.int8)
    return dict(codes=codes, arr=arr, nsat=len(sats))


def _call1(lib, engine, ptr, n, fs, a, sigma, seed):
    return lib.gs_generate(C.c_void_p(ptr), n, engine.device_id, fs, a["f_if"], a["codes"].ctypes.data_as(C.c_void_p), a["ncodes"],
                           a["code_len"], a["bit_periods"], a["arr"], a["nsat"], sigma, seed)


def _call2(lib, engine, ptr, n, fs, a, sigma, seed, flags, codes_bytes=None):
    return lib.gs_generate2(C.c_void_p(ptr), n, engine.device_id, fs, a["codes"].ctypes.data_as(C.c_void_p),
                            a["codes"].shape[0] if codes_bytes is None else codes_bytes, a["arr"], a["nsat"], sigma, seed, flags)


def _prepare(engine, n, dt, qi=False):
    """The engine's buffer: n + PAD samples of sentinel.  Returns (device pointer, the sentinel)."""
    from cu_sdr_collection_amd import _lib as L
    sent = _sentinel(2 * (n + PAD), dt)
    engine.load_if(sent, layout=L.GC_QI if qi else L.GC_IQ)
    engine.synchronize()
    ptr, have = engine.if_buffer()
    assert have == n + PAD and ptr % 16 == 0
    return ptr, sent


def _generate(lib, engine, sats, n, fs, sigma, seed, version, i16=False, qi=False):
    """Runs one entry point on a sentinel-filled buffer; returns the record's 2n components.  The PAD samples behind it must be
    untouched."""
    dt = np.int16 if i16 else np.int8
    assert version == 2 or not (i16 or qi)
    ptr, sent = _prepare(engine, n, dt, qi)
    if version == 1:
        rc = _call1(lib, engine, ptr, n, fs, _args1(sats), sigma, seed)
    else:
        rc = _call2(lib, engine, ptr, n, fs, _args2(sats), sigma, seed, int(i16) | (2 if qi else 0))
    assert rc == 0, rc
    got = engine.read_if(0, n + PAD, dtype=dt)
    assert np.array_equal(got[2 * n:], sent[2 * n:]), "the kernel wrote behind the record"
    return got[:2 * n]


def _hold(label, rec, m, cap_share=True):
    """The one comparison every case goes through: synth_model.compare, and a line for the log."""
    mism, dist, share = M.compare(rec, m, cap_share=cap_share)
    print(f"synth-band {label}: {rec.shape[0] // 2} samples, {mism} differ from the model's first choice, "
          f"largest distance from a half-integer {dist:.3e}, banded share {share:.5f}")
    return mism, dist, share


def _check(lib, engine, label, sats, n, fs, sigma, seed, version, i16=False, qi=False, cap_share=True):
    rec = _generate(lib, engine, sats, n, fs, sigma, seed, version, i16, qi)
    m = M.evaluate(sats, np.arange(n), fs, sigma, seed, version=version, limit=32767 if i16 else 127, qi=qi)
    stats = _hold(label, rec, m, cap_share)
    return rec, m, stats


def _short_code(seed, n=31):
    return (np.random.default_rng(seed).integers(0, 2, size=n) * 2 - 1).astype(np.int8)


def _l1(P, prn, doppler, cps, phase, amp, f_if=20e3, bit_periods=20):
    return M.ModelSat(prn=prn, code=P.codes.generateCAcode(prn).astype(np.int8), doppler=doppler, code_phase_samples=cps,
                      carrier_phase=phase, amplitude=amp, code_rate=1.023e6 * (1 + doppler / 1575.42e6), intermediate_freq=f_if,
                      bit_periods=bit_periods)


VARIANTS = [(1, False), (2, False), (2, True)]
VARIANT_IDS = ["v1-int8", "v2-int8", "v2-int16"]


# ---- 1. tails and overrun ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version,i16", VARIANTS, ids=VARIANT_IDS)
def test_partial_last_chunk_is_written_and_nothing_behind_it(lib, engine, version, i16):
    """Records of 1, 7, 8, 9, 2047 and 2053 samples (chunks of 8: empty tail, 7 of 8, 5 of 8) inside a longer buffer."""
    import cu_sdr_collection_amd as P
    sat = _l1(P, 7, 2345.0, 3.25, 0.7, 30.37)
    banded = total = 0
    for n in (1, 7, 8, 9, 2047, 2053):
        rec, m, _ = _check(lib, engine, f"tails {VARIANT_IDS[VARIANTS.index((version, i16))]} n={n}", [sat], n, FS, 20.0, 91, version,
                           i16, cap_share=False)
        banded += int(np.count_nonzero(m.near_half | m.near_chip))
        total += n
    assert banded <= M.BAND_SHARE_CAP * total, (banded, total)          # the cap holds over the case: its records are too short


# ---- 2. noise only -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version,i16", VARIANTS, ids=VARIANT_IDS)
def test_noise_alone_follows_the_model_and_its_moments(lib, engine, version, i16):
    """No satellite, sigma = 20, 2^16 samples.  The moment bounds are those of tests/test_synth_model_cpu.py, set there for 2^22
    samples; every one of them bounds an average whose spread goes with 1 / sqrt(samples), so they are 8 times wider here
    (sqrt(2^22 / 2^16) = 8).  Rounding to integers adds 1/12 to the variance: 2e-4 of sigma^2, far inside its bound."""
    n, sigma, seed = 1 << 16, 20.0, 4243
    rec, m, _ = _check(lib, engine, f"noise {VARIANT_IDS[VARIANTS.index((version, i16))]}", [], n, FS, sigma, seed, version, i16)
    i, q = rec[0::2].astype(np.float64), rec[1::2].astype(np.float64)
    both = np.concatenate([i, q])
    assert abs(i.mean()) < 8 * 0.05 and abs(q.mean()) < 8 * 0.05, (i.mean(), q.mean())
    assert abs(0.5 * (i.var() + q.var()) / sigma ** 2 - 1.0) < 8 * 1e-3
    assert abs(np.mean(i * q) / sigma ** 2) < 8 * 2e-3
    assert abs(0.5 * (np.mean(i[1:] * i[:-1]) + np.mean(q[1:] * q[:-1])) / sigma ** 2) < 8 * 2e-3
    assert abs(np.mean(both ** 4) / (3 * sigma ** 4) - 1.0) < 8 * 5e-3
    assert np.abs(both).max() < 127
    # a record is a function of (seed, sample index) alone
    again = _generate(lib, engine, [], n, FS, sigma, seed, version, i16)
    assert again.tobytes() == rec.tobytes()
    other = _generate(lib, engine, [], n, FS, sigma, seed + 1, version, i16)
    assert np.count_nonzero(other != rec) > n
    long = _generate(lib, engine, [], 8192, FS, sigma, seed, version, i16)
    short = _generate(lib, engine, [], 4096, FS, sigma, seed, version, i16)
    assert np.array_equal(short, long[:2 * 4096]) and np.array_equal(long, rec[:2 * 8192])


# ---- 3. code phase and data bits, noise off ----------------------------------------------------------------------------
@pytest.mark.parametrize("code_phase", [1234.567, 40000.25], ids=["start-inside", "start-beyond"])
@pytest.mark.parametrize("bit_periods", [1, 20])
@pytest.mark.parametrize("version", [1, 2])
def test_code_phase_and_data_bits_without_noise(lib, engine, version, bit_periods, code_phase):
    """A 31-chip code at 8.9 Mchip/s: 2^15 samples hold 520 periods.  With the code start beyond the record every chip, period and
    bit index is negative."""
    n, seed, amp = 1 << 15, 77, 40.37
    code = _short_code(5)
    sat = M.ModelSat(prn=13, code=code, doppler=-1500.0, code_phase_samples=code_phase, carrier_phase=1.1, amplitude=amp,
                     code_rate=8.9e6 + 3.7, intermediate_freq=20e3, bit_periods=bit_periods)
    rec, m, _ = _check(lib, engine, f"bits v{version} bit_periods={bit_periods} start={code_phase}", [sat], n, FS, 0.0, seed, version)
    # the data bit read off the record itself: the sign of the sample rotated back by the carrier, times the chip
    nn = np.arange(n, dtype=np.float64)
    cp = (nn - code_phase) * (sat.code_rate / FS)
    chip = np.floor(cp).astype(np.int64)
    period = np.floor_divide(chip, 31)
    theta = 2 * np.pi * (nn * ((sat.intermediate_freq + sat.doppler) / FS)) + sat.carrier_phase
    proj = rec[0::2] * np.cos(theta) + rec[1::2] * np.sin(theta)
    assert np.abs(proj).min() > amp - 1.5
    data = np.sign(proj) * code[np.mod(chip, 31)]
    keep = ~m.near_chip
    data, period = data[keep], period[keep]
    assert set(np.unique(data)) == {-1.0, 1.0}                       # both bit values occur
    flips = np.nonzero(np.diff(data) != 0)[0]
    assert flips.size > 5
    assert np.all(period[flips + 1] != period[flips]) and np.all(np.mod(period[flips + 1], bit_periods) == 0)
    if code_phase > n:
        assert period.max() < 0 and np.floor_divide(period, bit_periods).min() < -20 // bit_periods


# ---- 4. code rate above the sampling rate ------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
def test_more_than_one_chip_per_sample(lib, engine, version):
    import cu_sdr_collection_amd as P
    fs = 5e6
    sats = [M.ModelSat(prn=6, code=P.codes.generateL5Icode(6).astype(np.int8), doppler=1200.0, code_phase_samples=811.3,
                       carrier_phase=0.4, amplitude=30.37, code_rate=10.23e6 * (1 + 1200.0 / 1176.45e6), intermediate_freq=-0.4e6,
                       bit_periods=10),
            M.ModelSat(prn=9, code=P.codes.generateL5Icode(9).astype(np.int8), doppler=-2200.0, code_phase_samples=20000.6,
                       carrier_phase=2.4, amplitude=22.81, code_rate=3 * 10.23e6 + 0.77, intermediate_freq=-0.4e6, bit_periods=10)]
    _check(lib, engine, f"fast-code v{version}", sats, 1 << 14, fs, 20.0, 5, version)


# ---- 5. carrier --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
def test_carrier_frequency_and_phase_out_of_the_usual_range(lib, engine, version):
    """IF + Doppler negative, beyond +fs/2 and beyond -fs/2; carrier phase negative and above 2 pi.  Noise off."""
    import cu_sdr_collection_amd as P
    f_if = -1.2e6
    sats = [_l1(P, 2, -34567.8, 100.5, -2.5, 30.37, f_if), _l1(P, 5, 12.9e6, 7000.25, 7.9, 25.21, f_if),
            _l1(P, 8, -11.1e6, 12345.75, 0.0, 35.13, f_if)]
    assert sats[1].intermediate_freq + sats[1].doppler > FS / 2 and sats[2].intermediate_freq + sats[2].doppler < -FS / 2
    rec, m, _ = _check(lib, engine, f"carrier v{version}", sats, 1 << 14, FS, 0.0, 6, version)
    assert np.abs(rec).max() > 60


# ---- 6. width and refusals ---------------------------------------------------------------------------------------------
def _sixty_four(P, count=64):
    rng = np.random.default_rng(64)
    return [_l1(P, 1 + k % 32, float(rng.uniform(-5e3, 5e3)), float(rng.uniform(0, 18000)), float(rng.uniform(0, 6.28)), 1.2)
            for k in range(count)]


@pytest.mark.parametrize("version", [1, 2])
def test_sixty_four_satellites(lib, engine, version):
    import cu_sdr_collection_amd as P
    _check(lib, engine, f"64-satellites v{version}", _sixty_four(P), 1 << 14, FS, 20.0, 8, version)


def test_refusals_leave_the_buffer_alone(lib, engine):
    import cu_sdr_collection_amd as P
    n = 2048
    ptr, sent = _prepare(engine, n, np.int8)
    one = [_l1(P, 3, 100.0, 5.5, 0.1, 30.37)]
    a1, a2 = _args1(one), _args2(one)
    assert _call1(lib, engine, ptr, n, FS, _args1(_sixty_four(P, 65)), 20.0, 1) == -1          # 65 satellites
    assert _call2(lib, engine, ptr, n, FS, _args2(_sixty_four(P, 65)), 20.0, 1, 0) == -1
    for bad in (ptr + 8, ptr + 1, 0):                                                        # misaligned, null
        assert _call1(lib, engine, bad, n, FS, a1, 20.0, 1) == -1
        assert _call2(lib, engine, bad, n, FS, a2, 20.0, 1, 0) == -1
    assert _call1(lib, engine, ptr, n, FS, dict(a1, nsat=-1), 20.0, 1) == -1
    for key in ("code_len", "bit_periods"):                                                  # the kernel divides by both
        for v in (0, -3):
            assert _call1(lib, engine, ptr, n, FS, dict(a1, **{key: v}), 20.0, 1) == -1
            b = _args2(one)
            setattr(b["arr"][0], key, v)
            assert _call2(lib, engine, ptr, n, FS, b, 20.0, 1, 0) == -1
    b = _args1(one)
    b["arr"][0].code_index = 1                                                               # a row `codes` does not have
    assert _call1(lib, engine, ptr, n, FS, b, 20.0, 1) == -1
    assert _call2(lib, engine, ptr, n, FS, a2, 20.0, 1, 0, codes_bytes=1022) == -1             # chips beyond codes_bytes
    b = _args2(one)
    b["arr"][0].code_offset = 1
    assert _call2(lib, engine, ptr, n, FS, b, 20.0, 1, 0) == -1
    b["arr"][0].code_offset = -1
    assert _call2(lib, engine, ptr, n, FS, b, 20.0, 1, 0) == -1
    b = _args2(one)
    b["arr"][0].pilot_offset = 1                                                             # pilot chips beyond codes_bytes
    assert _call2(lib, engine, ptr, n, FS, b, 20.0, 1, 0) == -1
    engine.synchronize()
    assert np.array_equal(engine.read_if(0, n + PAD), sent)
    assert _call1(lib, engine, ptr, n, FS, a1, 20.0, 1) == 0 and _call2(lib, engine, ptr, n, FS, a2, 20.0, 1, 0) == 0   # the same arguments, intact


# ---- 7. clipping -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
def test_int8_clips_at_plus_minus_127(lib, engine, version):
    import cu_sdr_collection_amd as P
    sats = [_l1(P, 4, 2100.0, 300.5, 0.2, 90.3), _l1(P, 17, -3900.0, 9000.25, 1.9, 90.3)]
    rec, m, _ = _check(lib, engine, f"clip-int8 v{version}", sats, 1 << 14, FS, 20.0, 9, version)
    at_limit = (np.abs(rec[0::2]) == 127) | (np.abs(rec[1::2]) == 127)
    assert at_limit.mean() > 0.2, at_limit.mean()
    assert rec.max() == 127 and rec.min() == -127                      # never -128


def test_int16_clips_at_plus_minus_32767_and_keeps_what_int8_would_clip(lib, engine):
    """At amplitude 20 000 float32 is spaced 2^-9 apart and the carrier phase, rounded to float32, moves a sample by up to
    20 000 x 2 pi x 2^-25 = 4e-3: for a carrier in general position no half-integer band of 2^-8 can hold, whatever the kernel does.
    So the record that goes through the comparison has its two carriers at +-fs/4 with phase 0, where sine and cosine are 0 and
    +-1 and the kernel's float32 arithmetic is exact (the two satellites cancel to 0 or add up to +-40 000.74, on I for even and
    on Q for odd samples); a record with carriers in general position is held to 1 LSB and to its extremes."""
    import cu_sdr_collection_amd as P
    n = 1 << 14
    quarter = [_l1(P, 4, 0.0, 300.5, 0.0, 20000.37, FS / 4, bit_periods=1), _l1(P, 17, 0.0, 9000.25, 0.0, 20000.37, -FS / 4, bit_periods=1)]
    rec, m, _ = _check(lib, engine, "clip-int16 quarter-turn carriers", quarter, n, FS, 20.0, 10, 2, i16=True)
    assert rec.max() == 32767 and rec.min() == -32767
    assert np.count_nonzero(np.abs(rec) == 32767) > n // 4
    general = [_l1(P, 4, 2100.0, 300.5, 0.2, 20000.37), _l1(P, 17, -3900.0, 9000.25, 1.9, 20000.37)]
    rec = _generate(lib, engine, general, n, FS, 20.0, 10, 2, i16=True)
    want = M.evaluate(general, np.arange(n), FS, 20.0, 10, version=2, limit=32767).rounded
    assert np.abs(rec.astype(np.int64) - want).max() <= 1
    assert rec.max() == 32767 and rec.min() == -32767
    # amplitude 300: an int16 record keeps the values an int8 record would clip
    rec, m, _ = _check(lib, engine, "int16 amplitude 300", [_l1(P, 4, 2100.0, 300.5, 0.2, 300.3)], n, FS, 20.0, 11, 2, i16=True)
    assert np.count_nonzero(np.abs(rec) > 127) > n // 2 and np.abs(rec).max() > 300


# ---- 8. version 2 specifics --------------------------------------------------------------------------------------------
def _mixed_entries(P):
    """L1 C/A without pilot; E1 with its pilot in phase; L5 with its pilot at +90 degrees and an intermediate frequency of its
    own; two entries with the same PRN and the same short code, one bit per code period."""
    short = _short_code(9)
    return [_l1(P, 5, 1234.5, 777.25, 0.3, 12.31),
            M.ModelSat(prn=11, code=P.codes.generateE1Bcode(11).astype(np.int8), doppler=-2100.0, code_phase_samples=15000.25,
                       carrier_phase=4.0, amplitude=9.73, code_rate=2.046e6 * (1 - 2100.0 / 1575.42e6), intermediate_freq=20e3,
                       bit_periods=1, pilot=P.codes.generateE1Ccode(11).astype(np.int8), pilot_phase=0.0),
            M.ModelSat(prn=7, code=P.codes.generateL5Icode(7).astype(np.int8), doppler=-1800.0, code_phase_samples=9000.75,
                       carrier_phase=2.5, amplitude=8.17, code_rate=10.23e6 * (1 - 1800.0 / 1176.45e6), intermediate_freq=-1.5e6,
                       bit_periods=10, pilot=P.codes.generateL5Qcode(7).astype(np.int8), pilot_phase=np.pi / 2),
            M.ModelSat(prn=9, code=short, doppler=400.0, code_phase_samples=10.5, carrier_phase=1.0, amplitude=6.29,
                       code_rate=8.9e6, intermediate_freq=20e3, bit_periods=1),
            M.ModelSat(prn=9, code=short, doppler=-700.0, code_phase_samples=21.75, carrier_phase=5.0, amplitude=7.93,
                       code_rate=8.9e6, intermediate_freq=20e3, bit_periods=1)]


def test_version_2_entries_formats_and_sample_orders(lib, engine):
    import cu_sdr_collection_amd as P
    n, seed = 1 << 15, 12
    sats = _mixed_entries(P)
    b = np.arange(0, 500)
    assert not np.array_equal(M.data_bits(seed, 9, 3, b, 2), M.data_bits(seed, 9, 4, b, 2))   # what the record must show
    recs = {}
    for i16 in (False, True):
        for qi in (False, True):
            recs[i16, qi], _, _ = _check(lib, engine, f"mixed {'int16' if i16 else 'int8'} {'Q,I' if qi else 'I,Q'}", sats, n, FS,
                                         20.0, seed, 2, i16, qi)
        iq, qi_rec = recs[i16, False], recs[i16, True]
        assert qi_rec[0::2].tobytes() == iq[1::2].tobytes() and qi_rec[1::2].tobytes() == iq[0::2].tobytes()
    wide, narrow = recs[True, False], recs[False, False]
    assert np.array_equal(np.clip(wide, -127, 127), narrow)            # the formats differ in where they clip, nothing else


# ---- 9. the wrappers ---------------------------------------------------------------------------------------------------
def _amp(cn0, fs, sigma=20.0):
    return sigma * np.sqrt(2.0 * 10 ** (cn0 / 10.0) / fs)


def test_generate_if_gpu_on_a_twelve_satellite_scene(engine):
    import cu_sdr_collection_amd as P
    n, seed = 1 << 15, 21
    scene = P.synth.scene(12, 20241008 + 2, FS, cn0=58.0)
    P.synth.generate_if_gpu(engine, scene, n, FS, 20e3, P.codes.generateCAcode, 1.023e6, 1023, seed=seed)
    rec = engine.read_if(0, n)
    sats = [M.ModelSat(prn=s.prn, code=P.codes.generateCAcode(s.prn), doppler=s.doppler, code_phase_samples=s.code_phase_samples,
                       carrier_phase=s.carrier_phase, amplitude=_amp(58.0, FS), code_rate=1.023e6 + s.doppler / 1540.0,
                       intermediate_freq=20e3, bit_periods=20) for s in scene]
    _hold("wrapper generate_if_gpu", rec, M.evaluate(sats, np.arange(n), FS, 20.0, seed, version=1))


@pytest.mark.parametrize("i16,qi", [(False, False), (True, True)], ids=["int8-IQ", "int16-QI"])
def test_generate_if_mix_gpu_on_three_families(engine, i16, qi):
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import _lib as L
    n, seed = 1 << 15, 22
    S, G = P.synth.SatSpec, P.synth.SignalGroup
    groups = [G([S(5, 1234.5, 777.25, 0.3, 60.0), S(22, -3210.0, 17999.75, 5.1, 57.0)], P.codes.generateCAcode, 1.023e6, 1023),
              G([S(11, -2100.0, 15000.25, 4.0, 59.0)], P.codes.generateE1Bcode, 2.046e6, 8184, bit_periods=1,
                pilot_fn=P.codes.generateE1Ccode),
              G([S(7, -1800.0, 9000.75, 2.5, 58.0), S(5, 2600.0, 16500.5, 0.9, 61.0)], P.codes.generateL5Icode, 10.23e6, 10230,
                bit_periods=10, pilot_fn=P.codes.generateL5Qcode, pilot_phase=np.pi / 2, carrier_ratio=115.0, intermediate_freq=-1.5e6)]
    P.synth.generate_if_mix_gpu(engine, groups, n, FS, 20e3, seed, dtype=np.int16 if i16 else np.int8, qi_order=qi)
    assert engine.if_format() == (L.GC_I16 if i16 else L.GC_I8, L.GC_QI if qi else L.GC_IQ)
    rec = engine.read_if(0, n, dtype=np.int16 if i16 else np.int8)
    sats = []
    for g in groups:
        for s in g.sats:
            sats.append(M.ModelSat(prn=s.prn, code=g.code_fn(s.prn), doppler=s.doppler, code_phase_samples=s.code_phase_samples,
                                   carrier_phase=s.carrier_phase, amplitude=_amp(s.cn0_dbhz, FS),
                                   code_rate=g.code_rate + s.doppler / g.carrier_ratio * (g.code_rate / 1.023e6),
                                   intermediate_freq=20e3 if g.intermediate_freq is None else g.intermediate_freq,
                                   bit_periods=g.bit_periods, pilot=g.pilot_fn(s.prn) if g.pilot_fn else None, pilot_phase=g.pilot_phase))
    _hold(f"wrapper generate_if_mix_gpu {'int16 Q,I' if i16 else 'int8 I,Q'}", rec,
          M.evaluate(sats, np.arange(n), FS, 20.0, seed, version=2, limit=32767 if i16 else 127, qi=qi))


def test_attached_buffers_of_another_format_are_refused():
    """attached=True fills the buffer the engine already reads.  An int16 record written into an int8 buffer of as many samples
    would run over its end, an int8 record would fill half an int16 buffer: both wrappers look at the format first.  The memory
    here is sized for int16 under every attachment, so that nothing can leave it either way."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import _lib as L
    n = 4096
    S, G = P.synth.SatSpec, P.synth.SignalGroup
    scene = [S(5, 1234.5, 777.25, 0.3, 60.0)]
    groups = [G(scene, P.codes.generateCAcode, 1.023e6, 1023)]
    sent = _sentinel(2 * n, np.int16)
    owner, user = P.Engine(0), P.Engine(0)
    try:
        owner.load_if(sent)
        owner.synchronize()
        ptr, _ = owner.if_buffer()
        user.attach_if(ptr, n, np.int8, L.GC_IQ)
        with pytest.raises(ValueError, match="format"):
            P.synth.generate_if_mix_gpu(user, groups, n, FS, 20e3, 1, dtype=np.int16, attached=True)
        with pytest.raises(ValueError, match="format"):
            P.synth.generate_if_mix_gpu(user, groups, n, FS, 20e3, 1, dtype=np.int8, qi_order=True, attached=True)
        user.attach_if(ptr, n, np.int16, L.GC_IQ)
        with pytest.raises(ValueError, match="format"):
            P.synth.generate_if_gpu(user, scene, n, FS, 20e3, P.codes.generateCAcode, 1.023e6, 1023, seed=1, attached=True)
        with pytest.raises(ValueError, match="format"):
            P.synth.generate_if_mix_gpu(user, groups, n, FS, 20e3, 1, dtype=np.int8, attached=True)
        user.attach_if(ptr, n, np.int8, L.GC_QI)
        with pytest.raises(ValueError, match="format"):
            P.synth.generate_if_gpu(user, scene, n, FS, 20e3, P.codes.generateCAcode, 1.023e6, 1023, seed=1, attached=True)
        user.synchronize()
        assert np.array_equal(owner.read_if(0, n, dtype=np.int16), sent)
        # the matching format is filled, with the record the allocating call makes
        user.attach_if(ptr, n, np.int8, L.GC_IQ)
        P.synth.generate_if_gpu(user, scene, n, FS, 20e3, P.codes.generateCAcode, 1.023e6, 1023, seed=1, attached=True)
        filled = user.read_if(0, n)
        assert np.array_equal(owner.read_if(0, n, dtype=np.int16)[n:], sent[n:])             # int8: the first half of the memory
        user.attach_if(ptr, n, np.int16, L.GC_IQ)
        P.synth.generate_if_mix_gpu(user, groups, n, FS, 20e3, 1, dtype=np.int16, attached=True)
        mixed = user.read_if(0, n, dtype=np.int16)
        sat = M.ModelSat(prn=5, code=P.codes.generateCAcode(5), doppler=1234.5, code_phase_samples=777.25, carrier_phase=0.3,
                         amplitude=_amp(60.0, FS), code_rate=1.023e6 + 1234.5 / 1540.0, intermediate_freq=20e3, bit_periods=20)
        _hold("attached int8", filled, M.evaluate([sat], np.arange(n), FS, 20.0, 1, version=1))
        _hold("attached int16", mixed, M.evaluate([sat], np.arange(n), FS, 20.0, 1, version=2, limit=32767))
    finally:
        user.close()
        owner.close()


# ---- 10. deep in the headline's record ---------------------------------------------------------------------------------
def test_the_benchmark_record_at_its_start_middle_and_end(engine):
    """bench.py's own record: 12 x GPS L1 C/A, 60 s at 18 Msps, 2.16 GB.  The products n x (carrier turns per sample) and
    (n - code phase) x (chips per sample) only grow with n, so this is the one case that cannot be made small: windows of 4096
    samples at the start, from an index that is no multiple of 8 near the middle, and at the very end."""
    import cu_sdr_collection_amd as P
    S = P.initSettings()
    fs, seed = 18e6, 20241008 + 2
    n = int(60 * fs)
    scene = P.synth.scene(12, seed, fs)
    try:
        P.synth.generate_if_gpu(engine, scene, n, fs, S.IF, P.codes.generateCAcode, S.codeFreqBasis, 1023, seed=seed)
        sats = [M.ModelSat(prn=s.prn, code=P.codes.generateCAcode(s.prn), doppler=s.doppler, code_phase_samples=s.code_phase_samples,
                           carrier_phase=s.carrier_phase, amplitude=_amp(s.cn0_dbhz, fs),
                           code_rate=S.codeFreqBasis + s.doppler / 1540.0 * (S.codeFreqBasis / 1.023e6), intermediate_freq=S.IF,
                           bit_periods=20) for s in scene]
        for name, first in (("start", 0), ("middle", 540_000_003), ("end", n - 4096)):
            rec = engine.read_if(first, 4096)
            _hold(f"headline record {name} (from sample {first})", rec,
                  M.evaluate(sats, first + np.arange(4096), fs, 20.0, seed, version=1))
    finally:
        engine.load_if(np.zeros(64, dtype=np.int8))                    # give the 2.16 GB back
