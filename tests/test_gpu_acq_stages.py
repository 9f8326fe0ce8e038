"""The stages between a coarse peak and the returned carrFreq, each against a plain float64 restatement written here: the fine sums
cell by cell (gc_acquire_fine_sums, csrc/acq_fine.hip), GPS L1 C/A's fine pick (gc_acquire_fine_l1ca_batch), the front end sample by
sample (gc_acq_condition / gc_acq_signal_from_record, csrc/acq_cond.hip) and the signal statistics (gc_acq_signal_stats, the coarse
search's sigPower).  No GC_* knob is set: every path is reached in the shipped library through the shapes alone.

Every test prints the worst ratio error / bound it met (pytest -s shows them; DESIGN.md 4.4 records the measured ones).

Bound of a fine sum (u = 2^-24, the float32 unit roundoff; S = sum |x[n] - dc| over the cell's samples; r = |k mod 24 - 12| rotations
between bin k and the middle bin of its group of 24, whose carrier is the only one evaluated).  Per sample, as a complex error relative
to |x[n] - dc| (the code chip is -1, 0 or 1: its product is exact; the float64 phase product n*f/fs is exact to 1e-11):
  * x - dc rounds once per component:                                                                        1 u
  * the carrier's argument, 2 * frac(phase), is rounded to float32: at most 2^-24 half-turns = pi u radians:   pi u
  * sincospif is allowed 2 ulp = 4 u per component, sqrt(2) * 4 u as a vector:                              4 sqrt(2) u
  * re = cr*cs + cq*sn (and im): two products and a sum, |cr cs| + |cq sn| <= |x| by Cauchy-Schwarz, so each component is off by
    at most 2 u |x|, the pair by                                                                            2 sqrt(2) u
  a = 1 + pi + 6 sqrt(2) = 12.6 -> 13.  Per rotation w <- w * exp(-+i d):
  * exp(i d) comes from a second sincospif: argument rounding pi u + evaluation 4 sqrt(2) u = 8.8 u, the SAME error in every one of
    the r rotations, so it adds linearly;
  * the complex product's three float32 roundings per component (two products, one sum), 2 u each, 2 sqrt(2) u as a vector
  b = pi + 6 sqrt(2) = 11.6 -> 12.  The float64 accumulation (2^-53 per addition) and the reference's own error (1e-11) are far below
  one u.  |got - want| <= (13 + 12 r) u S; a wrong chip moves a cell by up to 2 * 181, ~1e2 .. 1e3 times this bound at these sizes."""
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FINE_A, FINE_B = 13.0, 12.0
N_REC = 60000                      # samples of the fine-sum records


def _lib():
    from cu_sdr_collection_amd import _lib as L
    return L


def _status(call):
    import cu_sdr_collection_amd as P
    with pytest.raises(P.GnssCorrError) as e:
        call()
    return e.value.status


# ---- 1. fine sums -----------------------------------------------------------------------------------------------------------------
def _code_index(n, off, fs, code_freq, code_len):
    """acquisition.m:215-218 as the reference evaluates it in float64; code_freq = 0: one replica entry per sample."""
    if code_freq > 0:
        ts, tc = 1.0 / fs, 1.0 / code_freq
        return np.remainder(np.floor(ts * (n + off) / tc), code_len).astype(np.int64)
    return (n + off) % code_len


def fine_parts(ncodes, ndet, nbins, spc, cus):
    """The launch-size rule of fine_sums_enqueue: workgroups per code period (runs summed by fine_parts_kernel when > 1)."""
    groups, parts = ncodes * ndet * ((nbins + 23) // 24), 1
    while parts < 8 and groups * parts < 4 * cus and spc // (2 * parts) >= 2048:
        parts *= 2
    return parts


@pytest.fixture(scope="module")
def fine_data():
    rng = np.random.default_rng(20250)
    rec = rng.integers(-128, 128, size=2 * N_REC, dtype=np.int64).astype(np.int8)        # full range, -128 included
    sig = ((rng.standard_normal(N_REC) + 1j * rng.standard_normal(N_REC)) * 50.0).astype(np.complex64)
    codes = {cl: np.stack([rng.choice(np.array([-1, 1], dtype=np.int8), size=cl),
                           rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=cl, p=[0.45, 0.1, 0.45])]) for cl in (777, 1023, 2046)}
    return {"rec": rec, "sig": sig, "codes": codes}


def _detections(fs):
    """Two detections: odd and even first sample, one carrier negative, one above fs / 2."""
    return [(1235, -21512.5), (4098, round(0.62 * fs) + 7.25)]


def _coherent_record(fs, code_freq, code_len, off, codes, first, f, n_total):
    """Amplitude-100 code x carrier exactly on a bin of detection 0, so that the kernel's rounding errors add up instead of averaging."""
    n = np.arange(n_total - first)
    z = 100.0 * codes[0][_code_index(n, off, fs, code_freq, code_len)] * np.exp(2j * np.pi * f * n / fs)
    x = np.zeros(n_total, dtype=np.complex128)
    x[first:] = z
    rec = np.empty(2 * n_total, dtype=np.int8)
    rec[0::2] = np.rint(x.real).astype(np.int8)
    rec[1::2] = np.rint(x.imag).astype(np.int8)
    return rec


def _check_fine(engine, data, kind, fs, code_freq, code_len, off, spc, ncodes, nbins, fstep, ndet, label):
    L = _lib()
    codes = data["codes"][code_len][:ndet] if ndet == 2 else data["codes"][code_len][1:2]
    dets = _detections(fs)[:ndet] if ndet == 2 else _detections(fs)[1:2]
    first = np.array([d[0] for d in dets], dtype=np.int64)
    f0 = np.array([d[1] for d in dets])
    if kind == "cond":
        engine.load_if(data["rec"], fs=fs)
        engine.acq_set_signal(data["sig"])
        x, source, dc = data["sig"].astype(np.complex128), 1, 0.375 - 2.5j
    else:
        if kind == "coherent":          # on bin min(nbins - 1, 17) of the first detection: an "above MID" bin where there is one
            rec = _coherent_record(fs, code_freq, code_len, off, codes, int(first[0]), f0[0] - fstep * min(nbins - 1, 17), N_REC)
        else:
            rec = data["rec"]
        engine.load_if(rec, fs=fs)
        x, source, dc = rec[0::2].astype(np.float64) + 1j * rec[1::2].astype(np.float64), 0, 3.25 - 1.5j
    fp = L.gc_fine_params(sampling_freq=fs, code_freq=code_freq, f0=0.0, fstep=fstep, first_sample=0, spc=spc, ncodes=ncodes, nbins=nbins,
                          code_len=code_len, index_offset=off, source=source, dc_re=dc.real, dc_im=dc.imag)
    got = engine.acquire_fine_sums_batch(fp, codes, first, f0)
    assert got.shape == (ndet, nbins, ncodes)
    n = np.arange(ncodes * spc)
    idx = _code_index(n, off, fs, code_freq, code_len)
    worst = np.zeros(13)
    for d in range(ndet):
        y = x[first[d]:first[d] + ncodes * spc] - dc
        S = np.abs(y).reshape(ncodes, spc).sum(axis=1)
        yc = y * codes[d][idx]
        for k in range(nbins):
            want = (yc * np.exp(-2j * np.pi * (f0[d] - k * fstep) * n / fs)).reshape(ncodes, spc).sum(axis=1)
            r = abs(k % 24 - 12)
            ratio = np.max(np.abs(got[d, k] - want) / (U * S))
            worst[r] = max(worst[r], ratio)
            assert ratio <= FINE_A + FINE_B * r, (label, d, k, r, ratio)
    print(f"FINE {label} worst |err| / (2^-24 S) per r: " + " ".join(f"{r}:{w:.3f}" for r, w in enumerate(worst) if w > 0))
    return idx


@pytest.mark.parametrize("kind", ["int8", "cond", "coherent"])
@pytest.mark.parametrize("nbins", [1, 12, 13, 23, 24, 25, 37, 48, 49])
def test_fine_sums_every_bin_of_every_group(engine, fine_data, nbins, kind):
    """nbins = 1 .. 12: the "below MID" arm only; 13: MID itself; 23 / 24: the "above MID" arm against its k < nb guard and a full group;
    25 / 37 / 48 / 49: a second and a third group (blockIdx.z > 0) whose last one holds nb = 1, 13, 24 and 1 bins.  Sampled-replica
    mode (code_freq = 0) with the index (n + 1) mod 777; one run per code period (spc = 1000)."""
    _check_fine(engine, fine_data, kind, 18e6, 0.0, 777, 1, 1000, 2, nbins, 25.0, 2, f"bins={nbins} {kind}")


SPLIT_SPC = [4095, 4096, 4097, 8191, 8193, 16383, 16385]


def _split_shape(spc, ncodes):
    """(ndet, nbins) of a period-split case: one detection with one code period, two with three; at most 24 bins."""
    return (1, 24) if ncodes == 1 else (2, 7)


def test_period_split_shapes_reach_every_run_count(engine):
    """fine_sums_enqueue cuts a code period into 1, 2, 4 or 8 runs (multiples of 256 samples, the last one short for 4097, 8193 and
    16385) by its launch-size rule; fine_parts() restates the rule with this device's compute units, so the claim is checked where the
    count differs from 256 too."""
    cus = engine.device_info()[1]
    parts = {(spc, nc): fine_parts(nc, _split_shape(spc, nc)[0], _split_shape(spc, nc)[1], spc, cus) for spc in SPLIT_SPC for nc in (1, 3)}
    print("FINE parts per (spc, ncodes):", parts, "on", cus, "compute units")
    assert set(parts.values()) == {1, 2, 4, 8}
    if cus == 256:
        assert [parts[(spc, 1)] for spc in SPLIT_SPC] == [1, 2, 2, 2, 4, 4, 8]


@pytest.mark.parametrize("kind", ["int8", "cond", "coherent"])
@pytest.mark.parametrize("ncodes", [1, 3])
@pytest.mark.parametrize("spc", SPLIT_SPC)
def test_fine_sums_with_the_code_period_cut_into_runs(engine, fine_data, spc, ncodes, kind):
    ndet, nbins = _split_shape(spc, ncodes)
    parts = fine_parts(ncodes, ndet, nbins, spc, engine.device_info()[1])
    _check_fine(engine, fine_data, kind, 18e6, 0.0, 777, 1, spc, ncodes, nbins, 333.25, ndet, f"spc={spc} ncodes={ncodes} parts={parts} {kind}")


@pytest.mark.parametrize("kind", ["int8", "cond"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("code_freq,code_len", [(1.023e6, 1023), (2.046e6, 2046)])
@pytest.mark.parametrize("fs", [4.092e6, 16.368e6, 18e6])
def test_fine_sums_code_index_is_the_references_float64_expression(engine, fine_data, fs, code_freq, code_len, off, kind):
    """tc > 0: floor(ts*(n + off)/tc) mod code_len in float64, two code periods (more than one table period).  Where the sampling rate
    is a whole multiple of the chipping rate (4.092 and 16.368 Msps) that expression differs from exact rational arithmetic at some
    samples - asserted, so that an index computed in integers would pick other chips there; at 18 Msps a chip edge falls on a
    sample only every 6 000 samples and the two agree over this range (checked in numpy), the case then covers the rate and the table."""
    spc = int(round(fs / 1000.0))
    idx = _check_fine(engine, fine_data, kind, fs, code_freq, code_len, off, spc, 2, 5, 25.0, 2, f"fs={fs:g} code={code_freq:g} off={off} {kind}")
    exact = np.array([((n + off) * int(code_freq)) // int(fs) % code_len for n in range(2 * spc)], dtype=np.int64)
    differ = int(np.count_nonzero(idx != exact))
    print(f"FINE index: float64 expression differs from exact integers at {differ} of {2 * spc} samples")
    if fs != 18e6:
        assert differ > 0


def test_fine_sums_argument_checks(engine, fine_data):
    """A negative index_offset is refused (GC_E_INVALID): fmod of a negative index is negative and would read in front of the code
    table - decided from the kernel's code, never launched.  The other refusals through their status codes."""
    L = _lib()
    fs, codes = 18e6, fine_data["codes"][777][:1]
    engine.load_if(fine_data["rec"], fs=fs)

    def call(source=0, first=0, off=1, code_freq=0.0):
        fp = L.gc_fine_params(sampling_freq=fs, code_freq=code_freq, f0=0.0, fstep=25.0, first_sample=0, spc=1000, ncodes=2, nbins=5,
                              code_len=777, index_offset=off, source=source, dc_re=0.0, dc_im=0.0)
        return engine.acquire_fine_sums_batch(fp, codes, np.array([first]), np.array([1000.0]))
    assert call().shape == (1, 5, 2)
    assert _status(lambda: call(off=-1)) == L.GC_E_INVALID
    assert _status(lambda: call(off=-1, code_freq=1.023e6)) == L.GC_E_INVALID
    assert _status(lambda: call(first=N_REC - 1999)) == L.GC_E_RANGE                 # one sample past the record
    assert call(first=N_REC - 2000).shape == (1, 5, 2)                               # the last window that fits
    assert _status(lambda: call(source=1)) == L.GC_E_STATE                           # no conditioned signal on this record yet
    engine.load_if(fine_data["rec"].astype(np.int16), fs=fs)
    assert _status(lambda: call()) == L.GC_E_UNSUPPORTED                             # source 0 reads int8 I/Q only


# ---- 2. GPS L1 C/A fine pick -------------------------------------------------------------------------------------------------------
def _l1ca_record(P, fs, step, dets, n_total, seed):
    """Three satellites in one int8 record: C/A code from the detection's code phase, a data-bit edge inside the 40 ms, the carrier
    exactly on fine bin `bin` of the detection's grid."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n_total) + 1j * rng.standard_normal(n_total)) * 8.0
    for prn, cp, coarse, fbin, edge_ms in dets:
        n = np.arange(n_total - (cp - 1))
        chips = P.codes.generateCAcode(prn).astype(np.float64)[_code_index(n, 0, fs, 1.023e6, 1023)]
        bit = np.where(n < edge_ms * 1e-3 * fs, 1.0, -1.0)
        f = coarse + step / 2 - 25.0 * fbin
        x[cp - 1:] += 25.0 * chips * bit * np.exp(2j * np.pi * f * n / fs)
    rec = np.empty(2 * n_total, dtype=np.int8)
    rec[0::2] = np.clip(np.rint(x.real), -127, 127)
    rec[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return rec


def _l1ca_pick_reference(x, fs, spc, step, code, cp, coarse):
    """acquisition.m:213-260 in float64: 40 per-code sums per fine bin, 20 bit-edge hypotheses, first maximum, 0 -> 1 Hz.  The bins'
    carriers follow from the first one by float64 rotations (81 of them lose 1e-14).  Returns (carrFreq, power per bin, bound per bin)."""
    nfine = int(math.floor(step / 25.0 + 0.5)) + 1
    n = np.arange(40 * spc)
    sig = x[cp - 1:cp - 1 + 40 * spc]
    f0 = coarse + step / 2
    y = sig * code[_code_index(n, 0, fs, 1.023e6, 1023)] * np.exp(-2j * np.pi * f0 * n / fs)
    rot = np.exp(2j * np.pi * 25.0 * n / fs)
    S = np.abs(sig).reshape(40, spc).sum(axis=1)
    power, bound = np.zeros(nfine), np.zeros(nfine)
    for k in range(nfine):
        per_code = y.reshape(40, spc).sum(axis=1)
        power[k] = max(abs(per_code[c0:c0 + 20].sum()) for c0 in range(20))
        r = abs(k % 24 - 12)
        bound[k] = (FINE_A + FINE_B * r) * U * max(S[c0:c0 + 20].sum() for c0 in range(20))
        y = y * rot
    best = int(np.argmax(power))                    # the first maximum
    f = f0 - 25.0 * best
    return (1.0 if f == 0 else f), power, bound, best


@pytest.mark.parametrize("step", [500.0, 2000.0])
@pytest.mark.parametrize("fs", [4.092e6, 18e6])
def test_l1ca_fine_pick_matches_the_float64_restatement(engine, fs, step):
    """Three detections in one call; search_step = 500: 21 bins, picked on the device (fine_l1ca_pick_kernel); 2000: 81 bins in four
    groups, picked by the host twin.  The expected bin is defined where the float64 winner leads every other bin by more than the two
    bins' part-1 bounds summed over 20 code periods - asserted on the reference first."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd.receiver import _acq_params
    S = P.initSettings()
    S.samplingFreq, S.acqSearchStep = fs, step
    spc = int(round(fs / 1000.0))
    nfine = int(step / 25) + 1
    # (PRN, code phase (1-based), coarse frequency, true fine bin, data-bit edge in ms): first / MID-side / last-group bins
    dets = [(3, 17, 20e3 + 1500.0, 2, 7.0), (11, spc // 2 + 4, 20e3 - 3000.0, nfine // 2 + 1, 13.5), (27, spc - 1, -4500.0, nfine - 2, 26.25)]
    n_total = 41 * spc + 8
    rec = _l1ca_record(P, fs, step, dets, n_total, seed=int(fs / 1000 + step))
    engine.load_if(rec, fs=fs)
    p = _acq_params(S, 0)
    codes = np.stack([P.codes.generateCAcode(d[0]) for d in dets]).astype(np.int8)
    got = engine.acquire_fine_l1ca_batch(p, codes, [d[1] for d in dets], [d[2] for d in dets])
    x = rec[0::2].astype(np.float64) + 1j * rec[1::2].astype(np.float64)
    for d, (prn, cp, coarse, fbin, _) in enumerate(dets):
        want, power, bound, best = _l1ca_pick_reference(x, fs, spc, step, codes[d].astype(np.float64), cp, coarse)
        others = np.delete(np.arange(nfine), best)
        margin = np.min((power[best] - power[others]) / (bound[best] + bound[others]))
        print(f"L1CA pick fs={fs:g} step={step:g} PRN {prn}: bin {best} (signal on {fbin}), margin / bound {margin:.3g}")
        assert margin > 1.0, (prn, best, margin)                                     # precondition: the winner is decided in float32 too
        assert best == fbin, (prn, best, fbin)
        assert got[d] == want, (prn, got[d], want)


@pytest.mark.parametrize("step", [500.0, 2000.0])
def test_l1ca_fine_pick_of_a_zero_record_is_the_first_bin_and_zero_becomes_one_hertz(engine, step):
    """Every bin's power is 0: max() returns the first one; with coarse_freq = -search_step / 2 that bin is exactly 0 Hz, which the
    reference replaces by 1 Hz (acquisition.m:258-260).  Device pick (21 bins) and host twin (81)."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd.receiver import _acq_params
    S = P.initSettings()
    S.samplingFreq, S.acqSearchStep = 4.092e6, step
    engine.load_if(np.zeros(2 * (41 * 4092), dtype=np.int8), fs=S.samplingFreq)
    codes = np.stack([P.codes.generateCAcode(q) for q in (1, 2, 3)]).astype(np.int8)
    got = engine.acquire_fine_l1ca_batch(_acq_params(S, 0), codes, [1, 100, 4092], [-step / 2, -step / 2, -step / 2 + 25.0])
    assert list(got) == [1.0, 1.0, 25.0]


# ---- 3. front end --------------------------------------------------------------------------------------------------------------------
BANDS = {  # name: (fs, IF, bandwidth, margin, Nyquist zone, new rate, new IF)
    "zone2": (38.192e6, 4.5e6, 2.546e6, 0.0, 2, 6113500.0, 4.5e6),
    "zone6": (53e6, 14.58e6, 2.546e6, 0.0, 6, 5303567.0, 3972866.0),
    "wide": (60e6, 15e6, 20.96e6, 0.002, 1, 50960000.0, 15e6),
    "zone1": (30e6, 6.5e6, 9e6, 0.002, 1, 22000000.0, 6.5e6),
}
FORMATS = {"i8_iq": (np.int8, "IQ"), "i8_qi": (np.int8, "QI"), "i8_real": (np.int8, "REAL"),
           "i16_iq": (np.int16, "IQ"), "i16_qi": (np.int16, "QI"), "i16_real": (np.int16, "REAL")}
N_FRONT = 48000


@pytest.fixture(scope="module")
def front_records():
    """One full-range record per format (the extremes of the type included) and its samples as complex128."""
    rng = np.random.default_rng(777)
    out = {}
    for name, (dt, lay) in FORMATS.items():
        info = np.iinfo(dt)
        comp = 1 if lay == "REAL" else 2
        raw = rng.integers(info.min, info.max + 1, size=comp * N_FRONT, dtype=np.int64)
        raw[:4 * comp] = [info.min, info.max] * (2 * comp)
        raw[-2 * comp:] = [info.max, info.min] * comp
        raw = raw.astype(dt)
        f = raw.astype(np.float64)
        x = f + 0j if lay == "REAL" else (f[0::2] + 1j * f[1::2] if lay == "IQ" else f[1::2] + 1j * f[0::2])
        out[name] = (raw, x)
    return out


def _load(engine, raw, lay, fs):
    L = _lib()
    engine.load_if(raw, layout={"IQ": L.GC_IQ, "QI": L.GC_QI, "REAL": L.GC_REAL}[lay], fs=fs)


def _front_reference(x, band, order):
    """acquisition.m:46-111 in float64: fir1 band-pass, filtfilt, band-pass-sampling rate, index selection, rem(IF, newFs).  Returns
    (signal, new rate, new IF, bound) with bound = 3 (order + 2) 2^-24 (sum |b|)^2 max |x_ext|:
    a pass is sum_k b32[k] v[k] as `order + 1` float32 FMAs with taps rounded to float32: per component at most (order + 2) u sum|b| max|v|
    (1 u for the taps, order + 1 for the chain, the final rounding in it).  The first pass leaves values up to sum|b| max|x_ext| carrying
    that error; the second multiplies the error by at most sum|b| and adds its own on inputs that large: 2 (order + 2) u (sum|b|)^2
    max|x_ext| per component, sqrt(2) times that for the complex sample: c = 2 sqrt(2) -> 3.  (The odd reflection 2 x(1) - x(k) is exact
    in float32 for int8 and int16; the float64 reference is right to 1e-13 of the same scale.)"""
    from scipy.signal import filtfilt, firwin
    fs, IF, bw, margin = band[:4]
    w1, w2 = (IF - bw / 2) * 2 / fs - margin, (IF + bw / 2) * 2 / fs + margin
    b = firwin(order + 1, [w1, w2], pass_zero=False)
    y = filtfilt(b, [1.0], x, padtype="odd", padlen=3 * order)
    fu, fl = IF + bw / 2, IF - bw / 2
    nz = max(1, int(math.floor(fu / bw)))
    lower = 2 * fu / nz
    upper = 2 * fl / (nz - 1) if nz > 1 else lower
    new_fs = float(math.ceil((lower + upper) / 2))
    length = int(math.floor((x.shape[0] - 1) / fs * new_fs))
    index = np.ceil(np.arange(length) / new_fs * fs).astype(np.int64)
    index[0] = 1
    ext = np.concatenate([2 * x[0] - x[3 * order:0:-1], x, 2 * x[-1] - x[-2:-3 * order - 2:-1]])
    bound = 3.0 * (order + 2) * U * np.sum(np.abs(b)) ** 2 * np.max(np.abs(ext))
    return y[index - 1], new_fs, math.fmod(IF, new_fs), bound, nz


def _check_front(engine, x, band, order, first, n, label):
    want, new_fs, new_if, bound, nz = _front_reference(x[first:first + n], band, order)
    got_fs, got_if, m = engine.acq_condition(band[0], band[1], band[2], first, n, fir_order=order, band_margin=band[3])
    assert (got_fs, got_if, m) == (new_fs, new_if, want.shape[0]), label
    assert m > 0
    got = engine.acq_conditioned(0, m)
    err = np.abs(got - want)
    print(f"FRONT {label}: {m} samples, worst |err| / bound {np.max(err) / bound:.4f} (first {err[0] / bound:.4f}, last {err[-1] / bound:.4f})")
    assert np.max(err) <= bound, (label, int(np.argmax(err)), float(np.max(err)), bound)
    return new_fs, new_if, nz


@pytest.mark.parametrize("first", [0, 1, 4097])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_front_end_reads_every_record_format(engine, front_records, fmt, first):
    """record_sample's six formats at three starts: gc_acq_signal_from_record bit-equal to the record as complex64, gc_acq_condition
    (order 254, the wide band) sample by sample."""
    L = _lib()
    raw, x = front_records[fmt]
    _load(engine, raw, FORMATS[fmt][1], BANDS["wide"][0])
    n = 5003
    assert engine._lib.gc_acq_signal_from_record(engine._ctx, first, n) == L.GC_OK
    got = engine.acq_conditioned(0, n)
    assert np.array_equal(got, x[first:first + n].astype(np.complex64)), fmt
    assert engine._lib.gc_acq_signal_from_record(engine._ctx, N_FRONT - n + 1, n) == L.GC_E_RANGE
    _check_front(engine, x, BANDS["wide"], 254, first, n, f"{fmt} first={first}")


def _front_lengths(order):
    """The minimal length 3*order + 1, and the lengths that put the extended signal's n + 6*order at 256 k - 1, 256 k, 256 k + 1 (the
    last tile of cond_fir_kernel one sample short, full, and a tile of one sample)."""
    lo = 3 * order + 1
    k = (lo + 6 * order) // 256 + 2
    return [lo] + [256 * k + d - 6 * order for d in (-1, 0, 1)]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("order", [2, 3, 254, 255, 256, 700, 4096])
def test_front_end_filter_orders_and_tile_edges(engine, front_records, order, which):
    """The wide band (decimation 60 -> 50.96 Msps keeps a few samples even of the shortest record: order 2 filters 7 samples into 5)."""
    L = _lib()
    raw, x = front_records["i16_iq"]
    band = BANDS["wide"]
    _load(engine, raw, "IQ", band[0])
    n = _front_lengths(order)[which]
    assert n > 3 * order and n + 1 <= N_FRONT
    if which == 0:
        assert _status(lambda: engine.acq_condition(band[0], band[1], band[2], 1, 3 * order, fir_order=order, band_margin=band[3])) == L.GC_E_RANGE
    else:
        assert (n + 6 * order) % 256 == (255, 0, 1)[which - 1]
    _check_front(engine, x, band, order, 1, n, f"order={order} n={n}")


@pytest.mark.parametrize("name", list(BANDS))
def test_front_end_bands_zones_and_decimation(engine, front_records, name):
    """The four bands of the table (Nyquist zones 2, 6 and 1; margin 0 and 0.002), order 700, 40 000 int8 samples from an odd start:
    rate, IF and length exactly, every output sample - the first (index 1) and the last decimation index included."""
    raw, x = front_records["i8_iq"]
    band = BANDS[name]
    _load(engine, raw, "IQ", band[0])
    new_fs, new_if, nz = _check_front(engine, x, band, 700, 4097, 40000, name)
    assert (nz, new_fs, new_if) == band[4:]


# ---- 4. statistics -------------------------------------------------------------------------------------------------------------------
N_STAT = 100000
STAT_LENGTHS = [2, 3, 1023, 1024, 1025, 65537]


def _near_constant_record():
    """100 000 samples of 127 - 128i, seven of them 126 - 128i: var = 7.0e-5 under |mean|^2 = 3.3e4."""
    rec = np.empty(2 * N_STAT, dtype=np.int8)
    rec[0::2], rec[1::2] = 127, -128
    rec[2 * np.array([2, 700, 1025, 5000, 30001, 60000, 99999])] = 126
    return rec


def _dc100_record():
    rng = np.random.default_rng(4)
    v = np.rint(100.0 + 60.0 * rng.standard_normal(2 * N_STAT))
    v[1::2] -= 170.0
    return np.clip(v, -128, 127).astype(np.int8)          # full range around a DC of about 100 - 70i, both rails hit


STAT_RECORDS = {"near_constant": _near_constant_record, "dc100": _dc100_record}


def _exact_stats(rec, first, n):
    a = [int(v) for v in rec[2 * first:2 * (first + n):2]]
    b = [int(v) for v in rec[2 * first + 1:2 * (first + n):2]]
    sr, si, s2 = sum(a), sum(b), sum(v * v for v in a) + sum(v * v for v in b)
    return Fraction(sr, n), Fraction(si, n), Fraction(n * s2 - sr * sr - si * si, n * (n - 1))


def _within_ulps(got, exact, ulps=4):
    return abs(Fraction(got) - exact) <= ulps * Fraction(2) ** -52 * abs(exact)


@pytest.mark.parametrize("n", STAT_LENGTHS + [N_STAT])
@pytest.mark.parametrize("name", list(STAT_RECORDS))
def test_signal_stats_of_the_int8_record_are_exact_to_a_few_ulp(engine, name, n):
    """mean = s / n and var = (n s2 - |s|^2) / (n (n - 1)) in Python integers; the library has the same integers and divides once:
    4 ulp (9e-16).  The float64 form (s2 - n |mean|^2) / (n - 1) returns 6.999579807e-05 for the whole near-constant record, 2.7e-8 off."""
    rec = STAT_RECORDS[name]()
    engine.load_if(rec, fs=18e6)
    for first in ((0,) if n == N_STAT else (1, 4097)):
        mean, var = engine.acq_signal_stats(first, n)
        mr, mi, v = _exact_stats(rec, first, n)
        rel = float(abs(Fraction(var) - v) / v) if v else abs(var)
        print(f"STATS int8 {name} n={n} first={first}: var {var!r}, relative error {rel:.2e}")
        assert _within_ulps(mean.real, mr) and _within_ulps(mean.imag, mi), (first, mean)
        assert _within_ulps(var, v), (first, var, float(v), rel)
    if name == "near_constant" and n == N_STAT:
        assert abs(var - 6.999579996e-05) < 1e-14


@pytest.mark.parametrize("n", STAT_LENGTHS)
@pytest.mark.parametrize("name", ["weak_on_dc", "zero_mean"])
def test_signal_stats_of_the_conditioned_signal(engine, name, n):
    """Float64 two-pass reference (sums by math.fsum); the library adds in float64 in a fixed order: n 2^-53 relative to s2 / (n - 1)."""
    rng = np.random.default_rng(9)
    z = rng.standard_normal(70000) + 1j * rng.standard_normal(70000)
    sig = ((100.0 - 50.0j) + 0.25 * z if name == "weak_on_dc" else 1000.0 * z).astype(np.complex64)
    engine.load_if(np.zeros(64, dtype=np.int8), fs=18e6)
    engine.acq_set_signal(sig)
    for first in (1, 4097):
        x = sig[first:first + n].astype(np.complex128)
        mr, mi = math.fsum(x.real) / n, math.fsum(x.imag) / n
        want = math.fsum((x.real - mr) ** 2 + (x.imag - mi) ** 2) / (n - 1)
        s2 = math.fsum(x.real ** 2 + x.imag ** 2)
        mean, var = engine.acq_signal_stats(first, n, source=1)
        bound = n * 2.0 ** -53 * s2 / (n - 1)
        print(f"STATS cond {name} n={n} first={first}: |var - ref| / bound {abs(var - want) / bound:.3g}, relative {abs(var - want) / want:.2e}")
        assert abs(var - want) <= bound, (first, var, want)
        assert abs(mean.real - mr) <= 2.0 ** -53 * math.fsum(np.abs(x.real)) and abs(mean.imag - mi) <= 2.0 ** -53 * math.fsum(np.abs(x.imag))


def test_coarse_search_sig_power_under_a_strong_dc(engine):
    """peakMetric = peak / sqrt(var(x(1:spc)) * spc) / H (acquisition.m:151, :200) where the first code period is the near-constant
    record's kind (127 - 128i, eight samples 126 - 128i) and the second one carries the signal: the peak is re-evaluated in float64 by
    the guard, so the metric must agree with the float64 restatement to the README's 1e-13 - which the cancelling form of var misses."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd.receiver import _acq_params
    S = P.initSettings()
    S.samplingFreq, S.acqSearchBand, S.acqSearchStep, S.acqNonCohTime = 4e6, 1000.0, 500.0, 1
    fs, spc = S.samplingFreq, 4000
    rng = np.random.default_rng(31)
    code = rng.choice(np.array([-1, 1], dtype=np.int8), size=spc)
    n = np.arange(3 * spc)
    x = np.full(3 * spc, 127.0 - 128.0j)
    x[np.arange(8) * 500 + 3] = 126.0 - 128.0j
    lag = 1717
    x[spc:] = 100.0 * np.roll(np.tile(code, 2), lag) * np.exp(2j * np.pi * (S.IF + 500.0) * n[spc:] / fs)
    rec = np.empty(6 * spc, dtype=np.int8)
    rec[0::2], rec[1::2] = np.rint(x.real), np.rint(x.imag)
    engine.load_if(rec, fs=fs)
    r = engine.acquire_coarse(_acq_params(S, 0), code[None, :])[0]
    xi = rec[0::2].astype(np.float64) + 1j * rec[1::2].astype(np.float64)
    code_fd = np.conj(np.fft.fft(np.concatenate([code.astype(np.float64), np.zeros(spc)])))
    results = np.stack([np.abs(np.fft.ifft(np.fft.fft(np.exp(-2j * np.pi * (S.IF + 1000.0 - 500.0 * b) * n[:2 * spc] / fs) * xi[:2 * spc]) * code_fd))
                        for b in range(5)])
    var = float(_exact_stats(rec, 0, spc)[2])
    want = results.max() / math.sqrt(var * spc) / 1
    b, tau = np.unravel_index(int(np.argmax(results)), results.shape)
    print(f"COARSE metric {r.peak_metric!r} vs {want!r}: relative {abs(r.peak_metric - want) / want:.2e}")
    assert (r.coarse_bin, r.code_phase) == (b + 1, tau + 1) and b == 1
    assert abs(r.peak_metric - want) <= 1e-13 * want
