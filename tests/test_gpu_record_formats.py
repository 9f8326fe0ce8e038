"""The six encodings of one record (int8 / int16 x I/Q, Q/I, I alone) through the kernels that read a record one sample at a time
with csrc/record_fmt.h's loader: the float64 correlator (corr_f64.hip), the mixed-multiplier kernel (corr_kernel.hip) and the tap
bank (corr_bank.hip).  A loader returns the same numbers for every encoding of a sample and these kernels add in an order that does
not depend on the format, so the comparisons are exact: the four complex encodings give identical sums, the two real ones give
identical sums.  (The lane, fast, multi and CBOC kernels are left out on purpose: their int16 instantiations have other workgroup
shapes, hence another summation order; test_gpu_variants.py and test_gpu_correlator*.py cover them against the oracle.)
The int8 I/Q and int8 real float64 sums also equal the Python float64 oracle to the 1e-12 of max|want| of
test_gpu_tracking_f64.py::test_f64_correlate_equals_the_float64_oracle_per_block."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import gnss_oracle as O

pytestmark = pytest.mark.gpu

FS = 4.092e6           # 4 samples per chip of a 1 023-chip code: blocks of ~4 092 samples
L = 1023.0
N_IF = 40000
COMPLEX = ("i8_iq", "i8_qi", "i16_iq", "i16_qi")
REAL = ("i8_real", "i16_real")


@pytest.fixture(scope="module")
def case():
    from cu_sdr_collection_amd import _lib as G
    rng = np.random.default_rng(20)
    chips = [rng.choice([-1.0, 1.0], size=1023) for _ in range(3)]
    boc11 = lambda c: np.repeat(c, 2) * np.tile([-1.0, 1.0], c.size)
    tab_ca = O.pad_code(chips[0])                                       # channel 0: one arm
    tab_d, tab_p = O.pad_code(boc11(chips[1])), O.pad_code(boc11(chips[2]))   # channel 1: two arms, index_scale 2
    tab_six = O.pad_code(rng.choice([-1.0, 1.0], size=12 * 1023))      # ... or, for the mixed kernel, a second arm read through
    #                                                                    ceil(6 t) that is NOT its neighbour times a sign
    # the record: noise plus channel 0's code on a carrier, int8 I/Q
    i = np.arange(N_IF)
    sig = chips[0][(np.floor(i * (1.023e6 / FS)).astype(np.int64) + 200) % 1023] * np.exp(2j * np.pi * 1200.0 * i / FS)
    x = 14 * (rng.standard_normal(N_IF) + 1j * rng.standard_normal(N_IF)) + 8 * sig
    iq = np.empty(2 * N_IF, dtype=np.int8)
    iq[0::2] = np.clip(np.rint(x.real), -127, 127)
    iq[1::2] = np.clip(np.rint(x.imag), -127, 127)
    qi = np.empty_like(iq)
    qi[0::2], qi[1::2] = iq[1::2], iq[0::2]
    records = {"i8_iq": (iq, G.GC_IQ), "i8_qi": (qi, G.GC_QI), "i16_iq": (iq.astype(np.int16), G.GC_IQ),
               "i16_qi": (qi.astype(np.int16), G.GC_QI), "i8_real": (iq[0::2].copy(), G.GC_REAL),
               "i16_real": (iq[0::2].astype(np.int16), G.GC_REAL)}
    # six blocks over the two channels: odd and even blksize (an odd one has the colon's middle element), odd and even first_sample
    descs = []
    for k in range(6):
        step = 1.023e6 / FS * (1 + float(rng.uniform(-3e-6, 3e-6)))
        rem = float(rng.uniform(0, step))
        n = O.blksize_for(L, rem, step)
        n -= (n + k) % 2 == 0                          # k even: odd n, k odd: even n
        s0 = int(rng.integers(0, (N_IF - n) // 2)) * 2 + (k // 2) % 2
        descs.append(SimpleNamespace(channel=k % 2, n=n, s0=s0, rem=rem, step=step, d=0.06, f=float(rng.uniform(-3e3, 3e3)),
                                     phi=float(rng.uniform(-3, 3))))
    assert {d.n % 2 for d in descs} == {0, 1} and {d.s0 % 2 for d in descs} == {0, 1}
    assert all(2000 < d.n < 5000 and d.s0 + d.n <= N_IF for d in descs)
    return SimpleNamespace(records=records, descs=descs, tab_ca=tab_ca, tab_d=tab_d, tab_p=tab_p, tab_six=tab_six)


def _blocks(engine, descs):
    b = engine.make_blocks(len(descs))
    for k, d in enumerate(descs):
        b[k].channel, b[k].blksize, b[k].first_sample = d.channel, d.n, d.s0
        b[k].rem_code_phase, b[k].code_phase_step, b[k].el_spacing = d.rem, d.step, d.d
        b[k].carr_freq, b[k].rem_carr_phase = d.f, d.phi
    return b


def _over_the_encodings(engine, case, run):
    """run(blocks) on every encoding of the record; the complex ones must agree to the bit, and so must the real ones."""
    blocks = _blocks(engine, case.descs)
    got = {}
    for name, (rec, layout) in case.records.items():
        engine.load_if(rec, layout=layout, fs=FS)
        got[name] = run(blocks)
    for group in (COMPLEX, REAL):
        for name in group[1:]:
            assert np.array_equal(got[name], got[group[0]]), (name, float(np.max(np.abs(got[name] - got[group[0]]))))
    assert np.any(got["i8_iq"] != 0) and not np.array_equal(got["i8_iq"], got["i8_real"])
    return got


def _equal_mult_channels(engine, case):
    engine.set_channel(0, [case.tab_ca.astype(np.int8)])
    engine.set_channel(1, [case.tab_d.astype(np.int8), case.tab_p.astype(np.int8)], index_scale=2.0)
    return {0: ([case.tab_ca], 1.0, None), 1: ([case.tab_d, case.tab_p], 2.0, None)}


def test_float64_correlator_over_the_six_encodings(engine, case):
    chans = _equal_mult_channels(engine, case)

    def run(blocks):
        got = engine.correlate(blocks)
        assert engine.last_kernel() == 6
        return got

    engine.set_precision("double")
    try:
        got = _over_the_encodings(engine, case, run)
    finally:
        engine.set_precision("single")
    for name, file_type in (("i8_iq", 2), ("i8_real", 1)):
        rec = case.records[name][0]
        want = np.zeros_like(got[name])
        for k, d in enumerate(case.descs):
            tabs, r, mult = chans[d.channel]
            s, _, _ = O.correlate_block(O.raw_from_if(rec, d.s0, d.n, file_type=file_type), tabs, d.rem, d.step, d.d, d.f, d.phi, FS, L,
                                        r=r, arm_mult=mult)
            want[k, :len(tabs)] = s
        rel = float(np.max(np.abs(got[name] - want))) / float(np.max(np.abs(want)))
        print(f"\n[record formats] float64 {name}: {rel:.1e} of max|want| against the Python float64 oracle")
        assert rel <= 1e-12, (name, rel)


def test_mixed_multiplier_kernel_over_the_six_encodings(engine, case):
    engine.set_channel(0, [case.tab_ca.astype(np.int8)])
    engine.set_channel(1, [case.tab_d.astype(np.int8), case.tab_six.astype(np.int8)], index_scale=2.0, arm_mult=[1, 6])

    def run(blocks):
        got = engine.correlate(blocks)
        assert engine.last_kernel() == -1
        return got

    _over_the_encodings(engine, case, run)


def test_tap_bank_over_the_six_encodings(engine, case):
    _equal_mult_channels(engine, case)
    _over_the_encodings(engine, case, lambda blocks: engine.correlate_bank(blocks, [-0.5, -0.06, 0.0, 0.06, 0.5]))
