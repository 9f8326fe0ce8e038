"""The tap bank family (csrc/corr_bank.hip: gc_correlate_bank, gc_correlate_ddm, gc_correlate_ddm_integrate, gc_correlate_ddm_search)
over the descriptors bank_validate (csrc/bank_plan.h) accepts, not only the ones a receiver produces.

The family's other tests run at eleven block lengths, four rates, rem in (-0.9, 1), a carrier near 20 kHz and one descriptor per
record format.  include/gnsscorr.h promises any blksize >= 1 and start sample, rem > -1 up to the int32 index limit, offsets up
to just under a code period either way, 2^-16 <= step * R * max(m_a) <= 1, any finite carrier and phase, six record encodings.
The chunk kernel's transition form rests on index arithmetic that must be right over all of that: p(i) non-decreasing, e(k) the
definition's boundary with ties included, (k - 1) % L for negative k, int32 indices up to 2 147 483 000.  tests/bank_edge_cases.py
generates the descriptors (seeded, deterministic; a descriptor is a block together with the tap offsets of its call); here every
block, arm and tap is compared with bank_cases.reference (float64, the oracle's colon).

Rigs (arm count and multipliers asserted): GPS L1 C/A (one arm, R = 1), Galileo E1 B + C (two arms, R = 2), BDS B1C wide-band
(three arms, multipliers 1, 1, 6, R = 2), GPS L5 I + Q (two arms on 10 230-chip tables); each with a second channel whose tables
are shorter.  Records of 40 009 complex samples in the six encodings (test_gpu_correlator_edges.Record: int8 with every value,
int16 with all 65 536 values, an all-zero stretch), and a record and its negation (exactly negated sums).

Axes (the small ranges enumerated):
  blksize        1..65, 127-129, 255-257, 1023-1025, 2047-2049, 4095-4097 (five chunks); 1..65 x every residue of first_sample
                 mod 16, per encoding
  first_sample   residues 0..15 mod 16, sample 0, a block that ends on the record's last sample
  rate           step * R * max(m) exactly 1 (with rem = 0 and integer offsets: the colon's integer path, every sample on an
                 edge), 0.999, 0.5, 0.2, the receiver's, 1/64, exactly 2^-16 (a 4 097-sample block inside one entry, another
                 across one edge), 2^-16 * 1.001
  rem            0, +-1e-13, -0.4, nextafter(-1, 0), 1000.25, 1000.5, the largest value the index bound lets through
  offsets        bank_cases.POOL, +- the largest offset under the rig's code period, the cancelling pairs (rem about a period, o
                 about minus a period) the ramp's end-point rule was found at; 1, 3, 9 and 64 taps
  carrier        f in {0, -IF, +-(fs/2 - 1), 1.5 fs} x phi in {0, +-2 pi, +-1e4, 1e-300}
  composition    calls of 1, 2, 63, 64, 65 and about a thousand blocks, one descriptor at positions 0, 31 and 64 of a call
                 (bit-identical), a one-sample block between 4 097-sample blocks of channels with different table lengths

Bound (the project's own): |got - ref| <= 2e-6 * sum_n(|I_n| + |Q_n|) of the block per output; `<=`, so an all-zero block passes
only with exact zeros.  One mis-assigned sample of a 64-sample block is 1.6e-2 in those units.

Completeness: per rig and encoding generated == compared + refused + outside.  A refusal is predicted, status and all, by
bank_cases.bank_refusal (rate > 1: GC_E_UNSUPPORTED; rate < 2^-16, an offset that reaches a period, an index beyond int32:
GC_E_INVALID), with a descriptor on either side of each limit, and leaves the output untouched.  `outside`: MATLAB's colon has
N - 1 elements for one of the taps; the definition does not cover those, they are not sent, and they are capped at 1 % of a rig's
descriptors and 5 % of any (rem class, rate class) cell (tests/test_bank_edges_cpu.py).

The family's identities, on a seeded subset of about 300 descriptors per rig that holds every extreme of every axis: every bin of
gc_correlate_ddm (1, 3, 4 and 5 bins: full and partial groups of GC_DDM_GROUP; offsets up to 1.5 fs) equals the bank at the
float64 sum carr_freq + f_m, gc_correlate_ddm_integrate over runs of one block with unit weights equals the DDM, and
gc_correlate_ddm_search with one hypothesis, no shift and no weights equals integrate - all array_equal.

Measured on an MI355X (worst error / bound over the six encodings; compared / refused / outside per encoding):
  rig    worst   i8_iq          i8_qi          i8_real        i16_iq         i16_qi         i16_real
  l1ca   0.280   3807 / 13 / 9  3810 / 13 / 6  3807 / 13 / 9  3808 / 13 / 8  3807 / 13 / 9  3807 / 13 / 9    of 3 829
  e1bc   0.567   3804 / 13 / 8  3806 / 13 / 6  3806 / 13 / 6  3805 / 13 / 7  3806 / 13 / 6  3802 / 13 / 10   of 3 825
  b1c    0.966   3799 / 13 / 13 3796 / 13 / 16 3799 / 13 / 13 3796 / 13 / 16 3798 / 13 / 14 3797 / 13 / 15   of 3 825
  l5     0.478   3804 / 13 / 8  3804 / 13 / 8  3804 / 13 / 8  3804 / 13 / 8  3804 / 13 / 8  3804 / 13 / 8    of 3 825
and the identities byte for byte on 300 descriptors per rig.

What the sweep found on its first run, both mended since:
  the ramp's end point   ramp64 (csrc/replica_f64.h) built the second half of a ramp from the written end point b, MATLAB builds it
                         from c = a + (N-1)*d unless c - b > -2 eps max(|a|, |b|).  Over the bound on every encoding: l1ca rem 1000.5,
                         o -1022.5, step 0.2, N 64 (samples 35 and 40 on another entry; 6 356 to 21 522 x the bound) and rem 1000.5,
                         o -1000, N 4 096 (sample 3 000; 18 to 323 x); e1bc and l5 rem 1000.5, o -1022.5, rate 0.2, N 32, both arms
                         (13 315 to 58 064 x).  The other two descriptors it was predicted at (o -1022.9, samples 3 900 and 2 400) do
                         get another index, between two equal chips of PRN 5: no output changes.
  float32 sums           b1c, real int16, N 1 024 at the receiver's rate: the BOC(6,1) arm at o = 1022.9, 1.22 x the bound (2.4e-6 of
                         sum |x|; the worst passing b1c descriptors stood at 0.38 to 0.87).  The chunk kernel added a pair's
                         transitions in float32, a lane per 64th entry: one sign per lane on a table that alternates.  Float64 sums
                         wherever a lane can hold more than one term (more than 64 entries per chunk; below that the bits are
                         the former ones) put that descriptor under the bound (with float64 across the lanes everywhere the sweep's worst was 0.285).  The
                         worst ones left, b1c 0.87 and 0.97, are blocks of 49 and 129 samples (int16) that cross fewer than 64
                         entries: the float32 tree over lanes of alternating sign, as it was.
"""
import ctypes as C

import numpy as np
import pytest

from bank_cases import _blocks, _raw, bank_reference
from bank_edge_cases import FORMATS, FS, RIGS, BankSweep, identity_subset, make_rig
from test_gpu_correlator_edges import Record

pytestmark = pytest.mark.gpu

TOL = 2e-6                      # test_gpu_correlate_bank.py


def _layout(fmt):
    return fmt.split("_")[1].upper()


def _call(engine, taps, cases):
    got = engine.correlate_bank(_blocks(engine, cases), taps)
    assert got.shape == (len(cases), 3, len(taps))
    return got


def _say(case):
    return (f"id {case['id']} cell {case['cell']} tags {sorted(case['tags'])} channel {case['channel']} n {case['n']} s0 {case['s0']} "
            f"rem {case['rem']!r} step {case['step']!r} f {case['f']!r} phi {case['phi']!r} taps {case['taps'][:9]}")


def _compare(rig, rec, case, got, misses):
    """One descriptor, every arm and tap, against the restatement; returns error / bound (0 for a zero block).  A descriptor over the
    bound goes to `misses` with its outputs (arm, tap) over the bound, so that a run names all of them."""
    ch = rig.chans[case["channel"]]
    arms = len(ch.tables)
    raw = _raw(rec.x, case["s0"], case["n"], _layout(rec.fmt))
    ref, _ = bank_reference(raw, ch.tables, case["rem"], case["step"], case["taps"], case["f"], case["phi"], rig.fs, ch.R, list(ch.mult))
    tol = TOL * rec.scale(case)
    dev = got[:arms] - ref
    err = float(max(np.abs(dev.real).max(), np.abs(dev.imag).max()))
    if not err <= tol:
        over = np.argwhere(np.maximum(np.abs(dev.real), np.abs(dev.imag)) > tol).tolist()
        misses.append(f"{rig.name} {rec.fmt}: error {err:.6g} > bound {tol:.6g} ({err / max(tol, 1e-300):.1f} x) at [arm, tap] {over[:12]}: {_say(case)}")
    assert not got[arms:].any(), (rig.name, rec.fmt, case["id"])
    if case["tags"].get("zero"):
        assert tol == 0.0 and not got.any(), (rig.name, rec.fmt, case["id"])
    return err / tol if tol > 0 else 0.0


def _refused(engine, case):
    """The status of the call, which must not have written its output."""
    off = np.asarray(case["taps"], dtype=np.float64)
    out = np.full((1, 3, off.shape[0], 2), 12345.0)
    rc = engine._lib.gc_correlate_bank(engine._ctx, 1, _blocks(engine, [case]), off.shape[0], off.ctypes.data_as(C.POINTER(C.c_double)),
                                       out.ctypes.data_as(C.POINTER(C.c_double)))
    assert np.all(out == 12345.0), ("a refused call must not write its output", case)
    return rc


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", RIGS)
def test_edge_descriptors_match_the_reference(engine, name, fmt):
    from cu_sdr_collection_amd import _lib as L
    rig, rec = make_rig(name), Record(fmt)
    sw = BankSweep(rig, fmt).build()
    assert (rec.nsamp, rec.zero_at) == (sw.nsamp, sw.zero_at)
    sw.check_caps()
    generated, n = len(sw.cases), sw.counts()
    rec.load(engine, rig.fs)
    rig.setup(engine)
    results = {}
    for taps, cases in sw.calls:
        got = _call(engine, taps, cases)
        for k, c in enumerate(cases):
            results[c["id"]] = got[k]
    refused = 0
    for case in sw.refused:
        assert _refused(engine, case) == getattr(L, case["refuse"][0]), case
        refused += 1
    # a record and its negation: exactly negated sums (the most negative value has no negation: one up first)
    lo = -32768 if rec.i16 else -128
    pos = np.where(rec.x == lo, lo + 1, rec.x).astype(rec.x.dtype)
    taps, sub = max(sw.calls, key=lambda call: len(call[1]))
    rec.load(engine, rig.fs, pos)
    plus = _call(engine, taps, sub)
    rec.load(engine, rig.fs, (-pos).astype(rec.x.dtype))
    minus = _call(engine, taps, sub)
    assert len(sub) > 1000 and plus.any() and np.array_equal(plus, -minus), (name, fmt, "negated record")
    worst, compared, misses, at = 0.0, 0, [], None
    for taps, cases in sw.calls:
        for case in cases:
            ratio = _compare(rig, rec, case, results[case["id"]], misses)
            worst, at = (ratio, case) if ratio > worst else (worst, at)
            compared += 1
    print(f"\n[bank edges] {name} {fmt}: worst at {_say(at)}")
    for m in misses:
        print(f"[bank edges] MISS {m}")
    assert not misses, misses[:4]
    twins = [results[c["id"]] for c in sw.cases if c["tags"].get("twin")]
    assert len(twins) == 3 and all(np.array_equal(twins[0], t) for t in twins[1:]), (name, fmt, "one descriptor at several positions of a call")
    sizes = {len(cases) for _, cases in sw.calls}
    assert {1, 2, 63, 64, 65} <= sizes and max(sizes) > 1000
    assert refused == n["refused"] and compared == n["inside"] and generated == compared + refused + n["outside"], (generated, compared, refused, n)
    print(f"\n[bank edges] {name} {fmt}: worst error / bound {worst:.3f}; compared {compared}, refused {refused}, outside {n['outside']} "
          f"of {generated}")


FREQ_SETS = ((0.0,), (1.5 * FS, 0.0, -250.0), (0.37, -1.5 * FS, 250.0, 0.0), (0.0, 1.5 * FS, -1.5 * FS, 0.37, -4e3))


@pytest.mark.parametrize("name", RIGS)
def test_family_identities_at_the_edges(engine, name):
    """DDM bin m == the bank at carr_freq + f_m; integrate over runs of one block, unit weights == the DDM; search with one
    hypothesis, no shift, no weights == integrate.  Each rig on another encoding."""
    fmt = FORMATS[(1 + 2 * RIGS.index(name)) % len(FORMATS)]
    rig, rec = make_rig(name), Record(fmt)
    sw = BankSweep(rig, fmt).build()
    rec.load(engine, rig.fs)
    rig.setup(engine)
    calls = identity_subset(sw)
    total, bins = 0, set()
    for k, (taps, cases) in enumerate(calls):
        freqs = FREQ_SETS[k % len(FREQ_SETS)]
        ddm = engine.correlate_ddm(_blocks(engine, cases), taps, freqs)
        assert ddm.shape == (len(cases), 3, len(freqs), len(taps)) and ddm.any()
        for m, f in enumerate(freqs):
            bank = engine.correlate_bank(_blocks(engine, cases, df=f), taps)
            assert np.array_equal(ddm[:, :, m], bank), (name, fmt, taps, f, "DDM bin != bank at carr_freq + f")
        runs = [1] * len(cases)
        coh, pw = engine.correlate_ddm_integrate(_blocks(engine, cases), taps, freqs, runs, map_len=[len(cases)])
        assert np.array_equal(coh, ddm), (name, fmt, taps, "integrate over runs of one block != DDM")
        scoh, spw, _ = engine.correlate_ddm_search(_blocks(engine, cases), taps, freqs, runs, map_len=[len(cases)], coherent=True)
        assert scoh.shape[0] == 1 and np.array_equal(scoh[0], coh) and np.array_equal(spw[0], pw), (name, fmt, taps, "search != integrate")
        total += len(cases)
        bins.add(len(freqs))
    assert bins == {1, 3, 4, 5} and 250 <= total <= 400, (bins, total)
    print(f"\n[bank edges] {name} {fmt}: identities bit for bit on {total} descriptors in {len(calls)} calls")
