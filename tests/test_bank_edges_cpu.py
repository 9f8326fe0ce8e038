"""That the tap bank's edge sweep (tests/bank_edge_cases.py, run on the device by tests/test_gpu_bank_edges.py) proves something,
without a GPU: the generator keeps its caps and covers its axes, its refusal predictor answers as bank_validate itself does
(tests/bank_plan_shim.hip), and the sweep reaches the one place where the float64 ramp of csrc/replica_f64.h could differ from
MATLAB's colon - the end point.

ramp64 builds the second half of a ramp backwards from b = (((N-1)*step + rem) + o)*R.  MATLAB's colon builds it from
c = a + n*d and takes b instead only when c - b > -tol, tol = 2 eps max(|a|, |b|).  When rem and o are large and of opposite sign,
a and b carry the rounding of intermediates much larger than themselves, c < b - tol, and the two second halves differ by a few
1e-14: a sample on a table edge then gets another index.  bank_cases.ramp_model restates ramp64 + colon_at in numpy with either
end point; with b itself it differs from the oracle's colon at (at least) the four descriptors it was found at, with MATLAB's
end point it equals the colon element for element on every inside descriptor of the sweep.  The E/P/L taps of gc_correlate
(rem > -1, offsets -d, 0, +d with d * R * m < 1) get there only where a tap cancels rem (rem = d, rem = -d + an ulp), and over the
correlator edge sweep's values no table index changes with the end point."""
import ctypes as C

import numpy as np
import pytest

import bank_edge_cases as E
from bank_cases import oracle_ramp, ramp_index, ramp_model
from oracle import gnss_oracle as O
from test_gpu_correlator_edges import Chan, d_at, d_half, low_ok, rem_min

_SWEEPS = {}


def _sweep(name, fmt):
    if (name, fmt) not in _SWEEPS:
        _SWEEPS[(name, fmt)] = E.BankSweep(E.make_rig(name), fmt).build()
    return _SWEEPS[(name, fmt)]


@pytest.mark.parametrize("name", E.RIGS)
def test_the_sweep_keeps_its_caps_and_covers_its_axes(name):
    for fmt in E.FORMATS:
        sw = _sweep(name, fmt)
        sw.check_caps()         # outside <= 1 % of the rig's descriptors, <= 5 % of every (rem, rate) cell; each refusal class; the four found
        n, ch0 = sw.counts(), sw.rig.chans[0]
        assert len(sw.cases) == n["inside"] + n["refused"] + n["outside"] and n["inside"] > 3500
        inside = [c for c in sw.cases if c["kind"] == "inside"]
        cells = sw.cells()
        for rem in E.REMS:
            for rate in E.RATES:
                assert cells[(rem, rate)][0] >= 38, (name, fmt, rem, rate)
                assert any(c["cell"] == (rem, rate) and c["n"] >= 4095 and len(c["taps"]) >= 5 for c in inside), (name, fmt, rem, rate)
        for rate in E.RATES:                                             # every length in every rate class
            assert {c["n"] for c in inside if c["cell"][1] == rate} >= set(E.LENGTHS), (name, fmt, rate)
        for n_ in range(1, 66):                                          # 1..65 x every head alignment
            heads = [c for c in sw.cases if c["n"] == n_ and c["taps"] == E.T_3 and c["cell"] == ("other", "nominal")]
            assert {c["s0"] % 16 for c in heads} == set(range(16)), (name, fmt, n_)
        heads = [c for c in sw.cases if c["taps"] == E.T_3 and c["cell"] == ("other", "nominal")]
        assert len(heads) >= 1040 and sum(c["kind"] != "inside" for c in heads) <= 10      # a few samples whose start cancels at a tap
        assert any(c["s0"] == 0 for c in inside) and any(c["s0"] + c["n"] == sw.nsamp for c in inside)
        assert {len(c["taps"]) for c in inside} >= {1, 3, 9, 64}
        # the accepted side of each limit: exactly one entry per sample, exactly 2^-16, the largest offset, the largest rem
        omax = E.offset_max([ch0])
        assert any(E.rate_of(ch0, c["step"]) == 1.0 for c in inside) and any(E.rate_of(ch0, c["step"]) == 2.0 ** -16 for c in inside)
        assert any(omax in c["taps"] and -omax in c["taps"] for c in inside)
        big = [c for c in inside if c["cell"][0] == "big"]
        assert all(E.refusal(ch0, c["n"], float(np.nextafter(c["rem"], np.inf)), c["step"], c["taps"]) == ("GC_E_INVALID", "int32") for c in big)
        assert max(c["rem"] * ch0.K for c in big) > 2.147e9
        sides = [c["tags"]["side"] for c in sw.refused]
        assert all(sides.count(s) >= 2 for s in ("rate_high", "rate_low", "period", "int32")), sides
        # rem = 0, one entry per sample, integer offsets: MATLAB's colon takes its integer path and every sample sits on an edge
        for c in (c for c in inside if c["tags"].get("integer_path")):
            for o in c["taps"]:
                t = oracle_ramp(c["rem"], o, c["step"], c["n"], ch0.R)
                if max(ch0.mult) == 1.0:                                  # (B1C's base ramp steps by fl(1/6) * 2: no integer path)
                    assert c["step"] * ch0.R == 1.0 and np.all(ramp_index(t) == t), (name, o)
        # the two blocks at exactly 2^-16: the prompt tap's fastest ramp stays inside one entry / crosses one edge
        for tag, edges in (("one_entry", 0), ("one_edge", 1)):
            c, = [c for c in inside if c["tags"].get(tag)]
            p = ramp_index(oracle_ramp(c["rem"], 0.0, c["step"], c["n"], ch0.R), max(ch0.mult))
            assert c["n"] == 4097 and p[-1] - p[0] == edges, (name, tag, p[0], p[-1])


def _shim():
    from test_bank_plan_cpu import _shim as plan_shim
    lib = plan_shim()
    lib.bank_shim_set_ramp.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double]
    return lib


@pytest.mark.parametrize("name", E.RIGS)
def test_the_refusal_predictor_answers_as_bank_validate_does(name):
    """Every descriptor of the sweep, alone, through bank_validate on the CPU: GC_OK for the inside and outside ones, the predicted
    status for the refused ones."""
    from cu_sdr_collection_amd import _lib as L
    from test_bank_plan_cpu import _blocks, _f64
    lib = _shim()
    for fmt in ("i8_iq", "i16_real"):
        sw = _sweep(name, fmt)
        ctx = lib.bank_shim_create(1, sw.nsamp, E.FS)
        try:
            for c, ch in enumerate(sw.rig.chans):
                lib.bank_shim_set_channel(ctx, c, len(ch.tables), len(ch.tables[0]), 0, 0)
                for a, (t, m) in enumerate(zip(ch.tables, ch.mult)):
                    lib.bank_shim_set_ramp(ctx, c, ch.R, a, len(t), m)
            seen = set()
            for case in sw.cases:
                off, offp = _f64(case["taps"])
                rc = lib.bank_shim_check(ctx, 1, _blocks([case]).ctypes.data, len(off), offp, 1, None)
                want = L.GC_OK if case["kind"] != "refused" else getattr(L, case["refuse"][0])
                assert rc == want, (name, fmt, case)
                seen.add(rc)
            assert seen == {L.GC_OK, L.GC_E_INVALID, L.GC_E_UNSUPPORTED}
        finally:
            lib.bank_shim_destroy(ctx)


def test_the_end_point_itself_differs_from_matlabs_at_the_cancelling_pairs():
    """ramp64 with b itself as the end of the ramp (what it took before this sweep), R = 1, one arm: another table index than the
    oracle's colon at the four descriptors of bank_edge_cases.CANCELLING - two samples of 64, then one of 4 096 each."""
    differ = []
    for rem, o, step, n in E.CANCELLING:
        t = oracle_ramp(rem, o, step, n)
        assert t.shape[0] == n
        differ.append(np.nonzero(ramp_index(ramp_model(rem, o, step, n, matlab_end=False)) != ramp_index(t))[0].tolist())
        assert np.array_equal(ramp_model(rem, o, step, n), t)
    assert differ == [[35, 40], [3900], [2400], [3000]], differ
    rem, o, step, n = E.CANCELLING[1]
    assert oracle_ramp(rem, o, step, n)[3900] == 198.99999999999997 and ramp_model(rem, o, step, n, matlab_end=False)[3900] == 199.00000000000009


@pytest.mark.parametrize("name", E.RIGS)
def test_matlabs_end_point_makes_the_ramp_the_colon_on_every_inside_descriptor(name):
    """Element for element, every tap of every inside descriptor; and the sweep has inside descriptors at which b itself would not do
    (so the device run tells the two end points apart)."""
    told_apart = 0
    for fmt in ("i8_iq", "i16_real"):
        sw = _sweep(name, fmt)
        for c in sw.cases:
            if c["kind"] != "inside":
                continue
            ch = sw.rig.chans[c["channel"]]
            apart = False
            for o in c["taps"]:
                t = oracle_ramp(c["rem"], o, c["step"], c["n"], ch.R)
                assert np.array_equal(ramp_model(c["rem"], o, c["step"], c["n"], ch.R), t), (name, fmt, c, o)
                old = ramp_model(c["rem"], o, c["step"], c["n"], ch.R, matlab_end=False)
                apart = apart or any(np.any(ramp_index(old, m) != ramp_index(t, m)) for m in set(ch.mult))
            told_apart += apart
    print(f"\n[bank edges] {name}: {told_apart} inside descriptors at which the end point b itself gives another table index")
    assert told_apart >= {"l1ca": 4, "e1bc": 1, "b1c": 0, "l5": 1}[name], (name, told_apart)


def test_the_early_prompt_and_late_taps_reach_the_corner_only_where_a_tap_cancels_rem():
    """gc_correlate's domain: rem > -1, taps -d, 0, +d with d * R * m < 1.  Over the correlator edge sweep's rem, spacing and step
    values and this sweep's lengths (233 083 ramps whose colon has N elements) MATLAB's end point is b itself, so ramp64's end point
    is the same before and after it learnt MATLAB's rule - except at 219 ramps where the tap cancels rem to a fifth of the spacing or
    less (rem = d at the early tap, rem = -d + an ulp at the late one, rem = 0.3 next to d = 0.25), nearly all at 1e-7 entries per
    sample.  So the three taps CAN reach the corner; on this grid none of those ramps has a sample close enough to a table edge for
    the other end point to give another index."""
    checked, corner = 0, 0
    for ch in (Chan([np.ones(1025)], 1023), Chan([np.ones(8186)] * 2, 4092, R=2.0), Chan([np.ones(2048), np.ones(2048), np.ones(12278)], 1023, R=2.0,
                                                                                         mult=[1, 1, 6])):
        per_entry = ch.R * ch.mult[0]
        steps = [(t / q) * (1 + e) / per_entry for t, q in ((0.995, 15.0), (0.995, 7.0)) for e in (-1e-9, 1e-9, 0.045)]
        steps += [1e-7 / per_entry, 3.3 / per_entry, 1.023e6 / 18e6, 10.23e6 / 18e6]
        for d in (0.0, 1e-9, d_half(ch), d_at(ch, 0.999), 0.6 * d_half(ch)):
            for rem in (0.0, 1e-13, -1e-13, -0.4, rem_min(ch, d), 0.3, 0.999):
                if not low_ok(ch, rem, d):
                    continue
                for step in steps:
                    for n in E.LENGTHS + [min(int(np.ceil((ch.L - rem) / step)), 40009)]:      # a full period, where a record holds one
                        for tap in (-d, 0.0, d):
                            a, b = (rem + tap) * ch.R, (((n - 1) * step + rem) + tap) * ch.R
                            t = O.colon(a, step * ch.R, b)
                            if t.shape[0] != n:
                                continue
                            checked += 1
                            if t[-1] != b:                          # (where it is b, the two end points are one and the same)
                                corner += 1
                                new, old = ramp_model(rem, tap, step, n, ch.R), ramp_model(rem, tap, step, n, ch.R, matlab_end=False)
                                assert np.array_equal(new, t) and not np.array_equal(old, t), (ch.K, rem, d, step, n, tap)
                                assert tap != 0.0 and abs(rem + tap) <= 0.2 * abs(tap) * (1 + 1e-12), (ch.K, rem, d, step, n, tap)
                                assert all(np.array_equal(ramp_index(old, m), ramp_index(t, m)) for m in set(ch.mult)), (ch.K, rem, d, step, n, tap)
    print(f"\n[bank edges] E/P/L grid: {checked} ramps, MATLAB's end point is not b at {corner}")
    assert checked > 200000 and 0 < corner <= checked // 1000, (checked, corner)
