"""That gc_cancel's edge sweep (tests/cancel_edge_cases.py, run on the device by tests/test_gpu_cancel_edges.py) proves something,
without a GPU: the generator keeps its caps, reaches every class of its refusal predictor and every value of its axes inside the
domain; the model-only conditions the device test relies on hold for the reference alone (the `near` count of every call, the
exact class's ties and clamps); and the model's ramp (bank_cases.ramp_model: csrc/replica_f64.h's, with MATLAB's end point) is
MATLAB's colon wherever that has N elements, and moves no byte of tests/test_gpu_cancel.py's scene."""
import math

import numpy as np
import pytest

import cancel_edge_cases as E
import cancel_model as M
from bank_cases import oracle_ramp, ramp_index, ramp_model

_SWEEPS = {}


def _sweep(name, fmt):
    if (name, fmt) not in _SWEEPS:
        _SWEEPS[(name, fmt)] = E.CancelSweep(E.make_rig(name), fmt).build()
    return _SWEEPS[(name, fmt)]


def test_no_record_is_a_multiple_of_16_bytes_and_every_value_is_there():
    sizes = set()
    for fmt, (dtype, layout) in E.FORMATS.items():
        x = E.make_record(fmt)
        assert x.dtype == dtype and x.shape[0] == E.NS * (1 if layout == M.REAL else 2) and x.nbytes % 16 != 0
        sizes.add(x.nbytes)
        info = np.iinfo(dtype)
        assert x.min() == info.min and x.max() == info.max
        assert len(np.unique(x)) >= min(info.max - info.min + 1, 25000)
        per = x.shape[0] // E.NS
        assert not x[per * E.ZERO_AT:per * (E.ZERO_AT + E.ZERO_LEN)].any()
    assert sizes == {80018, 160036, 40009}


@pytest.mark.parametrize("name", E.RIGS)
def test_the_sweep_keeps_its_caps_and_covers_its_axes(name):
    for fmt in E.FORMATS:
        sw = _sweep(name, fmt)
        sw.check_caps()             # generated == inside + refused + outside, outside <= 1 %, every refusal class, no overlap in a call
        rig, n = sw.rig, sw.counts()
        ch0 = rig.chans[0]
        inside = sw.sent()
        print(f"\n[cancel edges] {name} {fmt}: generated {len(sw.cases)} = inside {n['inside']} + refused {n['refused']} + outside {n['outside']}"
              f" in {len(sw.calls)} calls")
        assert n["inside"] >= 7700
        # every axis value in at least one inside descriptor (rem -0.4 where check_block lets it through: K * 0.4 < 1 ...)
        rems = {c["cell"][0] for c in inside}
        low04 = not -0.4 * ch0.K > -1.0
        assert rems >= set(E.REMS) - ({"-0.4"} if low04 else set()), (name, fmt, rems)
        if low04:                   # ... and in the refusal class "low" where it does not
            assert all(c["refuse"] == "low" for c in sw.cases if c["cell"][0] == "-0.4")
        assert {c["cell"][1] for c in inside} >= set(E.RATES), (name, fmt)
        assert {c["n"] for c in inside} >= set(E.LENGTHS) | {E.NS}, (name, fmt)
        assert sum(bool(c["tags"].get("fast")) for c in inside) >= 12                       # 3.5 entries per sample
        assert any(B_rate(rig, c) == 1.0 for c in inside) and any(B_rate(rig, c) > 3.0 for c in inside)
        assert any(B_rate(rig, c) <= 2.0 ** -40 for c in inside)
        for f in E.F_SET:
            assert {c["phi"] for c in inside if c["f"] == f} >= set(E.PHI_SET), (name, fmt, f)
        assert any(c["s0"] == 0 and c["n"] < E.NS for c in inside) and any(c["s0"] + c["n"] == E.NS and c["s0"] > 0 for c in inside)
        assert any(c["s0"] > 0 for label, call in sw.calls for c in [min(call, key=lambda q: q["s0"])]), "some call leaves the head uncovered"
        for ln in range(1, 18):
            heads = [c for c in inside if c["n"] == ln and isinstance(c["pin"], int)]
            assert {c["s0"] % 16 for c in heads} == set(range(16)) and all(c["s0"] % 16 == c["pin"] for c in heads), (name, fmt, ln)
            assert {(c["s0"] + c["n"]) % 16 for c in inside if c["n"] == ln} == set(range(16))
        # the accepted side of the table's end and of the low index: one ulp further is refused
        tops = [c for c in inside if c["cell"][0] == "top" or c["tags"].get("side_ok") == "table_end"]
        assert len(tops) >= 20
        for c in tops:
            ch = rig.chans[c["chan"]]
            up = float(np.nextafter(c["rem"], np.inf))
            assert E.refusal(ch, rig.windows[c["chan"]], E.NS, c["n"], c["s0"], up, c["step"], c["off"]) == "table_end", c
        lows = [c for c in inside if c["cell"][0] == "min"]
        for c in lows:
            down = float(np.nextafter(c["rem"], -np.inf))
            assert E.refusal(rig.chans[c["chan"]], rig.windows[c["chan"]], E.NS, c["n"], c["s0"], down, c["step"]) in ("low", "descriptor")
        # a block inside one table entry; a block of 20 chunks
        c, = [c for c in inside if c["tags"].get("one_entry")]
        p = ramp_index(oracle_ramp(c["rem"], 0.0, c["step"], c["n"], ch0.R), max(ch0.mult))
        assert c["n"] == 4097 and p[0] == p[-1]
        assert sum(c["n"] == E.NS for c in inside) >= 2
        # the named calls
        calls = dict(sw.calls)
        many = calls["chan64"]
        assert len(many) == 64 and {c["ch"] for c in many} == set(range(64)) and {(c["s0"], c["n"]) for c in many} == {(20003, 300)}
        tiny = calls["tiny4100"]
        assert len(tiny) >= 4096 and len({c["ch"] for c in tiny}) == 1 and all(1 <= c["n"] <= 3 for c in tiny)
        assert all(a["s0"] + a["n"] == b["s0"] for a, b in zip(tiny, tiny[1:]))
        mixed = calls["tiny3000+big"]
        assert len(mixed) >= 2990 and mixed[-1]["n"] == 20000 and mixed[-2]["s0"] + mixed[-2]["n"] <= 8000 <= mixed[-1]["s0"]
        assert sorted(sw.shuffled["tiny3000+big"]) == list(range(len(mixed)))


def B_rate(rig, c):
    ch = rig.chans[c["chan"]]
    return c["step"] * ch.R * max(ch.mult)


def test_the_wide_rig_has_zero_energy_blocks_a_window_and_the_largest_offset():
    sw = _sweep("wide", "i8_iq")
    rig, chans = sw.rig, sw.rig.model_chans()
    inside = sw.sent()
    zero = [c for c in inside if c["tags"].get("zeros")]
    assert len(zero) == 5 and all(not M.replica(c, chans[c["ch"]], E.FS)[2].any() for c in zero)              # E == 0
    some = [M.replica(c, chans[c["ch"]], E.FS)[2][0] for c in inside if c["chan"] == 0 and c["n"] >= 255][:20]
    assert any(0 < np.sum(c * c) < c.shape[0] for c in some)                                                   # E < N
    win = [c for c in inside if c["tags"].get("windowed") and c["cell"][0] == "top"]
    assert win and all(math.ceil(((c["n"] - 1) * c["step"] + c["rem"]) * 2.0) == 1499 for c in win)            # the window's last entry
    off = [c for c in inside if c["tags"].get("offset")]
    ch2 = rig.chans[2]
    assert any(c["off"] == [len(ch2.tables[0]) - 3, len(ch2.tables[1]) - 3] for c in off) and len(off) >= 30
    assert any(c["tags"].get("alone") and c["off"] == [len(t) - 3 for t in rig.chans[0].tables] for c in inside)
    assert {"offset"} <= {c["refuse"] for c in sw.refused}


@pytest.mark.parametrize("name", E.RIGS)
def test_the_models_ramp_is_matlabs_colon_on_every_inside_descriptor(name):
    """cancel_model.oracle_ok is what makes a descriptor `inside`; where it holds, ramp_model equals the oracle's colon element for
    element - so the model is the definition, not its approximation."""
    checked = 0
    for fmt in ("i8_iq", "i16_real", list(E.FORMATS)[(E.RIGS.index(name)) % 6]):
        sw = _sweep(name, fmt)
        for c in sw.cases:
            if c["kind"] == "refused":
                continue
            r = sw.rig.chans[c["chan"]].R
            t = oracle_ramp(c["rem"], 0.0, c["step"], c["n"], r)
            assert (t.shape[0] == c["n"]) == M.oracle_ok(c, {"r": r}) == (c["kind"] == "inside")
            if c["kind"] == "inside":
                assert np.array_equal(ramp_model(c["rem"], 0.0, c["step"], c["n"], r), t), (name, fmt, c)
                checked += 1
    assert checked > 2000


def test_matlabs_end_point_moves_no_byte_of_the_existing_scene():
    """Every model output of tests/test_gpu_cancel.py's scene - six formats, both orders, both modes, both amplitude sources - with the
    ramp's second half from the written end point b (the model before this change) and from MATLAB's: byte-identical."""
    import test_gpu_cancel as T
    new_replica = M.replica
    old_replica = lambda blk, chan, fs, matlab_end=True: new_replica(blk, chan, fs, matlab_end=False)      # noqa: E731
    differ = []
    for d in [b for lst in T.PER.values() for b in lst]:
        chan = T.CHANS[d["ch"]]
        assert M.oracle_ok(d, chan)
        if not np.array_equal(new_replica(d, chan, T.FS)[2], old_replica(d, chan, T.FS)[2]):
            differ.append(d)
    assert not differ, differ
    try:
        for fmt, (dtype, layout) in T.FORMATS.items():
            raw = T._record(dtype, layout)
            for order in ("epoch_major", "shuffled"):
                descs = T._order(order)
                for amp in (None, T._amps(descs, dtype)):
                    for mode in ("subtract", "model"):
                        M.replica = new_replica
                        new = M.cancel(raw, dtype, layout, descs, T.CHANS, T.FS, amp=amp, mode=mode)
                        M.replica = old_replica
                        old = M.cancel(raw, dtype, layout, descs, T.CHANS, T.FS, amp=amp, mode=mode)
                        assert new[0].tobytes() == old[0].tobytes() and new[1].tobytes() == old[1].tobytes(), (fmt, order, mode)
                        assert all(np.array_equal(a, b) for a, b in zip(new[2:], old[2:]))
    finally:
        M.replica = new_replica


@pytest.mark.parametrize("name", E.RIGS)
def test_the_reference_alone_keeps_the_near_count_of_every_call(name):
    """The device test compares every byte outside `near` (a model value within 1e-9 of a half-integer) and allows one count inside
    it; this is what keeps `near` from hiding anything: at most 10 per 100 000 samples in every call, amplitude source and mode.
    All six formats; the two calls of thousands of blocks in one format per rig here (in all six on the device, where the same
    assertion runs before every comparison)."""
    for fmt, (dtype, layout) in E.FORMATS.items():
        sw = _sweep(name, fmt)
        raw, chans = E.make_record(fmt), sw.rig.model_chans()
        worst = 0
        for label, call in sw.calls:
            if len(call) > 1000 and list(E.FORMATS).index(fmt) != E.RIGS.index(name):
                continue
            reps = {}
            for amp in (None, E.amplitudes(sw, call, dtype, 77)):
                for mode in ("subtract", "model"):
                    near = M.cancel(raw, dtype, layout, call, chans, E.FS, amp=amp, mode=mode, reps=reps)[5]
                    worst = max(worst, int(near.sum()))
                    assert int(near.sum()) <= E.NS * 10 // 100000, (name, fmt, label, mode, int(near.sum()))
        print(f"\n[cancel edges] {name} {fmt}: at most {worst} of {E.NS} samples within 1e-9 of a half-integer in any call")


@pytest.mark.parametrize("fmt", list(E.FORMATS))
def test_the_exact_class_has_ties_to_even_both_ways_and_clamps_at_both_ends(fmt):
    dtype, layout = E.FORMATS[fmt]
    rig = E.make_rig(("l1ca", "wide")[list(E.FORMATS).index(fmt) % 2])
    blocks, amp = E.exact_call(rig, fmt)
    assert np.array_equal(amp.real * 4, np.rint(amp.real * 4)) and np.array_equal(amp.imag * 4, np.rint(amp.imag * 4))
    assert all(b["f"] == 0.0 and b["phi"] == 0.0 for b in blocks)
    raw, chans = E.make_record(fmt), rig.model_chans()
    info = np.iinfo(dtype)
    for mode in ("subtract", "model"):
        y = E.exact_values(raw, dtype, layout, blocks, chans, amp, mode)
        assert np.array_equal(y * 4, np.rint(y * 4))                        # exact quarters: nothing was rounded on the way
        tie = (y - np.floor(y) == 0.5) & (y > info.min) & (y < info.max)
        down = int(np.sum(tie & (np.floor(y) % 2 == 0)))
        up = int(np.sum(tie & (np.floor(y) % 2 == 1)))
        lo, hi = int(np.sum(y < info.min - 1)), int(np.sum(y > info.max + 1))
        print(f"\n[cancel edges] exact class {fmt} {mode}: {down} ties round down to even, {up} up to even; {lo} clamp low, {hi} clamp high")
        assert down >= 100 and up >= 100 and lo >= 100 and hi >= 100, (fmt, mode, down, up, lo, hi)
        # and the model rounds them as the header says: rint to even, then the clamp
        want = np.clip(np.where(tie, 2 * np.rint(y / 2), np.rint(y)), info.min, info.max)
        got = M.cancel(raw, dtype, layout, blocks, chans, E.FS, amp=amp, mode=mode)[0]
        assert np.array_equal(got.reshape(y.shape).astype(np.float64), want)
