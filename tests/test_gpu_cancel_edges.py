"""gc_cancel (csrc/cancel.hip) over the descriptors and call shapes check_block accepts, not only the ones a receiver produces.

tests/test_gpu_cancel.py feeds receiver-shaped blocks: rem in [0, 0.9), one nominal step, carriers near 20 kHz, ten sizes, no block
at sample 0 or on the record's last sample.  tests/cancel_edge_cases.py generates the rest (seeded; tests/test_cancel_edges_cpu.py
checks the generator itself): five rigs (GPS L1 C/A, Galileo E1 B + C with R = 2, BDS B1C with multipliers 1, 1, 6, GPS L5, and
`wide`: a ternary table with runs of zeros, a code window, table offsets up to the largest accepted) on records of 40 009 samples in
the six formats (no byte count a multiple of 16), full-range values.

Axes: lengths 1..65, 127..129, ... 4095..4097, 6145 and the whole record as one block (20 projection chunks); rates step * R * max(m)
of exactly 1, 0.999, 0.5, 0.2, the receiver's, 1/64, 2^-16, 2^-40 (a block inside one table entry) and 3.5; rem 0, +-1e-13, -0.4,
the most negative and the largest value check_block lets through (found with nextafter), 1000.25, 1000.5; carriers f in {0, -IF,
+-(fs/2 - 1), 1.5 fs} x phi in {0, +-2 pi, +-1e4, 1e-300}; a block at sample 0, one ending on the record's last sample, every
residue of 16 for starts and ends with lengths 1..17.  The packer lays the blocks of four slots end to end (gaps 0, 1, 7, 64), the
slots overlapping freely; named calls: 64 channels on the same 300 samples (slots configured in descending order), 4 100 adjacent
blocks of 1..3 samples, and 3 000 such blocks followed by one of 20 000 samples, sorted and shuffled.

a. Sweep: every call, both amplitude sources, both modes, out of place.  array_equal with cancel_model outside `near` (a model value
   within 1e-9 of a half-integer; at most 10 per 100 000 samples, asserted), at most one count apart inside it; uncovered samples
   copied or zero; amp_out within |dP| <= (N + 8) 2^-52 sum_i |c_a(i)| (|re| + |im|), exactly 0 where E == 0.
b. Identities, byte for byte: in place == out of place == a dst that shares src's record; a shuffled list == the sorted one (amp_out
   in its own order); a block alone == the block inside its call (its amplitude; its bytes next to the call's blocks that do not touch its samples); a second run.
c. The exact class, nothing excluded: carr_freq = 0, rem_carr_phase = 0, amplitudes multiples of 1/4 - every product and sum exact,
   thousands of exact ties either way and of clamps at both ends (counted in the CPU module): every byte equals the model, and with
   the projection amp_out is bitwise the model's.
d. amp_out * E against the prompt sums of gc_correlate under GC_PREC_F64 (el_spacing = 0), within twice the bound of (a).
e. Refusals as cancel_edge_cases.refusal predicts them, each sent alone: the status, dst and amp_out untouched.
generated == compared + refused + outside per rig and format."""
import ctypes as C

import numpy as np
import pytest

import cancel_edge_cases as E
import cancel_model as M

pytestmark = pytest.mark.gpu
FS, NS = E.FS, E.NS
MAX_LEFT_OUT = NS * 10 // 100000          # 10 per 100 000 samples
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def dst_engine():
    import cu_sdr_collection_amd as P
    eng = P.Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def share_engine():
    import cu_sdr_collection_amd as P
    eng = P.Engine(0)
    yield eng
    eng.close()


def _per_sample(raw, layout):
    return raw.reshape(NS, 1 if layout == M.REAL else 2)


def _say(c):
    return (f"id {c['id']} slot {c['ch']} chan {c['chan']} n {c['n']} s0 {c['s0']} rem {c['rem']!r} step {c['step']!r} f {c['f']!r} "
            f"phi {c['phi']!r} off {c['off']} cell {c['cell']} tags {sorted(c['tags'])}")


def _out_of_place(engine, dst, raw, dtype, layout, blocks, amp, mode):
    dst.load_if(np.full_like(raw, 85), layout=layout)
    used = engine.cancel(blocks, dst=dst, amp=amp, mode=mode)
    return dst.read_if(0, NS, dtype=dtype, layout=layout), used


def _weights(raw, layout, call, reps):
    """sum_i |c_a(i)| (|re| + |im|) per block and arm."""
    re, im = M.components(raw, layout)
    ax = np.abs(re) + np.abs(im)
    w = np.zeros((len(call), 3))
    for k, c in enumerate(call):
        code = reps[k][2]
        w[k, :code.shape[0]] = np.abs(code) @ ax[c["s0"]:c["s0"] + c["n"]]
    return w


def _check_bytes(tag, call, got, want, near, layout):
    g, w = _per_sample(got, layout).astype(np.int64), _per_sample(want, layout).astype(np.int64)
    bad = np.any(g != w, axis=1) & ~near
    bad |= np.any(np.abs(g - w) > 1, axis=1)
    if bad.any():
        n = int(np.flatnonzero(bad)[0])
        over = [_say(c) for c in call if c["s0"] <= n < c["s0"] + c["n"]]
        raise AssertionError(f"{tag}: {int(bad.sum())} samples differ from the model; first at sample {n}: got {g[n].tolist()}, model {w[n].tolist()}, "
                             f"near {bool(near[n])}; covered by {over}")


def _check_amp(tag, call, got, used, E_, w, worst):
    for k, c in enumerate(call):
        for a in range(3):
            if E_[k, a] == 0:
                assert got[k, a] == 0, (tag, a, _say(c))       # no arm, or a block on zero entries: exactly 0
                continue
            bound = (c["n"] + 8) * EPS * w[k, a]
            dP = abs(got[k, a] - used[k, a]) * E_[k, a]
            assert dP <= bound, (tag, a, dP, bound, _say(c))
            if bound > 0:
                worst[0] = max(worst[0], dP / bound)


def _refused(engine, dst, lib, case):
    a_out = np.full((1, 3, 2), 7.5)
    rc = lib.gc_cancel(engine._ctx, dst._ctx, 1, E.blocks_of(engine, [case]), None, a_out.ctypes.data_as(C.POINTER(C.c_double)), 0)
    assert np.all(a_out == 7.5), ("amp_out written by a refused call", case)
    return rc


def test_a_table_value_beyond_one_is_refused_before_it_reaches_gc_cancel(engine):
    """gc_set_code: values in {-1, 0, +1} only - why the `wide` rig's table is ternary and not full-range int8."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import _lib as L
    tab = np.array([1, -1, 0, 127, -127, 2, 1, -1, 1], dtype=np.int8)
    with pytest.raises(P.GnssCorrError) as e:
        engine.set_channel(90, [tab])
    assert e.value.status == L.GC_E_INVALID
    engine.set_channel(90, [np.clip(tab, -1, 1)])


@pytest.mark.parametrize("fmt", list(E.FORMATS))
@pytest.mark.parametrize("name", E.RIGS)
def test_edge_calls_match_the_model(engine, dst_engine, name, fmt):
    from cu_sdr_collection_amd import _lib as L
    dtype, layout = E.FORMATS[fmt]
    rig = E.make_rig(name)
    sw = E.CancelSweep(rig, fmt).build()
    sw.check_caps()
    n = sw.counts()
    raw, chans = E.make_record(fmt), rig.model_chans()
    x = _per_sample(raw, layout)
    rig.setup(engine)
    engine.load_if(raw, layout=layout, fs=FS)
    compared, refused, left_out, worst, zero_e = 0, 0, 0, [0.0], 0
    try:
        for label, call in sw.calls:
            blocks, reps = E.blocks_of(engine, call), {}
            for amp in (None, E.amplitudes(sw, call, dtype, 1000 + compared)):
                for mode in ("subtract", "model"):
                    tag = f"{name} {fmt} {label} amp={'given' if amp is not None else 'projected'} {mode}"
                    want, used, P_, E_, sx, near, covered = M.cancel(raw, dtype, layout, call, chans, FS, amp=amp, mode=mode, reps=reps)
                    assert int(near.sum()) <= MAX_LEFT_OUT, (tag, int(near.sum()))
                    left_out = max(left_out, int(near.sum()))
                    got, a_out = _out_of_place(engine, dst_engine, raw, dtype, layout, blocks, amp, mode)
                    _check_bytes(tag, call, got, want, near, layout)
                    g = _per_sample(got, layout)
                    assert np.array_equal(g[~covered], x[~covered] if mode == "subtract" else np.zeros_like(x[~covered])), tag
                    if amp is None:
                        _check_amp(tag, call, a_out, used, E_, _weights(raw, layout, call, reps), worst)
                        if mode == "subtract":
                            zero_e += sum(1 for k, c in enumerate(call) if not E_[k, :len(rig.chans[c["chan"]].tables)].all())
                    else:
                        assert np.array_equal(a_out, amp), tag
            compared += len(call)
        assert engine.read_if(0, NS, dtype=dtype, layout=layout).tobytes() == raw.tobytes()          # the source stays as it was
        # (e) every refused descriptor alone: the predicted status, nothing written
        lib = L.load()
        sentinel = np.full_like(raw, 85)
        dst_engine.load_if(sentinel, layout=layout)
        for case in sw.refused:
            assert _refused(engine, dst_engine, lib, case) == getattr(L, E.STATUS[case["refuse"]]), (case["refuse"], _say(case))
            refused += 1
        assert dst_engine.read_if(0, NS, dtype=dtype, layout=layout).tobytes() == sentinel.tobytes()
    finally:
        rig.clear_windows(engine)
    if name == "wide":
        assert zero_e >= 5                                  # blocks on zero entries: E == 0 and the amplitude exactly 0
    generated = len(sw.cases)
    assert compared == n["inside"] and refused == n["refused"] and generated == compared + refused + n["outside"], (generated, compared, refused, n)
    print(f"\n[cancel edges] {name} {fmt}: generated {generated} = compared {compared} + refused {refused} + outside {n['outside']} in "
          f"{len(sw.calls)} calls; worst |dP| / bound {worst[0]:.3g}; at most {left_out} of {NS} samples within 1e-9 of a half-integer")


@pytest.mark.parametrize("fmt", list(E.FORMATS))
@pytest.mark.parametrize("name", E.RIGS)
def test_identities_byte_for_byte(engine, dst_engine, share_engine, name, fmt):
    dtype, layout = E.FORMATS[fmt]
    rig = E.make_rig(name)
    sw = E.CancelSweep(rig, fmt).build()
    raw = E.make_record(fmt)
    rig.setup(engine)
    rng = np.random.default_rng(31 + rig.seed)

    def in_place(blocks, amp, mode, via=None):
        engine.load_if(raw, layout=layout, fs=FS)
        if via is not None:
            via.share_if(engine)
        used = engine.cancel(blocks, dst=via, amp=amp, mode=mode)
        out = engine.read_if(0, NS, dtype=dtype, layout=layout)
        return out, used

    try:
        calls = dict(sw.calls)
        picked = ["packed0", "packed1", "chan64", "tiny4100", "tiny3000+big"]
        for j, label in enumerate(picked):
            call = calls[label]
            blocks = E.blocks_of(engine, call)
            for amp, mode in ((None, "subtract"), (E.amplitudes(sw, call, dtype, 50 + j), ("model", "subtract")[j % 2])):
                tag = (name, fmt, label, amp is None, mode)
                engine.load_if(raw, layout=layout, fs=FS)
                first, a_first = _out_of_place(engine, dst_engine, raw, dtype, layout, blocks, amp, mode)
                again, a_again = _out_of_place(engine, dst_engine, raw, dtype, layout, blocks, amp, mode)
                assert first.tobytes() == again.tobytes() and a_first.tobytes() == a_again.tobytes(), (tag, "a second run")
                assert first.tobytes() != raw.tobytes()
                inp, a_inp = in_place(blocks, amp, mode)
                assert inp.tobytes() == first.tobytes() and a_inp.tobytes() == a_first.tobytes(), (tag, "in place")
                shared, a_shared = in_place(blocks, amp, mode, via=share_engine)
                assert shared.tobytes() == first.tobytes() and a_shared.tobytes() == a_first.tobytes(), (tag, "a dst that shares src's record")
                perm = sw.shuffled[label] if label in sw.shuffled else [int(i) for i in rng.permutation(len(call))]
                engine.load_if(raw, layout=layout, fs=FS)
                mixed, a_mixed = _out_of_place(engine, dst_engine, raw, dtype, layout, E.blocks_of(engine, [call[i] for i in perm]),
                                               None if amp is None else amp[perm], mode)
                assert mixed.tobytes() == first.tobytes() and a_mixed.tobytes() == a_first[perm].tobytes(), (tag, "shuffled")
            # a block alone: its amplitude as inside its call, its bytes as inside the call's blocks that do not touch its samples
            if label.startswith("packed"):
                engine.load_if(raw, layout=layout, fs=FS)
                whole, a_whole = _out_of_place(engine, dst_engine, raw, dtype, layout, blocks, None, "subtract")
                for k in sorted({0, len(call) - 1} | {int(i) for i in rng.choice(len(call), size=10, replace=False)}):
                    c = call[k]
                    lo, hi = c["s0"], c["s0"] + c["n"]
                    alone, a_alone = _out_of_place(engine, dst_engine, raw, dtype, layout, E.blocks_of(engine, [c]), None, "subtract")
                    assert a_alone[0].tobytes() == a_whole[k].tobytes(), (name, fmt, label, "alone", _say(c))
                    others = [d for d in call if d is not c and (d["s0"] + d["n"] <= lo or d["s0"] >= hi)]
                    assert len(others) >= len(call) // 4 or c["n"] > NS // 2
                    longer = others[:len(others) // 2] + [c] + others[len(others) // 2:]
                    inside, a_inside = _out_of_place(engine, dst_engine, raw, dtype, layout, E.blocks_of(engine, longer), None, "subtract")
                    assert _per_sample(alone, layout)[lo:hi].tobytes() == _per_sample(inside, layout)[lo:hi].tobytes(), (name, fmt, label, _say(c))
                    assert a_inside[len(others) // 2].tobytes() == a_alone[0].tobytes()
    finally:
        rig.clear_windows(engine)


@pytest.mark.parametrize("fmt", list(E.FORMATS))
def test_the_exact_class_matches_byte_for_byte_with_nothing_left_out(engine, dst_engine, fmt):
    """Ties round to even, clamps at both ends of the dtype, both modes; tests/test_cancel_edges_cpu.py counts them (thousands of
    each per format and mode).  A quantise that rounded halves away from zero fails here on every format."""
    dtype, layout = E.FORMATS[fmt]
    rig = E.make_rig(("l1ca", "wide")[list(E.FORMATS).index(fmt) % 2])
    blocks_, amp = E.exact_call(rig, fmt)
    raw, chans = E.make_record(fmt), rig.model_chans()
    rig.setup(engine)
    engine.load_if(raw, layout=layout, fs=FS)
    try:
        blocks, reps = E.blocks_of(engine, blocks_), {}
        for given in (amp, None):
            for mode in ("subtract", "model"):
                want, used, P_, E_, sx, near, covered = M.cancel(raw, dtype, layout, blocks_, chans, FS, amp=given, mode=mode, reps=reps)
                got, a_out = _out_of_place(engine, dst_engine, raw, dtype, layout, blocks, given, mode)
                differ = np.flatnonzero(np.any(_per_sample(got, layout) != _per_sample(want, layout), axis=1))
                assert differ.shape[0] == 0, (fmt, mode, given is None, differ.shape[0], int(differ[0]), _per_sample(got, layout)[differ[0]],
                                              _per_sample(want, layout)[differ[0]])
                assert a_out.tobytes() == used.tobytes(), (fmt, mode, "amp_out is not bitwise the model's")
                if given is None:
                    assert np.array_equal(P_.real, np.rint(P_.real)) and np.array_equal(P_.imag, np.rint(P_.imag))      # P an exact integer
    finally:
        rig.clear_windows(engine)


@pytest.mark.parametrize("name", E.RIGS)
def test_projections_agree_with_the_float64_correlators_prompt_sums(engine, dst_engine, name):
    """amp_out * E against gc_correlate under GC_PREC_F64 with el_spacing = 0: both build the replica from csrc/replica_f64.h, only the
    order of additions differs - within twice the bound of the sweep.  Channels without a code window, blocks without a table offset
    (what the float64 correlator is run on elsewhere); each rig on another format."""
    fmt = list(E.FORMATS)[(2 * E.RIGS.index(name)) % 6 + (E.RIGS.index(name) // 3)]
    dtype, layout = E.FORMATS[fmt]
    rig = E.make_rig(name)
    sw = E.CancelSweep(rig, fmt).build()
    raw, chans = E.make_record(fmt), rig.model_chans()
    rig.setup(engine)
    engine.load_if(raw, layout=layout, fs=FS)
    total, worst = 0, 0.0
    try:
        for label, call in sw.calls:
            if not label.startswith("packed") and label != "chan64":
                continue
            reps = {}
            _, used, P_, E_, sx, _, _ = M.cancel(raw, dtype, layout, call, chans, FS, reps=reps)
            w = _weights(raw, layout, call, reps)
            _, a_out = _out_of_place(engine, dst_engine, raw, dtype, layout, E.blocks_of(engine, call), None, "subtract")
            keep = [k for k, c in enumerate(call) if not c["off"] and rig.windows[c["chan"]] is None]
            engine.set_precision("double")
            try:
                sums = engine.correlate(E.blocks_of(engine, [dict(call[k], d=0.0) for k in keep]))
            finally:
                engine.set_precision("single")
            for q, k in enumerate(keep):
                c = call[k]
                for a in range(len(rig.chans[c["chan"]].tables)):
                    prompt = sums[q, a, 2] + 1j * sums[q, a, 3]
                    assert np.array_equal(sums[q, a, 0:2], sums[q, a, 2:4]) and np.array_equal(sums[q, a, 4:6], sums[q, a, 2:4])
                    bound = 2 * (c["n"] + 8) * EPS * w[k, a]
                    dev = abs(a_out[k, a] * E_[k, a] - prompt)
                    assert dev <= bound, (name, fmt, label, a, dev, bound, _say(c))
                    if bound > 0:
                        worst = max(worst, dev / bound)
                total += 1
    finally:
        rig.clear_windows(engine)
    assert total >= 500
    print(f"\n[cancel edges] {name} {fmt}: amp_out * E against the float64 correlator on {total} blocks, worst deviation / (2 x bound) {worst:.3g}")
