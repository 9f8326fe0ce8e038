"""tests/loop_epochs.py proves itself without a GPU: what tests/test_gpu_loop_epochs.py relies on when it holds every epoch of the
closed loops to the float64 oracle of its own block.

  self-consistency   the oracle fed its own sums through the hook: records bit-identical to the plain run (so correlate=None and the
                     hooked loops - tracking_l2c's new hook and the ready-folded pilot of pilot_combine 4 / 5 included - are one
                     loop), state difference exactly 0, sums within 1e-6 of the bound (exactly 0 where the Python correlate_block
                     serves both runs; oracle/gnss_oracle.c adds the same products in another order)
  reference fixtures the hook fed the sums the REFERENCE'S OWN tracking.m recorded (tests/golden/ref_track_<scene>.npz; pilot sums
                     the reference computes and drops taken from the oracle's plain run, as test_loop_closure_cpu.py does):
                     the state equals the fixture's at 1e-10 - all 16 scenes, the folding ones too
  mutations          a loop whose correlator is wrong in one epoch, and records changed in one place, are reported at exactly
                     that epoch, channel and field, and nowhere else"""
import copy
import os

import numpy as np
import pytest

import loop_epochs as LE
import ref_scenes as RS
from oracle import gnss_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_FIELDS = RS.TRACK_FIELDS + RS.PILOT_FIELDS
_PLAIN = {}


def _plain(sc):
    """(S, rec, layout, ch, the oracle's plain run) of a scene, computed once."""
    if sc.name not in _PLAIN:
        import cu_sdr_collection_amd as P
        S, rec, layout, ch = RS.scene_inputs(P, sc)
        _PLAIN[sc.name] = (S, rec, layout, ch, sc.oracle(O, rec, ch, S))
    return _PLAIN[sc.name]


@pytest.mark.parametrize("sc", RS.TRACK_SCENES, ids=[s.name for s in RS.TRACK_SCENES])
def test_the_oracle_fed_its_own_sums_is_the_plain_oracle(sc):
    assert sc.oracle is not None
    S, rec, layout, ch, plain = _plain(sc)
    res = LE.check(sc, rec, layout, ch, S, plain)
    print(f"\n[loop epochs] {sc.name} self: {LE.describe(res)}")
    assert res.failures == []
    assert res.compared == sum(len(t.carrFreq) for t in plain if t.status != "-") > 0
    for k, (a, b) in enumerate(zip(plain, res.oracle)):
        assert a.status == b.status and a.PRN == b.PRN
        for f in _FIELDS:
            if hasattr(a, f):
                assert np.array_equal(getattr(a, f), getattr(b, f)), (sc.name, k, f)
    assert res.worst_sum[0] <= 1e-6 and res.worst_state[0] == 0.0, (res.worst_sum, res.worst_state)
    for c, st in res.state_ratio.items():
        assert not st["absoluteSample"].any()


@pytest.mark.parametrize("sc", RS.TRACK_SCENES, ids=[s.name for s in RS.TRACK_SCENES])
def test_the_oracle_fed_the_references_sums_reaches_the_references_state(sc):
    S, rec, layout, ch, plain = _plain(sc)
    z = np.load(os.path.join(GOLD, f"ref_track_{sc.name}.npz"))
    assert RS.crc(rec) == int(z["record_crc32"][0])
    tr, filled = [], set()
    for k in range(len(ch)):
        t = copy.deepcopy(plain[k])
        t.status = str(z["status"][k])
        for f in _FIELDS:
            if "f_" + f in z.files:
                setattr(t, f, np.array(z["f_" + f][k], dtype=np.float64))
            elif hasattr(t, f):
                filled.add(f)                  # computed and dropped by the reference: the float64 oracle's
        tr.append(t)
    assert filled <= set(RS.PILOT_FIELDS), filled
    res = LE.check(sc, rec, layout, ch, S, tr)
    print(f"\n[loop epochs] {sc.name} reference: {LE.describe(res)}; from the oracle: {sorted(filled)}")
    assert res.compared == sum(len(t.carrFreq) for t in tr if t.status != "-") > 0
    assert res.failures == []


# ---- mutations, on the GPS L1 C/A scene ------------------------------------------------------------------------------------------
_SC = RS.TRACK_SCENES[0]
_AT = (1, 37)        # channel, epoch


def _loop_with_a_faulty_correlator(wrong):
    """trackResults of a closed loop whose correlator returns wrong(want, descriptor) at _AT and the float64 sums everywhere else."""
    S, rec, layout, ch, plain = _plain(_SC)
    seen = []

    def feed(c, e, have, want, desc):
        if (c, e) != _AT:
            return want
        seen.append(desc)
        return wrong(want.copy(), desc)
    tr = LE.check(_SC, rec, layout, ch, S, plain, feed=feed).oracle
    assert len(seen) == 1
    return tr, seen[0]


def test_a_loop_with_a_sound_correlator_passes():
    S, rec, layout, ch, _ = _plain(_SC)
    tr, _ = _loop_with_a_faulty_correlator(lambda want, desc: want)
    assert LE.check(_SC, rec, layout, ch, S, tr).failures == []


def test_twice_the_bound_on_one_output_of_one_epoch_is_reported_there():
    S, rec, layout, ch, _ = _plain(_SC)

    def wrong(want, desc):
        want[0, 2] += 4e-6 * desc["scale"]
        return want
    tr, _ = _loop_with_a_faulty_correlator(wrong)
    res = LE.check(_SC, rec, layout, ch, S, tr)
    assert [(k, e, c, f) for k, _, e, c, f in res.failures] == [("sum", _AT[1], _AT[0], "I_P")], res.failures
    assert abs(res.failures[0][1] - 2.0) < 1e-3 and res.worst_sum[1:] == (_AT[1], _AT[0], "I_P")
    assert res.worst_state[0] <= 1.0


def test_one_sample_dropped_from_one_epochs_sums_is_reported_there():
    """What a team-member seam that loses a sample does: one int8 sample is about 1e-5 of sum|x| at 18 000 samples per block."""
    S, rec, layout, ch, _ = _plain(_SC)
    delta = {}

    def wrong(want, desc):
        j = desc["n"] // 2                                   # a sample in the middle of the block
        cut = rec.copy()
        cut[2 * (desc["pos"] + j):2 * (desc["pos"] + j) + 2] = 0
        less, _, _ = O.correlate_block(O.raw_from_if(cut, desc["pos"], desc["n"]), desc["tables"], desc["rem"], desc["step"], desc["d"],
                                       desc["carr_freq"], desc["rem_carr"], S.samplingFreq, S.codeLength)
        delta["v"] = np.abs(less - want).reshape(-1) / (LE.TOL * desc["scale"])
        return less
    tr, _ = _loop_with_a_faulty_correlator(wrong)
    res = LE.check(_SC, rec, layout, ch, S, tr)
    expect = [("sum", _AT[1], _AT[0], LE.SUMS[v]) for v in range(6) if delta["v"][v] > 1.0]
    assert len(expect) >= 3, delta                            # the sample is worth more than the bound on the I or the Q outputs at least
    assert [(k, e, c, f) for k, _, e, c, f in res.failures] == expect, res.failures
    for (_, ratio, _, _, f) in res.failures:
        assert abs(ratio - delta["v"][LE.SUMS.index(f)]) < 1e-3 * ratio


def test_a_changed_state_record_is_reported_there():
    S, rec, layout, ch, plain = _plain(_SC)
    c, e = _AT
    tr = copy.deepcopy(plain)
    tr[c].codeFreq[e] *= 1.0 + 1e-8
    res = LE.check(_SC, rec, layout, ch, S, tr)
    assert [(k, ee, cc, f) for k, _, ee, cc, f in res.failures] == [("state", e, c, "codeFreq")], res.failures
    assert 90.0 < res.failures[0][1] < 110.0 and res.worst_state[1:] == (e, c, "codeFreq")
    tr = copy.deepcopy(plain)
    tr[c].absoluteSample[e] += 1.0
    res = LE.check(_SC, rec, layout, ch, S, tr)
    assert res.failures == [("state", 1.0, e, c, "absoluteSample")], res.failures
