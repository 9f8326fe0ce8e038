"""What gc_acq_shift_search_batch returns - each PRN's row, code phase, peak and second peak - through the real call, against the
float64 model of the reference's rules on the float64 surface (tests/shift_pick_model.py), for the three rules and the three ways a
block length runs: 72 000 (specialised passes with per-tile candidates, two PRN lanes, winning rows transformed again into slots),
18 000 (no specialised shape: rows written, PRN after PRN) and 16 368 (a padded transform).

The scenes are tests/shift_pick_scenes.py's; tests/test_shift_pick_cpu.py shows on the CPU that each is what it claims: a CLEAR scene
has no other candidate within eps of any decided cell, a TIE scene has its contested cells 1e-10 .. eps / 4 apart (about 1e-9) and
everything else of that decision clear of them, in both directions - one of which necessarily goes against the float32 pass.

Present PRNs: row and code_phase equal the model's, peak and second_peak within 1e-9 (relative), the tolerance the suite uses for
guarded values.  The absent PRN of every call: `peak` is the float64 value of the returned cell to 1e-9, and that value is within eps
of the model's maximum.  Tie scenes also report ties >= 1 (gc_acq_guard_stats), and print whether the float32 per-PRN path
(gc_acq_shift_search / gc_acq_shift_row with the rules on its float32 rows) decides otherwise than the model - reported, not asserted."""
import functools

import numpy as np
import pytest

import shift_pick_model as M
import shift_pick_scenes as SC

pytestmark = pytest.mark.gpu

RTOL = 1e-9


@functools.lru_cache(maxsize=None)
def _scene(kind, name):
    return (SC.CLEAR if kind == "clear" else SC.TIES)[name]()


def _search(eng, sc, call):
    from cu_sdr_collection_amd import _lib as L
    if call.conditioned:
        z = call.x.astype(np.complex64)
        assert np.all(z.astype(np.complex128) == call.x)             # integer-valued and below 2^24: nothing is lost
        eng.acq_set_signal(z)
    else:
        iq = np.empty(2 * len(call.x), dtype=np.int8)
        iq[0::2], iq[1::2] = call.x.real, call.x.imag
        eng.load_if(iq, fs=SC.FS)
    nc, ns, nb = sc.geom
    sp = L.gc_acq_shift_params(sampling_freq=SC.FS, carrier_f0=sc.f0, carrier_step=sc.fstep, first_sample=call.first_sample, n=sc.n, n_signals=ns,
                               n_carriers=nc, n_bins=nb, n_arms_max=sc.codes.shape[1], source=1 if call.conditioned else 0)
    eng.acq_shift_prepare(sp)
    picks = eng.acq_shift_search_batch(sc.codes, sc.weights, sc.rule, call.exclude, call.period)
    assert picks is not None
    return sp, picks, eng.acq_guard_stats()


def _check(sc, call, picks, stats, label):
    eps = min(stats["eps"], SC.eps_of(sc.n))
    assert 0.0 < stats["eps"]
    for ip, surf in enumerate(sc.surfaces(call)):
        pk = picks[ip]
        m = M.pick(surf, *sc.geom, sc.rule, call.exclude, call.period)
        got = (pk.row, pk.code_phase, pk.peak, pk.second_peak)
        if ip == sc.absent:
            assert 0 <= pk.row < surf.shape[0] and 0 <= pk.code_phase < sc.n, (label, ip, got)
            cell = surf[pk.row, pk.code_phase]
            assert abs(pk.peak - cell) <= RTOL * cell, (label, ip, got, cell)
            assert cell >= m["peak"] * (1.0 - eps), (label, ip, got, m)
            continue
        assert (pk.row, pk.code_phase) == (m["row"], m["code_phase"]) == call.expect[ip], (label, ip, got, m, call.expect[ip])
        assert abs(pk.peak - m["peak"]) <= RTOL * m["peak"], (label, ip, got, m)
        assert abs(pk.second_peak - m["second_peak"]) <= RTOL * m["second_peak"], (label, ip, got, m)


def _float32_path_differs(eng, sc, call, sp, ip=0):
    """The per-PRN calls with the rules on their float32 rows, as a caller without the batch call decides: True where row, code phase or
    the second peak's column is not the model's."""
    m = M.pick(sc.surfaces(call)[ip], *sc.geom, sc.rule, call.exclude, call.period)
    eng.acq_shift_prepare(sp)
    rmax, rarg = eng.acq_shift_search(sc.codes[ip], sc.weights)
    if sc.rule == M.GLOBAL:
        row = int(np.argmax(rmax))
        return (row, int(rarg[rmax == rmax.max()].min())) != (m["row"], m["code_phase"])
    row = M.sequential_row(rmax, *sc.geom)
    corr = eng.acq_shift_row(row).astype(np.float64)
    cp = int(np.argmax(corr))
    return (row, cp, M.second_peak(corr, cp + 1, call.exclude, call.period)[1]) != (m["row"], m["code_phase"], m["second_col"])


@pytest.mark.parametrize("name", list(SC.CLEAR))
def test_clear_scenes(engine, name):
    """Noise and two strong satellites in an int8 record (the third PRN is absent): over the calls the peak stands at the edges of the
    second-peak window's three range cases, in every period of the row and at its end, and the winner on carrier 0 and 1, signal
    block 1 and 2, bin 0 and the last eligible bin - `peak` to 1e-9 also proves the exact cell's mapping for every kind of row."""
    sc = _scene("clear", name)
    for call in sc.calls:
        _, picks, stats = _search(engine, sc, call)
        _check(sc, call, picks, stats, (name, call.label))


@pytest.mark.parametrize("name", list(SC.TIES))
def test_tie_scenes(engine, name):
    sc = _scene("ties", name)
    moved = []
    for call in sc.calls:
        sp, picks, stats = _search(engine, sc, call)
        _check(sc, call, picks, stats, (name, call.label))
        assert stats["ties"] >= 1, (name, call.label, stats)
        moved.append(_float32_path_differs(engine, sc, call, sp))
    print(f"tie scene {name}: the float32 per-PRN path decides otherwise than float64 in {sum(moved)} of {len(moved)} directions {moved}")


_AT_72000 = [n for n in SC.TIES if n.endswith("-72000")]
_KNOBS = [({"GC_ACQ_ROWMAX_KERNEL": "1"}, _AT_72000), ({"GC_ACQ_GENERIC": "1"}, _AT_72000),          # 72 000 down the written path
          ({"GC_ACQ_SHIFT_LANES": "1"}, _AT_72000), ({"GC_ACQ_SHIFT_LANES": "2"}, _AT_72000),
          ({"GC_ACQ_GUARD_EPS": "0.02"}, _AT_72000),                                                   # everything down the slow path
          ({"GC_ACQ_GUARD_EPS": "0.02"}, [n for n in SC.TIES if n.endswith("-18000")])]


@pytest.mark.tuning
@pytest.mark.parametrize("env,names", _KNOBS, ids=["+".join(f"{k}={v}" for k, v in e.items()) + names[0][names[0].rindex("-"):] for e, names in _KNOBS])
def test_tie_scenes_behind_the_tuning_knobs(monkeypatch, env, names):
    """The tie scenes down the other paths of the batch call: the same answers."""
    import cu_sdr_collection_amd as P
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with P.Engine(0) as eng:                      # a context of its own: the knobs that are read once per scratch see a fresh one
        for name in names:
            sc = _scene("ties", name)
            for call in sc.calls:
                _, picks, stats = _search(eng, sc, call)
                _check(sc, call, picks, stats, (name, call.label, env))
                assert stats["ties"] >= 1, (name, call.label, stats)
                if "GC_ACQ_GUARD_EPS" in env:
                    assert stats["eps"] == 0.02
