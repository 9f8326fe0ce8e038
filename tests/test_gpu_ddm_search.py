"""gc_correlate_ddm_search (csrc/corr_bank.hip): gc_correlate_ddm_integrate under many hypotheses from one pass over the samples,
every power map's peak picked on the device.

The definition (include/gnsscorr.h) is an identity.  With nused = sum(run_len), hypothesis h is, bit for bit,

    gc_correlate_ddm_integrate(blocks + block_shift[h], nblocks = nused, block_weights + h * nblocks + block_shift[h] (or null),
                               the same taps, bins, run_len, map_len)

and peaks[h][q][arm] is the first maximum of pow[h][q][arm] walked bin-major with the tap fastest (numpy.argmax's first occurrence).
`_windows` makes those nhyp calls; every comparison is of bytes.  The two receiver searches are checked on signals whose answer is
known by construction: a record written here with a ten-chip pattern at a chosen phase, and the data bits of a tracked channel."""
import ctypes as C

import numpy as np
import pytest

from bank_cases import FS, _blocks, ca_table, noise_record  # noqa: F401  (fixtures)
from oracle import gnss_oracle as O

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)
WEIGHT_POOL = np.array([1.0, -1.0, 0.0, 0.5, -2.5])
FREQ_POOL = [0.0, 0.37, -0.37, 250.0, -250.0, 500.0, -500.0, 1e3, -1e3, 1e4, -1e4, 4.5e6, -4.5e6, 125.0, -125.0, 50.0, -50.0]
PARTIAL_BUDGET = 256 << 20     # the library's budget for one sub-batch's partial sums (csrc/bank_plan.h BankBudget::partial_bytes)


def _desc(rng, n, s0, channel=0):
    return dict(channel=channel, n=int(n), s0=int(s0), rem=float(rng.uniform(-0.9, 1.0)), step=(1.023e6 + float(rng.uniform(-5, 5))) / FS,
                f=20e3 + float(rng.uniform(-5e3, 5e3)), phi=float(rng.uniform(-2 * np.pi, 2 * np.pi)))


def _three_arms(ca_table):
    return [ca_table, O.pad_code(O.generate_ca_code(8)).astype(np.int8), O.pad_code(O.generate_ca_code(9)).astype(np.int8)]


def _windows(engine, descs, offsets, freqs, run_len, map_len, shifts, weights):
    """The definition: one gc_correlate_ddm_integrate call per hypothesis on its window.  Returns (coh [nhyp, nruns, ...], pow [nhyp,
    nmaps, ...])."""
    nused = int(sum(run_len))
    nhyp = len(shifts) if shifts is not None else 1 if weights is None else len(weights)
    coh, pw = [], []
    for h in range(nhyp):
        s = 0 if shifts is None else int(shifts[h])
        w = None if weights is None else np.ascontiguousarray(weights[h][s:s + nused])
        c, p = engine.correlate_ddm_integrate(_blocks(engine, descs[s:s + nused]), offsets, freqs, run_len, weights=w, map_len=map_len)
        coh.append(c)
        pw.append(p)
    return np.stack(coh), np.stack(pw)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _first_maxima(pw):
    """The header's walk over every [nfreq, ntaps] plane of pw [..., nfreq, ntaps]: (power, bin, tap) arrays of shape pw.shape[:-2]."""
    flat = pw.reshape(pw.shape[:-2] + (-1,))
    idx = np.argmax(flat, axis=-1)                       # the first occurrence of the maximum
    val = np.take_along_axis(flat, idx[..., None], axis=-1)[..., 0]
    return val, idx // pw.shape[-1], idx % pw.shape[-1]


def _check_peaks(pk, pw):
    val, m, j = _first_maxima(pw)
    assert pk.shape == pw.shape[:-2]
    assert pk["power"].tobytes() == val.tobytes() and np.array_equal(pk["bin"], m) and np.array_equal(pk["tap"], j)


RUNS = [1, 2, 3, 7, 2, 3, 1, 7, 3]                       # 29 blocks
MAPS = [1, 3, 1, 3, 1]


@pytest.mark.parametrize("nhyp,nfreq,ntaps,weighted", [(1, 1, 1, True), (3, 4, 3, True), (20, 5, 33, True), (3, 17, 3, False), (20, 17, 1, True),
                                                       (3, 1, 33, False)])
def test_every_hypothesis_is_the_integrate_call_on_its_window(engine, noise_record, ca_table, nhyp, nfreq, ntaps, weighted):
    """Blocks of every size around the wavefront, the chunk and several chunks at first_sample 0, 1 and 7 on a three-arm channel; runs of
    1, 2, 3 and 7 blocks, maps of 1 and 3 runs; shifts 0, 1 and 7 out of order with repeats; weight rows from +1, -1, 0, 0.5, -2.5 or the
    null pointer.  coh, pow: the bytes of the nhyp integrate calls; peaks: the first maxima of the call's own pow."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, _three_arms(ca_table))
    rng = np.random.default_rng(900 + 100 * nhyp + nfreq)
    descs = [_desc(rng, n, s0) for n in SIZES for s0 in (0, 1, 7)] + [_desc(rng, n, rng.integers(8, 60000 - n)) for n in SIZES[:6]]
    descs = [descs[k] for k in rng.permutation(len(descs))]
    assert sum(RUNS) == 29 and sum(MAPS) == len(RUNS) and len(descs) == 36 == sum(RUNS) + 7
    shifts = [0] if nhyp == 1 else ([7, 0, 1, 7] + [int(x) for x in rng.choice([0, 1, 7], size=16)])[:nhyp]
    assert nhyp < 20 or (sorted(set(shifts)) == [0, 1, 7] and shifts[0] > shifts[1])
    weights = rng.choice(WEIGHT_POOL, size=(nhyp, len(descs))) if weighted else None
    offsets = [float(x) for x in rng.permutation(np.linspace(-2.0, 2.0, 33))[:ntaps]]
    freqs = [float(x) for x in rng.permutation(np.array(FREQ_POOL))[:nfreq]]
    want_coh, want_pow = _windows(engine, descs, offsets, freqs, RUNS, MAPS, shifts, weights)
    coh, pw, pk = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, RUNS, map_len=MAPS, shifts=shifts, weights=weights,
                                              coherent=True)
    assert coh.shape == (nhyp, len(RUNS), 3, nfreq, ntaps) and pw.shape == (nhyp, len(MAPS), 3, nfreq, ntaps)
    assert np.abs(want_coh).max() > 0 and want_pow.max() > 0
    assert _same(coh, want_coh) and _same(pw, want_pow)
    _check_peaks(pk, pw)


def test_one_hypothesis_without_shift_and_weights_is_the_integrate_call(engine, noise_record, ca_table):
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, _three_arms(ca_table))
    rng = np.random.default_rng(41)
    descs = [_desc(rng, SIZES[k % len(SIZES)], (0, 1, 7)[k % 3]) for k in range(sum(RUNS))]
    offsets, freqs = [0.0, 0.5, -0.5], [0.0, 250.0, -250.0, 0.37]
    want_coh, want_pow = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, freqs, RUNS, map_len=MAPS)
    coh, pw, pk = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, RUNS, map_len=MAPS, coherent=True)
    assert _same(coh[0], want_coh) and _same(pw[0], want_pow) and coh.shape[0] == 1
    _check_peaks(pk, pw)
    only, none, nopk = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, RUNS, map_len=None, coherent=True, power=False,
                                                   peaks=False)
    assert none is None and nopk is None and _same(only, coh)             # without maps: the same coherent bytes


def test_a_one_arm_and_a_three_arm_channel_in_different_runs(engine, noise_record, ca_table):
    """Shift 0, three weight rows: the runs alternate between a one-arm and a three-arm channel.  The one-arm runs' other arms are zero,
    and a map made of one-arm runs alone has the peak {0.0, 0, 0} there."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, [ca_table])
    engine.set_channel(1, _three_arms(ca_table))
    rng = np.random.default_rng(42)
    run_len, chans = [2, 3, 1, 7, 3, 2], [0, 1, 0, 1, 0, 0]
    descs = [_desc(rng, SIZES[(3 * k + i) % len(SIZES)], (0, 1, 7)[(k + i) % 3], channel=c) for k, (L, c) in enumerate(zip(run_len, chans))
             for i in range(L)]
    map_len = [1, 3, 2]                                                   # map 0: one-arm; map 1: mixed; map 2: one-arm
    weights = rng.choice(WEIGHT_POOL[:2], size=(3, len(descs)))
    offsets, freqs = [0.25, 0.0, -0.25], [50.0, 0.0, -50.0, 1e3, 0.37]
    want_coh, want_pow = _windows(engine, descs, offsets, freqs, run_len, map_len, None, weights)
    coh, pw, pk = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, run_len, map_len=map_len, weights=weights, coherent=True)
    assert _same(coh, want_coh) and _same(pw, want_pow)
    _check_peaks(pk, pw)
    for q in (0, 2):
        assert not pw[:, q, 1:].any()
        for name in ("power", "bin", "tap"):
            assert not pk[name][:, q, 1:].any()
    assert pw[:, 1].min() > 0 and pk["power"][:, :, 0].min() > 0


def test_exact_ties_report_the_smallest_index(engine, noise_record, ca_table):
    """A 64 x 64 plane whose 21 distinct bins and 13 distinct taps are repeated along both axes: by the DDM's definition a cell does
    not depend on the other bins or taps, so the cell (m, j) has bit-equal twins at (m + 21a, j + 13b) - in other rows, other
    wavefronts (21 is odd: the rows of the twins fall to other waves of the reduction) and other lanes.  The maximum therefore occurs
    several times and the first occurrence must be reported.  The lists reversed put the first occurrence elsewhere.  peaks alone -
    neither maps nor coherent sums asked for - gives the same records."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, _three_arms(ca_table))
    rng = np.random.default_rng(43)
    descs = [_desc(rng, n, s0) for n, s0 in zip((2049, 1025, 4097, 65, 1023, 1024), (0, 1, 7, 300, 20001, 7))]
    run_len, map_len = [2, 1, 3], [1, 2]
    weights = rng.choice(WEIGHT_POOL, size=(3, len(descs)))
    f21 = [float(x) for x in rng.permutation(np.linspace(-500.0, 500.0, 21))]
    o13 = [float(x) for x in rng.permutation(np.linspace(-1.5, 1.5, 13))]
    for freqs, offsets in (((f21 * 4)[:64], (o13 * 5)[:64]), ((f21 * 4)[:64][::-1], (o13 * 5)[:64][::-1])):
        _, pw, pk = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, run_len, map_len=map_len, weights=weights)
        assert pw.shape == (3, 2, 3, 64, 64)
        _check_peaks(pk, pw)
        for h in range(3):
            for q in range(2):
                for arm in range(3):
                    plane, p = pw[h, q, arm], pk[h, q, arm]
                    twins = np.argwhere(plane == p["power"])
                    fs_, os_ = np.asarray(freqs), np.asarray(offsets)
                    same_cell = [(m, j) for m, j in twins if fs_[m] == fs_[p["bin"]] and os_[j] == os_[p["tap"]]]
                    assert len(same_cell) >= 6, (h, q, arm, len(same_cell))                # the twins the construction promises
                    assert len({m % 4 for m, _ in same_cell}) > 1 and len({j for _, j in same_cell}) > 1
                    assert (int(p["bin"]), int(p["tap"])) == min(same_cell)                 # bin-major: the smallest linear index
        none_c, none_p, alone = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, run_len, map_len=map_len, weights=weights,
                                                            power=False)
        assert none_c is None and none_p is None and alone.tobytes() == pk.tobytes()


def test_independence_and_reproducibility(engine, noise_record, ca_table):
    """A hypothesis's bytes alone, among others, in another position, and with unrelated blocks appended outside its window; the call
    twice."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, _three_arms(ca_table))
    engine.set_channel(1, [ca_table])
    rng = np.random.default_rng(44)
    descs = [_desc(rng, SIZES[(7 * k) % len(SIZES)], int(rng.integers(0, 50000))) for k in range(sum(RUNS) + 7)]
    nb = len(descs)
    offsets, freqs = [j / 4 for j in range(-4, 5)], [125.0 * m for m in range(-2, 3)]
    shifts = [7, 0, 1, 7, 1]
    weights = rng.choice(WEIGHT_POOL, size=(5, nb))
    kw = dict(map_len=MAPS, coherent=True)
    coh, pw, pk = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, RUNS, shifts=shifts, weights=weights, **kw)
    again = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, RUNS, shifts=shifts, weights=weights, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((coh, pw, pk), again))
    for h in range(5):                                                    # alone
        one = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, RUNS, shifts=[shifts[h]], weights=weights[h:h + 1], **kw)
        assert all(a[0].tobytes() == b[h].tobytes() for a, b in zip(one, (coh, pw, pk))), h
    order = [3, 4, 0, 2, 1, 0]                                            # another position, one of them twice
    perm = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, RUNS, shifts=[shifts[h] for h in order], weights=weights[order], **kw)
    for k, h in enumerate(order):
        assert all(a[k].tobytes() == b[h].tobytes() for a, b in zip(perm, (coh, pw, pk))), (k, h)
    extra = [_desc(rng, 777, int(rng.integers(0, 50000)), channel=1) for _ in range(5)]     # another channel, outside every window
    wide = np.concatenate([weights, rng.choice(WEIGHT_POOL, size=(5, len(extra)))], axis=1)
    more = engine.correlate_ddm_search(_blocks(engine, descs + extra), offsets, freqs, RUNS, shifts=shifts, weights=wide, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(more, (coh, pw, pk)))


def test_sub_batch_seams_do_not_show(engine, noise_record, ca_table):
    """The seam shape of the integrate tests: 3 arms x 64 taps x 64 bins, 300 blocks of five chunks against the 1 365-chunk budget: the
    first sub-batch ends after 273 blocks.  Hypotheses at shifts 0, 1 and 7 (and 3) with 41 runs of 7 in maps of 20 and 21 runs: the cut
    falls 0, 6, 0 and 4 blocks into a run of theirs and inside a map of each; the blocks of a sub-batch are integrated in tiles of
    fewer blocks than a sub-batch, which cuts further runs of every hypothesis.  The bytes are those of the integrate calls on the
    windows, and again with the block order reversed."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, _three_arms(ca_table))
    n, nb = 4097, 300
    chunk_bytes = 3 * 64 * 64 * 16
    seam = (PARTIAL_BUDGET // chunk_bytes) // (-(-n // 1024))
    assert chunk_bytes == 196608 and seam == 273 < nb
    shifts, run_len, map_len = [0, 1, 7, 3], [7] * 41, [20, 21]
    assert [(seam - s) % 7 for s in shifts] == [0, 6, 0, 4] and max(shifts) + sum(run_len) <= nb
    assert all(s + 7 * 20 < seam < s + 7 * 41 for s in shifts)            # inside the second map of every hypothesis
    rng = np.random.default_rng(66)
    rem, s0, f = rng.uniform(0, 1, nb), rng.integers(0, 60000 - n, nb), rng.uniform(-3e4, 3e4, nb)
    descs = [dict(n=n, s0=int(s0[k]), rem=float(rem[k]), step=1.023e6 / FS, f=float(f[k]), phi=0.3) for k in range(nb)]
    weights = rng.choice(np.array([1.0, -1.0, 0.5]), size=(4, nb))
    offsets = [float(x) for x in np.linspace(-3.0, 3.0, 64)]
    freqs = [float(x) for x in np.linspace(-1575.0, 1575.0, 64)]
    for order in (slice(None), slice(None, None, -1)):
        d, w = descs[order], np.ascontiguousarray(weights[:, order])
        want_coh, want_pow = _windows(engine, d, offsets, freqs, run_len, map_len, shifts, w)
        coh, pw, pk = engine.correlate_ddm_search(_blocks(engine, d), offsets, freqs, run_len, map_len=map_len, shifts=shifts, weights=w,
                                                  coherent=True)
        assert np.abs(want_coh).min() > 0
        assert _same(coh, want_coh) and _same(pw, want_pow)
        _check_peaks(pk, pw)


def test_refusals_leave_all_three_outputs_untouched(engine, noise_record, ca_table):
    import cu_sdr_collection_amd as P
    L = P._lib
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, [ca_table])
    engine.set_channel(1, [ca_table])
    engine.set_channel(5, [ca_table], windows=[512])
    broken = ca_table.copy()
    broken[0] = -broken[0]                                   # [c(end) c c(1)] with a wrong first pad
    engine.set_channel(6, [broken])
    good = dict(channel=0, n=2049, s0=3, rem=0.2, step=1.023e6 / FS, f=2e4, phi=0.1)
    six = [good, dict(good, s0=20000), dict(good, s0=40000), dict(good, s0=100), dict(good, s0=30000), dict(good, s0=7)]
    dp = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda x: None if x is None else np.asarray(x, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731

    def call(descs=six, nhyp=2, shifts=(0, 2), weights=None, offsets=(0.0, 0.5), freqs=(0.0, 50.0), run_len=(2, 2), map_len=(1, 1), nruns=None,
             nmaps=None, want=(True, True, True)):
        off, frq = np.asarray(offsets, dtype=np.float64), np.asarray(freqs, dtype=np.float64)
        runs, maps = np.asarray(run_len, dtype=np.int32), np.asarray(map_len, dtype=np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        coh = np.full((4, 8, 3, max(len(frq), 1), max(len(off), 1), 2), 12345.0)
        pw = np.full((4, 8, 3, max(len(frq), 1), max(len(off), 1)), 12345.0)
        pk = np.zeros((4, 8, 3), dtype=L.DDM_PEAK_DTYPE)
        pk["power"], pk["bin"], pk["tap"] = 12345.0, 77, 88
        rc = engine._lib.gc_correlate_ddm_search(engine._ctx, len(descs), _blocks(engine, descs), nhyp, ip(shifts), dp(w), len(off), dp(off),
                                                 len(frq), dp(frq), len(runs) if nruns is None else nruns, ip(runs),
                                                 len(maps) if nmaps is None else nmaps, ip(maps), dp(coh) if want[0] else None,
                                                 dp(pw) if want[1] else None, pk.ctypes.data_as(C.POINTER(L.gc_ddm_peak)) if want[2] else None)
        assert np.all(coh == 12345.0) and np.all(pw == 12345.0), "a refused call must not write its outputs"
        assert np.all(pk["power"] == 12345.0) and np.all(pk["bin"] == 77) and np.all(pk["tap"] == 88)
        return rc

    ones = np.ones((2, 6))
    # what this function adds
    assert call(nhyp=0) == L.GC_E_INVALID
    assert call(nhyp=L.GC_DDM_MAX_HYP + 1, shifts=[0] * (L.GC_DDM_MAX_HYP + 1)) == L.GC_E_INVALID
    assert call(shifts=(0, -1)) == L.GC_E_INVALID                                    # a negative shift
    assert call(shifts=(0, 3)) == L.GC_E_INVALID                                     # 3 + 4 > 6
    assert call(nruns=0, nmaps=0, want=(True, False, False)) == L.GC_E_INVALID       # blocks present, no runs
    assert call(run_len=(4, 0)) == L.GC_E_INVALID                                    # a run of no blocks
    assert call(run_len=(5, -1)) == L.GC_E_INVALID
    assert call(run_len=(5, 2)) == L.GC_E_INVALID                                    # more than the blocks
    assert call(map_len=(2, 0)) == L.GC_E_INVALID                                    # a map of no runs
    assert call(map_len=(1,)) == L.GC_E_INVALID                                      # the maps do not sum to the runs
    assert call(map_len=(1, 2)) == L.GC_E_INVALID
    assert call(nmaps=-1) == L.GC_E_INVALID
    mixed = six[:2] + [dict(six[2], channel=1), dict(six[3], channel=1)] + [dict(d, channel=1) for d in six[4:]]
    assert call(descs=mixed, shifts=(0, 1)) == L.GC_E_INVALID                        # two channels in a run of the window at shift 1 only
    for bad in (float("nan"), float("inf"), float("-inf")):
        w = ones.copy()
        w[0, 5] = bad                                                                # outside hypothesis 0's window: any entry counts
        assert call(weights=w) == L.GC_E_INVALID
    assert call(map_len=(), want=(True, True, False)) == L.GC_E_INVALID              # pow without a map
    assert call(map_len=(), want=(True, False, True)) == L.GC_E_INVALID              # peaks without a map
    assert call(want=(False, False, False)) == L.GC_E_INVALID                        # no output at all
    assert call(map_len=(), want=(False, False, False)) == L.GC_E_INVALID
    # one each of what gc_correlate_ddm_integrate refuses through the bank's check, over the whole list, with its status
    assert call(freqs=(0.0, float("nan"))) == L.GC_E_INVALID
    assert call(offsets=np.zeros(65)) == L.GC_E_INVALID
    assert call(descs=[dict(d, channel=5) for d in six]) == L.GC_E_UNSUPPORTED       # windowed channel
    assert call(descs=[dict(d, channel=6) for d in six]) == L.GC_E_INVALID           # broken pads
    assert call(descs=six[:5] + [dict(good, s0=60000 - 2048)], shifts=(0, 1)) == L.GC_E_RANGE   # a block outside every window counts too
    assert call(descs=[dict(d, channel=200) for d in six]) == L.GC_E_STATE
    engine.set_precision("double")
    try:
        assert call() == L.GC_E_UNSUPPORTED
    finally:
        engine.set_precision("single")
    # and the same arguments are accepted
    coh, pw, pk = engine.correlate_ddm_search(_blocks(engine, six), [0.0, 0.5], [0.0, 50.0], [2, 2], map_len=[1, 1], shifts=[0, 2], coherent=True)
    assert coh.shape == (2, 2, 3, 2, 2) and pw.shape == (2, 2, 3, 2, 2) and pk.shape == (2, 2, 3)
    assert np.abs(coh[:, :, 0]).min() > 0 and not coh[:, :, 1:].any() and pk["power"][:, :, 0].min() > 0
    assert _same(coh[0, 1], coh[1, 0]) and _same(pw[0, 1], pw[1, 0])                 # blocks 2, 3: run 1 at shift 0, run 0 at shift 2
    ok, _, _ = engine.correlate_ddm_search(_blocks(engine, mixed), [0.0], [0.0], [2, 2], shifts=[0, 2], coherent=True, power=False, peaks=False)
    assert ok.shape == (2, 2, 3, 1, 1)                                               # one channel per run of every window


def test_an_empty_call_is_no_error_even_before_a_record_is_loaded():
    import cu_sdr_collection_amd as P
    with P.Engine(0) as fresh:
        coh, pw, pk = fresh.correlate_ddm_search(fresh.make_blocks(0), [0.0, 0.5], [0.0, 1.0, 2.0], [], coherent=True)
        assert coh.shape == (1, 0, 3, 3, 2) and pw.shape == (1, 0, 3, 3, 2) and pk.shape == (1, 0, 3)
        with pytest.raises(P.GnssCorrError) as e:
            fresh.correlate_ddm_search(fresh.make_blocks(0), [0.0], [float("nan")], [], coherent=True)
        assert e.value.status == P._lib.GC_E_INVALID
        with pytest.raises(P.GnssCorrError) as e:
            fresh.correlate_ddm_search(fresh.make_blocks(0), [0.0], [0.0], [1], coherent=True)     # a run without blocks
        assert e.value.status == P._lib.GC_E_INVALID
        with pytest.raises(P.GnssCorrError) as e:
            fresh.correlate_ddm_search(fresh.make_blocks(0), [0.0], [0.0], [])                       # nothing asked for that could exist
        assert e.value.status == P._lib.GC_E_INVALID


NH10 = "0000110101"


def test_a_known_secondary_code_phase(engine):
    """A noise-free int8 I/Q record written here: 41 ms at 4 Msps of one GPS C/A code (PRN 7) at 1 250 Hz, code period k multiplied
    by c[(k + h0) % 10], c the NH10 pattern as +-1 and h0 = 6.  The descriptors come from the construction's own code phase and
    Doppler; forty blocks in runs of 10, one map, ten hypotheses whose row h weights block n with c[(n + h) % 10].  Only h0 wipes
    every chip: the winner is h0, its peak at (0 Hz, 0 chips), and the numpy restatement of the definition on gc_correlate_ddm's output
    names the same winner."""
    c = np.array([1.0 if ch == "0" else -1.0 for ch in NH10])
    acf = np.array([float(np.dot(c, np.roll(c, -lag))) for lag in range(10)])
    assert acf[0] == 10.0 and np.all(acf[1:] < 10.0), acf                 # the phase is identifiable: a unique maximum at lag 0
    assert np.all(np.abs(acf[1:]) <= 6.0), acf
    fs, fd, phi0, h0, i0, amp = 4e6, 1250.0, 0.7, 6, 137.25, 90.0
    nsamp = int(0.041 * fs)
    assert nsamp <= int(0.1 * fs)
    code = O.generate_ca_code(7).astype(np.float64)
    step = 1.023e6 / fs
    i = np.arange(nsamp, dtype=np.float64)
    chip = np.floor((i - i0) * step).astype(np.int64)                     # chips since the start of code period 0 (negative before it)
    sec = c[((chip // 1023) + h0) % 10]
    z = amp * code[chip % 1023] * sec * np.exp(1j * (2.0 * np.pi * fd * i / fs + phi0))
    rec = np.empty(2 * nsamp, dtype=np.int8)
    rec[0::2], rec[1::2] = np.rint(z.real).astype(np.int8), np.rint(z.imag).astype(np.int8)
    descs = []
    for k in range(40):
        first = int(np.ceil(i0 + 1023 * k / step))                        # the first sample of code period k
        rem = (first - i0) * step - 1023 * k
        assert 0 <= rem < step
        descs.append(dict(n=int(np.ceil((1023 - rem) / step)), s0=first, rem=float(rem), step=step, f=fd,
                          phi=float(np.mod(2.0 * np.pi * fd * first / fs + phi0, 2.0 * np.pi))))
    assert descs[-1]["s0"] + descs[-1]["n"] <= nsamp
    engine.load_if(rec, fs=fs)
    engine.set_channel(0, [O.pad_code(O.generate_ca_code(7)).astype(np.int8)])
    offsets, freqs = [-0.5, 0.0, 0.5], [-50.0, 0.0, 50.0]
    n = np.arange(40)
    weights = c[(n[None, :] + np.arange(10)[:, None]) % 10]
    D = engine.correlate_ddm(_blocks(engine, descs), offsets, freqs)[:, 0]                 # [40, 3, 3]
    s0 = np.array([d["s0"] for d in descs], dtype=np.float64)
    f = np.asarray(freqs)
    ref = np.zeros((10, 3, 3))
    for h in range(10):
        for r in range(4):
            acc = np.zeros((3, 3), dtype=np.complex128)
            for b in range(10 * r, 10 * r + 10):
                x = (f * (s0[b] - s0[10 * r])) / fs
                acc = acc + weights[h, b] * np.exp(-2j * np.pi * (x - np.rint(x)))[:, None] * D[b]
            ref[h] = ref[h] + (acc.real * acc.real + acc.imag * acc.imag)
    ref_winner = int(np.argmax(ref.reshape(10, -1).max(axis=1)))
    _, pw, pk = engine.correlate_ddm_search(_blocks(engine, descs), offsets, freqs, [10] * 4, weights=weights)
    assert pk.shape == (10, 1, 3) and pw.shape == (10, 1, 3, 3, 3)
    _check_peaks(pk, pw)
    rel = np.abs(pw[:, 0, 0] - ref) / ref.max()
    print(f"search against the numpy restatement: worst |dp| / max p = {rel.max():.2e}; peak power by phase {pk['power'][:, 0, 0]}")
    assert rel.max() < 1e-12                                              # cos / sin against sincospi, 10 + 4 additions: 1e-15 of the peak
    winner = int(np.argmax(pk["power"][:, 0, 0]))
    assert winner == h0 == ref_winner
    assert (int(pk["bin"][h0, 0, 0]), int(pk["tap"][h0, 0, 0])) == (1, 1)
    second = np.sort(pk["power"][:, 0, 0])[-2]
    assert second < 0.5 * pk["power"][h0, 0, 0]                           # |acf| <= 6 off the peak: (6 / 10)^2 of the power at most


def test_a_known_bit_edge_on_a_tracked_channel(engine, l1ca_scene):
    """PRN 17 of the scene, tracked for 100 epochs; receiver.bit_edge_search(period=20) on epochs 20 .. 99 at taps 0, +-1/2 chip and bins
    0, +-25 Hz.  Precondition, asserted: the sign changes of the recorded I_P inside those epochs all fall on one residue modulo 20 and
    there are at least three.  The winning shift is that residue and its peak is at (0 Hz, 0 chips)."""
    import cu_sdr_collection_amd as P
    from types import SimpleNamespace
    S, sats, iq = l1ca_scene
    ms, nch = S.msToProcess, S.numberOfChannels
    sat = [s for s in sats if s.prn == 17][0]
    try:
        S.msToProcess, S.numberOfChannels = 100, 1
        ch = [SimpleNamespace(PRN=sat.prn, acquiredFreq=S.IF + sat.doppler + 4.0, codePhase=int(np.ceil(sat.code_phase_samples)) + 1, status="T")]
        engine.load_if(iq, fs=S.samplingFreq)
        tr, _ = P.tracking(engine, ch, S)
        epochs = np.arange(20, 100)
        peaks, shift = P.bit_edge_search(engine, tr[0], ch[0], S, [-0.5, 0.0, 0.5], [-25.0, 0.0, 25.0], 20, epochs=epochs)
        maps, shift2 = P.bit_edge_search(engine, tr[0], ch[0], S, [-0.5, 0.0, 0.5], [-25.0, 0.0, 25.0], 20, noncoherent=1, epochs=epochs)
    finally:
        S.msToProcess, S.numberOfChannels = ms, nch
    sign = np.asarray(tr[0].I_P, dtype=np.float64)[:100] >= 0
    changes = [e for e in range(21, 100) if sign[e] != sign[e - 1]]
    residues = {(e - 20) % 20 for e in changes}
    print(f"I_P changes sign at epochs {changes}; summed peak power by shift {peaks['power'][:, :, 0].sum(axis=1)}")
    assert len(changes) >= 3 and len(residues) == 1, changes               # the precondition
    assert peaks.shape == (20, 1, 1) and maps.shape == (20, 3, 1)
    assert shift == residues.pop() == shift2
    assert (int(peaks["bin"][shift, 0, 0]), int(peaks["tap"][shift, 0, 0])) == (1, 1)
    assert shift == int(np.argmax(peaks["power"][:, 0, 0]))
