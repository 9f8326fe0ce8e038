"""gc_correlate_ddm_integrate (csrc/corr_bank.hip): delay-Doppler maps added coherently over runs of blocks, then as power over runs.

The definition (include/gnsscorr.h) builds on gc_correlate_ddm's cell D[b][arm][m][j], bit for bit.  With b0 the run's first block:

    dn = first_sample[b] - first_sample[b0]      x = (f_m * dn) / fs      u = x - rint(x)      c = cospi(2u), s = sinpi(2u)
    re += w_b * (c * D.re + s * D.im)            im += w_b * (c * D.im - s * D.re)            (block order, from +0.0)
    pow += (re * re + im * im)                                                                 (run order, from +0.0)

`_restate` is that, in numpy, from the library's own gc_correlate_ddm output, with a Python loop over the blocks (np.sum adds pairwise).
x and u are the same bits on both sides; what differs is the two sincospi against numpy's cos / sin of the rounded product 2 pi u, four
products and L additions per component: the bound per cell is (16 + L) * 2^-52 * sum_b |w_b| (|D.re| + |D.im|), L the run length.
Where f_m == 0 the rotation is exactly 1 on both sides, so with weights +-1 the comparison is `==`.

Measured on an MI355X (worst error as a fraction of its bound; every test prints its own): mixed runs 0.043, a tracked channel's
coherent maps 0.041 and power map 0.013; against the float64 per-sample definition of the blocks (bound 2e-6 * sum_b |w_b| sum |x_b|)
0.009."""
import ctypes as C

import numpy as np
import pytest

from bank_cases import FS, PERIOD_L1, POOL, _blocks, _colon_has_n_elements, _raw, ca_table, ddm_reference, noise_record  # noqa: F401  (fixtures)
from oracle import gnss_oracle as O

pytestmark = pytest.mark.gpu
TOL = 2e-6                     # the DDM tests' correlator-versus-definition figure, of sum |x| per block
FREQ_POOL = [0.0, 0.37, -0.37, 250.0, -250.0, 500.0, -500.0, 1e3, -1e3, 1e4, -1e4, 4.5e6, -4.5e6]
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)
PARTIAL_BUDGET = 256 << 20     # the library's budget for one sub-batch's partial sums (csrc/bank_plan.h BankBudget::partial_bytes)
EPS = 2.0 ** -52


def _desc(rng, n, s0, channel=0):
    return dict(channel=channel, n=int(n), s0=int(s0), rem=float(rng.uniform(-0.9, 1.0)), step=(1.023e6 + float(rng.uniform(-5, 5))) / FS,
                f=20e3 + float(rng.uniform(-5e3, 5e3)), phi=float(rng.uniform(-2 * np.pi, 2 * np.pi)))


def _restate(D, s0, freqs, run_len, weights, fs):
    """The definition from the per-block cells D [nblocks, arms, nfreq, ntaps] (complex128).  Returns (coh complex128 [nruns, ...],
    bound float64 [nruns, ...])."""
    f = np.asarray(freqs, dtype=np.float64)
    coh = np.zeros((len(run_len),) + D.shape[1:], dtype=np.complex128)
    bound = np.zeros(coh.shape)
    b0 = 0
    for r, L in enumerate(run_len):
        re, im, mag = np.zeros(D.shape[1:]), np.zeros(D.shape[1:]), np.zeros(D.shape[1:])
        for b in range(b0, b0 + L):
            dn = float(int(s0[b]) - int(s0[b0]))
            x = (f * dn) / fs
            u = x - np.rint(x)
            c, s = np.cos(2.0 * np.pi * u)[None, :, None], np.sin(2.0 * np.pi * u)[None, :, None]
            w = 1.0 if weights is None else float(weights[b])
            re = re + w * (c * D[b].real + s * D[b].imag)
            im = im + w * (c * D[b].imag - s * D[b].real)
            mag = mag + abs(w) * (np.abs(D[b].real) + np.abs(D[b].imag))
        coh[r] = re + 1j * im
        bound[r] = (16 + L) * EPS * mag
        b0 += L
    return coh, bound


def _power(coh, map_len):
    """pow of the definition from coherent cells, runs in order."""
    out = np.zeros((len(map_len),) + coh.shape[1:])
    r0 = 0
    for q, M in enumerate(map_len):
        p = np.zeros(coh.shape[1:])
        for r in range(r0, r0 + M):
            p = p + (coh[r].real * coh[r].real + coh[r].imag * coh[r].imag)
        out[q] = p
        r0 += M
    return out


def _fraction(got, ref, bound):
    """Worst |got - ref| per component as a fraction of the bound; cells whose bound is 0 must agree exactly."""
    dev = np.maximum(np.abs(got.real - ref.real), np.abs(got.imag - ref.imag))
    assert not dev[bound == 0].any()
    return float((dev[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _three_arms(ca_table):
    return [ca_table, O.pad_code(O.generate_ca_code(8)).astype(np.int8), O.pad_code(O.generate_ca_code(9)).astype(np.int8)]


@pytest.mark.parametrize("nfreq", [1, 4, 5, 17])
def test_runs_of_one_block_are_the_ddm(engine, noise_record, ca_table, nfreq):
    """run_len all 1, no weights: the rotation is exp(0) and coh is gc_correlate_ddm's output value for value (`==`: signed zeros may
    differ, 0.0 + -0.0 is +0.0).  Block sizes around the wavefront, the chunk and several chunks at first_sample 0, 1, 7 and scattered."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, [ca_table])
    rng = np.random.default_rng(500 + nfreq)
    descs = [_desc(rng, n, s0) for n in SIZES for s0 in (0, 1, 7)] + [_desc(rng, n, rng.integers(8, 60000 - n)) for n in SIZES]
    fill = list(rng.uniform(-2.0, 2.0, size=33 - len(POOL)))
    for offsets in ([-1.0 / 3], [0.0, 1022.9, -17.25], [float(x) for x in rng.permutation(np.array(POOL + fill))]):
        freqs = [0.0] + [float(x) for x in rng.choice(np.array(FREQ_POOL[1:]), size=nfreq - 1, replace=nfreq - 1 > 12)]
        freqs = [float(x) for x in rng.permutation(np.array(freqs))]
        want = engine.correlate_ddm(_blocks(engine, descs), offsets, freqs)
        coh, pw = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, freqs, [1] * len(descs))
        assert pw is None and coh.shape == want.shape == (len(descs), 3, nfreq, len(offsets)) and coh.dtype == np.complex128
        assert np.array_equal(coh, want), (nfreq, len(offsets))
        assert np.abs(coh[:, 0]).max() > 0 and not coh[:, 1:].any()


def _mixed_call(rng):
    """Runs of 1, 2, 3, 7 and 20 blocks on a one-arm channel (0) and a three-arm channel (1); first_sample inside a run increasing,
    decreasing, repeated and scattered; sizes from SIZES."""
    run_len, descs = [], []
    order = ["up", "down", "same", "scatter"]
    for k, (L, chan) in enumerate([(1, 0), (2, 1), (3, 0), (7, 1), (20, 0), (20, 1), (7, 0), (3, 1), (2, 0), (1, 1), (20, 0), (7, 1)]):
        sizes = [SIZES[(k + 3 * i) % len(SIZES)] for i in range(L)]
        kind = order[k % 4]
        if kind == "up":
            s0 = np.cumsum([int(rng.integers(0, 2500)) for _ in range(L)]) + (0, 1, 7)[k % 3]
        elif kind == "down":
            s0 = (np.cumsum([int(rng.integers(0, 2500)) for _ in range(L)]) + (0, 1, 7)[k % 3])[::-1]
        elif kind == "same":
            s0 = np.full(L, (0, 1, 7, 31234)[k % 4])
        else:
            s0 = rng.integers(0, 60000 - 4097, size=L)
        assert int(np.max(s0)) + 4097 <= 60000
        run_len.append(L)
        descs += [_desc(rng, n, s, channel=chan) for n, s in zip(sizes, s0)]
    return run_len, descs


def test_against_the_definition_restated_from_the_ddm(engine, noise_record, ca_table):
    """One call mixing runs of 1, 2, 3, 7 and 20 blocks, weights from +1, -1, 0, 0.5, -2.5, bins unordered with a duplicate, a three-arm
    channel next to a one-arm channel.  Every cell within (16 + L) 2^-52 sum_b |w_b| (|D.re| + |D.im|) of the restatement; the one-arm
    channel's other arms zero; with weights +-1 the bins at 0 Hz equal the sequential float64 sum of +-D exactly."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, [ca_table])
    engine.set_channel(1, _three_arms(ca_table))
    rng = np.random.default_rng(77)
    run_len, descs = _mixed_call(rng)
    assert sorted(set(run_len)) == [1, 2, 3, 7, 20] and len(descs) == sum(run_len)
    offsets = [0.0, 0.5, -0.5, 17.25, -1022.9]
    freqs = [250.0, -4.5e6, 0.0, 0.37, 1e4, -0.37, 4.5e6, -500.0, 0.0, 1e3, 250.0]
    assert set(freqs) <= set(FREQ_POOL) and len(set(freqs)) < len(freqs)
    s0 = [d["s0"] for d in descs]
    D = engine.correlate_ddm(_blocks(engine, descs), offsets, freqs)
    zero = [m for m, f in enumerate(freqs) if f == 0.0]
    for name, weights in (("mixed", rng.choice(np.array([1.0, -1.0, 0.0, 0.5, -2.5]), size=len(descs))),
                          ("signs", rng.choice(np.array([1.0, -1.0]), size=len(descs))), ("none", None)):
        coh, pw = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, freqs, run_len, weights=weights, map_len=[len(run_len)])
        ref, bound = _restate(D, s0, freqs, run_len, weights, FS)
        assert coh.shape == ref.shape == (len(run_len), 3, len(freqs), len(offsets)) and pw.shape == (1,) + coh.shape[1:]
        frac = _fraction(coh, ref, bound)
        print(f"{name} weights: worst error {frac:.3f} of the bound (16 + L) 2^-52 sum |w| (|D.re| + |D.im|)")
        assert frac <= 1.0, (name, frac)
        b0 = 0
        for r, L in enumerate(run_len):
            if descs[b0]["channel"] == 0:
                assert not coh[r, 1:].any(), r                      # arms the run's channel does not have
            else:
                assert np.abs(coh[r]).min() > 0 or weights is not None, r
            b0 += L
        if name != "mixed":                                          # 0 Hz, weights +-1: the sequential sum of +-D, exactly
            w = np.ones(len(descs)) if weights is None else weights
            b0 = 0
            for r, L in enumerate(run_len):
                acc_re, acc_im = np.zeros(D.shape[1:]), np.zeros(D.shape[1:])
                for b in range(b0, b0 + L):
                    acc_re = acc_re + w[b] * D[b].real
                    acc_im = acc_im + w[b] * D[b].imag
                for m in zero:
                    assert np.array_equal(coh[r, :, m].real, acc_re[:, m]) and np.array_equal(coh[r, :, m].imag, acc_im[:, m]), (name, r, m)
                b0 += L


def test_a_small_case_against_the_per_sample_definition(engine, noise_record, ca_table):
    """So that the chain does not rest on the library's own DDM alone: the blocks' cells from the float64 per-sample definition
    (bank_cases.ddm_reference), combined by the definition above.  Bound: 2e-6 * sum_b |w_b| sum |x_b|, the DDM tests' TOL per block."""
    engine.load_if(noise_record, fs=FS)
    tabs = _three_arms(ca_table)
    engine.set_channel(0, [ca_table])
    engine.set_channel(1, tabs)
    descs = [dict(channel=0, n=2049, s0=7, rem=0.25, step=(1.023e6 - 2.0) / FS, f=2.5e4, phi=1.1),
             dict(channel=0, n=1025, s0=20007, rem=0.0, step=1.023e6 / FS, f=2.5e4, phi=-0.4),
             dict(channel=0, n=4097, s0=3, rem=0.31, step=(1.023e6 + 3.0) / FS, f=2.4e4, phi=2.0),
             dict(channel=1, n=4097, s0=50001, rem=0.5, step=1.023e6 / FS, f=1.7e4, phi=-0.3),
             dict(channel=1, n=65, s0=1, rem=0.2, step=(1.023e6 + 1.0) / FS, f=1.7e4, phi=0.9)]
    offsets = [-0.5, 0.0, 0.5, 17.25]
    freqs = [0.0, -731.5, 5000.0]
    assert all(_colon_has_n_elements(d, o) for d in descs for o in offsets)
    run_len, weights = [3, 2], np.array([1.0, -1.0, 0.5, -2.5, 1.0])
    D = np.zeros((len(descs), 3, len(freqs), len(offsets)), dtype=np.complex128)
    scale = np.zeros(len(descs))
    for k, d in enumerate(descs):
        raw = _raw(noise_record, d["s0"], d["n"])
        t = tabs if d["channel"] == 1 else [ca_table]
        D[k, :len(t)], _ = ddm_reference(raw, t, d["rem"], d["step"], offsets, d["f"], freqs, d["phi"], FS)
        scale[k] = float(np.sum(np.abs(raw.real) + np.abs(raw.imag)))
    ref, _ = _restate(D, [d["s0"] for d in descs], freqs, run_len, weights, FS)
    coh, pw = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, freqs, run_len, weights=weights)
    assert pw is None and coh.shape == ref.shape
    worst = 0.0
    for r, (b0, b1) in enumerate([(0, 3), (3, 5)]):
        bound = TOL * float(np.sum(np.abs(weights[b0:b1]) * scale[b0:b1]))
        dev = max(np.abs(coh[r].real - ref[r].real).max(), np.abs(coh[r].imag - ref[r].imag).max())
        worst = max(worst, dev / bound)
        assert dev < bound, (r, dev, bound)
    print(f"against the per-sample definition: worst error {worst:.3f} of the bound {TOL:.0e} sum |w| sum |x|")
    assert not coh[0, 1:].any() and np.abs(coh[1]).min() > 0


def test_power_is_the_sum_over_the_calls_own_coherent_cells(engine, noise_record, ca_table):
    """pow == sum_r (re * re + im * im) over the same call's coh, sequentially, exactly - for maps of one run, of several and of all;
    a call without coh returns the same pow bytes, a call without maps the same coh bytes."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, [ca_table])
    engine.set_channel(1, _three_arms(ca_table))
    rng = np.random.default_rng(78)
    run_len, descs = _mixed_call(rng)
    weights = rng.choice(np.array([1.0, -1.0, 0.0, 0.5, -2.5]), size=len(descs))
    offsets, freqs = [0.0, 0.25, -0.25], [0.0, 250.0, -250.0, 1e3, 0.37]
    nr = len(run_len)
    only_coh, none = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, freqs, run_len, weights=weights)
    assert none is None
    for map_len in ([1] * nr, [1, 4, 2, 5], [nr], [3] * 4):
        assert sum(map_len) == nr
        coh, pw = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, freqs, run_len, weights=weights, map_len=map_len)
        assert coh.tobytes() == only_coh.tobytes()
        assert pw.shape == (len(map_len), 3, len(freqs), len(offsets)) and pw.dtype == np.float64
        assert np.array_equal(pw, _power(coh, map_len)), map_len
        assert pw.min() >= 0 and pw[:, 0].max() > 0
        nocoh, pw2 = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, freqs, run_len, weights=weights, map_len=map_len,
                                                    coherent=False)
        assert nocoh is None and pw2.tobytes() == pw.tobytes()


def test_independence_and_reproducibility(engine, noise_record, ca_table):
    """The call twice: equal bytes.  Each run alone: the bytes of its rows.  A subset of taps, a single bin: the bytes of their cells."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, [ca_table])
    engine.set_channel(1, _three_arms(ca_table))
    rng = np.random.default_rng(79)
    run_len, descs = _mixed_call(rng)
    weights = rng.choice(np.array([1.0, -1.0, 0.0, 0.5, -2.5]), size=len(descs))
    offsets = [j / 4 for j in range(-8, 9)]
    freqs = [125.0 * m for m in range(-4, 5)]
    maps = [1] * len(run_len)
    whole, wpow = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, freqs, run_len, weights=weights, map_len=maps)
    again, apow = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, freqs, run_len, weights=weights, map_len=maps)
    assert again.tobytes() == whole.tobytes() and apow.tobytes() == wpow.tobytes()
    b0 = 0
    for r, L in enumerate(run_len):
        one, opow = engine.correlate_ddm_integrate(_blocks(engine, descs[b0:b0 + L]), offsets, freqs, [L], weights=weights[b0:b0 + L], map_len=[1])
        assert one[0].tobytes() == whole[r].tobytes() and opow[0].tobytes() == wpow[r].tobytes(), r
        b0 += L
    cols = [0, 3, 4, 11, 16]
    sub, spow = engine.correlate_ddm_integrate(_blocks(engine, descs), [offsets[j] for j in cols], freqs, run_len, weights=weights, map_len=maps)
    assert sub.tobytes() == np.ascontiguousarray(whole[:, :, :, cols]).tobytes()
    assert spow.tobytes() == np.ascontiguousarray(wpow[:, :, :, cols]).tobytes()
    for m in (0, 4, 7):
        one, opow = engine.correlate_ddm_integrate(_blocks(engine, descs), offsets, [freqs[m]], run_len, weights=weights, map_len=maps)
        assert one[:, :, 0].tobytes() == np.ascontiguousarray(whole[:, :, m]).tobytes(), m
        assert opow[:, :, 0].tobytes() == np.ascontiguousarray(wpow[:, :, m]).tobytes(), m


def test_a_sub_batch_seam_inside_a_run_does_not_show(engine, noise_record, ca_table):
    """Three arms, 64 taps and 64 bins: a chunk's partial sums are 196 608 bytes and the 256 MB budget holds 1 365 chunks.  A filler run
    of 200 blocks of 4 097 samples (1 000 chunks) is followed by a run X of 100 such blocks (500 chunks): the first sub-batch ends
    after 273 blocks, inside X.  X's coherent rows and its map have the bytes of X called alone (one sub-batch); with X first the seam
    falls inside the filler and both runs' bytes are the same again.  The same list as three runs of 100 with maps of 1 and 2 runs
    cuts a map as well: its power is the sequential sum over the call's own coherent cells."""
    engine.load_if(noise_record, fs=FS)
    engine.set_channel(0, _three_arms(ca_table))
    n, nfill, nx = 4097, 200, 100
    chunk_bytes = 3 * 64 * 64 * 16
    budget = PARTIAL_BUDGET // chunk_bytes
    per_block = -(-n // 1024)
    seam = budget // per_block
    assert chunk_bytes == 196608 and budget == 1365 and per_block == 5 and seam == 273
    assert nfill * per_block == 1000 and nx * per_block == 500 <= budget          # X alone is one sub-batch
    assert nfill < seam < nfill + nx                                              # filler first: the seam is inside X
    assert nx < seam < nx + nfill                                                 # X first: inside the filler
    rng = np.random.default_rng(65)
    nb = nfill + nx
    rem, s0, f = rng.uniform(0, 1, nb), rng.integers(0, 60000 - n, nb), rng.uniform(-3e4, 3e4, nb)
    descs = [dict(n=n, s0=int(s0[k]), rem=float(rem[k]), step=1.023e6 / FS, f=float(f[k]), phi=0.3) for k in range(nb)]
    weights = rng.choice(np.array([1.0, -1.0, 0.5]), size=nb)
    fill, X, wf, wx = descs[:nfill], descs[nfill:], weights[:nfill], weights[nfill:]
    offsets = [float(x) for x in np.linspace(-3.0, 3.0, 64)]
    freqs = [float(x) for x in np.linspace(-1575.0, 1575.0, 64)]
    alone, apow = engine.correlate_ddm_integrate(_blocks(engine, X), offsets, freqs, [nx], weights=wx, map_len=[1])
    assert alone.shape == (1, 3, 64, 64) and np.abs(alone).min() > 0
    coh, pw = engine.correlate_ddm_integrate(_blocks(engine, fill + X), offsets, freqs, [nfill, nx], weights=weights, map_len=[1, 1])
    assert coh[1].tobytes() == alone[0].tobytes() and pw[1].tobytes() == apow[0].tobytes()
    swapped, spow = engine.correlate_ddm_integrate(_blocks(engine, X + fill), offsets, freqs, [nx, nfill], weights=np.concatenate([wx, wf]),
                                                   map_len=[1, 1])
    assert swapped[0].tobytes() == alone[0].tobytes() and spow[0].tobytes() == apow[0].tobytes()
    assert swapped[1].tobytes() == coh[0].tobytes() and spow[1].tobytes() == pw[0].tobytes()
    thirds, tpow = engine.correlate_ddm_integrate(_blocks(engine, fill + X), offsets, freqs, [100, 100, nx], weights=weights, map_len=[1, 2])
    assert thirds[2].tobytes() == alone[0].tobytes()
    assert np.array_equal(tpow, _power(thirds, [1, 2]))


def test_refusals_leave_both_outputs_untouched(engine, noise_record, ca_table):
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
    four = [good, dict(good, s0=20000), dict(good, s0=40000), dict(good, s0=100)]
    dp = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda x: np.asarray(x, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731

    def call(descs=four, offsets=(0.0, 0.5), freqs=(0.0, 50.0), run_len=(2, 2), map_len=(1, 1), weights=None, nruns=None, nmaps=None,
             want_coh=True, want_pow=True):
        off, frq = np.asarray(offsets, dtype=np.float64), np.asarray(freqs, dtype=np.float64)
        runs, maps = np.asarray(run_len, dtype=np.int32), np.asarray(map_len, dtype=np.int32)
        w = None if weights is None else np.asarray(weights, dtype=np.float64)
        coh = np.full((8, 3, max(len(frq), 1), max(len(off), 1), 2), 12345.0)
        pw = np.full((8, 3, max(len(frq), 1), max(len(off), 1)), 12345.0)
        rc = engine._lib.gc_correlate_ddm_integrate(engine._ctx, len(descs), _blocks(engine, descs), dp(w), len(off), dp(off), len(frq), dp(frq),
                                                    len(runs) if nruns is None else nruns, ip(runs), len(maps) if nmaps is None else nmaps,
                                                    ip(maps), dp(coh) if want_coh else None, dp(pw) if want_pow else None)
        assert np.all(coh == 12345.0) and np.all(pw == 12345.0), "a refused call must not write its outputs"
        return rc

    # what this function adds
    assert call(nruns=0, nmaps=0) == L.GC_E_INVALID                                  # blocks present, no runs
    assert call(run_len=(4, 0)) == L.GC_E_INVALID                                    # a run of no blocks
    assert call(run_len=(5, -1)) == L.GC_E_INVALID
    assert call(run_len=(2, 1)) == L.GC_E_INVALID                                    # the runs do not sum to the blocks
    assert call(run_len=(2, 3)) == L.GC_E_INVALID
    assert call(map_len=(2, 0)) == L.GC_E_INVALID                                    # a map of no runs
    assert call(map_len=(1,)) == L.GC_E_INVALID                                      # the maps do not sum to the runs
    assert call(map_len=(1, 2)) == L.GC_E_INVALID
    assert call(descs=[good, dict(good, channel=1), good, good]) == L.GC_E_INVALID   # two channels in one run
    assert call(weights=[1.0, float("nan"), 1.0, 1.0]) == L.GC_E_INVALID
    assert call(weights=[1.0, 1.0, 1.0, float("-inf")]) == L.GC_E_INVALID
    assert call(nmaps=-1) == L.GC_E_INVALID
    assert call(want_pow=False) == L.GC_E_INVALID                                    # maps asked for, nowhere to put them
    assert call(map_len=(), want_coh=False) == L.GC_E_INVALID                        # neither output asked for
    assert call(map_len=(), want_coh=False, want_pow=False) == L.GC_E_INVALID
    # one each of what gc_correlate_ddm refuses, with its status
    assert call(freqs=(0.0, float("nan"))) == L.GC_E_INVALID
    assert call(offsets=np.zeros(65)) == L.GC_E_INVALID
    assert call(descs=[dict(d, channel=5) for d in four]) == L.GC_E_UNSUPPORTED      # windowed channel
    assert call(descs=[dict(d, channel=6) for d in four]) == L.GC_E_INVALID          # broken pads
    assert call(descs=four[:3] + [dict(good, s0=60000 - 2048)], ) == L.GC_E_RANGE    # one sample past the record
    assert call(descs=[dict(d, channel=200) for d in four]) == L.GC_E_STATE
    engine.set_precision("double")
    try:
        assert call() == L.GC_E_UNSUPPORTED
    finally:
        engine.set_precision("single")
    # and the same arguments are accepted
    coh, pw = engine.correlate_ddm_integrate(_blocks(engine, four), [0.0, 0.5], [0.0, 50.0], [2, 2], map_len=[1, 1])
    assert coh.shape == (2, 3, 2, 2) and pw.shape == (2, 3, 2, 2) and np.abs(coh[:, 0]).min() > 0 and not coh[:, 1:].any()
    two_ch, _ = engine.correlate_ddm_integrate(_blocks(engine, [good, good, dict(good, channel=1), dict(good, channel=1)]), [0.0], [0.0], [2, 2])
    assert two_ch[0].tobytes() == two_ch[1].tobytes()                                # one channel per run, not per call


def test_an_empty_call_is_no_error_even_before_a_record_is_loaded():
    import cu_sdr_collection_amd as P
    with P.Engine(0) as fresh:
        coh, pw = fresh.correlate_ddm_integrate(fresh.make_blocks(0), [0.0, 0.5], [0.0, 1.0, 2.0], [])
        assert coh.shape == (0, 3, 3, 2) and pw is None
        coh, pw = fresh.correlate_ddm_integrate(fresh.make_blocks(0), [0.0, 0.5], [0.0, 1.0, 2.0], [], map_len=[])
        assert coh.shape == (0, 3, 3, 2) and pw.shape == (0, 3, 3, 2)
        with pytest.raises(P.GnssCorrError) as e:
            fresh.correlate_ddm_integrate(fresh.make_blocks(0), [0.0], [float("nan")], [])
        assert e.value.status == P._lib.GC_E_INVALID
        with pytest.raises(P.GnssCorrError) as e:
            fresh.correlate_ddm_integrate(fresh.make_blocks(0), [0.0], [0.0], [1])     # a run without blocks
        assert e.value.status == P._lib.GC_E_INVALID


def test_integrated_map_of_a_tracked_channel(engine, l1ca_scene):
    """receiver.integrated_delay_doppler_map on a 40-epoch tracking run, coherent = 10 (the value the issue names first: the restatement
    shows the ordering at it), wipe = "prompt", bins 0, +-50, +-100 Hz, offsets 0, +-1/4, +-1/2 chip.  A 10 ms run has its first null at
    100 Hz (noiseless amplitudes 1, 0.64, 0), which no single 1 ms block resolves.  Coherent maps (4 runs) and the power map of the 4
    runs agree with the restatement formed from delay_doppler_map's output and the signs of the recorded I_P, within the bound of the
    definition test (for the power: that bound carried through p = sum re^2 + im^2).  Restatement first, then library: the power map
    peaks at (0 Hz, 0 chips) and falls over 0, 50, 100 Hz on both sides."""
    import cu_sdr_collection_amd as P
    from types import SimpleNamespace
    S, sats, iq = l1ca_scene
    ms, nch = S.msToProcess, S.numberOfChannels
    offsets = [-0.5, -0.25, 0.0, 0.25, 0.5]
    freqs = [-100.0, -50.0, 0.0, 50.0, 100.0]
    idm = P.integrated_delay_doppler_map
    try:
        S.msToProcess, S.numberOfChannels = 40, 2
        ch = [SimpleNamespace(PRN=s.prn, acquiredFreq=S.IF + s.doppler + 4.0, codePhase=int(np.ceil(s.code_phase_samples)) + 1, status="T")
              for s in sats[:2]]
        engine.load_if(iq, fs=S.samplingFreq)
        tr, _ = P.tracking(engine, ch, S)
        per_epoch = P.delay_doppler_map(engine, tr[0], ch[0], S, offsets, freqs)
        coh = idm(engine, tr[0], ch[0], S, offsets, freqs, 10)
        pw = idm(engine, tr[0], ch[0], S, offsets, freqs, 10, noncoherent=4)
        short = idm(engine, tr[0], ch[0], S, offsets, freqs, 10, epochs=np.arange(25))
        short_pw = idm(engine, tr[0], ch[0], S, offsets, freqs, 10, noncoherent=2, epochs=np.arange(35))
        unwiped = idm(engine, tr[0], ch[0], S, offsets, freqs, 10, wipe=None)
        own = np.linspace(-1.0, 1.0, 40)
        weighted = idm(engine, tr[0], ch[0], S, offsets, freqs, 10, wipe=own)
        blocks, arms = P.receiver._tracked_blocks(engine, tr[0], ch[0], S, "GPS_L1CA", None)
        eng_unwiped, _ = engine.correlate_ddm_integrate(blocks, offsets, freqs, [10] * 4)
        eng_weighted, _ = engine.correlate_ddm_integrate(blocks, offsets, freqs, [10] * 4, weights=own)
    finally:
        S.msToProcess, S.numberOfChannels = ms, nch
    assert per_epoch.shape == (40, 1, 5, 5) and arms == 1
    assert coh.shape == (4, 1, 5, 5) and coh.dtype == np.complex128
    assert pw.shape == (1, 1, 5, 5) and pw.dtype == np.float64
    assert short.shape == (2, 1, 5, 5) and short.tobytes() == coh[:2].tobytes()          # 25 epochs: the incomplete third run is dropped
    assert short_pw.shape == (1, 1, 5, 5) and np.array_equal(short_pw, _power(coh[:2], [2]))   # 35 epochs: 3 runs, one map of 2
    assert unwiped.tobytes() == np.ascontiguousarray(eng_unwiped[:, :1]).tobytes()
    assert weighted.tobytes() == np.ascontiguousarray(eng_weighted[:, :1]).tobytes()
    w = np.where(np.asarray(tr[0].I_P, dtype=np.float64)[:40] >= 0, 1.0, -1.0)
    s0 = [int(x) for x in np.asarray(tr[0].absoluteSample)[:40]]
    assert [int(b.first_sample) for b in blocks] == s0
    ref, bound = _restate(per_epoch, s0, freqs, [10] * 4, w, S.samplingFreq)
    frac = _fraction(coh, ref, bound)
    print(f"tracked channel, coherent maps: worst error {frac:.3f} of the bound")
    assert frac <= 1.0, frac
    ref_pw = _power(ref, [4])
    # |p - p_ref| <= sum_r [2 (|re_r| + |im_r|) B_r + 2 B_r^2] for components within B_r, and the 3 roundings per run of either side
    pbound = np.sum(2.0 * (np.abs(ref.real) + np.abs(ref.imag)) * bound + 2.0 * bound * bound, axis=0)[None] + 2 * 3 * 4 * EPS * ref_pw
    pfrac = float((np.abs(pw - ref_pw) / pbound).max())
    print(f"tracked channel, power map: worst error {pfrac:.3f} of the bound")
    assert pfrac <= 1.0, pfrac
    for name, p in (("restatement", ref_pw[0, 0]), ("library", pw[0, 0])):                 # [bin, tap]
        assert np.unravel_index(int(np.argmax(p)), p.shape) == (2, 2), (name, p)
        for side in (+1, -1):
            along_f = [p[2 + side * m, 2] for m in range(3)]                                # |f| = 0, 50, 100 Hz at o = 0
            assert along_f[0] > along_f[1] > along_f[2], (name, side, along_f)
