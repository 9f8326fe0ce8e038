"""The acquisition's transforms and search surfaces cell by cell (csrc/acq_fft.hip, acq_coarse.hip, acq_shift.hip).

Transforms: gc_debug_fft, forward and inverse, against numpy.fft in complex128 over the lengths of tests/acq_fft_lengths.py (whose
plans tests/test_acq_fft_plan_cpu.py shows to reach every radix in every stage position of both passes), with unit impulses and
single tones - a wrong output index shows at full scale there - next to Gaussian rows.  Bound: 3e-6 * max|ref| * log2(n), the bound
of test_gpu_acquisition.py::test_fft_matches_numpy.

Surfaces: every cell of results(bin, tau) (acquisition.m:167-191) of one present and one absent PRN against a plain complex128
restatement, within half of the float64 guard's tie band relative to the surface's maximum - the premise csrc/acq_guard.h rests on:
|got - ref| <= (eps / 2) * max(ref) with eps = gc_acq_tie_eps(N) as gc_acq_guard_stats reports it.  Each case prints its worst
ratio |got - ref| / max(ref) (DESIGN.md 4.4 keeps the table)."""
import numpy as np
import pytest

import acq_fft_lengths as FL

pytestmark = pytest.mark.gpu

GC_E_UNSUPPORTED = -6


# ---- transforms -----------------------------------------------------------------------------------------------------------------------
def _fft_inputs(n, rng):
    """(kind, complex64 rows) for one length: impulses and tones at 0, 1, n1, n2, n-1 and two seeded places, one Gaussian row."""
    import cu_sdr_collection_amd as P
    p = P.Engine.debug_fft_plan(n)
    places = [v % n for v in (0, 1, p["n1"], p["n2"], n - 1)] + [int(v) for v in rng.integers(0, n, 2)]
    imp = np.zeros((len(places), n), dtype=np.complex64)
    imp[np.arange(len(places)), places] = 1.0
    k = np.arange(n, dtype=np.int64)
    w = np.exp(2j * np.pi * k / n).astype(np.complex64)
    tones = np.stack([w[(m * k) % n] for m in places])
    gauss = (rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n))).astype(np.complex64)
    return [("impulse", imp), ("tone", tones), ("gauss", gauss)]


def _fft_worst_ratio(engine, x, batch=3):
    """max over rows, directions and outputs of |got - ref| / (3e-6 * max|ref| * log2 n); rows go through the library `batch` at a time."""
    n = x.shape[1]
    worst = 0.0
    for r0 in range(0, x.shape[0], batch):
        xs = x[r0:r0 + batch]
        fwd = np.fft.fft(xs.astype(np.complex128), axis=1)
        bound = 3e-6 * np.max(np.abs(fwd)) * np.log2(n)
        for inverse in (False, True):
            got = engine.debug_fft(xs, inverse=inverse)
            ref = np.roll(fwd[:, ::-1], 1, axis=1) if inverse else fwd   # n * ifft(x)[k] = fft(x)[-k mod n]
            worst = max(worst, float(np.max(np.abs(got - ref))) / bound)
    return worst


def _sweep(engine, lengths, seed):
    rng = np.random.default_rng(seed)
    report = {}
    for n in lengths:
        report[n] = {kind: _fft_worst_ratio(engine, x) for kind, x in _fft_inputs(n, rng)}
    bad = {n: r for n, r in report.items() if max(r.values()) >= 1.0}
    worst = {n: round(max(r.values()), 4) for n, r in report.items()}
    print("fft sweep, worst error / bound per length:", worst)
    assert not bad, f"error / bound >= 1 at {bad}; worst ratio per length {worst}"


def test_fft_sweep_small_lengths(engine):
    _sweep(engine, FL.SWEEP_SMALL, 20251)


@pytest.mark.parametrize("n", list(FL.PRODUCTION))
def test_fft_production_lengths(engine, n):
    _sweep(engine, [n], 20252 + n)


def test_fft_largest_plan(engine):
    """2048 x 2048: pass vectors of 2048 (one vector per tile) and indices up to 2^22."""
    _sweep(engine, [FL.LARGEST], 20253)


def test_fft_batch_of_257_rows(engine):
    """More rows than any tile or wave count: the generic kernel's batch and tile index arithmetic."""
    rng = np.random.default_rng(20254)
    for n in (240, 100):
        x = (rng.standard_normal((257, n)) + 1j * rng.standard_normal((257, n))).astype(np.complex64)
        ratio = _fft_worst_ratio(engine, x, batch=257)
        assert ratio < 1.0, (n, ratio)


def test_refused_length_leaves_the_context_usable(engine):
    import cu_sdr_collection_amd as P
    x = np.ones((1, 3584), dtype=np.complex64)   # 2^9 * 7
    with pytest.raises(P.GnssCorrError) as e:
        engine.debug_fft(x)
    assert e.value.status == GC_E_UNSUPPORTED
    _sweep(engine, [60], 20255)


@pytest.mark.tuning
@pytest.mark.parametrize("n", list(FL.PRODUCTION))
def test_fft_production_lengths_on_the_generic_kernel(engine, monkeypatch, n):
    monkeypatch.setenv("GC_ACQ_GENERIC", "1")
    _sweep(engine, [n], 20256 + n)


# ---- search surfaces ------------------------------------------------------------------------------------------------------------------
def _chips(rng, nchips):
    return (2 * rng.integers(0, 2, nchips) - 1).astype(np.int8)


def _sampled(chips, spc):
    """One code period at spc samples (chip of sample k: floor(k * nchips / spc))."""
    return chips[(np.arange(spc) * len(chips)) // spc]


def _record(rng, n, fs, replicas, tau, freq, cn0_dbhz=50.0, sigma=16.0):
    """int8 I/Q record of n samples: complex Gaussian noise (sigma per component) + the periodic replicas (one per arm, the second in
    quadrature) delayed by tau samples on a carrier of `freq` Hz at C/N0 = cn0 per arm.  Returns (interleaved int8, complex128 samples)."""
    k = np.arange(n)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    amp = np.sqrt(10 ** (cn0_dbhz / 10) * 2 * sigma ** 2 / fs)
    for a, rep in enumerate(replicas):
        x += amp * (1j ** a) * rep[(k - tau) % len(rep)] * np.exp(2j * np.pi * ((freq * k / fs) % 1.0) + 0.7j)
    iq = np.empty(2 * n, dtype=np.int8)
    iq[0::2] = np.clip(np.rint(x.real), -127, 127)
    iq[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return iq, iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)


def _coarse_ref(x, fs, f0, step, nbins, hops, spc, blk, codes, weights):
    """results(bin, tau) of acquisition.m:167-191 in complex128: per bin and hop abs(ifft(fft(x .* exp(-i f_b phasePoints)) .*
    conj(fft([code zeros])))), summed over the hops and, with their weights, over the code arms."""
    k = np.arange(blk)
    cspec = [np.conj(np.fft.fft(np.concatenate([c.astype(np.float64), np.zeros(blk - len(c))]))) for c in codes]
    out = np.zeros((nbins, blk))
    for b in range(nbins):
        carrier = np.exp(-2j * np.pi * (((f0 - step * b) * k / fs) % 1.0))
        for h in range(hops):
            spec = np.fft.fft(x[h * spc:h * spc + blk] * carrier)
            for c, w in zip(cspec, weights):
                out[b] += w * np.abs(np.fft.ifft(spec * c))
    return out


def _check_surface(label, got, ref, eps):
    """Every cell of the valid lags within eps / 2 of the float64 value relative to the surface's maximum."""
    valid = ref.shape[1]
    assert got.shape[0] == ref.shape[0] and got.shape[1] >= valid, (label, got.shape, ref.shape)
    err = np.abs(got[:, :valid].astype(np.float64) - ref)
    ratio = float(err.max() / ref.max())
    at = np.unravel_index(int(np.argmax(err)), err.shape)
    print(f"surface {label}: N = {got.shape[1]}, {ref.shape[0]} x {valid} cells, worst |got - ref| / max(ref) = {ratio:.3e} "
          f"(eps / 2 = {eps / 2:.3e}), peak / mean = {ref.max() / ref.mean():.2f}")
    assert ratio <= eps / 2, f"{label}: cell {at} off by {ratio:.3e} of the maximum, eps / 2 = {eps / 2:.3e}"
    return ratio


def _check_winner(label, ref, eps, row, col, peak):
    """The production call's pick against the float64 surface: its indices whenever the runner-up is clear of the tie band, its
    (float64, guarded) peak always."""
    flat = np.sort(ref, axis=None)
    if flat[-2] < flat[-1] * (1.0 - eps):
        assert row == int(np.argmax(np.max(ref, axis=1))) and col == int(np.argmax(np.max(ref, axis=0))), label
    assert abs(peak - ref.max()) <= 1e-9 * ref.max(), (label, peak, ref.max())


class Coarse:
    """One coarse-search case: a record with PRN 0 present and PRN 1 absent."""

    def __init__(self, label, fs, code_rate, nchips, step, nbins, hops, narms=1, weights=None, conditioned=False, seed=1, hop_groups=None):
        self.hop_groups = hop_groups
        self.label, self.fs, self.code_rate, self.nchips, self.step, self.nbins, self.hops = label, fs, code_rate, nchips, step, nbins, hops
        self.narms, self.conditioned = narms, conditioned
        self.weights = weights or [0.0] * narms      # 0: the library's "weight 1"
        self.spc = int(round(fs / (code_rate / nchips)))
        self.blk = 2 * self.spc
        self.fi = 20e3
        rng = np.random.default_rng(seed)
        self.codes = np.stack([np.stack([_sampled(_chips(rng, nchips), self.spc) for _ in range(narms)]) for _ in range(2)])
        self.band = step * (nbins // 2)
        n = (hops + 1) * self.spc
        self.iq, self.x = _record(rng, n, fs, list(self.codes[0]), tau=int(rng.integers(1, self.spc)), freq=self.fi + 0.3 * step)

    def params(self):
        from cu_sdr_collection_amd import _lib as L
        p = L.gc_acq_params()
        p.sampling_freq, p.code_freq_basis, p.code_length = self.fs, self.code_rate, self.nchips
        p.intermediate_freq, p.search_band, p.search_step = self.fi, self.band, self.step
        p.non_coh_time, p.n_bins, p.first_sample = self.hops, self.nbins, 0
        p.source = 1 if self.conditioned else 0
        for a, w in enumerate(self.weights):
            p.arm_weight[a] = w
        return p

    def run(self, engine):
        if self.conditioned:
            engine.acq_set_signal(self.x.astype(np.complex64))
        else:
            engine.load_if(self.iq, fs=self.fs)
        p = self.params()
        if self.hop_groups is not None:
            # launch_abs_pass splits a bin's hops over groups while tiles x bins stays under four workgroups per CU (one lane: the
            # surface is written by the slow path's re-search); the case must sit on the side of that rule it is here for
            import cu_sdr_collection_amd as P
            plan = P.Engine.debug_fft_plan(self.blk)
            tiles = -(-plan["n2"] // plan["cols1"])
            assert (tiles * self.nbins < 4 * engine.device_info()[1]) == self.hop_groups, (tiles, self.nbins, engine.device_info())
        res = engine.acquire_coarse(p, self.codes if self.narms > 1 else self.codes[:, 0])
        eps = engine.acq_guard_stats()["eps"]
        w = [v if v != 0.0 else 1.0 for v in self.weights]
        worst = 0.0
        for ip, kind in enumerate(("present", "absent")):
            ref = _coarse_ref(self.x, self.fs, self.fi + self.band, self.step, self.nbins, self.hops, self.spc, self.blk, self.codes[ip], w)
            got = engine.debug_acq_surface(p, self.codes[ip])
            assert engine.acq_guard_stats()["eps"] == eps
            worst = max(worst, _check_surface(f"{self.label} ({kind})", got, ref, eps))
            _check_winner(f"{self.label} ({kind})", ref, eps, res[ip].coarse_bin - 1, res[ip].code_phase - 1, res[ip].peak)
            if kind == "present":
                assert ref.max() > 4 * np.median(ref)          # the scene is what it claims to be
        return worst


COARSE = {
    "l1ca-2hops": dict(fs=18e6, code_rate=1.023e6, nchips=1023, step=500.0, nbins=3, hops=2, hop_groups=True),   # 180 x 200
    "l1ca-5hops": dict(fs=18e6, code_rate=1.023e6, nchips=1023, step=500.0, nbins=3, hops=5, hop_groups=True),   # (see below)
    "l1ca-42bins": dict(fs=18e6, code_rate=1.023e6, nchips=1023, step=500.0, nbins=42, hops=2, hop_groups=False),   # no hop groups
    "glonass": dict(fs=12e6, code_rate=0.511e6, nchips=511, step=500.0, nbins=3, hops=2),                     # 150 x 160
    "e1-two-arms": dict(fs=18e6, code_rate=1.023e6, nchips=4092, step=125.0, nbins=3, hops=1, narms=2),       # 375 x 384, arms merged
    "l5-i+q": dict(fs=18e6, code_rate=10.23e6, nchips=10230, step=500.0, nbins=3, hops=3, narms=2),           # arm after arm
    "16.368-msps": dict(fs=16.368e6, code_rate=1.023e6, nchips=1023, step=500.0, nbins=3, hops=2),            # 32 736 in a padded transform
    "conditioned": dict(fs=18e6, code_rate=1.023e6, nchips=1023, step=500.0, nbins=3, hops=2, conditioned=True),
}
# Hop groups (launch_abs_pass): the hops of a bin are split over the largest divisor g of the hop count while tiles x bins x (the
# previous g) stays under four workgroups per CU - with 25 tiles x 3 bins every hop is a group of its own (2 and 5 groups) and
# abs_combine_kernel adds them; 25 tiles x 42 bins are more than 4 x 256 workgroups, so the columns pass itself walks both hops and
# writes the sums.  Coarse.run asserts the side of the rule (hop_groups=) with the device's CU count.


def test_restated_reference_equals_the_oracles_results():
    """The plain restatement above and oracle.gnss_oracle.acquisition_coarse_results on the L1 C/A case: two restatements, one surface."""
    import cu_sdr_collection_amd as P
    from oracle import gnss_oracle as O
    S = P.initSettings()
    S.acqNonCohTime = 2
    rng = np.random.default_rng(7)
    spc = 18000
    table = np.asarray(P.codes.makeCaTable(5, S))
    iq, x = _record(rng, 3 * spc, S.samplingFreq, [table.astype(np.int8)], tau=4321, freq=S.IF + 1200.0)
    want = O.acquisition_coarse_results(x, 5, S)
    nbins = want.shape[0]
    from cu_sdr_collection_amd.receiver import _acq_params
    p = _acq_params(S, 0)
    mine = _coarse_ref(x, S.samplingFreq, p.intermediate_freq + p.search_band, p.search_step, nbins, 2, spc, 2 * spc, [table], [1.0])
    assert mine.shape == want.shape
    assert np.max(np.abs(mine - want)) <= 1e-11 * want.max()


@pytest.mark.parametrize("case", list(COARSE))
def test_coarse_surface_matches_float64(engine, case):
    Coarse(case, seed=sum(map(ord, case)), **COARSE[case]).run(engine)


def test_more_code_arms_than_bins_times_hops(engine):
    """Five PRNs over 3 bins x 1 hop: the code spectra's forward transforms are more than the search's own bins x hops, and their
    intermediate is the search's (ensure_scratch sizes it for both)."""
    c = Coarse("5 prns, 3 bins x 1 hop", seed=23, **dict(COARSE["l1ca-2hops"], hops=1))
    rng = np.random.default_rng(24)
    codes = np.concatenate([c.codes[:, 0]] + [_sampled(_chips(rng, c.nchips), c.spc)[None, :] for _ in range(3)])
    engine.load_if(c.iq, fs=c.fs)
    res = engine.acquire_coarse(c.params(), codes)
    eps = engine.acq_guard_stats()["eps"]
    for ip in range(codes.shape[0]):
        ref = _coarse_ref(c.x, c.fs, c.fi + c.band, c.step, c.nbins, 1, c.spc, c.blk, [codes[ip]], [1.0])
        _check_winner(f"prn {ip} of 5", ref, eps, res[ip].coarse_bin - 1, res[ip].code_phase - 1, res[ip].peak)


@pytest.mark.tuning
def test_two_arm_surface_with_the_arms_searched_separately(engine, monkeypatch):
    monkeypatch.setenv("GC_ACQ_ARMS_SEPARATE", "1")
    Coarse("e1-two-arms, separate", seed=11, **COARSE["e1-two-arms"]).run(engine)


SHIFT = {
    "b1i": dict(fs=18e6, n=72000, nchips=2046, code_rate=2.046e6, n_signals=2, narms=1, weights=None),                       # 250 x 288
    "b1c": dict(fs=18e6, n=360000, nchips=10230, code_rate=1.023e6, n_signals=1, narms=2,
                weights=[float(np.sqrt(11 / 40)), float(np.sqrt(29 / 40))]),                                                  # 600 x 600
    "l2c": dict(fs=8e6, n=320000, nchips=10230, code_rate=0.5115e6, n_signals=1, narms=1, weights=None),                     # 320 x 1000
}


@pytest.mark.parametrize("case", list(SHIFT))
def test_shift_surface_matches_float64(engine, case):
    """The circshift family: row ((carrier, signal block), bin) = sum over arms of w * abs(ifft(circshift(fft(x .* carrier), bin) .*
    conj(fft(code)))) - every row of gc_acq_shift_search / gc_acq_shift_row, and gc_acq_shift_search_batch's pick."""
    from cu_sdr_collection_amd import _lib as L
    c = SHIFT[case]
    fs, n, narms, nsig = c["fs"], c["n"], c["narms"], c["n_signals"]
    ncar, nbins = 2, 3
    rng = np.random.default_rng(sum(map(ord, case)))
    half = n // 2                                        # the replica covers half a block, zeros behind it (acquisition.m:44-45)
    period = int(round(fs * c["nchips"] / c["code_rate"]))
    reps = np.stack([np.stack([np.tile(_sampled(_chips(rng, c["nchips"]), period), -(-half // period))[:half] for _ in range(narms)])
                     for _ in range(2)])
    codes = np.zeros((2, narms, n), dtype=np.int8)
    codes[:, :, :half] = reps
    bin_hz = fs / n
    f0, fstep = 20e3 - bin_hz, bin_hz / ncar             # the signal sits one bin and a bit above the first carrier
    iq, x = _record(rng, nsig * n + 16, fs, list(reps[0]), tau=int(rng.integers(1, half)), freq=20e3 + 0.2 * bin_hz, cn0_dbhz=50.0)
    engine.load_if(iq, fs=fs)
    sp = L.gc_acq_shift_params(sampling_freq=fs, carrier_f0=f0, carrier_step=fstep, first_sample=0, n=n, n_signals=nsig, n_carriers=ncar,
                               n_bins=nbins, n_arms_max=narms, source=0)
    engine.acq_shift_prepare(sp)
    picks = engine.acq_shift_search_batch(codes, c["weights"], L.GC_SHIFT_PICK_GLOBAL)
    assert picks is not None
    eps = engine.acq_guard_stats()["eps"]
    w = c["weights"] or [1.0] * narms
    k = np.arange(n)
    spectra = [[np.fft.fft(x[s * n:(s + 1) * n] * np.exp(-2j * np.pi * (((f0 + fstep * ci) * k / fs) % 1.0))) for s in range(nsig)] for ci in range(ncar)]
    for ip, kind in enumerate(("present", "absent")):
        cspec = [np.conj(np.fft.fft(codes[ip, a].astype(np.float64))) for a in range(narms)]
        ref = np.stack([sum(wa * np.abs(np.fft.ifft(np.roll(spectra[ci][s], b) * cs)) for wa, cs in zip(w, cspec))
                        for ci in range(ncar) for s in range(nsig) for b in range(nbins)])
        engine.acq_shift_prepare(sp)
        rmax, rarg = engine.acq_shift_search(codes[ip], c["weights"])
        got = np.stack([engine.acq_shift_row(r) for r in range(ref.shape[0])])
        _check_surface(f"shift {case} ({kind})", got, ref, eps)
        # the row maxima the search itself reports (arms merged where the rows handed out are summed arm after arm): the same bound
        assert np.max(np.abs(rmax - ref.max(axis=1))) <= eps / 2 * ref.max()
        assert np.all(ref[np.arange(ref.shape[0]), rarg] >= ref.max(axis=1) - eps * ref.max())
        _check_winner(f"shift {case} ({kind})", ref, eps, picks[ip].row, picks[ip].code_phase, picks[ip].peak)
        if kind == "present":
            assert ref.max() > 4 * np.median(ref)
