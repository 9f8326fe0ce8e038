"""Scenes for the decisions of gc_acq_shift_search_batch, built from seeds (numpy only): tests/test_gpu_shift_picks.py searches them on
the device, tests/test_shift_pick_cpu.py holds each to what it claims on the float64 surface (tests/shift_pick_model.py).

Every scene carries three PRNs, one of them absent, and a list of calls; a call is one record (or conditioned signal), one
first_sample, the rule's exclude / period, and the (row, code_phase) its present PRNs are built to give.

CLEAR scenes: an int8 record of noise and two satellites, each a frame of period n - the zero-padded replica itself, so that the
correlation has ONE peak, at the planted lag - on the carrier of one (carrier, bin) and stronger in one signal block: over the calls
the peak visits the edges of the three range cases of the second-peak window, every period of the row and the row's end, the winner
every kind of row.

TIE scenes: a conditioned signal (gc_acq_set_signal) of integer-valued complex64 samples, amplitude 3e4, zero carrier for the tied
cells, so that those are exact integers near 1e9 (3e8 at the short block) and single-sample bumps set their difference to exactly 1:
1e-9 relative, far above float64's rounding and far below what float32 resolves.  Each scene comes in both directions; one of the two
necessarily goes against whatever the float32 pass prefers.  Tied rows are the conjugate rows of a real carrier (their gap is set by
one sample of Q and is asserted, not constructed to the unit)."""
from types import SimpleNamespace

import numpy as np

import shift_pick_model as M

FS = 18e6
EXCLUDE = 9
AMP = 30000


def eps_of(n):
    """An upper bound of the library's gc_acq_tie_eps (8 log2 N 2^-24) for a block of n points: its transform has n points, or the
    first plannable length from 2 n up (below 4 n)."""
    return 8.0 * np.log2(4.0 * n) * 2.0 ** -24


def _chips(rng, nchips):
    return (2 * rng.integers(0, 2, nchips) - 1).astype(np.int8)


def _replica(rng, n, rule):
    """(zero-padded replica [n], period): SEQUENTIAL / GLOBAL one period of n / 2 samples, PAIRS two periods of n / 4, about nine
    samples per chip."""
    period = n // 4 if rule == M.SEQUENTIAL_PAIRS else n // 2
    chips = _chips(rng, period // 9)
    code = chips[(np.arange(period) * len(chips)) // period]
    out = np.zeros(n, dtype=np.int8)
    out[:n // 2] = np.tile(code, (n // 2) // period)
    return out, period


class Scene:
    def __init__(self, n, rule, geom, f0, fstep, codes, weights, absent, calls):
        self.n, self.rule, self.geom, self.f0, self.fstep = n, rule, geom, f0, fstep
        self.codes, self.weights, self.absent, self.calls = codes, weights, absent, calls       # codes int8 [3, narms, n]

    def carriers(self):
        return [self.f0 + self.fstep * c for c in range(self.geom[0])]

    def surfaces(self, call):
        """The float64 surface of every PRN of the call (computed once per call)."""
        if call.surf is None:
            call.surf = [M.surface(call.x, FS, self.n, self.geom[1], self.carriers(), self.geom[2], self.codes[ip], self.weights, call.first_sample)
                         for ip in range(self.codes.shape[0])]
        return call.surf


def _call(label, x, first_sample, exclude, period, expect, conditioned=False, contested=None):
    return SimpleNamespace(label=label, x=x, first_sample=first_sample, exclude=exclude, period=period, expect=expect, conditioned=conditioned,
                           contested=contested, surf=None)


def _row(geom, c, s, b):
    return (c * geom[1] + s) * geom[2] + b


# ---- clear scenes ------------------------------------------------------------------------------------------------------------------------
def _clear(n, rule, seed):
    rng = np.random.default_rng(seed)
    if rule == M.GLOBAL:
        geom, narms, weights = (1, 1, 4), 2, [float(np.sqrt(11 / 40)), float(np.sqrt(29 / 40))]
    else:
        geom, narms, weights = (2, 2 if rule == M.SEQUENTIAL_PAIRS else 1, 3), 1, None
    nc, ns, nb = geom
    bin_hz = FS / n
    f0 = 20e3
    fstep = {M.GLOBAL: 0.0, M.SEQUENTIAL: -bin_hz / 2, M.SEQUENTIAL_PAIRS: bin_hz / 2}[rule]     # (L2C steps down, B1I up)
    reps = [[_replica(rng, n, rule) for _ in range(narms)] for _ in range(3)]
    period = reps[0][0][1] if rule != M.GLOBAL else 0
    codes = np.stack([np.stack([r[0] for r in arms]) for arms in reps])
    # winner positions: carrier 0 and 1, signal block 1 and 2, bin 0 and the last eligible bin
    places = [(c, s, b) for c in range(nc) for s in range(ns) for b in (0, nb - 1 - (1 if c > 0 and rule != M.GLOBAL else 0))]
    if rule == M.GLOBAL:
        places = [(0, 0, b) for b in range(nb)]
        cps = [1, n // 3, n // 2 + 1, n]
    else:
        e, p = EXCLUDE, period
        cps = [1, e, e + 1, e + 2, p - e - 1, p - e, p, p + 1, p + p // 3, n - p + p // 5, n]     # ... a later period, the last one, the row's end
    sigma, amp = 16.0, 8.0
    noise = sigma * (rng.standard_normal(ns * n + 2000) + 1j * rng.standard_normal(ns * n + 2000))
    k = np.arange(n)
    calls = []
    for i, cp in enumerate(cps):
        first = (0, 5, 1234)[i % 3]
        x = noise.copy()
        expect = {}
        for ip, (place, cpi) in ((0, (places[i % len(places)], cp)), (2, (places[(i + 3) % len(places)], cps[(i + 4) % len(cps)]))):
            c, s, b = place
            f_sat = f0 + c * fstep - b * bin_hz                        # wiped by carrier c and undone by circshift(spectrum, b)
            for blk in range(ns):
                a = amp if blk == s else 0.6 * amp
                sig = sum((1j ** arm) * codes[ip, arm][(k - (cpi - 1)) % n] for arm in range(narms))
                x[first + blk * n + k] += a * sig * np.exp(2j * np.pi * ((f_sat * k / FS) % 1.0) + 0.7j)
            expect[ip] = (_row(geom, c, s, b), cpi - 1)
        x = np.clip(np.rint(x.real), -127, 127) + 1j * np.clip(np.rint(x.imag), -127, 127)
        calls.append(_call(f"cp {cp} at {places[i % len(places)]}", x, first, EXCLUDE if rule != M.GLOBAL else 0, period or 1, expect))
    return Scene(n, rule, geom, f0, fstep, codes, weights, 1, calls)


_RULES = {"global": M.GLOBAL, "sequential": M.SEQUENTIAL, "pairs": M.SEQUENTIAL_PAIRS}
SIZES = (72000, 18000, 16368)        # specialised passes and two lanes; rows written; a padded transform
CLEAR = {f"{name}-{n}": (lambda n=n, rule=rule, name=name: _clear(n, rule, 100 * n + rule)) for name, rule in _RULES.items() for n in SIZES}


# ---- tie scenes --------------------------------------------------------------------------------------------------------------------------
def _support(first, n, code, tau):
    """Record positions cell tau of the block at `first` sums over, and the replica's entries there."""
    m = np.flatnonzero(code)
    return first + (tau + m) % n, code[m].astype(np.int64)


def _cell(x, first, n, code, tau):
    """The cell at zero carrier and shift, exactly: |sum x[(tau + m) mod n] code[m]| of a real integer-valued signal."""
    idx, c = _support(first, n, code, tau)
    return abs(int(np.sum(np.rint(x.real[idx]).astype(np.int64) * c)))


def _level(x, n, code, cells, extra, dmax=2 * AMP):
    """Bumps on single samples until cell i = (first, tau) holds (the largest of them) + extra[i]: each on samples no other listed cell
    sums over, with the replica's sign, at most dmax a sample."""
    target = max(_cell(x, f, n, code, t) for f, t in cells)
    for i, (f, t) in enumerate(cells):
        idx, c = _support(f, n, code, t)
        others = np.concatenate([_support(f2, n, code, t2)[0] for j, (f2, t2) in enumerate(cells) if j != i])
        own = ~np.isin(idx, others)
        need = target + extra[i] - _cell(x, f, n, code, t)
        assert 0 <= need <= dmax * int(own.sum()), (need, int(own.sum()))
        full, rest = divmod(need, dmax)
        d = np.zeros(int(own.sum()), dtype=np.int64)
        d[:full] = dmax
        d[full:full + 1] = rest
        x.real[idx[own]] += d * c[own]
    for i, (f, t) in enumerate(cells):
        assert _cell(x, f, n, code, t) == target + extra[i]
    assert np.max(np.abs(x.real)) < 2 ** 24 and np.all(x.real == np.rint(x.real))


def _frame(code, n, tau, length=None):
    """The replica as a signal of period n delayed by tau; with `length`, the code repeated over that many samples from tau instead."""
    k = np.arange(n)
    if length is None:
        return code[(k - tau) % n].astype(np.float64)
    period = length[1]
    return np.where((k - tau) % n < length[0], code[((k - tau) % n) % period], 0).astype(np.float64)


def _ties(n, rule, kind, seed):
    """kind: rows / blocks / columns / second.  Two calls, the two directions."""
    rng = np.random.default_rng(seed)
    geom = (1, 1, 3) if rule == M.GLOBAL and kind != "rows" else (2, 2 if rule == M.SEQUENTIAL_PAIRS else 1, 2)
    nc, ns, nb = geom
    bin_hz = FS / n
    (code_a, period), (code_b, _), (code_c, _) = [_replica(rng, n, rule) for _ in range(3)]
    exclude, per = (EXCLUDE, period) if rule != M.GLOBAL else (0, 1)
    first = 7
    k = np.arange(n)
    total = first + ns * n + 9
    tau0 = int(0.6 * period) + 11
    calls = []
    if kind == "rows":
        # a real carrier at delta: the rows wiped with +delta and -delta are complex conjugates of each other
        # (carriers at +0.3 and -0.3 of a bin; the second bin of each lies a whole bin below)
        delta = 0.3 * bin_hz
        f0, fstep = delta, -2 * delta
        rows = (_row(geom, 0, 0, 0), _row(geom, 1, 0, 0))
        codes = np.stack([code_a, code_b, code_a])[:, None, :]
        for q in (3.0, -3.0):
            x = np.zeros(total, dtype=np.complex128)
            for blk in range(ns):
                x[first + blk * n + k] = np.rint((1.0 if blk == 0 else 0.6) * AMP * _frame(code_a, n, tau0) * np.cos(2 * np.pi * delta * k / FS))
            x[first + tau0 + n // 8] += 1j * q                       # tilts the conjugate rows
            calls.append(_call(f"rows, Q {q:+.0f}", x, first, exclude, per, None, True, ("rows", [(r, tau0) for r in rows])))
        absent, present = 1, (0, 2)
    else:
        f0, fstep = 0.0, bin_hz / 2
        codes = np.stack([code_a, code_b, code_c])[:, None, :]
        absent, present = 1, (0, 2)
        tau_c = int(0.8 * period) + 5
        for direction in (0, 1):
            x = np.zeros(total, dtype=np.complex128)
            x[first + k] += 0.5 * AMP * _frame(code_c, n, tau_c)     # the third PRN: the first block only
            extra = [1, 0] if direction == 0 else [0, 1]
            if kind == "blocks":
                for blk in range(2):
                    x[first + blk * n + k] += AMP * _frame(code_a, n, tau0)
                cells = [(first, tau0), (first + n, tau0)]
                contested = ("rows", [(_row(geom, 0, 0, 0), tau0), (_row(geom, 0, 1, 0), tau0)])
            elif kind == "columns":
                # the code over one period more than the replica is long: columns tau0 and tau0 + period hold the whole replica; a weaker
                # copy a period long (two, pairs) before tau0 lies in the window around tau0 and not in the one around tau0 + period
                x[first + k] += AMP * _frame(code_a, n, tau0, (n // 2 + period, period))
                x[first + k] += 0.2 * AMP * _frame(code_a, n, int(0.25 * period) + 3)
                cells = [(first, tau0), (first, tau0 + period)]
                contested = ("first", [(0, tau0), (0, tau0 + period)])
            else:
                assert kind == "second"
                x[first + k] += AMP * _frame(code_a, n, tau0)
                tau1, tau2 = int(0.1 * period) + 2, int(0.4 * period) + 7
                for t in (tau1, tau2):
                    x[first + k] += 0.5 * AMP * _frame(code_a, n, t)
                cells = [(first, tau1), (first, tau2)]
                contested = ("second", [(0, tau1), (0, tau2)])
            _level(x, n, code_a, cells, extra)
            calls.append(_call(f"{kind}, direction {direction}", x, first, exclude, per, None, True, contested))
    sc = Scene(n, rule, geom, f0, fstep, codes, None, absent, calls)
    for call in calls:                                               # what the model says of the present PRNs is what the scene expects
        surf = sc.surfaces(call)
        call.expect = {ip: (lambda m: (m["row"], m["code_phase"]))(M.pick(surf[ip], *geom, rule, call.exclude, call.period)) for ip in present}
    return sc


_KINDS = {"global": ("rows", "columns"), "sequential": ("rows", "columns", "second"), "pairs": ("rows", "blocks", "columns", "second")}
TIES = {f"{name}-{kind}-{n}": (lambda n=n, rule=rule, kind=kind, i=i: _ties(n, rule, kind, 7 * n + 10 * rule + i))
        for name, rule in _RULES.items() for i, kind in enumerate(_KINDS[name]) for n in SIZES[:2]}
