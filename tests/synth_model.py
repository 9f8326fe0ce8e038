"""A float64 model of the record synthesiser (csrc/synth.hip: gs_generate, gs_generate2), written from the signal model in
cu_sdr_collection_amd/synth.py's docstring and the struct comments of synth.hip.  Helper module: no tests in it.

Every sample is a closed-form function of (seed, sample index): no chunks of 8, no phasor recurrence, no float32.

    noise   h = splitmix64(seed * 0xD1342543DE82EF95 + n);  u1 = ((h >> 40) + 0.5) / 2^24;  u2 = (h & 0xFFFFFF) / 2^24
            r = sigma * sqrt(-2 ln u1);  I += r cos(2 pi u2);  Q += r sin(2 pi u2)
    chips   cp = (n - code_phase_samples) * (code_rate / fs)   (exactly these two double operations)
            chip = floor(cp);  idx, period = chip mod / floor-div code_len;  bit index = period floor-div bit_periods
    data    version 1: splitmix64(seed ^ (prn << 48) ^ b * 0x9E3779B97F4A7C15); version 2 also xors (s << 40), s the position
            in the satellite list; odd hash +1, even hash -1.  `bits=` replaces the hash by a callable (s, bit index) -> +-1.
    signal  amplitude * (data * code[idx] + pilot[idx] * exp(j pilot_phase)) * exp(+j 2 pi frac(carrier_phase / 2 pi + n (IF + fd) / fs))
    output  rint, clip to +-limit, I,Q or Q,I order

Where float32 arithmetic may legitimately land on the other side of an edge the model says so in two masks:

    near_half   a component's unrounded value lies within `delta` of a half-integer (and is not clipped: beyond
                limit - 0.5 + delta both roundings give +-limit);
    near_chip   some satellite's cp lies within 16 * 2^-23 * max(1, code_rate / fs) of an integer.  The kernel advances the chip
                fraction in float32: at most 9 roundings of <= 2^-23 per chunk of 8 plus 8 x the rounding of the float32 step;
                the band leaves about a factor 2 over that sum.  For such samples `alts` holds the record with the neighbouring
                chips, floor(cp - band) and floor(cp + band), and `multi` every combination where two satellites sit on an edge
                at the same sample.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field

import numpy as np

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_NOISE_MUL = 0xD1342543DE82EF95
DELTA_F32 = 2.0 ** -8          # half-integer band for a float32 kernel (float32 emulation stayed within 6.3e-4: factor 6)
CHIP_BAND = 16 * 2.0 ** -23    # x max(1, code_rate / fs)
BAND_SHARE_CAP = 0.025         # near_half | near_chip may cover this share of a case at most (expected: 4 * 2^-8 + < 2e-4)


def splitmix64(x) -> np.ndarray:
    """The published splitmix64 output function on uint64 arrays: splitmix64(0) = 0xE220A8397B1DCDAF."""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
    with np.errstate(over="ignore"):
        x = x + np.uint64(_GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


@dataclass
class ModelSat:
    prn: int
    code: np.ndarray                 # +-1 (or 0) chips, one code period
    doppler: float                   # Hz
    code_phase_samples: float        # sample index at which a code period starts
    carrier_phase: float             # rad at n = 0
    amplitude: float                 # LSB
    code_rate: float                 # chips/s including code Doppler
    intermediate_freq: float = 0.0   # Hz
    bit_periods: int = 20            # code periods per data bit
    pilot: np.ndarray | None = None  # pilot chips (same length, no data bits)
    pilot_phase: float = 0.0         # rad


@dataclass
class ModelRecord:
    i: np.ndarray            # unrounded, noise included
    q: np.ndarray
    rounded: np.ndarray      # interleaved as the record is written
    near_half: np.ndarray
    near_chip: np.ndarray
    alts: list               # records with floor(cp - band) and floor(cp + band) for every satellite
    multi: dict = field(default_factory=dict)   # position -> list of (first, second) written values, every chip combination
    qi: bool = False         # Q,I order: `rounded` and `alts` hold Q first


def noise(n: np.ndarray, sigma: float, seed: int) -> np.ndarray:
    """Complex noise at sample indices n (uint64)."""
    key = np.uint64((int(seed) * _NOISE_MUL) & _M64)
    with np.errstate(over="ignore"):
        h = splitmix64(key + np.asarray(n, dtype=np.uint64))
    u1 = ((h >> np.uint64(40)).astype(np.float64) + 0.5) / 16777216.0
    u2 = (h & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    r = sigma * np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2) + 1j * r * np.sin(2.0 * np.pi * u2)


def data_bits(seed: int, prn: int, s: int, b: np.ndarray, version: int) -> np.ndarray:
    """+-1 of satellite (prn, list position s) at bit indices b (int64, may be negative)."""
    const = (int(seed) ^ ((int(prn) << 48) & _M64)) & _M64
    if version == 2:
        const ^= (int(s) << 40) & _M64
    with np.errstate(over="ignore"):
        h = splitmix64(np.uint64(const) ^ (np.asarray(b, dtype=np.int64).view(np.uint64) * np.uint64(_GOLDEN)))
    return np.where((h & np.uint64(1)) != 0, 1.0, -1.0)


def _near_half(z: np.ndarray, delta: float, limit: int) -> np.ndarray:
    out = np.zeros(z.shape[0], dtype=bool)
    for v in (z.real, z.imag):
        d = np.abs(v - np.floor(v) - 0.5)
        out |= (d <= delta) & (np.abs(v) < limit - 0.5 + delta)
    return out


def _written(z: np.ndarray, limit: int, qi: bool) -> np.ndarray:
    dt = np.int8 if limit == 127 else np.int16
    a = np.clip(np.rint(z.real), -limit, limit).astype(dt)
    b = np.clip(np.rint(z.imag), -limit, limit).astype(dt)
    out = np.empty(2 * z.shape[0], dtype=dt)
    out[0::2], out[1::2] = (b, a) if qi else (a, b)
    return out


def evaluate(sats, n, fs: float, sigma: float, seed: int, version: int = 2, limit: int = 127, qi: bool = False, bits=None,
             delta: float = DELTA_F32, with_noise: bool = True) -> ModelRecord:
    """The record at sample indices n (any integers >= 0, in any order)."""
    assert version in (1, 2) and limit in (127, 32767)
    n = np.atleast_1d(np.asarray(n)).astype(np.int64)
    nf = n.astype(np.float64)
    base = noise(n.astype(np.uint64), sigma, seed) if (with_noise and sigma != 0.0) else np.zeros(n.shape[0], dtype=np.complex128)
    near_chip = np.zeros(n.shape[0], dtype=bool)
    edges = []                                   # per satellite with edge samples: (positions, lo - base, hi - base)
    for s, st in enumerate(sats):
        code = np.asarray(st.code, dtype=np.float64)
        pilot = None if st.pilot is None else np.asarray(st.pilot, dtype=np.float64) * np.exp(1j * st.pilot_phase)
        code_len = code.shape[0]
        ratio = st.code_rate / fs
        cp = (nf - st.code_phase_samples) * ratio
        t = st.carrier_phase / (2.0 * np.pi) + nf * ((st.intermediate_freq + st.doppler) / fs)
        carrier = st.amplitude * np.exp(2j * np.pi * (t - np.floor(t)))

        def component(chip_f, sel=slice(None)):
            chip = chip_f.astype(np.int64)
            idx = np.mod(chip, code_len)
            b = np.floor_divide(np.floor_divide(chip, code_len), st.bit_periods)
            d = data_bits(seed, st.prn, s, b, version) if bits is None else np.asarray(bits(s, b), dtype=np.float64)
            c = d * code[idx]
            if pilot is not None:
                c = c + pilot[idx]
            return c * carrier[sel]

        mine = component(np.floor(cp))
        base = base + mine
        band = CHIP_BAND * max(1.0, ratio)
        pos = np.nonzero(np.abs(cp - np.rint(cp)) <= band)[0]
        if pos.size:
            near_chip[pos] = True
            edges.append((pos, component(np.floor(cp[pos] - band), pos) - mine[pos], component(np.floor(cp[pos] + band), pos) - mine[pos]))
    lo, hi = base.copy(), base.copy()
    count = np.zeros(n.shape[0], dtype=np.int64)
    for pos, dlo, dhi in edges:
        lo[pos] += dlo
        hi[pos] += dhi
        count[pos] += 1
    near_half = _near_half(base, delta, limit) | _near_half(lo, delta, limit) | _near_half(hi, delta, limit)
    multi = {}
    for p in np.nonzero(count >= 2)[0]:
        choices = [(0.0, dlo[pos == p][0], dhi[pos == p][0]) for pos, dlo, dhi in edges if np.any(pos == p)]
        z = np.array([base[p] + sum(c) for c in itertools.product(*choices)])
        near_half[p] |= bool(_near_half(z, delta, limit).any())
        w = _written(z, limit, qi)
        multi[int(p)] = [(int(w[2 * k]), int(w[2 * k + 1])) for k in range(z.shape[0])]
    return ModelRecord(i=base.real, q=base.imag, rounded=_written(base, limit, qi), near_half=near_half, near_chip=near_chip,
                       alts=[_written(lo, limit, qi), _written(hi, limit, qi)], multi=multi, qi=qi)


def compare(record: np.ndarray, m: ModelRecord, chip_band: bool = True, cap_share: bool = True):
    """Holds a record (interleaved, as read back) to the model.  All of:
      * every component of every sample differs from the model's rounded value by at most 1;
      * outside near_half | near_chip the record equals the model exactly;
      * inside near_chip and outside near_half the record equals the model for one of the neighbouring chips;
      * near_half | near_chip covers at most BAND_SHARE_CAP of the samples.
    chip_band=False (a float64 generator with the model's own chip phase): near_chip excuses nothing.
    cap_share=False: the caller sums the banded shares of several short records of one case and caps the total itself.
    Returns (mismatching samples, largest distance from a half-integer among the mismatching components, banded share)."""
    rec = np.asarray(record)
    assert rec.dtype == m.rounded.dtype and rec.shape == m.rounded.shape, (rec.dtype, rec.shape, m.rounded.dtype, m.rounded.shape)
    diff = rec.astype(np.int64) - m.rounded.astype(np.int64)
    worst = int(np.abs(diff).max()) if diff.size else 0
    assert worst <= 1, f"a component is {worst} away from the model at component index {int(np.argmax(np.abs(diff)))}"
    bad = (diff[0::2] != 0) | (diff[1::2] != 0)
    near_chip = m.near_chip if chip_band else np.zeros_like(m.near_chip)
    banded = m.near_half | near_chip
    stray = np.nonzero(bad & ~banded)[0]
    assert stray.size == 0, f"{stray.size} samples differ from the model outside the bands, first at position {int(stray[0])}"
    for p in np.nonzero(bad & near_chip & ~m.near_half)[0]:
        got = (int(rec[2 * p]), int(rec[2 * p + 1]))
        cands = [(int(a[2 * p]), int(a[2 * p + 1])) for a in m.alts] + m.multi.get(int(p), [])
        assert got in cands, f"position {int(p)} on a chip edge: {got} is the model's value for neither neighbouring chip {cands}"
    share = float(np.count_nonzero(banded)) / max(1, banded.shape[0])
    if cap_share:
        assert share <= BAND_SHARE_CAP, f"the bands cover {share:.4f} of the samples"
    # distance from a half-integer of the components that came out differently (chip-edge samples aside)
    first, second = (m.q, m.i) if m.qi else (m.i, m.q)
    dist = 0.0
    sel = bad & m.near_half
    for v, d in ((first, diff[0::2]), (second, diff[1::2])):
        k = sel & (d != 0) & ~near_chip
        if k.any():
            dist = max(dist, float(np.abs(v[k] - np.floor(v[k]) - 0.5).max()))
    return int(np.count_nonzero(bad)), dist, share

