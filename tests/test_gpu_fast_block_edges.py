"""The replay instantiations of the fast kernel (csrc/corr_fast.hip) at the edges of a block.

Since round 9 these instantiations mask a block's first and last chunk from a wave-uniform sample range (one lane of the first
iteration, one of the last, masks formed on the scalar unit by the range form of mask_words), read the channel's constants once per
workgroup, update the accumulators of the Horner step in place and add the wavefront's sums with one DPP add per broadcast step.
None of that changes what a lane computes; what can go wrong sits at the edges: a mask on the wrong lane or of the wrong width,
head and tail mask in one chunk, a last iteration without idle lanes (or with one active lane), an idle lane that takes the tail
lane's mask or keeps a stale table index, the exact path in a masked chunk.  So the lists here cross the alignments of a block's
first and last sample with the lengths at which the walk changes shape.

Lists (12 interleaved channels at the GPS L1 C/A rate; rigs, records, oracle calls and the bound are those of
tests/test_gpu_correlator_edges.py, the rig and replay helpers those of tests/test_gpu_fast_pipeline.py - imported, not copied):
  alignment      first sample mod 16 in {0, 1, 15} x (first sample + length) mod 16 in {0, 1, 15}: no head mask / 15 and 1 valid
                 samples in the first chunk, no tail mask / 1 and 15 valid samples in the last chunk
  lengths        per alignment pair the SHORTEST block there is (1 .. 16 samples: one chunk that carries head and tail mask
                 together, or two chunks; the validator and the planner take blocks from one sample on), exactly 64 chunks (one
                 iteration, no idle lane), 65 chunks (the last iteration has ONE active lane) and 127 chunks (128 - 1)
  exact path     blocks with rem_code_phase = 0 and the rational step 1.023e6 / 18e6: sample 0 sits on a chip edge, the first
                 chunk takes the float64 path; in every length class, so also in a first chunk that is the last one as well
  spacing        one list with el_spacing = 0.3 chip: three ramps instead of the shared early/late one
  record end     the list's last block ends on the record's last sample, with a partial last chunk
  epochs         4 x CUs + 5 (csrc/launch_plan.h: the four-wave kernels from 4 epochs per compute unit on)
  kernels        3 = four waves, float tables (bench.py's headline instantiation); 2 = four waves, int8-pair tables (two-arm
                 channels); 1 = one wave, from 8 x CUs + 7 of the same blocks in an order without a channel period
Expected values: the float64 oracle under test_gpu_correlator_edges.bound (2e-6 * sum(|I| + |Q|) per output), every block.
Neighbour independence: a block's sums are bitwise the same when the epochs of every channel are rotated by one position.
"""
import numpy as np
import pytest

import test_gpu_correlator_edges as E
import test_gpu_fast_pipeline as PL

pytestmark = pytest.mark.gpu

NCH = PL.NCH
ALIGN = (0, 1, 15)
CLASSES = ("short", 64, 65, 127)                       # chunks of 16 samples
COMBOS = [(a, b, k) for k in CLASSES for a in ALIGN for b in ALIGN]
_CACHE = {}


def _length(a, b, k):
    """Samples of a block that starts a samples into a chunk, ends b samples into one (0: on a chunk boundary) and covers k chunks."""
    if k == "short":
        k = 1 if (b == 0 or b > a) else 2
    return (16 * k - a) if b == 0 else (16 * (k - 1) + b - a)


def _chunks(d):
    return ((d["s0"] + d["n"] - 1) >> 4) - (d["s0"] >> 4) + 1


def _list(kernel, kind, cus):
    """(rig, record, descriptors, combo of every descriptor); descriptor i = epoch i // NCH of channel i % NCH."""
    key = (kernel, kind, cus)
    if key in _CACHE:
        return _CACHE[key]
    rig = PL._rig(kernel)
    rng = np.random.default_rng(9900 + 10 * kernel + len(kind))
    epochs = 4 * cus + 5
    at = [3 + 7 * c for c in range(NCH)]
    descs, combos = [None] * (epochs * NCH), [None] * (epochs * NCH)
    for e in range(epochs):
        for c in range(NCH):
            i = e * NCH + c
            a, b, k = COMBOS[(e + 3 * c) % len(COMBOS)]
            if i == epochs * NCH - 1:                              # the list's last block: behind every other one, partial last chunk
                a, b, k = 1, 15, 65
                at[c] = max(at)
            s0 = at[c] + (a - at[c]) % 16
            n = _length(a, b, k)
            exact = (e + c) % 5 == 0
            step = PL.STEP_RATIONAL if exact else rig.step0 * (1 + float(rng.uniform(-3e-6, 3e-6)))
            descs[i] = dict(channel=c, n=n, s0=s0, rem=0.0 if exact else float(rng.uniform(0, step)), step=step,
                            d=0.3 if kind == "spacing" else rig.d0, f=E.IF + float(rng.uniform(-5e3, 5e3)),
                            phi=float(rng.uniform(-3, 3)), tags={})
            combos[i] = (a, b, k, exact)
            at[c] = s0 + n + int(rng.integers(0, 3))               # the next block of the channel: right behind, or a sample or two on
    nsamp = descs[-1]["s0"] + descs[-1]["n"]
    assert nsamp >= max(at) - 2 and all(d["s0"] + d["n"] <= nsamp for d in descs)
    rec = E.Record("i8_iq", seed=60 + kernel, nsamp=nsamp, plain=True)
    _CACHE[key] = (rig, rec, descs, combos)
    return _CACHE[key]


def _check_list(rec, descs, combos):
    """The list is what the docstring says it is."""
    for d, (a, b, k, _) in zip(descs, combos):
        assert d["s0"] % 16 == a and (d["s0"] + d["n"]) % 16 == b and d["n"] >= 1
        assert _chunks(d) == (k if k != "short" else (1 if (b == 0 or b > a) else 2))
    seen = {(a, b, k, x) for a, b, k, x in combos}
    assert {(a, b, k) for a, b, k, x in seen} >= set(COMBOS)                                 # every alignment pair in every length class
    assert {(k, x) for a, b, k, x in seen} == {(k, x) for k in CLASSES for x in (False, True)}   # the exact path in every class
    short = [d for d, cb in zip(descs, combos) if cb[2] == "short"]
    assert min(d["n"] for d in short) == 1 and max(d["n"] for d in short) == 16
    assert any(_chunks(d) == 1 and d["s0"] % 16 and (d["s0"] + d["n"]) % 16 for d in short)  # head and tail mask in one chunk
    assert any(cb == (1, 15, "short", True) for cb in combos)                                # ... on the exact path too
    assert descs[-1]["s0"] + descs[-1]["n"] == rec.nsamp and rec.nsamp % 16 == 15


@pytest.mark.parametrize("kind", ["edges", "spacing"])
@pytest.mark.parametrize("kernel", [2, 3])
def test_block_edges_match_the_oracle(engine, kernel, kind):
    _, cus = engine.device_info()
    rig, rec, descs, combos = _list(kernel, kind, cus)
    _check_list(rec, descs, combos)
    rec.load(engine, rig.fs)
    rig.setup(engine)
    got = PL._replay(engine, descs)
    assert engine.last_kernel() == kernel, (kernel, kind, engine.last_kernel())
    worst = 0.0
    for i, d in enumerate(descs):
        worst = max(worst, E.compare(rig, rec, d, [got[i]]))
    E.note(f"block edges kernel {kernel} / {kind}", worst, len(descs))


@pytest.mark.parametrize("kernel", [2, 3])
def test_a_blocks_sums_do_not_depend_on_its_neighbours(engine, kernel):
    _, cus = engine.device_info()
    rig, rec, descs, _ = _list(kernel, "edges", cus)
    rec.load(engine, rig.fs)
    rig.setup(engine)
    epochs = len(descs) // NCH
    base = PL._replay(engine, descs)
    assert engine.last_kernel() == kernel and base.any()
    rot = [descs[((i // NCH - 1) % epochs) * NCH + i % NCH] for i in range(len(descs))]
    got = PL._replay(engine, rot)
    assert engine.last_kernel() == kernel
    back = got.reshape(epochs, NCH, *got.shape[1:])
    back = np.roll(back, -1, axis=0).reshape(got.shape)           # rotated list, position e + 1 -> the block of epoch e
    assert np.array_equal(back, base), (kernel, np.argwhere(np.any(back != base, axis=(1, 2)))[:8].ravel())


@pytest.mark.parametrize("kernel", [2, 3])
def test_the_same_blocks_on_the_one_wave_replay_kernel(engine, kernel):
    _, cus = engine.device_info()
    rig, rec, descs, combos = _list(kernel, "edges", cus)
    rec.load(engine, rig.fs)
    rig.setup(engine)
    rng = np.random.default_rng(99)
    # no channel period, and enough blocks for one workgroup per block (fewer are split over several)
    pick = [int(x) for x in rng.permutation(len(descs) - 1)[:8 * cus + 6]] + [len(descs) - 1]       # ... and the record's last block
    sub = [descs[i] for i in pick]
    assert {combos[i][:3] for i in pick} >= set(COMBOS)
    got = PL._replay(engine, sub)
    assert engine.last_kernel() == 1, engine.last_kernel()
    worst = 0.0
    for k, d in enumerate(sub):
        worst = max(worst, E.compare(rig, rec, d, [got[k]]))
    E.note(f"block edges kernel {kernel}'s blocks on the one-wave kernel", worst, len(sub))
