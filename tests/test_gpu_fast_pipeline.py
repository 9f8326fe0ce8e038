"""The replay instantiations of the fast kernel (csrc/corr_fast.hip) across chunk and block boundaries.

Since round 7 a wave issues the load of the next chunk only after the wait for the current chunk's words (two word buffers
alternate).  That changes nothing a lane computes; what can go wrong is state that crosses a boundary: words of the wrong chunk or
block in a buffer, a buffer overwritten while it is still read, the odd and even exits of the two-buffer loop, a walk that ends
early.  So the lists here are short blocks of mixed length - a wave's consecutive blocks run 1, 2, 3 and 4 iterations of the chunk
loop, in every order - instead of the workload's 18-iteration blocks.

Lists (12 interleaved channels at the GPS L1 C/A rate, 17.6 samples per chip at 18 Msps; built like the big lists of
tests/test_gpu_correlator_edges.py, whose rigs, records, oracle calls and bound are imported, not copied):
  lengths        600, 1 100, 2 100, 3 100 samples (38, 69, 132, 194 chunks of 16 = 1, 2, 3, 4 iterations of 64 lanes), assigned so that
                 the two blocks of a wave (epochs e and e + 4 of a channel) always differ; every last iteration has idle lanes
  alignment      a channel's epochs follow one another in the record from a start that is no multiple of 16, lengths that are no
                 multiple of 16: blocks start and end off a chunk boundary
  exact path     rem_code_phase = 0 with the rational step 1.023e6 / 18e6: samples 0 and 3000 k sit on a chip edge (prompt at 0,
                 early and late at 3000), their chunks take the float64 path: in the first iteration (sample 0), a middle one
                 (sample 3000 of a 3 100-sample block) and the last one (sample 3000 of a 3 010-sample block); these blocks are the
                 ones the host does not mark tie-free, the random ones around them are marked (asserted with the host's own
                 edge search, gc_debug_first_sample_near_edge, at half and at twice the band gc_mark_tie_free uses)
  spacing        one list with el_spacing = 0.3 chip: three ramps instead of the shared early/late one
  record end     the last block of every list ends on the record's last sample
  epochs         the planner gives a list the four-wave kernels from 4 epochs per compute unit on (csrc/launch_plan.h), so a list has
                 4 x CUs + 5 epochs (1 029 on an MI355X: the 64 - 128 the blocks would need do not reach these kernels); the + 5
                 leaves the last workgroups a short walk (lb >= nblocks)
  kernels        2 = four waves, int8-pair tables (two-arm channels, the rig of _replay_rig(2) widened to 12 channels);
                 3 = four waves, float tables (one-arm channels): bench.py's headline instantiation; 1 = one wave, from 8 x CUs + 7 of
                 the same blocks in an order without a channel period (one block per workgroup)
Expected values: the float64 oracle under test_gpu_correlator_edges.bound (2e-6 * sum(|I| + |Q|) per output), every block.
Run time: the ten cases take 4.2 s in all on an MI355X (every block of every list against the oracle; the lists are cached).
Neighbour independence: a block's sums are bitwise the same when the epochs of every channel are rotated by 1, 2 and 3 positions,
which puts the block on another wave, at another place of the walk and behind another block.
"""
import numpy as np
import pytest

import test_gpu_correlator_edges as E
from oracle import gnss_oracle as O

pytestmark = pytest.mark.gpu

NCH = 12
FS = 18e6
STEP_RATIONAL = 1.023e6 / 18e6
LENGTHS = (600, 1100, 2100, 3100)
LAST_ITER_EXACT = 3010            # 189 chunks: three iterations, sample 3000 in the last one
_CACHE = {}


def _rig(kernel):
    rng = np.random.default_rng(700 + kernel)
    if kernel == 2:    # as _replay_rig(2): two-arm channels at the L1 C/A rate
        chans = [E.Chan([O.pad_code(E._chips(rng, 1023)) for _ in range(2)], 1023) for _ in range(NCH)]
    else:              # one-arm L1 C/A channels
        chans = [E.Chan([O.pad_code(O.generate_ca_code(p))], 1023) for p in range(1, NCH + 1)]
    return E.Rig(f"pipeline{kernel}", FS, chans, 1.023e6, 0.5, seed=70 + kernel)


def _length(e, kind, c):
    """Length class of epoch e: epochs e and e + 4 (the two blocks of a wave) differ, and so do neighbours."""
    n = LENGTHS[(e + (e >> 2) + c) & 3]
    if kind == "exact" and n == 2100 and (e >> 4) & 1:            # still three iterations
        n = LAST_ITER_EXACT
    return n + (e * 5 + c) % 13       # no multiple of 16, not the same twice in a row


def _list(kernel, kind, cus):
    """(rig, record, descriptors) of one list; descriptor i = epoch i // NCH of channel i % NCH."""
    key = (kernel, kind, cus)
    if key in _CACHE:
        return _CACHE[key]
    rig = _rig(kernel)
    rng = np.random.default_rng(9000 + 10 * kernel + len(kind))
    epochs = 4 * cus + 5
    start = [3 + 7 * c + (5000 if c == NCH - 1 else 0) for c in range(NCH)]   # the last channel ends last: the list's last block ends the record
    descs = [None] * (epochs * NCH)
    at = list(start)
    for e in range(epochs):
        for c in range(NCH):
            n = _length(e, kind, c)
            exact = kind == "exact" and (e + c) % 3 == 0
            step = STEP_RATIONAL if exact else rig.step0 * (1 + float(rng.uniform(-3e-6, 3e-6)))
            descs[e * NCH + c] = dict(channel=c, n=n, s0=at[c], rem=0.0 if exact else float(rng.uniform(0, step)), step=step,
                                      d=0.3 if kind == "spacing" else rig.d0, f=E.IF + float(rng.uniform(-5e3, 5e3)),
                                      phi=float(rng.uniform(-3, 3)), tags={})
            at[c] += n
    last = descs[-1]
    nsamp = last["s0"] + last["n"]
    assert nsamp == max(at)                                       # the list's last block ends on the record's last sample
    rec = E.Record("i8_iq", seed=40 + kernel, nsamp=nsamp, plain=True)
    _CACHE[key] = (rig, rec, descs)
    return _CACHE[key]


def _edge_within(d, factor):
    """A sample of one of the block's three ramps lies within factor x 8e-6 samples of ramp of a table edge (gnsscorr.hip,
    gc_mark_tie_free: that band, for these block lengths, decides the tie-free mark of a fast-kernel list)."""
    from cu_sdr_collection_amd import _lib as L
    eps = factor * 8e-6 * d["step"]
    return any(L.load().gc_debug_first_sample_near_edge(a, d["step"], d["n"], eps) >= 0
               for a in (d["rem"] - d["d"], d["rem"], d["rem"] + d["d"]))


def _replay(engine, descs):
    engine.replay_prepare(E.blocks_of(engine, descs))
    engine.replay_launch()
    return engine.replay_fetch()


def _iters(d):
    chunks = ((d["s0"] + d["n"] - 1) >> 4) - (d["s0"] >> 4) + 1
    return (chunks + 63) // 64, chunks


@pytest.mark.parametrize("kind", ["mixed", "exact", "spacing"])
@pytest.mark.parametrize("kernel", [2, 3])
def test_short_blocks_of_mixed_length_match_the_oracle(engine, kernel, kind):
    _, cus = engine.device_info()
    rig, rec, descs = _list(kernel, kind, cus)
    # the list is what the docstring says it is
    its = [_iters(d) for d in descs]
    assert {i for i, _ in its} == {1, 2, 3, 4}
    assert all(ch % 64 != 0 for _, ch in its)                                              # idle lanes in every last iteration
    assert all(its[i][0] != its[i + 4 * NCH][0] for i in range(len(descs) - 4 * NCH))       # a wave's two blocks differ
    assert any(d["s0"] % 16 and (d["s0"] + d["n"]) % 16 for d in descs)
    assert descs[-1]["s0"] + descs[-1]["n"] == rec.nsamp
    if kind == "exact":
        ex = [d for d in descs if d["rem"] == 0.0]
        assert any(_iters(d)[0] == 1 for d in ex)                                          # sample 0: first = last iteration
        assert any(d["n"] > 3100 and _iters(d)[0] == 4 for d in ex)                        # sample 3000 in iteration 2 of 4
        assert any(3000 < d["n"] < 3100 and _iters(d)[0] == 3 and ((3000 + d["s0"] % 16) >> 4) >= 128 for d in ex)   # ... in the last of 3
        # both values of the tie-free mark occur: a sample well inside the band (not marked), none within twice the band (marked)
        assert all(_edge_within(d, 0.5) for d in ex)
        assert sum(not _edge_within(d, 2.0) for d in descs if d["rem"] != 0.0) > len(descs) // 2
    rec.load(engine, rig.fs)
    rig.setup(engine)
    got = _replay(engine, descs)
    assert engine.last_kernel() == kernel, (kernel, kind, engine.last_kernel())
    worst = 0.0
    for i, d in enumerate(descs):
        worst = max(worst, E.compare(rig, rec, d, [got[i]]))
    E.note(f"pipeline kernel {kernel} / {kind}", worst, len(descs))


@pytest.mark.parametrize("kernel", [2, 3])
def test_a_blocks_sums_do_not_depend_on_its_neighbours(engine, kernel):
    _, cus = engine.device_info()
    rig, rec, descs = _list(kernel, "exact", cus)
    rec.load(engine, rig.fs)
    rig.setup(engine)
    epochs = len(descs) // NCH
    base = _replay(engine, descs)
    assert engine.last_kernel() == kernel and base.any()
    for r in (1, 2, 3):
        rot = [descs[((i // NCH - r) % epochs) * NCH + i % NCH] for i in range(len(descs))]
        got = _replay(engine, rot)
        assert engine.last_kernel() == kernel
        back = got.reshape(epochs, NCH, *got.shape[1:])
        back = np.roll(back, -r, axis=0).reshape(got.shape)       # rotated list, position (e + r) -> the block of epoch e
        assert np.array_equal(back, base), (kernel, r, np.argwhere(np.any(back != base, axis=(1, 2)))[:8].ravel())


@pytest.mark.parametrize("kernel", [2, 3])
def test_the_same_blocks_on_the_one_wave_replay_kernel(engine, kernel):
    _, cus = engine.device_info()
    rig, rec, descs = _list(kernel, "exact", cus)
    rec.load(engine, rig.fs)
    rig.setup(engine)
    rng = np.random.default_rng(77)
    # no channel period, and enough blocks for one workgroup per block (fewer are split over several, one iteration each)
    pick = [int(x) for x in rng.permutation(len(descs) - 1)[:8 * cus + 6]] + [len(descs) - 1]       # ... and the record's last block
    sub = [descs[i] for i in pick]
    assert {_iters(d)[0] for d in sub} == {1, 2, 3, 4}
    got = _replay(engine, sub)
    assert engine.last_kernel() == 1, engine.last_kernel()
    worst = 0.0
    for k, d in enumerate(sub):
        worst = max(worst, E.compare(rig, rec, d, [got[k]]))
    E.note(f"pipeline kernel {kernel}'s blocks on the one-wave kernel", worst, len(sub))
