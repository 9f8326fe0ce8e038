"""The acquisition FFT's planner (csrc/acq_fft.hip: make_plan, factor, choose_cols) without a GPU, through the host-only hook
gc_debug_fft_plan: the coverage that the transform sweep of tests/test_gpu_acq_surfaces.py relies on is asserted here on the sweep's
own length list (tests/acq_fft_lengths.py).

Stage positions: factor() lists a pass's radices in non-increasing order and takes the FEWEST stages, so a radix-2 stage is always
the last one - a second 2 (or anything smaller) behind it would have been merged into a 4.  Radix 2 therefore has no inner position
in any plan; test_radix_2_is_never_an_inner_stage proves that over every pass length, and the coverage test asks for every other
(radix, position) pair in both passes.

Storage order: csrc/fft_plan.h states once which natural bin a storage position of a transform holds (every kernel that reads a
transform, and gc_debug_fft, go through it); tests/fft_order_shim.hip runs the two functions on the CPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import acq_fft_lengths as FL

RADICES = (2, 3, 4, 5, 6, 8)
GC_E_UNSUPPORTED = -6


def _plan(n):
    import cu_sdr_collection_amd as P
    return P.Engine.debug_fft_plan(n)


def _positions(rad):
    """{(radix, position)} of one pass: a single stage is both the first and the last one."""
    pos = set()
    if rad:
        pos.add((rad[0], "first"))
        pos.add((rad[-1], "last"))
        pos.update((r, "inner") for r in rad[1:-1])
    return pos


def test_plans_are_factorisations_within_the_kernels_limits():
    for n in FL.SWEEP:
        p = _plan(n)
        assert p["n1"] * p["n2"] == n and 1 <= p["n1"] and p["n2"] <= 2048, (n, p)
        for length, rad, cols, stride in ((p["n1"], p["rad1"], p["cols1"], p["n2"]), (p["n2"], p["rad2"], p["cols2"], 1)):
            prod = 1
            for r in rad:
                prod *= r
            assert prod == length and all(r in RADICES for r in rad) and rad == sorted(rad, reverse=True), (n, p)
            # a tile is cols vectors in LDS twice over and at most 8 x 256 accumulator slots (choose_cols, kFftSlots)
            assert 1 <= cols <= 16 and length * cols <= 2048, (n, p)


def test_sweep_lengths_reach_every_stage_position_and_tile_case():
    plans = {n: _plan(n) for n in FL.SWEEP}
    want = {(r, pos) for r in RADICES for pos in ("first", "inner", "last")} - {(2, "inner")}   # (module docstring)
    for key in ("rad1", "rad2"):
        seen = set().union(*(_positions(p[key]) for p in plans.values()))
        assert want <= seen, (key, sorted(want - seen))
    assert any(p["n1"] == 1 for p in plans.values())
    assert any(2048 in (p["n1"], p["n2"]) for p in plans.values())
    # more than one tile and a last tile that is not full, in a columns pass (n2 vectors) and in a rows pass (n1 vectors)
    assert any(p["n2"] > p["cols1"] and p["n2"] % p["cols1"] for p in plans.values())
    assert any(p["n1"] > p["cols2"] and p["n1"] % p["cols2"] for p in plans.values())
    small = [n for n in FL.SWEEP_SMALL if n < 10000]
    assert len(FL.SWEEP_SMALL) <= 45 and len(small) >= 0.8 * len(FL.SWEEP_SMALL)


def test_radix_2_is_never_an_inner_stage():
    """The exception the coverage test makes, over every pass length the kernels take: length x length plans both passes alike."""
    import cu_sdr_collection_amd as P
    for length in range(2, 2049):
        try:
            p = _plan(length * length)
        except P.GnssCorrError:
            continue                          # a prime factor above 5
        assert p["n1"] == length and p["n2"] == length
        assert (2, "inner") not in _positions(p["rad1"]) and p["rad1"].count(2) <= 1, (length, p)


def test_production_shapes_are_the_specialised_ones():
    for n, (n1, n2) in FL.PRODUCTION.items():
        p = _plan(n)
        rad1, rad2 = FL.PRODUCTION_SHAPES[n]
        assert (p["n1"], p["n2"], p["rad1"], p["rad2"]) == (n1, n2, rad1, rad2), (n, p)
    assert _plan(320000)["n1"] == 320    # make_plan's kSplit, not the most square 512 x 625


@pytest.mark.parametrize("n", FL.REFUSED_PRIME + FL.REFUSED_LONG)
def test_lengths_the_planner_refuses(n):
    import cu_sdr_collection_amd as P
    with pytest.raises(P.GnssCorrError) as e:
        _plan(n)
    assert e.value.status == GC_E_UNSUPPORTED
    if n in FL.REFUSED_LONG:   # these factor into {2, 3, 5}: it is the rows pass that is too long
        m = n
        for q in (2, 3, 5):
            while m % q == 0:
                m //= q
        assert m == 1


def _order_shim():
    from cu_sdr_collection_amd import build as B
    here = os.path.dirname(os.path.abspath(__file__))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src, out = os.path.join(here, "fft_order_shim.hip"), os.path.join(here, "build", "libfft_order_shim.so")
    deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = [f for f in B._tu_flags("probe.hip") if f != "--offload-compress"]
        subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.order_shim_bin_at.argtypes = lib.order_shim_pos_of.argtypes = [C.c_int, C.c_int, C.c_int]
    return lib


def test_storage_order_is_a_bijection_with_its_inverse_and_the_stated_layout():
    """Position k1 n2 + k2 holds bin k1 + n1 k2.  6, 12, 60, 72, 1000 and 32768 split into n1 != n2: a swapped pair fails there
    (and passes at the squares 4, 100 and 4096)."""
    lib = _order_shim()
    for n in (4, 6, 12, 60, 72, 100, 1000, 4096, 32768):
        p = _plan(n)
        n1, n2 = p["n1"], p["n2"]
        assert n1 * n2 == n
        if n in (6, 12, 60, 72, 1000, 32768):
            assert n1 != n2, (n, n1, n2)
        pos = [lib.order_shim_pos_of(b, n1, n2) for b in range(n)]
        assert sorted(pos) == list(range(n)), n                                            # bin -> storage: a bijection of [0, n)
        assert all(lib.order_shim_bin_at(pos[b], n1, n2) == b for b in range(n)), n        # storage -> bin: its inverse
        assert all(lib.order_shim_bin_at(k1 * n2 + k2, n1, n2) == k1 + n1 * k2 and pos[k1 + n1 * k2] == k1 * n2 + k2
                   for k1 in range(n1) for k2 in range(n2)), n
