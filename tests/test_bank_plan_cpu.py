"""The host plan of the tap bank family (csrc/bank_plan.h: the argument checks, the sub-batch cut, the integrate walk, the search
walk) without a GPU: tests/bank_plan_shim.hip runs it on the CPU under budgets of a few chunks and blocks, so that short lists are
cut where the tests choose, and returns every index, flag and row number the drivers hand to the kernels and the copies.

The kernels are modelled symbolically: an accumulator is the list of (block, the block its dn refers to, weight) added to it, a map
the list of such lists.  ddm_integrate_kernel, ddm_power_kernel and search_integrate_kernel are "reset or carry, append, store";
the drivers' fetches and moves are list assignments.  What comes back must be every run's blocks and every map's runs, in order,
once, in the caller's row - wherever the cuts fall.

Refusals: the status lists of the four GPU refusal tests (test_gpu_correlate_bank.py, test_gpu_correlate_ddm.py,
test_gpu_ddm_integrate.py, test_gpu_ddm_search.py) restated on channel facts, with the accepted calls that close them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FS = 18e6
SIZES = (1, 1023, 1024, 1025, 4097)                      # 1, 1, 1, 2 and 5 chunks
BUDGETS = (1, 2, 3, 5, 7, 0)                             # chunks per sub-batch; 0: the library's budget, everything in one
TILES = (1, 2, 3, 0)                                     # blocks per tile; 0: the library's budget, a sub-batch in one
LONG_RUN = 30                                            # blocks of >= 1 chunk against <= 7 chunks: more than four sub-batches
SRCH_IN, SRCH_RUN_START, SRCH_RUN_END, SRCH_MAP_START, SRCH_MAP_END = 1, 2, 4, 8, 16
BLOCK = np.dtype([("channel", "<i4"), ("blksize", "<i4"), ("first_sample", "<i8"), ("rem", "<f8"), ("step", "<f8"), ("d", "<f8"),
                  ("f", "<f8"), ("phi", "<f8"), ("off", "<i4", 3), ("res", "<i4")])
I32P, F64P, I64P = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_longlong)
_LIB = []


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    return hipcc


def _built(name, out, extra):
    """tests/<name> compiled with the flags of corr_bank.hip (+ extra) to tests/build/<out>, when it or a header is newer."""
    from cu_sdr_collection_amd import build as B
    src, out = os.path.join(HERE, name), os.path.join(HERE, "build", out)
    deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = [f for f in B._tu_flags("corr_bank.hip") if f != "--offload-compress"]
        subprocess.run([_hipcc(), *flags, *extra, src, "-o", out], check=True)
    return out


def _shim():
    if not _LIB:
        from cu_sdr_collection_amd import _lib as L
        assert BLOCK.itemsize == C.sizeof(L.gc_block)
        lib = C.CDLL(_built("bank_plan_shim.hip", "libbank_plan_shim.so", ["-shared"]))
        lib.bank_shim_create.restype = C.c_void_p
        lib.bank_shim_create.argtypes = [C.c_int, C.c_ulonglong, C.c_double]
        lib.bank_shim_destroy.argtypes = [C.c_void_p]
        lib.bank_shim_set_double.argtypes = [C.c_void_p, C.c_int]
        lib.bank_shim_set_channel.argtypes = [C.c_void_p] + [C.c_int] * 5
        lib.bank_shim_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, F64P, C.c_int, F64P]
        lib.bank_shim_check_integrate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, F64P, C.c_int, F64P, C.c_int, F64P, C.c_int, I32P, C.c_int, I32P,
                                                  C.c_int, C.c_int]
        lib.bank_shim_check_search.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, I32P, F64P, C.c_int, F64P, C.c_int, F64P, C.c_int, I32P,
                                               C.c_int, I32P, C.c_int, C.c_int, C.c_int]
        lib.bank_shim_tile_blocks.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_longlong]
        lib.bank_shim_cut.restype = lib.bank_shim_integrate.restype = lib.bank_shim_search.restype = C.c_longlong
        lib.bank_shim_cut.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_longlong, I64P, C.c_longlong]
        lib.bank_shim_integrate.argtypes = [C.c_int, C.c_void_p, F64P, C.c_int, I32P, C.c_int, I32P, C.c_longlong, C.c_longlong, I64P, C.c_longlong,
                                            F64P]
        lib.bank_shim_search.argtypes = [C.c_int, C.c_void_p, F64P, C.c_int, I32P, C.c_int, I32P, C.c_int, I32P] + [C.c_int] * 5 + \
                                        [C.c_longlong, C.c_longlong, I64P, C.c_longlong, F64P]
        _LIB.append(lib)
    return _LIB[0]


def _i32(x):
    a = np.ascontiguousarray(x, dtype=np.int32)
    return a, a.ctypes.data_as(I32P)


def _f64(x):
    if x is None:
        return None, None
    a = np.ascontiguousarray(x, dtype=np.float64)
    return a, a.ctypes.data_as(F64P)


# ---- the seeded lists ---------------------------------------------------------------------------------------------------------------
class Case:
    """Blocks of SIZES; runs of 1, 2, 3 and 7 blocks and one of LONG_RUN; maps of 1 and 3 runs (or none); seven blocks more than the
    runs hold, so that windows at shifts up to 7 fit.  first_sample is distinct per block: a dn names the block it refers to."""

    def __init__(self, seed, budget):
        rng = np.random.default_rng(seed)
        self.budget = budget
        self.map_len = [int(x) for x in rng.choice((1, 3), size=int(rng.integers(3, 7)))]
        nruns = sum(self.map_len)
        self.run_len = [int(x) for x in rng.choice((1, 2, 3, 7), size=nruns)]
        self.run_len[int(rng.integers(0, nruns))] = LONG_RUN
        if seed % 4 == 3:
            self.map_len = []
        self.nused = sum(self.run_len)
        nb = self.nused + 7
        self.blocks = np.zeros(nb, dtype=BLOCK)
        self.blocks["blksize"] = rng.choice(SIZES, size=nb)
        self.blocks["first_sample"] = rng.permutation(nb) * 5000 + rng.integers(0, 100, nb)
        self.run_start = np.concatenate([[0], np.cumsum(self.run_len)]).astype(int)
        self.map_start = np.concatenate([[0], np.cumsum(self.map_len)]).astype(int)
        self.block_of = {int(s): k for k, s in enumerate(self.blocks["first_sample"])}
        self.chunks = -(-self.blocks["blksize"].astype(int) // 1024)

    def expected(self, shift, weights):
        """(runs, maps) of the window at `shift`: what the definition adds, in its order."""
        runs = [[(shift + b, shift + int(self.run_start[r]), float(weights[shift + b])) for b in range(self.run_start[r], self.run_start[r + 1])]
                for r in range(len(self.run_len))]
        maps = [[tuple(runs[r]) for r in range(self.map_start[q], self.map_start[q + 1])] for q in range(len(self.map_len))]
        return runs, maps


CASES = [Case(100 * k + i, b) for k, b in enumerate(BUDGETS) for i in range(8)]


# ---- sub-batches ----------------------------------------------------------------------------------------------------------------------
def _cut(case, row=2):
    out = np.zeros(3 * len(case.blocks), dtype=np.int64)
    n = _shim().bank_shim_cut(len(case.blocks), case.blocks.ctypes.data, row, 8 * row * case.budget, out.ctypes.data_as(I64P), out.size)
    assert 0 < n <= out.size and n % 3 == 0
    return out[:n].reshape(-1, 3)


def test_sub_batches_cover_the_list_once_in_order_within_the_budget():
    singles = 0
    for case in CASES:
        for row in (2, 24):
            cuts = _cut(case, row)
            assert cuts[0, 0] == 0 and np.array_equal(cuts[1:, 0], (cuts[:, 0] + cuts[:, 1])[:-1]) and cuts[-1, 0] + cuts[-1, 1] == len(case.blocks)
            for first, nb, chunks in cuts:
                assert nb >= 1 and chunks == case.chunks[first:first + nb].sum()
                if case.budget:
                    assert chunks <= case.budget or nb == 1
                    singles += chunks > case.budget
                    if first + nb < len(case.blocks):                  # and the next block would not have fitted
                        assert chunks + case.chunks[first + nb] > case.budget
            assert case.budget or len(cuts) == 1
    assert singles > 10                                                 # blocks larger than the budget go alone


# ---- integrate ------------------------------------------------------------------------------------------------------------------------
def _integrate_walk(case, blocks, weights):
    """The shim's walk over `blocks` (the runs hold them all), parsed: (sizes, steps)."""
    lib = _shim()
    out = np.zeros(64 * len(blocks) + 64, dtype=np.int64)
    wout = np.zeros(len(blocks))
    _, runs = _i32(case.run_len)
    _, maps = _i32(case.map_len)
    _, w = _f64(weights)
    n = lib.bank_shim_integrate(len(blocks), blocks.ctypes.data, w, len(case.run_len), runs, len(case.map_len), maps, 1, 16 * case.budget,
                                out.ctypes.data_as(I64P), out.size, wout.ctypes.data_as(F64P))
    assert 4 <= n <= out.size and out[0] == 0
    sizes, pos, steps = tuple(int(x) for x in out[1:4]), 4, []
    names = ("first", "nb", "r0", "nr", "nfin", "q0", "nm", "mfin", "carry_run", "carry_map", "keep_run", "keep_map", "chunks")
    while pos < n:
        s = dict(zip(names, (int(x) for x in out[pos:pos + 13])))
        pos += 13
        for key, count in (("run_base", s["nr"] + 1), ("map_base", s["nm"] + 1 if s["nm"] else 0), ("dn", s["nb"])):
            s[key] = [int(x) for x in out[pos:pos + count]]
            pos += count
        s["w"] = wout[s["first"]:s["first"] + s["nb"]]
        steps.append(s)
    assert pos == n
    return sizes, steps


def _integrate_model(case, blocks, shift, sizes, steps):
    """The kernels and copies of ddm_integrate_run on lists.  Returns what reaches the caller: ({run: list}, {map: list})."""
    max_nb, max_nr, max_nm = sizes
    coh, pw = [None] * max_nr, [None] * max(max_nm, 1)                  # BANK_COH, BANK_POW as the pre-walk sized them
    runs_out, maps_out = {}, {}
    for s in steps:
        assert 1 <= s["nb"] <= max_nb and 1 <= s["nr"] <= max_nr and s["nm"] <= max_nm
        assert s["run_base"][0] == 0 and s["run_base"][-1] == s["nb"]
        for r in range(s["nr"]):                                         # ddm_integrate_kernel
            acc = list(coh[0]) if r == 0 and s["carry_run"] else []
            for b in range(s["run_base"][r], s["run_base"][r + 1]):
                ref = case.block_of[int(blocks["first_sample"][s["first"] + b]) - s["dn"][b]]
                acc.append((shift + s["first"] + b, ref, float(s["w"][b])))
            coh[r] = acc
        if s["nm"] > 0:
            assert s["map_base"][0] == 0 and s["map_base"][-1] == s["nfin"]
            for q in range(s["nm"]):                                     # ddm_power_kernel
                acc = list(pw[0]) if q == 0 and s["carry_map"] else []
                acc += [tuple(coh[r]) for r in range(s["map_base"][q], s["map_base"][q + 1])]
                pw[q] = acc
            for k in range(s["mfin"]):
                assert s["q0"] + k not in maps_out
                maps_out[s["q0"] + k] = pw[k]
            if s["keep_map"]:
                pw[0] = pw[s["keep_map"]]
        for k in range(s["nfin"]):
            assert s["r0"] + k not in runs_out
            runs_out[s["r0"] + k] = coh[k]
        if s["keep_run"]:
            coh[0] = coh[s["keep_run"]]
    return runs_out, maps_out


def _integrate(case, shift=0):
    blocks = np.ascontiguousarray(case.blocks[shift:shift + case.nused])
    weights = np.arange(len(case.blocks)) + 0.25
    sizes, steps = _integrate_walk(case, blocks, weights[shift:shift + case.nused])
    return steps, _integrate_model(case, blocks, shift, sizes, steps), case.expected(shift, weights)


def test_the_integrate_walk_adds_every_run_and_map_once_in_order_wherever_it_is_cut():
    seen = dict(on_run_boundary=0, inside_run=0, run_cut_twice=0, map_and_run_cut=0, map_ends_with_sub_batch=0)
    for case in CASES:
        steps, (runs_out, maps_out), (runs, maps) = _integrate(case)
        assert [s["first"] for s in steps] == [int(c[0]) for c in _cut(case) if c[0] < case.nused]      # bank_cut's walk, whatever the runs
        assert sum(s["nb"] for s in steps) == case.nused
        for s in steps:
            assert s["chunks"] <= case.budget or s["nb"] == 1 or not case.budget
        assert runs_out == dict(enumerate(runs)) and maps_out == dict(enumerate(maps))     # exact, each once, nothing unfinished
        for r, run in enumerate(runs):
            assert all(ref == case.run_start[r] for _, ref, _ in run)                      # dn refers to the run's first block
        seams = [s["first"] for s in steps[1:]]
        inside = {}
        for seam in seams:
            r = int(np.searchsorted(case.run_start, seam, side="right")) - 1
            if case.run_start[r] == seam:
                seen["on_run_boundary"] += 1
                seen["map_ends_with_sub_batch"] += any(case.run_start[m] == seam for m in case.map_start[1:])
            else:
                seen["inside_run"] += 1
                inside[r] = inside.get(r, 0) + 1
                if case.map_len:
                    q = int(np.searchsorted(case.map_start, r, side="right")) - 1
                    seen["map_and_run_cut"] += case.map_start[q] < r                          # the map already holds finished runs
        seen["run_cut_twice"] += sum(n >= 2 for n in inside.values())
    print(f"\n[bank plan] integrate seams: {seen}")
    assert min(seen.values()) >= 5, seen


def test_the_integrate_walk_without_weights_weighs_every_block_with_one():
    case = CASES[0]
    _, steps = _integrate_walk(case, np.ascontiguousarray(case.blocks[:case.nused]), None)
    assert all((s["w"] == 1.0).all() for s in steps)


# ---- search ---------------------------------------------------------------------------------------------------------------------------
def _per_block(nhyp, nfreq, cells, arms, want_coh, want_maps):
    """What a block of a tile costs (search_tile_blocks): SearchAux, rotations, a finished run, a finished map and its peaks."""
    return nhyp * (24 + 16 * nfreq + (16 * cells if want_coh else 0) + ((8 * cells + 16 * arms) if want_maps else 0))


def _search_walk(case, shifts, weights, tile, want_maps):
    lib = _shim()
    nb, nhyp = len(case.blocks), len(shifts)
    out = np.zeros(8 * nb * (nhyp + 2) + 64, dtype=np.int64)
    wout = np.full((nhyp, nb), np.nan)
    _, runs = _i32(case.run_len)
    _, maps = _i32(case.map_len)
    _, sh = _i32(shifts)
    _, w = _f64(weights)
    n = lib.bank_shim_search(nb, case.blocks.ctypes.data, w, nhyp, sh, len(case.run_len), runs, len(case.map_len), maps, 1, int(want_maps), 1, 1, 1,
                             16 * case.budget, tile * _per_block(nhyp, 1, 1, 1, True, want_maps), out.ctypes.data_as(I64P), out.size,
                             wout.ctypes.data_as(F64P))
    assert 2 <= n <= out.size and out[0] == 0
    assert tile == 0 or out[1] == tile
    pos, tiles = 2, []
    while pos < n:
        t = dict(zip(("first", "t0", "nt", "any", "nslot_r", "nslot_m"), (int(x) for x in out[pos:pos + 6])))
        pos += 6
        per = out[pos:pos + 4 * nhyp].reshape(nhyp, 4)
        pos += 4 * nhyp
        t["runs_now"], t["maps_now"], t["runs_done"], t["maps_done"] = (per[:, k].tolist() for k in range(4))
        aux = out[pos:pos + 2 * nhyp * t["nt"]].reshape(nhyp, t["nt"], 2)
        pos += 2 * nhyp * t["nt"]
        t["dn"], t["flags"] = aux[:, :, 0], aux[:, :, 1]
        tiles.append(t)
    assert pos == n
    return tiles, wout


def _search_model(case, nhyp, tiles, wout, want_maps):
    """search_integrate_kernel and the driver's scatter on lists.  Returns per hypothesis ({run: list}, {map: list}) and the number
    of tiles no hypothesis looks at."""
    racc, macc = [[] for _ in range(nhyp)], [[] for _ in range(nhyp)]     # BANK_RACC, BANK_MACC
    runs_out, maps_out = [{} for _ in range(nhyp)], [{} for _ in range(nhyp)]
    done, skipped, b_next = [[0, 0] for _ in range(nhyp)], 0, 0
    for t in tiles:
        assert t["first"] + t["t0"] == b_next                             # the tiles cover the list once, in order
        b_next += t["nt"]
        assert [d[0] for d in done] == t["runs_done"] and [d[1] for d in done] == t["maps_done"]
        if not t["any"]:                                                  # skipped by the driver: nothing may have been asked of it
            skipped += 1
            assert not t["flags"].any() and not any(t["runs_now"]) and not any(t["maps_now"])
            continue
        assert t["flags"].any()
        for h in range(nhyp):
            assert t["runs_now"][h] <= t["nslot_r"] and t["maps_now"][h] <= t["nslot_m"]
            coh_slot, pow_slot = [], []
            for k in range(t["nt"]):
                f, b = int(t["flags"][h, k]), t["first"] + t["t0"] + k
                if not f & SRCH_IN:
                    assert f == 0
                    continue
                if f & SRCH_RUN_START:
                    racc[h] = []
                if f & SRCH_MAP_START:
                    macc[h] = []
                racc[h] = racc[h] + [(b, case.block_of[int(case.blocks["first_sample"][b]) - int(t["dn"][h, k])], float(wout[h, b]))]
                if f & SRCH_RUN_END:
                    coh_slot.append(racc[h])
                    macc[h] = macc[h] + [tuple(racc[h])]
                    if f & SRCH_MAP_END:
                        pow_slot.append(macc[h])
            assert len(coh_slot) == t["runs_now"][h] and len(pow_slot) == t["maps_now"][h]
            for k, run in enumerate(coh_slot):                            # the scatter: slot k to the caller's row done + k
                assert t["runs_done"][h] + k not in runs_out[h]
                runs_out[h][t["runs_done"][h] + k] = run
            for k, m in enumerate(pow_slot):
                assert t["maps_done"][h] + k not in maps_out[h]
                maps_out[h][t["maps_done"][h] + k] = m
            done[h][0] += len(coh_slot)
            done[h][1] += len(pow_slot)
        assert t["nslot_r"] == max(t["runs_now"]) and t["nslot_m"] == max(t["maps_now"])
    assert b_next == len(case.blocks)
    return runs_out, maps_out, skipped


def _shifts(nhyp, rng):
    return [int(rng.choice((0, 7)))] if nhyp == 1 else ([7, 0, 1, 7] + [int(x) for x in rng.choice([0, 1, 7], size=16)])[:nhyp]


def test_every_hypothesis_of_the_search_walk_is_the_integrate_walk_on_its_window():
    skipped, one_block_tiles, walks = 0, 0, 0
    window = {}                                                           # (case, shift): the integrate model on that window
    for ci, case in enumerate(CASES):
        rng = np.random.default_rng(7000 + ci)
        for nhyp in (1, 3, 20):
            tile = TILES[(ci + nhyp) % 4]
            want_maps = bool(case.map_len) and (ci + nhyp) % 5 != 0
            shifts = _shifts(nhyp, rng)
            assert nhyp < 20 or (sorted(set(shifts)) == [0, 1, 7] and shifts[0] > shifts[1])
            weights = None if (ci + nhyp) % 3 == 0 else (np.arange(nhyp * len(case.blocks)).reshape(nhyp, -1) % 977) - 400.5
            tiles, wout = _search_walk(case, shifts, weights, tile, want_maps)
            runs_out, maps_out, sk = _search_model(case, nhyp, tiles, wout, want_maps)
            skipped += sk
            one_block_tiles += sum(t["nt"] == 1 for t in tiles)
            walks += 1
            for h, s in enumerate(shifts):
                if (ci, s) not in window:
                    _, got, want = _integrate(case, s)
                    assert got == (dict(enumerate(want[0])), dict(enumerate(want[1])))
                    window[(ci, s)] = got
                w_h = np.ones(len(case.blocks)) if weights is None else weights[h]
                strip = lambda runs: [[(b, ref) for b, ref, _ in run] for run in runs]  # noqa: E731  (the integrate walk had other weights)
                iruns, imaps = window[(ci, s)]
                assert sorted(runs_out[h]) == sorted(iruns) and sorted(maps_out[h]) == (sorted(imaps) if want_maps else [])
                assert strip(runs_out[h][r] for r in sorted(runs_out[h])) == strip(iruns[r] for r in sorted(iruns))
                for r, run in runs_out[h].items():
                    assert [w for _, _, w in run] == [float(w_h[b]) for b, _, _ in run]
                for q, m in maps_out[h].items():
                    assert m == [tuple(runs_out[h][r]) for r in range(case.map_start[q], case.map_start[q + 1])]
                    assert strip(m) == strip(imaps[q])
    print(f"\n[bank plan] {walks} search walks, {skipped} tiles no hypothesis looks at, {one_block_tiles} one-block tiles")
    assert skipped >= 20 and one_block_tiles >= 100


def test_search_tile_blocks_at_the_limits_and_at_the_defaults():
    lib = _shim()
    cells = 3 * 64 * 64
    assert lib.bank_shim_tile_blocks(128, 64, cells, 3, 1, 1, 0) >= 1
    assert _per_block(128, 64, cells, 3, True, True) == 37889024 and (128 << 20) // 37889024 == 3    # "a block costs 37.9 MB"
    assert lib.bank_shim_tile_blocks(128, 64, cells, 3, 1, 1, 0) == 3
    assert lib.bank_shim_tile_blocks(128, 64, cells, 3, 1, 1, 1000) == 1                     # a budget below one block: one block
    # the 17 x 33 grid under 20 hypotheses (scripts/ddm_search_timing.py's bit-edge search, one arm), every choice of outputs: the
    # function as corr_bank.hip had it before the plan moved here - kSearchTileBytes = 128 MB over what a block costs, 2^20 at most
    for arms in (1, 3):
        for want_coh in (0, 1):
            for want_maps in (0, 1):
                was = max(1, min((128 << 20) // _per_block(20, 17, arms * 17 * 33, arms, want_coh, want_maps), 1 << 20))
                assert lib.bank_shim_tile_blocks(20, 17, arms * 17 * 33, arms, want_coh, want_maps, 0) == was, (arms, want_coh, want_maps)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
class Facts:
    """The channels of the GPU refusal tests as facts: 0 and 1 a C/A table, 5 with a code window, 6 with a wrong first pad; a record
    of 60 000 samples at 18 Msps."""

    def __init__(self, record=True):
        self.lib = _shim()
        self.p = self.lib.bank_shim_create(int(record), 60000, FS)
        for ch, window, broken in ((0, 0, 0), (1, 0, 0), (5, 512, 0), (6, 0, 1)):
            self.lib.bank_shim_set_channel(self.p, ch, 1, 1025, window, broken)

    def __del__(self):
        self.lib.bank_shim_destroy(self.p)

    def double(self, on):
        self.lib.bank_shim_set_double(self.p, int(on))


def _blocks(descs):
    b = np.zeros(len(descs), dtype=BLOCK)
    for k, d in enumerate(descs):
        b[k]["channel"], b[k]["blksize"], b[k]["first_sample"] = d.get("channel", 0), d["n"], d["s0"]
        b[k]["rem"], b[k]["step"], b[k]["f"], b[k]["phi"] = d["rem"], d["step"], d["f"], d["phi"]
    return b


GOOD = dict(channel=0, n=2049, s0=3, rem=0.2, step=1.023e6 / FS, f=2e4, phi=0.1)


def _statuses():
    from cu_sdr_collection_amd import _lib as L
    return L.GC_OK, L.GC_E_INVALID, L.GC_E_RANGE, L.GC_E_STATE, L.GC_E_UNSUPPORTED


def test_the_bank_and_the_ddm_refuse_what_the_gpu_tests_say():
    ok, invalid, rng_, state, unsupported = _statuses()
    facts = Facts()

    def call(desc, offsets, freqs=None, ntaps=None, nfreq=None, nblocks=1):
        b = _blocks([desc])
        off, offp = _f64(offsets)
        frq, frqp = _f64(freqs)
        return facts.lib.bank_shim_check(facts.p, nblocks, b.ctypes.data, len(off) if ntaps is None else ntaps, offp,
                                         (1 if frq is None else len(frq)) if nfreq is None else nfreq, frqp)

    for freqs in (None, [0.0]):                                          # gc_correlate_bank's list, then the same through gc_correlate_ddm
        assert call(GOOD, [0.0], freqs, ntaps=0) == invalid
        assert call(GOOD, np.zeros(65), freqs) == invalid
        assert call(GOOD, [0.0, float("nan")], freqs) == invalid
        assert call(GOOD, [0.0, float("inf")], freqs) == invalid
        assert call(GOOD, [0.0, 1023.0], freqs) == invalid                # a full period
        assert call(GOOD, [0.0, -1023.0], freqs) == invalid
        assert call(dict(GOOD, channel=5), [0.0], freqs) == unsupported   # windowed channel
        assert call(dict(GOOD, channel=6), [0.0], freqs) == invalid       # broken pads
        assert call(dict(GOOD, step=1.5), [0.0], freqs) == unsupported    # more than one table entry per sample
        assert call(dict(GOOD, s0=60000 - 2048), [0.0], freqs) == rng_    # one sample past the record
        assert call(dict(GOOD, channel=200), [0.0], freqs) == state
        facts.double(True)
        assert call(GOOD, [0.0], freqs) == unsupported
        facts.double(False)
        assert call(GOOD, [0.0, 1022.9], freqs if freqs is None else [0.0, 250.0]) == ok
        assert call(GOOD, [0.0], freqs, nblocks=0) == ok
    # what gc_correlate_ddm adds
    assert call(GOOD, [0.0], [0.0], nfreq=0) == invalid
    assert call(GOOD, [0.0], np.zeros(65)) == invalid
    assert call(GOOD, [0.0], [0.0, float("nan")]) == invalid
    assert call(GOOD, [0.0], [0.0, float("inf")]) == invalid
    facts = Facts(record=False)                                          # an empty list needs no record
    assert call(GOOD, [0.0], [0.0, 1.0], nblocks=0) == ok and call(GOOD, [0.0], [float("nan")], nblocks=0) == invalid
    assert call(GOOD, [0.0], [0.0]) == state


def test_integrate_refuses_what_the_gpu_test_says():
    ok, invalid, rng_, state, unsupported = _statuses()
    facts = Facts()
    four = [GOOD, dict(GOOD, s0=20000), dict(GOOD, s0=40000), dict(GOOD, s0=100)]

    def call(descs=four, offsets=(0.0, 0.5), freqs=(0.0, 50.0), run_len=(2, 2), map_len=(1, 1), weights=None, nruns=None, nmaps=None,
             want_coh=True, want_pow=True):
        b = _blocks(descs)
        off, offp = _f64(offsets)
        frq, frqp = _f64(freqs)
        runs, runsp = _i32(run_len)
        maps, mapsp = _i32(map_len)
        w, wp = _f64(weights)
        return facts.lib.bank_shim_check_integrate(facts.p, len(descs), b.ctypes.data, wp, len(off), offp, len(frq), frqp,
                                                   len(runs) if nruns is None else nruns, runsp, len(maps) if nmaps is None else nmaps, mapsp,
                                                   int(want_coh), int(want_pow))

    assert call(nruns=0, nmaps=0) == invalid                             # blocks present, no runs
    assert call(run_len=(4, 0)) == invalid                               # a run of no blocks
    assert call(run_len=(5, -1)) == invalid
    assert call(run_len=(2, 1)) == invalid                               # the runs do not sum to the blocks
    assert call(run_len=(2, 3)) == invalid
    assert call(map_len=(2, 0)) == invalid                               # a map of no runs
    assert call(map_len=(1,)) == invalid                                 # the maps do not sum to the runs
    assert call(map_len=(1, 2)) == invalid
    assert call(descs=[GOOD, dict(GOOD, channel=1), GOOD, GOOD]) == invalid   # two channels in one run
    assert call(weights=[1.0, float("nan"), 1.0, 1.0]) == invalid
    assert call(weights=[1.0, 1.0, 1.0, float("-inf")]) == invalid
    assert call(nmaps=-1) == invalid
    assert call(want_pow=False) == invalid                               # maps asked for, nowhere to put them
    assert call(map_len=(), want_coh=False) == invalid                   # neither output asked for
    assert call(map_len=(), want_coh=False, want_pow=False) == invalid
    assert call(freqs=(0.0, float("nan"))) == invalid
    assert call(offsets=np.zeros(65)) == invalid
    assert call(descs=[dict(d, channel=5) for d in four]) == unsupported
    assert call(descs=[dict(d, channel=6) for d in four]) == invalid
    assert call(descs=four[:3] + [dict(GOOD, s0=60000 - 2048)]) == rng_
    assert call(descs=[dict(d, channel=200) for d in four]) == state
    facts.double(True)
    assert call() == unsupported
    facts.double(False)
    assert call() == ok
    assert call(descs=[GOOD, GOOD, dict(GOOD, channel=1), dict(GOOD, channel=1)], offsets=[0.0], freqs=[0.0], map_len=(), want_pow=False) == ok
    assert call(descs=[], run_len=(), map_len=(), want_pow=False) == ok and call(descs=[], run_len=(), map_len=()) == ok
    assert call(descs=[], run_len=(1,), map_len=(), want_pow=False) == invalid               # a run without blocks


def test_the_search_refuses_what_the_gpu_test_says():
    ok, invalid, rng_, state, unsupported = _statuses()
    facts = Facts()
    six = [GOOD, dict(GOOD, s0=20000), dict(GOOD, s0=40000), dict(GOOD, s0=100), dict(GOOD, s0=30000), dict(GOOD, s0=7)]

    def call(descs=six, nhyp=2, shifts=(0, 2), weights=None, offsets=(0.0, 0.5), freqs=(0.0, 50.0), run_len=(2, 2), map_len=(1, 1), nruns=None,
             nmaps=None, want=(True, True, True)):
        b = _blocks(descs)
        off, offp = _f64(offsets)
        frq, frqp = _f64(freqs)
        runs, runsp = _i32(run_len)
        maps, mapsp = _i32(map_len)
        sh, shp = _i32(shifts)
        w, wp = _f64(weights)
        return facts.lib.bank_shim_check_search(facts.p, len(descs), b.ctypes.data, nhyp, shp, wp, len(off), offp, len(frq), frqp,
                                                len(runs) if nruns is None else nruns, runsp, len(maps) if nmaps is None else nmaps, mapsp,
                                                *(int(x) for x in want))

    ones = np.ones((2, 6))
    assert call(nhyp=0) == invalid
    assert call(nhyp=129, shifts=[0] * 129) == invalid
    assert call(shifts=(0, -1)) == invalid                               # a negative shift
    assert call(shifts=(0, 3)) == invalid                                # 3 + 4 > 6
    assert call(nruns=0, nmaps=0, want=(True, False, False)) == invalid  # blocks present, no runs
    assert call(run_len=(4, 0)) == invalid                               # a run of no blocks
    assert call(run_len=(5, -1)) == invalid
    assert call(run_len=(5, 2)) == invalid                               # more than the blocks
    assert call(map_len=(2, 0)) == invalid                               # a map of no runs
    assert call(map_len=(1,)) == invalid                                 # the maps do not sum to the runs
    assert call(map_len=(1, 2)) == invalid
    assert call(nmaps=-1) == invalid
    mixed = six[:2] + [dict(six[2], channel=1), dict(six[3], channel=1)] + [dict(d, channel=1) for d in six[4:]]
    assert call(descs=mixed, shifts=(0, 1)) == invalid                   # two channels in a run of the window at shift 1 only
    for bad in (float("nan"), float("inf"), float("-inf")):
        w = ones.copy()
        w[0, 5] = bad                                                    # outside hypothesis 0's window: any entry counts
        assert call(weights=w) == invalid
    assert call(map_len=(), want=(True, True, False)) == invalid         # pow without a map
    assert call(map_len=(), want=(True, False, True)) == invalid         # peaks without a map
    assert call(want=(False, False, False)) == invalid                   # no output at all
    assert call(map_len=(), want=(False, False, False)) == invalid
    assert call(freqs=(0.0, float("nan"))) == invalid
    assert call(offsets=np.zeros(65)) == invalid
    assert call(descs=[dict(d, channel=5) for d in six]) == unsupported
    assert call(descs=[dict(d, channel=6) for d in six]) == invalid
    assert call(descs=six[:5] + [dict(GOOD, s0=60000 - 2048)], shifts=(0, 1)) == rng_      # a block outside every window counts too
    assert call(descs=[dict(d, channel=200) for d in six]) == state
    facts.double(True)
    assert call() == unsupported
    facts.double(False)
    assert call() == ok
    assert call(weights=ones) == ok
    assert call(run_len=(2, 1), shifts=(0, 3)) == ok                     # the runs need not hold every block: that is the integrate call's rule
    assert call(descs=mixed, offsets=[0.0], freqs=[0.0], map_len=(), want=(True, False, False)) == ok   # one channel per run of every window
    assert call(descs=[], nhyp=1, shifts=(0,), run_len=(), map_len=(), want=(True, False, False)) == ok


# ---- the walks as a program of their own, under the sanitizers ------------------------------------------------------------------------
def test_the_walks_run_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/bank_plan_sweep.hip over the lists of this module, each under 1, 3 and 20 hypotheses and every tile size: a child
    process that exits with 0."""
    exe = _built("bank_plan_sweep.hip", "bank_plan_sweep", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"])
    lines = []
    for ci, case in enumerate(CASES):
        rng = np.random.default_rng(7000 + ci)
        for nhyp in (1, 3, 20):
            shifts = _shifts(nhyp, rng)
            for tile in TILES:
                nums = [len(case.blocks)] + [int(x) for pair in zip(case.blocks["blksize"], case.blocks["first_sample"]) for x in pair]
                for lst in (case.run_len, case.map_len, shifts):
                    nums += [len(lst)] + list(lst)
                lines.append(" ".join(str(x) for x in nums + [case.budget, tile]))
    path = tmp_path / "lists.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == f"{len(lines)} cases"
