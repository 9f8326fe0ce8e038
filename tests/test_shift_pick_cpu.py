"""What gc_acq_shift_search_batch DECIDES (csrc/shift_pick.h: the package's rule over the rows, the first maximum, the second-peak
window, and the float64 guard over all three) without a GPU, against a float64 model of the reference's rules
(tests/shift_pick_model.py).

tests/shift_pick_shim.hip runs the header on the CPU over a surface given twice: as float64 - what the guard's exact cells answer with
- and as float32 - what the transforms would have left.  The float32 surface is the float64 one with every cell moved by at most
eps / 8 (relative), the margin the suite asserts for the real transforms (|float32 peak - float64 peak| / float64 peak < eps / 8,
tests/test_gpu_acquisition.py), with the signs chosen AGAINST the float64 decision: the cells the model decides for are lowered, every
other cell is raised.  eps is an argument of the shim (1e-3 here, so that ties are frequent on small surfaces).

Requirement: row, code_phase, peak and second_peak equal the model's on the float64 surface - the values bit for bit, they are looked
up - for both orders of calls the batch call uses (rows written / rows fused).  Three documented exceptions are pinned as they are
(include/gnsscorr.h at gc_acq_guard_stats): more than 64 tied rows, a tied row whose band overflows the list cap, an overflow while the
peaks of the chosen row are resolved.

The first tests hold the MODEL against the two other restatements in the tree (oracle.gnss_oracle._second_peak_ratio, the product's
host rules acq_shift._first_maximum / _second_peak) over exhaustive small grids; the last ones hold the scenes of
tests/test_gpu_shift_picks.py to what they claim on the float64 surface.  Neither needs the shim."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import shift_pick_model as M
import shift_pick_scenes as SC

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-3
CAP = 4096
_LIB = []


class Pick(C.Structure):
    _fields_ = [("row", C.c_int32), ("code_phase", C.c_int32), ("peak", C.c_double), ("second_peak", C.c_double)]


def _shim():
    if not _LIB:
        from cu_sdr_collection_amd import build as B
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not found")
        src, out = os.path.join(HERE, "shift_pick_shim.hip"), os.path.join(HERE, "build", "libshift_pick_shim.so")
        deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = [f for f in B._tu_flags("acq_shift.hip") if f != "--offload-compress"]
            subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
        lib = C.CDLL(out)
        lib.shift_pick_shim_run.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_double] + [C.c_int] * 3 + [C.POINTER(Pick), C.POINTER(C.c_longlong)]
        lib.shift_pick_shim_window.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int)]
        _LIB.append(lib)
    return _LIB[0]


def against(f64, favoured=(), eps=EPS):
    """The float32 surface: every cell lowered by eps / 9 (relative), the cells {(row, col)} in `favoured` raised by as much; the
    float32 rounding on top keeps each within eps / 8."""
    f = np.asarray(f64, dtype=np.float64) * (1.0 - eps / 9)
    for cell in favoured:
        f[cell] = f64[cell] * (1.0 + eps / 9)
    out = f.astype(np.float32)
    assert np.all(np.abs(out.astype(np.float64) - f64) <= eps / 8 * np.abs(f64))
    return out


def run(f64, f32, geom, rule, exclude=0, period=0, eps=EPS, cap=CAP, fused=0, guard=1):
    nc, ns, nb = geom
    f64 = np.ascontiguousarray(f64, dtype=np.float64)
    f32 = np.ascontiguousarray(f32, dtype=np.float32)
    assert f64.shape == f32.shape == (nc * ns * nb, f64.shape[1])
    pk, stats = Pick(), (C.c_longlong * 4)()
    rc = _shim().shift_pick_shim_run(f64.ctypes.data, f32.ctypes.data, nc, ns, nb, f64.shape[1], rule, exclude, period, eps, cap, fused, guard, C.byref(pk), stats)
    assert rc == 0
    return dict(row=pk.row, code_phase=pk.code_phase, peak=pk.peak, second_peak=pk.second_peak), dict(zip(("ties", "collects", "exact", "forced"), stats))


def check(f64, f32, geom, rule, exclude=0, period=0, want=None, **kw):
    """Both orders of calls against the model (or `want`); returns the written order's stats."""
    m = dict(M.pick(f64, *geom, rule, exclude, period))
    m.pop("second_col")
    if want is not None:
        m.update(want)
    stats = None
    for fused in (0, 1):
        got, st = run(f64, f32, geom, rule, exclude, period, fused=fused, **kw)
        assert got == m, (("fused" if fused else "written"), got, m)
        stats = stats or st
    return stats


def both_ways(f64, cells, geom, rule, exclude=0, period=0, **kw):
    """The float64 surface as it is, then with the contested cells' values swapped round (a cyclic shift of them): each time the float32
    surface raises every contested cell BUT the one the model decides for - and, for the measure, the exact float32 image as well."""
    cells = list(cells)
    vals = [f64[c] for c in cells]
    ties = []
    for shift in range(len(cells)):
        g = np.array(f64, dtype=np.float64)
        for c, v in zip(cells, vals[shift:] + vals[:shift]):
            g[c] = v
        m = M.pick(g, *geom, rule, exclude, period)
        decided = {(m["row"], m["code_phase"]), (m["row"], m["second_col"])}
        ties.append(check(g, against(g, [c for c in cells if c not in decided]), geom, rule, exclude, period, **kw)["ties"])
        check(g, g.astype(np.float32), geom, rule, exclude, period, **kw)
    return ties


def background(rng, rows, n, top):
    """Distinct integer values below `top`: no two cells tie."""
    return rng.permutation(np.arange(1, rows * n + 1)).reshape(rows, n).astype(np.float64) * (top // (2 * rows * n) or 1)


# ---- the model against the other restatements (passes without the header) ----------------------------------------------------------------
def test_model_equals_the_oracles_and_the_products_host_rules():
    from oracle import gnss_oracle as O
    from cu_sdr_collection_amd import acq_shift as A
    rng = np.random.default_rng(5)
    nwin = 0
    for n in (6, 9, 12):
        corr = rng.integers(0, 4, n).astype(np.float64)              # few levels: exact ties inside the ranges
        for period in range(1, n + 1):
            for exclude in range(0, period + 2):
                for cp in range(1, n + 1):
                    rng1 = M.second_range(cp, exclude, period)
                    if rng1.size == 0 or rng1.min() < 1 or rng1.max() > n:
                        continue                                       # (the reference indexes out of the row or takes max([]) there)
                    want = O._second_peak_ratio(corr, cp, exclude, period)
                    assert want == A._second_peak(corr, cp, exclude, period)
                    got, col = M.second_peak(corr, cp, exclude, period)
                    assert got == want and corr[col] == want and (col + 1) in rng1
                    assert not np.any(corr[rng1[rng1 < col + 1] - 1] == want)    # the first position holding it
                    nwin += 1
    assert nwin > 800
    ngrid = 0
    for nc, nb in ((1, 1), (1, 3), (2, 2), (3, 3), (2, 1)):
        for v in itertools.product(range(3), repeat=nc * nb):          # every [carriers, bins] array over three levels
            arr = np.array(v, dtype=np.float64).reshape(nc, nb)
            want = A._first_maximum(arr)
            row = M.sequential_row(arr.reshape(-1), nc, 1, nb)
            assert row == (-1 if want is None else want[0] * nb + want[1])
            ngrid += 1
    assert ngrid > 19000
    # pairs: the product's host restatement (acquisition_B1I: _first_maximum over the larger of the blocks, block 1 only if strictly larger)
    for nc, nb in ((1, 2), (2, 2)):
        for v in itertools.product(range(3), repeat=nc * 2 * nb):
            rm = np.array(v, dtype=np.float64).reshape(nc, 2, nb)
            p1, p2 = rm[:, 0, :], rm[:, 1, :]
            win = A._first_maximum(np.maximum(p1, p2))
            want = -1 if win is None else (win[0] * 2 + (0 if p1[win] > p2[win] else 1)) * nb + win[1]
            assert M.sequential_row(rm.reshape(-1), nc, 2, nb) == want


def test_window_equals_the_models_ranges():
    out = (C.c_int * 4)()
    for period in range(1, 14):
        for exclude in range(0, period + 2):
            for cp in range(1, 30):
                _shim().shift_pick_shim_window(cp, exclude, period, out)
                mine = set(range(out[0], out[1] + 1)) | set(range(out[2], out[3] + 1))
                assert mine == set(M.second_range(cp, exclude, period).tolist()), (cp, exclude, period)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
def _rows_surface(rng, geom, n, maxima):
    """Background below 4000 and one cell per named row: maxima = {row: (col, value)}."""
    rows = geom[0] * geom[1] * geom[2]
    f = background(rng, rows, n, 4000)
    for r, (col, v) in maxima.items():
        f[r, col] = v
    return f


def test_two_tied_rows_under_the_sequential_rule():
    rng = np.random.default_rng(11)
    geom = (2, 1, 3)
    f = _rows_surface(rng, geom, 24, {1: (5, 10000.0), 3: (9, 10001.0)})
    assert both_ways(f, [(1, 5), (3, 9)], geom, M.SEQUENTIAL, 2, 12) == [1, 1]
    f[3, 9] = 10000.0                                                   # exactly equal: the first in scan order, whatever float32 prefers
    check(f, against(f, [(3, 9)]), geom, M.SEQUENTIAL, 2, 12, want=dict(row=1))


def test_a_skipped_row_is_never_chosen():
    """The last bin of carrier 1 holds the larger maximum; the last bin of carrier 0 is eligible and wins."""
    rng = np.random.default_rng(12)
    for rule, geom, skipped, eligible in ((M.SEQUENTIAL, (2, 1, 3), 5, 2), (M.SEQUENTIAL_PAIRS, (2, 2, 3), 11, 2)):
        f = _rows_surface(rng, geom, 24, {skipped: (4, 10001.0), eligible: (7, 10000.0)})
        for fav in ([(skipped, 4)], [(eligible, 7)]):
            st = check(f, against(f, fav), geom, rule, 2, 12, want=dict(row=eligible, code_phase=7, peak=10000.0))
            assert st["ties"] >= 1


def test_pairs_tied_blocks():
    rng = np.random.default_rng(13)
    geom = (2, 2, 2)                                                    # row (carrier * 2 + block) * 2 + bin
    f = _rows_surface(rng, geom, 24, {1: (5, 10000.0), 3: (9, 10001.0)})    # carrier 0, bin 1: block 1 and block 2
    assert both_ways(f, [(1, 5), (3, 9)], geom, M.SEQUENTIAL_PAIRS, 2, 12) == [1, 1]
    f[3, 9] = 10000.0                                                   # equal in float64: block 2
    for fav in ([(1, 5)], [(3, 9)]):
        check(f, against(f, fav), geom, M.SEQUENTIAL_PAIRS, 2, 12, want=dict(row=3))


def test_pairs_ties_across_carrier_and_bin_with_the_maxima_in_different_blocks():
    rng = np.random.default_rng(14)
    geom = (2, 2, 2)
    f = _rows_surface(rng, geom, 24, {2: (5, 10000.0), 4: (9, 10001.0), 0: (3, 9000.0), 6: (8, 9500.0)})   # (0, block 2, bin 0) and (1, block 1, bin 0)
    assert both_ways(f, [(2, 5), (4, 9)], geom, M.SEQUENTIAL_PAIRS, 2, 12) == [1, 1]
    f[4, 9] = 10000.0
    check(f, against(f, [(4, 9)]), geom, M.SEQUENTIAL_PAIRS, 2, 12, want=dict(row=2))


def test_global_tied_rows():
    rng = np.random.default_rng(15)
    geom = (1, 1, 4)
    f = _rows_surface(rng, geom, 24, {1: (15, 10000.0), 2: (6, 10001.0)})
    assert both_ways(f, [(1, 15), (2, 6)], geom, M.GLOBAL) == [1, 1]
    # equal maxima in two rows at different columns: the FIRST row, the first column holding the maximum in any row, the maximum itself
    f[2, 6] = 10000.0
    for fav in ([(1, 15)], [(2, 6)], []):
        check(f, against(f, fav), geom, M.GLOBAL, want=dict(row=1, code_phase=6, peak=10000.0))
    f[1, 20] = 9999.0                                                   # ... and with a near-tied cell in the chosen row, so that its peaks are resolved too
    for fav in ([(1, 20)], [(2, 6), (1, 20)]):
        check(f, against(f, fav), geom, M.GLOBAL, want=dict(row=1, code_phase=6, peak=10000.0))


def test_all_zero_surface():
    z = np.zeros((4, 16))
    for rule, geom in ((M.SEQUENTIAL, (2, 1, 2)), (M.SEQUENTIAL_PAIRS, (1, 2, 2))):
        for fused in (0, 1):
            got, _ = run(z, z, geom, rule, 2, 8, fused=fused)
            assert got == dict(row=-1, code_phase=0, peak=0.0, second_peak=0.0)
    for fused in (0, 1):                                                # max(max(results)) of zeros: the first row, the first column, 0
        got, _ = run(z, z, (1, 1, 4), M.GLOBAL, fused=fused)
        assert got == dict(row=0, code_phase=0, peak=0.0, second_peak=0.0)


# ---- the documented exceptions, pinned ----------------------------------------------------------------------------------------------------
def test_64_tied_rows_are_resolved_and_65_are_not():
    for nrows, resolved in ((64, True), (65, False)):
        f = np.full((nrows, 8), 100.0)
        f[:, 3] = 10000.0
        f[nrows - 1, 3] = 10001.0                                       # the last row holds the maximum; float32 prefers the first
        f32 = against(f, [(0, 3)])
        for fused in (0, 1):
            got, st = run(f, f32, (1, 1, nrows), M.GLOBAL, fused=fused)
            assert got["row"] == (nrows - 1 if resolved else 0) and got["peak"] == f[got["row"], 3], (nrows, got)
            assert st["ties"] == (1 if resolved else 0)


def test_a_tied_row_whose_band_overflows_keeps_its_float32_maximum():
    f = np.full((2, 16), 100.0)
    f[0, 2:8] = 10001.0                                                 # a plateau of six in the row the model takes
    f[1, 5] = 10000.0
    f32 = against(f, [(1, 5)])
    assert M.pick(f, 1, 1, 2, M.SEQUENTIAL, 2, 16)["row"] == 0
    for fused in (0, 1):
        got, st = run(f, f32, (1, 1, 2), M.SEQUENTIAL, 2, 16, cap=4, fused=fused)
        assert got["row"] == 1 and got["peak"] == 10000.0 and st["ties"] >= 1    # row 0 stood with its (lowered) float32 maximum
        got, _ = run(f, f32, (1, 1, 2), M.SEQUENTIAL, 2, 16, cap=6, fused=fused)
        assert got["row"] == 0 and got["code_phase"] == 2 and got["peak"] == 10001.0


def test_an_overflow_while_the_peaks_are_resolved_leaves_the_pick():
    f = np.full((1, 32), 100.0)
    f[0, [3, 9, 12, 20, 25]] = 10000.0
    f[0, 28] = 10001.0
    f32 = against(f, [(0, 12)])
    for fused in (0, 1):
        got, st = run(f, f32, (1, 1, 1), M.SEQUENTIAL, 1, 32, cap=5, fused=fused)
        assert (got["row"], got["code_phase"], got["peak"]) == (0, 12, 10000.0) and st["ties"] == 1 and st["forced"] == 0
        got, _ = run(f, f32, (1, 1, 1), M.SEQUENTIAL, 1, 32, cap=6, fused=fused)
        assert (got["code_phase"], got["peak"]) == (28, 10001.0)


# ---- first maximum, window, second peak -----------------------------------------------------------------------------------------------------
def test_tied_columns_of_the_first_maximum():
    rng = np.random.default_rng(21)
    for cols in ([7, 33], [7, 20, 33]):
        f = background(rng, 1, 48, 4000)
        for i, c in enumerate(cols):
            f[0, c] = 10000.0 + i
        cells = [(0, c) for c in cols]
        assert both_ways(f, cells, (1, 1, 1), M.SEQUENTIAL, 2, 12) == [1] * len(cols)
        assert both_ways(f, cells, (1, 1, 1), M.GLOBAL) == [1] * len(cols)
        for c in cols:
            f[0, c] = 10000.0                                           # exactly equal: MATLAB's first occurrence
        for fav in cells:
            check(f, against(f, [fav]), (1, 1, 1), M.SEQUENTIAL, 2, 12, want=dict(code_phase=7))
            check(f, against(f, [fav]), (1, 1, 1), M.GLOBAL, want=dict(code_phase=7))


WINDOWS = [(48, 16, 3, cp) for cp in (1, 3, 4, 5, 12, 13, 16, 17, 30, 48)] + \
          [(48, 16, 0, cp) for cp in (1, 2, 9, 16, 17, 48)] + \
          [(48, 48, 3, cp) for cp in (1, 3, 4, 5, 44, 45, 48)] + \
          [(48, 4, 3, 1), (48, 5, 3, 2), (48, 1, 0, 1), (48, 1, 1, 7)]


@pytest.mark.parametrize("n,period,exclude,cp", WINDOWS)
def test_second_peak_window(n, period, exclude, cp):
    """The peak at 1-based cp: the edges of the three range cases, a later period, the row's end, exclude 0 (the window holds the peak
    itself), empty windows (second_peak 0), period = n."""
    rng = np.random.default_rng(n * 1000 + period * 50 + exclude * 7 + cp)
    f = background(rng, 1, n, 4000)
    f[0, cp - 1] = 10000.0
    m = M.pick(f, 1, 1, 1, M.SEQUENTIAL, exclude, period)
    assert m["code_phase"] == cp - 1
    if (period, exclude) in ((4, 3), (1, 1)):
        assert m["second_peak"] == 0.0 and m["second_col"] == -1
    if exclude == 0 and cp <= period:
        assert m["second_peak"] == 10000.0
    check(f, f.astype(np.float32), (1, 1, 1), M.SEQUENTIAL, exclude, period)
    # the two largest cells of the window within eps of each other, float32 against the larger
    if m["second_col"] >= 0 and m["second_peak"] < 10000.0:
        rng1 = M.second_range(cp, exclude, period)
        rng1 = rng1[(rng1 >= 1) & (rng1 <= n)] - 1
        others = [c for c in rng1 if c != m["second_col"]]
        if others:
            f[0, others[-1]] = m["second_peak"] - 1.0
            st = check(f, against(f, [(0, others[-1])]), (1, 1, 1), M.SEQUENTIAL, exclude, period)
            assert st["ties"] == 1


def test_two_window_cells_tied():
    rng = np.random.default_rng(23)
    f = background(rng, 1, 48, 2000)
    f[0, 9] = 10000.0                                                   # (1-based 10: the window is 1 .. 8 and 12 .. 16)
    f[0, 4], f[0, 11] = 5000.0, 5001.0
    assert both_ways(f, [(0, 4), (0, 11)], (1, 1, 1), M.SEQUENTIAL, 2, 16) == [1, 1]
    f[0, 11] = 5000.0
    check(f, against(f, [(0, 11)]), (1, 1, 1), M.SEQUENTIAL, 2, 16, want=dict(second_peak=5000.0))


def _moved_surface(later_is_true):
    """n = 40, period 20, exclude 2: near-tied columns 5 and 25 (1-based 6 and 26).  Around 6 the window is 1..4, 8..20; around 26 it is
    9..24.  Column 1 (1-based 2) lies in the first window only, columns 12 and 14 in both, column 22 in the second only."""
    f = np.full((1, 40), 100.0)
    f[0, 5], f[0, 25] = (100000.0, 100001.0) if later_is_true else (100001.0, 100000.0)
    return f


def test_moved_first_maximum_with_no_collected_cell_in_the_new_window():
    """(a) The float32 pass prefers the other column; the old second peak lies outside the window of the float64 first maximum and no
    collected cell lies inside it: the second peak must be looked for again there."""
    for later in (True, False):
        f = _moved_surface(later)
        true_col, f32_col = (25, 5) if later else (5, 25)
        # the float32 first maximum's window alone holds the large cell; the true one's window holds only small ones
        f[0, 1 if later else 22] = 50000.0
        f[0, 14] = 20000.0
        m = M.pick(f, 1, 1, 1, M.SEQUENTIAL, 2, 20)
        assert (m["code_phase"], m["second_peak"]) == (true_col, 20000.0)
        st = check(f, against(f, [(0, f32_col)]), (1, 1, 1), M.SEQUENTIAL, 2, 20)
        assert st["ties"] == 1 and st["forced"] == 1
        # float32 agreeing with float64: the slow path runs (two cells within eps), nothing moves, no further pick
        st = check(f, against(f, [(0, true_col)]), (1, 1, 1), M.SEQUENTIAL, 2, 20)
        assert st["ties"] == 1 and st["forced"] == 0


def test_moved_first_maximum_whose_windows_largest_cell_was_not_collected():
    """(b) A collected cell lies inside the new window, but the window's largest float64 cell is below the float32 collection threshold
    (it was lowered, the collected one raised): the largest collected cell is not the second peak."""
    for later in (True, False):
        f = _moved_surface(later)
        true_col, f32_col = (25, 5) if later else (5, 25)
        old_only = 1 if later else 22
        f[0, old_only] = 50000.0                                         # the float32 second peak, raised: the threshold is 50000 (1 + eps / 9)(1 - eps)
        f[0, 12], f[0, 14] = 49952.0, 49953.0                            # both windows; 12 raised (collected), 14 lowered (not collected)
        f32 = against(f, [(0, f32_col), (0, old_only), (0, 12)])
        thr = np.float32(float(f32[0, old_only]) * (1.0 - EPS))
        assert f32[0, 12] >= thr > f32[0, 14]
        m = M.pick(f, 1, 1, 1, M.SEQUENTIAL, 2, 20)
        assert (m["code_phase"], m["second_peak"], m["second_col"]) == (true_col, 49953.0, 14)
        st = check(f, f32, (1, 1, 1), M.SEQUENTIAL, 2, 20)
        assert st["ties"] == 1 and st["forced"] == 1


def test_moved_first_maximum_into_an_empty_window():
    """period 4, exclude 3: around 1-based 1 the range is empty, around 5 it is 5 - 4 + 1 + 3 .. 2: empty too; around 2 .. 4 (e1 < 2) it
    is e2 .. 4 + e1.  Columns 0 and 1 tie: the window of column 1 (1-based 2) is 5 .. 3, empty; both ways give second_peak 0."""
    f = np.full((1, 12), 100.0)
    f[0, 0], f[0, 1] = 10000.0, 10001.0
    both_ways(f, [(0, 0), (0, 1)], (1, 1, 1), M.SEQUENTIAL, 3, 4)


def test_a_search_that_does_not_tie_takes_the_fast_path():
    rng = np.random.default_rng(31)
    f = background(rng, 6, 48, 4000)
    f[3, 17] = 10000.0
    f[3, 40] = 6000.0
    for rule, geom in ((M.SEQUENTIAL, (2, 1, 3)), (M.SEQUENTIAL_PAIRS, (1, 2, 3)), (M.GLOBAL, (1, 1, 6))):
        st = check(f, against(f), geom, rule, 2, 24)
        assert st == dict(ties=0, collects=0, exact=1 if rule == M.GLOBAL else 2, forced=0)


def test_without_the_guard_the_float32_decisions_stand():
    f = np.full((1, 40), 100.0)
    f[0, 5], f[0, 25], f[0, 1] = 100000.0, 100001.0, 50000.0
    f32 = against(f, [(0, 5)])
    for fused in (0, 1):
        got, st = run(f, f32, (1, 1, 1), M.SEQUENTIAL, 2, 20, fused=fused, guard=0)
        assert got == dict(row=0, code_phase=5, peak=float(f32[0, 5]), second_peak=float(f32[0, 1])) and st["exact"] == 0


# ---- random surfaces ------------------------------------------------------------------------------------------------------------------------
def _random_surface(rng, rows, n):
    """Integer-valued cells: a background, and three levels (top, about top / 2, about top / 3) each held by a few cells 0 .. 3 units
    apart - 1e-4 relative per unit at the top: exact ties and near ties that eps / 8 reorders."""
    top = int(rng.integers(8000, 12000))
    f = rng.integers(0, top // 4, (rows, n)).astype(np.float64)
    for level in (top, top // 2, top // 3):
        for _ in range(int(rng.integers(1, 5))):
            f[rng.integers(0, rows), rng.integers(0, n)] = level - int(rng.integers(0, 4))
    return f


@pytest.mark.parametrize("rule", [M.GLOBAL, M.SEQUENTIAL, M.SEQUENTIAL_PAIRS])
def test_random_surfaces(rule):
    rng = np.random.default_rng(1000 + rule)
    ties = forced = 0
    for it in range(1500):
        ns = 2 if rule == M.SEQUENTIAL_PAIRS else 1
        nc, nb = [(1, 1), (1, 4), (2, 2), (2, 3), (3, 2), (1, 6)][int(rng.integers(0, 6))]
        n = int(rng.integers(4, 97))
        rows = nc * ns * nb
        f = _random_surface(rng, rows, n)
        period = int(rng.integers(1, n + 1))
        exclude = int(rng.integers(0, max(1, period // 2) + 1))
        m = M.pick(f, nc, ns, nb, rule, exclude, period)
        if it % 3 == 0:
            f32 = against(f)                                           # everything lowered alike: the order stands
        elif it % 3 == 1:
            signs = rng.choice([-1.0, 1.0], f.shape)
            f32 = (f * (1.0 + signs * EPS / 9)).astype(np.float32)
        else:                                                           # against the model's cells
            fav = np.ones(f.shape, dtype=bool)
            if m["row"] >= 0:
                fav[m["row"], m["code_phase"]] = False
                if m["second_col"] >= 0:
                    fav[m["row"], m["second_col"]] = False
            f32 = (f * np.where(fav, 1.0 + EPS / 9, 1.0 - EPS / 9)).astype(np.float32)
        st = check(f, f32, (nc, ns, nb), rule, exclude, period)
        ties += st["ties"]
        forced += st["forced"]
    print(f"rule {rule}: {ties} ties and {forced} moved first maxima over 1500 surfaces")
    assert ties > 300 and (rule == M.GLOBAL or forced > 10)


# ---- the scenes of tests/test_gpu_shift_picks.py are what they claim to be -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CLEAR))
def test_clear_scenes_are_clear(name):
    sc = SC.CLEAR[name]()
    for call in sc.calls:
        for ip, surf in enumerate(sc.surfaces(call)):
            if ip == sc.absent:
                continue
            assert M.clear(surf, *sc.geom, sc.rule, call.exclude, call.period, SC.eps_of(sc.n)), (name, call, ip)
            m = M.pick(surf, *sc.geom, sc.rule, call.exclude, call.period)
            want = call.expect[ip]
            assert (m["row"], m["code_phase"]) == want, (name, call, ip, m, want)


@pytest.mark.parametrize("name", list(SC.TIES))
def test_tie_scenes_hold_their_gaps(name):
    sc = SC.TIES[name]()
    eps = SC.eps_of(sc.n)
    for call in sc.calls:
        surf = sc.surfaces(call)[0]
        m, rm, window = M.decision_cells(surf, *sc.geom, sc.rule, call.exclude, call.period)
        kind, cells = call.contested
        vals = np.sort([surf[c] for c in cells])
        gaps = np.diff(vals) / vals[-1]
        assert np.all((gaps >= 1e-10) & (gaps <= eps / 4)), (name, call.label, gaps)
        # every other cell of that decision is clear of the contested ones
        if kind == "rows":
            assert sorted(np.flatnonzero(rm >= vals[-1] * (1.0 - eps))) == sorted({r for r, _ in cells}), (name, call.label)
            assert (m["row"], m["code_phase"]) == max(cells, key=lambda c: surf[c])
        elif kind == "first":
            pool = surf if sc.rule == M.GLOBAL else surf[m["row"]]
            assert np.sum(pool >= vals[-1] * (1.0 - eps)) == len(cells), (name, call.label)
            assert (m["row"], m["code_phase"]) == max(cells, key=lambda c: surf[c])
            if sc.rule != M.GLOBAL:                                 # the windows around the two columns hold different second peaks
                other = min(cells, key=lambda c: surf[c])
                alt, _ = M.second_peak(surf[other[0]], other[1] + 1, call.exclude, call.period)
                assert abs(alt - m["second_peak"]) > 0.1 * m["second_peak"], (name, call.label, alt, m["second_peak"])
        else:
            assert kind == "second"
            assert np.sum(window >= vals[-1] * (1.0 - eps)) == len(cells), (name, call.label)
            assert (m["row"], m["second_col"]) == max(cells, key=lambda c: surf[c])
            assert m["peak"] / m["second_peak"] <= 4.0
            assert np.sum(surf[m["row"]] >= m["peak"] * (1.0 - eps)) == 1
        assert call.expect[0] == (m["row"], m["code_phase"])
    # the two directions decide differently
    picks = [M.pick(sc.surfaces(call)[0], *sc.geom, sc.rule, call.exclude, call.period) for call in sc.calls]
    assert len({(p["row"], p["code_phase"], p["second_col"]) for p in picks}) == 2, (name, picks)
