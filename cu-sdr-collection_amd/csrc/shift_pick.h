// shift_pick.h - what gc_acq_shift_search_batch (acq_shift.hip) DECIDES: which row the package's rule takes, the row's first maximum,
// where its second peak is looked for, and what the float64 guard does when two candidates of such a decision lie within eps of each
// other.  Reference: BDS/B1I/include/acquisition.m:87-166, GPS/GPS_L2C/include/acquisition.m:46-112, BDS/B1C/include/acquisition.m:193-197.
//
// Nothing here calls HIP, allocates on the device or launches (int2 is the only thing taken from the HIP headers): the float32 cells of
// a row, the float64 value of a cell and the device's pick of a row come in as callbacks, so tests/shift_pick_shim.hip runs every line
// of it on the CPU against tests/shift_pick_model.py.  Both ways the batch call runs (rows written / rows fused into per-tile
// candidates) call the same functions; they differ in where a row's float32 sums come from.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

#include "../../include/gnsscorr.h"

#if defined(__HIPCC__)
#define GC_SHIFT_HD __host__ __device__
#else
#define GC_SHIFT_HD
#endif

// What shift_pick_kernel leaves per PRN (device-internal; the public gc_acq_shift_pick is filled from it and from the float64 guard)
struct ShiftPickDev {
  int row;          // in: the winning row (-1: none)
  int code_phase;   // 0-based first maximum of the row
  int second_col;   // 0-based first position of the second peak (-1: no second peak asked for or range empty)
  int near_peak;    // cells of the row at or above peak * (1 - eps), the maximum itself included
  int near_second;  // cells of the second-peak range at or above second * (1 - eps)
  float peak, second;
  int forced_cp;    // in: 0: the row's first maximum is looked for; c > 0: it IS column c (1-based) - the float64 guard found it there
};

// Where the second peak is looked for: the row's first `period` samples outside +-exclude samples of the first maximum `cp` - the
// reference's three range cases (B1I :141-156, L2C :77-91; 1-based there as here: e1 = codePhase - exclude, e2 = codePhase + exclude;
// e1 < 2: e2 .. period + e1; e2 >= period: e2 - period + 1 .. e1; else 1 .. e1 and e2 .. period).  period <= 0: nowhere.
struct SecondWindow {
  int lo0 = 1, hi0 = 0, lo1 = 1, hi1 = 0;  // 1-based inclusive ranges
  GC_SHIFT_HD bool holds(int c1) const { return (c1 >= lo0 && c1 <= hi0) || (c1 >= lo1 && c1 <= hi1); }
};
GC_SHIFT_HD inline SecondWindow second_window(int cp, int exclude, int period) {
  SecondWindow w;
  if (period <= 0) return w;
  const int e1 = cp - exclude, e2 = cp + exclude;
  if (e1 < 2) {
    w.lo0 = e2;
    w.hi0 = period + e1;
  } else if (e2 >= period) {
    w.lo0 = e2 - period + 1;
    w.hi0 = e1;
  } else {
    w.lo0 = 1;
    w.hi0 = e1;
    w.lo1 = e2;
    w.hi1 = period;
  }
  return w;
}

// ---- what the kernels leave, stated serially (tests/shift_pick_shim.hip only: the library runs the kernels) --------------------------
// shift_pick_kernel on one row r[0 .. n): the first maximum (pk.forced_cp > 0: that column instead), the largest value inside
// second_window() of it with its first column - ranges clipped to the row -, and how many cells lie within eps (relative, float32) of
// either.  period <= 0: no second peak.
inline void shift_pick_serial(const float* r, int n, int exclude, int period, float eps, ShiftPickDev& pk) {
  if (pk.row < 0) return;
  float peak = -1.0f;
  int cp = 1;
  for (int i = 0; i < n; ++i)
    if (r[i] > peak) {
      peak = r[i];
      cp = i + 1;
    }
  if (pk.forced_cp > 0) {
    cp = pk.forced_cp;
    peak = r[cp - 1];
  }
  // (the kernel walks the two ranges one after the other: with exclude == 0 the middle case holds column cp in both, and near_second
  // counts it twice - a trip through the slow path that changes nothing)
  const SecondWindow w = second_window(cp, exclude, period);
  const int lo[2] = {w.lo0, w.lo1}, hi[2] = {w.hi0, w.hi1};
  float sec = -1.0f;
  int sc = 0x7fffffff;
  for (int k = 0; k < 2; ++k)
    for (int i = std::max(lo[k] - 1, 0); i < hi[k] && i < n; ++i)
      if (r[i] > sec || (r[i] == sec && i < sc)) {
        sec = r[i];
        sc = i;
      }
  const float tp = peak * (1.0f - eps), ts = sec * (1.0f - eps);
  int np = 0, ns = 0;
  for (int i = 0; i < n; ++i) np += r[i] >= tp ? 1 : 0;
  if (sec >= 0.0f)
    for (int k = 0; k < 2; ++k)
      for (int i = std::max(lo[k] - 1, 0); i < hi[k] && i < n; ++i) ns += r[i] >= ts ? 1 : 0;
  pk.code_phase = cp - 1;
  pk.peak = peak;
  pk.second = sec >= 0.0f ? sec : 0.0f;
  pk.second_col = sec >= 0.0f ? sc : -1;
  pk.near_peak = np;
  pk.near_second = ns;
}

// rowmax_kernel (and the per-tile candidates of the specialised passes) on one row: its maximum, the first column holding it, and the
// row's runner-up - the largest value at any OTHER column (== the maximum when a second column holds it).
inline void shift_rowmax_serial(const float* r, int n, float* vmax, int* amax, float* vsecond) {
  float best = -1.0f;
  int bi = 0;
  for (int i = 0; i < n; ++i)
    if (r[i] > best) {
      best = r[i];
      bi = i;
    }
  float sec = -1.0f;
  for (int i = 0; i < n; ++i)
    if (i != bi) sec = std::max(sec, r[i]);
  *vmax = best;
  *amax = bi;
  *vsecond = std::min(sec, best);
}

// ---- the rules ---------------------------------------------------------------------------------------------------------------------
// The reference's sequential selection over the (carrier, bin) grid (BDS/B1I acquisition.m:87-122, GPS_L2C :46-66): a value is taken
// only if it EXCEEDS the largest so far, starting from 0, and the last bin of every carrier but the first is not looked at - the
// first position, in scan order, of the largest value, if that is above 0.  v(carrier, bin) = rowmax, or the larger of the two signal
// blocks' (pairs).  Returns the public row index ((carrier * n_signals + signal) * n_bins + bin), or -1.
template <class T>
int pick_sequential(int n_carriers, int n_bins, const T* rmax, bool pairs) {
  T best = 0;
  int row = -1;
  for (int c = 0; c < n_carriers; ++c)
    for (int b = 0; b < n_bins; ++b) {
      if (c > 0 && b == n_bins - 1) continue;
      if (!pairs) {
        const int r = c * n_bins + b;
        if (rmax[r] > best) {
          best = rmax[r];
          row = r;
        }
      } else {
        const int r1 = (c * 2 + 0) * n_bins + b, r2 = (c * 2 + 1) * n_bins + b;
        const T v = std::max(rmax[r1], rmax[r2]);
        if (v > best) {
          best = v;
          row = rmax[r1] > rmax[r2] ? r1 : r2;
        }
      }
    }
  return row;
}

// ---- the float64 guard of the batch call (acq_guard.h) ---------------------------------------------------------------------------
// Row maxima, first maxima and second peaks come out of float32 transforms; the reference's sequential `>` tests (B1I :98-119,
// L2C :46-66), `[~, codePhase] = max(corr)` and `max_peak / second > threshold` (B1I :126-166) are float64.  Wherever two candidates
// are closer than eps the cells that close are evaluated again as float64 correlations at one lag, and peak / second_peak of every
// PRN always are (the two numbers the caller divides and thresholds).
//
// What the decisions read.  They launch nothing themselves: a row's float32 cells, the float64 value of a cell and the device's pick
// of a row around a given first maximum come in as callbacks.
constexpr int kShiftTiedRowsMax = 64;  // more rows than this within eps of the chosen one: the float32 choice stands
struct ShiftPickRules {
  int n_carriers = 1, n_signals = 1, n_bins = 1;  // public row ((carrier * n_signals + signal) * n_bins + bin)
  int rule = GC_SHIFT_PICK_GLOBAL, exclude = 0, period = 0;
  bool guard = true;  // false (GC_ACQ_NO_GUARD in the tuning build): the float32 decisions stand
  double eps = 0.0;   // gc_acq_tie_eps of the transform
  // cells {row, col} of PRN k's public row `row` at or above thr (<= kGuardListCap of them, else *overflow and none)
  std::function<int(int k, int row, float thr, std::vector<int2>& list, bool* overflow)> row_cells;
  // float64 values of cells {row, col} of PRN k's results
  std::function<int(int k, const std::vector<int2>& cells, std::vector<double>& vals)> exact_values;
  // shift_pick_kernel on PRN k's public row `row` with the first maximum forced to column `col` (0-based): second, second_col and
  // near_second of the window around THAT column.  Called right after row_cells(k, row, ...): the row's sums are where that left them.
  std::function<int(int k, int row, int col, ShiftPickDev& d)> pick_forced;
  bool second() const { return rule != GC_SHIFT_PICK_GLOBAL; }
};

// the largest of the cells' float64 values and the smallest column that holds it (MATLAB's first occurrence)
inline void first_maximum(const std::vector<int2>& cells, const std::vector<double>& vals, double* best, int* col) {
  *best = -1.0;
  *col = 0;
  for (size_t i = 0; i < cells.size(); ++i)
    if (vals[i] > *best || (vals[i] == *best && cells[i].y < *col)) {
      *best = vals[i];
      *col = cells[i].y;
    }
}

// the package's selection rule on the row maxima rmd and their columns rad (public row order)
inline void apply_rule(const ShiftPickRules& g, const std::vector<double>& rmd, const std::vector<int>& rad, gc_acq_shift_pick& pk) {
  if (g.rule == GC_SHIFT_PICK_GLOBAL) {
    // BDS/B1C acquisition.m:193-197: the row of max(max(results,[],2)) (first), the first column holding the global maximum
    const int rows = (int)rmd.size();
    int best = 0;
    for (int r = 1; r < rows; ++r)
      if (rmd[(size_t)r] > rmd[(size_t)best]) best = r;
    int col = rad[(size_t)best];
    for (int r = 0; r < rows; ++r)
      if (rmd[(size_t)r] == rmd[(size_t)best] && rad[(size_t)r] < col) col = rad[(size_t)r];
    pk.row = best;
    pk.code_phase = col;
    pk.peak = rmd[(size_t)best];
  } else {
    pk.row = pick_sequential(g.n_carriers, g.n_bins, rmd.data(), g.rule == GC_SHIFT_PICK_SEQUENTIAL_PAIRS);
  }
}

// PRN k's row: the rule on the float32 row maxima, then rows whose maximum is within eps of the chosen one - which of them the rule
// takes is decided on their float64 maxima (rmd / rad are overwritten with those).  More than kShiftTiedRowsMax such rows: the float32
// choice stands.  Afterwards rad[pk.row] is the first maximum of the chosen row itself (GC_SHIFT_PICK_GLOBAL: pk.code_phase is the
// first column holding the global maximum in ANY row).
inline int pick_row(const ShiftPickRules& g, int k, std::vector<double>& rmd, std::vector<int>& rad, gc_acq_shift_pick& pk, int& ties) {
  pk.row = -1;
  pk.code_phase = 0;
  pk.peak = 0.0;
  pk.second_peak = 0.0;
  apply_rule(g, rmd, rad, pk);
  if (!g.guard || pk.row < 0) return GC_OK;
  const double near = rmd[(size_t)pk.row] * (1.0 - g.eps);
  std::vector<int> tied;
  for (int r = 0; r < (int)rmd.size(); ++r)
    if (rmd[(size_t)r] >= near && rmd[(size_t)r] > 0.0) tied.push_back(r);
  if (tied.size() <= 1 || tied.size() > (size_t)kShiftTiedRowsMax) return GC_OK;
  ++ties;
  for (int r : tied) {
    std::vector<int2> list;
    bool overflow = false;
    int rc = g.row_cells(k, r, (float)(rmd[(size_t)r] * (1.0 - g.eps)), list, &overflow);
    if (rc) return rc;
    if (overflow || list.empty()) continue;  // a plateau: the float32 maximum stands for this row
    std::vector<double> vals;
    rc = g.exact_values(k, list, vals);
    if (rc) return rc;
    first_maximum(list, vals, &rmd[(size_t)r], &rad[(size_t)r]);
  }
  apply_rule(g, rmd, rad, pk);
  return GC_OK;
}

// GC_SHIFT_PICK_GLOBAL where the rows are not written: the chosen row is not transformed again - what shift_pick_kernel would say of it
// comes from the row's maximum, its column `own_col` (rad[pk.row] after pick_row) and the row's runner-up (float32, as the passes
// left them)
inline void pick_dev_from_runner_up(const ShiftPickRules& g, const gc_acq_shift_pick& pk, int own_col, float row_max, float row_second, ShiftPickDev& d) {
  d.code_phase = own_col;
  d.peak = (float)pk.peak;
  d.near_peak = (double)row_second >= (double)row_max * (1.0 - g.eps) ? 2 : 1;
  d.near_second = 0;
}

// The device's (float32) pick `d` of PRN k's chosen row into pk, and the cells whose float64 values replace pk.peak and
// pk.second_peak: the row's own first maximum and, where there is one, the second peak.  Returns how many cells (1 or 2).
// GC_SHIFT_PICK_GLOBAL keeps the rule's pk.code_phase, which may name the column of ANOTHER row that holds the same maximum
// (acquisition.m:196 takes the first column of max(results)): the cell that is evaluated is the chosen row's own.
inline int pick_from_dev(const ShiftPickRules& g, const ShiftPickDev& d, gc_acq_shift_pick& pk, int2 cells[2]) {
  if (g.second()) pk.code_phase = d.code_phase;
  pk.peak = (double)d.peak;
  pk.second_peak = g.second() ? (double)d.second : 0.0;
  cells[0] = make_int2(pk.row, d.code_phase);
  if (!g.second() || d.second_col < 0) return 1;
  cells[1] = make_int2(pk.row, d.second_col);
  return 2;
}

// ... and their float64 values in their place; max_dev: the largest |float32 - float64| / float64 seen
inline void pick_set_exact(const double* vals, int ncells, gc_acq_shift_pick& pk, double& max_dev) {
  double* const dst[2] = {&pk.peak, &pk.second_peak};
  for (int i = 0; i < ncells; ++i) {
    if (vals[i] > 0.0) max_dev = std::max(max_dev, std::fabs(*dst[i] - vals[i]) / vals[i]);
    *dst[i] = vals[i];
  }
}

// PRN k's first maximum and second peak when shift_pick_kernel (or the row's runner-up) found another cell within eps of either, `d`
// holding the float32 values: every cell of the chosen row that could be the first maximum or the second peak - all those at or
// above the smaller of the two float32 values less eps (the peak's lobe is among them) - then the reference's rules on the float64
// values.  An overflowed or empty list: pk stays.
//
// The list was collected for the window around the FLOAT32 first maximum.  Where the float64 values name another column the window
// moves with it, and neither the old second peak nor the list's threshold says anything about the cells of the new window: the
// device picks the row once more around the new first maximum (pick_forced), that second peak is evaluated in float64, and cells of
// the new window within eps of it are resolved like any other tie (an overflowed list there: the float64 value of the device's cell
// stays).  An empty new window: second_peak 0.
inline int resolve_peaks(const ShiftPickRules& g, int k, const ShiftPickDev& d, gc_acq_shift_pick& pk, int& ties) {
  if (d.near_peak <= 1 && d.near_second <= 1) return GC_OK;
  ++ties;
  const float low = g.second() && d.second_col >= 0 ? std::min(d.peak, d.second) : d.peak;
  std::vector<int2> list;
  bool overflow = false;
  int rc = g.row_cells(k, pk.row, (float)((double)low * (1.0 - g.eps)), list, &overflow);
  if (rc) return rc;
  if (overflow || list.empty()) return GC_OK;
  std::vector<double> vals;
  rc = g.exact_values(k, list, vals);
  if (rc) return rc;
  int col = 0;
  first_maximum(list, vals, &pk.peak, &col);
  if (!g.second()) {
    // (a smaller column of another row that holds the same maximum stays: see pick_from_dev)
    if (!(pk.code_phase < col && pk.code_phase != d.code_phase)) pk.code_phase = col;
    return GC_OK;
  }
  pk.code_phase = col;
  auto window_max = [&](const SecondWindow& w, double sec) {
    for (size_t i = 0; i < list.size(); ++i)
      if (w.holds(list[i].y + 1)) sec = std::max(sec, vals[i]);
    return sec;
  };
  const SecondWindow w = second_window(pk.code_phase + 1, g.exclude, g.period);
  if (pk.code_phase == d.code_phase) {
    const double sec = window_max(w, -1.0);
    if (sec >= 0.0) pk.second_peak = sec;
    return GC_OK;
  }
  ShiftPickDev m;
  rc = g.pick_forced(k, pk.row, pk.code_phase, m);
  if (rc) return rc;
  pk.second_peak = 0.0;
  if (m.second_col < 0) return GC_OK;
  list.assign(1, make_int2(pk.row, m.second_col));
  rc = g.exact_values(k, list, vals);
  if (rc) return rc;
  pk.second_peak = vals[0];
  if (m.near_second <= 1) return GC_OK;
  rc = g.row_cells(k, pk.row, (float)((double)m.second * (1.0 - g.eps)), list, &overflow);
  if (rc) return rc;
  if (overflow || list.empty()) return GC_OK;
  rc = g.exact_values(k, list, vals);
  if (rc) return rc;
  pk.second_peak = window_max(w, pk.second_peak);
  return GC_OK;
}
