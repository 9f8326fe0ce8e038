// The decisions of gc_acq_shift_search_batch (csrc/shift_pick.h) on the CPU: ONE PRN's search over a surface the caller hands in twice -
// as float64 (what `exact_values` answers with) and as float32 (what the passes would have left: `row_cells` serves its cells at or
// above a threshold, with overflow beyond `cap`; the serial statements of the kernels in shift_pick.h supply the row maxima, their
// runner-ups and ShiftPickDev).  Both orders of calls the batch call uses are driven: rows written (pick_row, the kernel's pick, the two
// exact cells, resolve_peaks) and rows fused (the same, with GC_SHIFT_PICK_GLOBAL taking near_peak from the row's runner-up instead of
// a pick).  Built by tests/test_shift_pick_cpu.py with the flags of acq_shift.hip; no GPU is touched.
#include "../cu-sdr-collection_amd/csrc/shift_pick.h"

extern "C" {

// out: the pick; stats = {ties, row_cells calls, exact cells, pick_forced calls}.  Surfaces: [rows][n], rows = carriers * signals * bins.
int shift_pick_shim_run(const double* f64, const float* f32, int n_carriers, int n_signals, int n_bins, int n, int rule, int exclude, int period, double eps,
                        int cap, int fused, int guard, gc_acq_shift_pick* out, long long* stats) {
  const int rows = n_carriers * n_signals * n_bins;
  ShiftPickRules g;
  g.n_carriers = n_carriers;
  g.n_signals = n_signals;
  g.n_bins = n_bins;
  g.rule = rule;
  g.exclude = exclude;
  g.period = period;
  g.guard = guard != 0;
  g.eps = eps;
  int ties = 0;
  long long ncollect = 0, nexact = 0, nforced = 0;
  g.row_cells = [&](int, int row, float thr, std::vector<int2>& list, bool* overflow) {
    ++ncollect;
    list.clear();
    int count = 0;
    for (int c = 0; c < n; ++c) count += f32[(size_t)row * n + c] >= thr ? 1 : 0;
    *overflow = count > cap;
    if (*overflow) return (int)GC_OK;
    for (int c = n - 1; c >= 0; --c)  // (in no particular order)
      if (f32[(size_t)row * n + c] >= thr) list.push_back(make_int2(row, c));
    return (int)GC_OK;
  };
  g.exact_values = [&](int, const std::vector<int2>& cells, std::vector<double>& vals) {
    vals.resize(cells.size());
    for (size_t i = 0; i < cells.size(); ++i) vals[i] = f64[(size_t)cells[i].x * n + cells[i].y];
    nexact += (long long)cells.size();
    return (int)GC_OK;
  };
  auto device_pick = [&](int row, int forced_cp, ShiftPickDev& d) {
    std::memset(&d, 0, sizeof d);
    d.row = row;
    d.second_col = -1;
    d.forced_cp = forced_cp;
    shift_pick_serial(f32 + (size_t)row * n, n, exclude, g.second() ? period : 0, (float)eps, d);
  };
  g.pick_forced = [&](int, int row, int col, ShiftPickDev& d) {
    ++nforced;
    device_pick(row, col + 1, d);
    return (int)GC_OK;
  };
  std::vector<float> hmax((size_t)rows), hsecond((size_t)rows);
  std::vector<int> harg((size_t)rows);
  for (int r = 0; r < rows; ++r) shift_rowmax_serial(f32 + (size_t)r * n, n, &hmax[(size_t)r], &harg[(size_t)r], &hsecond[(size_t)r]);
  std::vector<double> rmd(hmax.begin(), hmax.end());
  std::vector<int> rad(harg);
  gc_acq_shift_pick& pk = *out;
  double max_dev = 0.0;
  auto done = [&](int rc) {
    stats[0] = ties;
    stats[1] = ncollect;
    stats[2] = nexact;
    stats[3] = nforced;
    return rc;
  };
  int rc = pick_row(g, 0, rmd, rad, pk, ties);
  if (rc || pk.row < 0) return done(rc);
  ShiftPickDev d;
  if (!fused || g.second()) {
    device_pick(pk.row, 0, d);
  } else {
    if (!g.guard) return done(GC_OK);
    std::memset(&d, 0, sizeof d);
    d.row = pk.row;
    d.second_col = -1;
    pick_dev_from_runner_up(g, pk, rad[(size_t)pk.row], hmax[(size_t)pk.row], hsecond[(size_t)pk.row], d);
  }
  int2 two[2];
  const int ntwo = pick_from_dev(g, d, pk, two);
  if (!g.guard) return done(GC_OK);
  std::vector<double> vals;
  rc = g.exact_values(0, std::vector<int2>(two, two + ntwo), vals);
  if (rc) return done(rc);
  pick_set_exact(vals.data(), ntwo, pk, max_dev);
  return done(resolve_peaks(g, 0, d, pk, ties));
}

// second_window(cp, exclude, period) as {lo0, hi0, lo1, hi1}
void shift_pick_shim_window(int cp, int exclude, int period, int* out) {
  const SecondWindow w = second_window(cp, exclude, period);
  out[0] = w.lo0;
  out[1] = w.hi0;
  out[2] = w.lo1;
  out[3] = w.hi1;
}

}  // extern "C"
