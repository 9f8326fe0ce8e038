// bank_plan.h — what the drivers of the tap bank family (corr_bank.hip: gc_correlate_bank, gc_correlate_ddm,
// gc_correlate_ddm_integrate, gc_correlate_ddm_search) decide on the host, from integers: the argument checks, the two memory
// budgets, the cut of a block list into sub-batches, and per sub-batch (integrate) or per tile of blocks (search) every index,
// flag and row number the kernels and the copies are given.  Nothing here calls HIP, allocates on the device or launches: the
// drivers upload, launch and fetch what these functions produce, tests/bank_plan_shim.hip runs all of it without a device.
// From the context the checks read the channel tables' host side (ctx->ch) and precision, d_if, fs, if_nsamples.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "corr_common.h"

constexpr int kBankChunk = 1024;  // S: samples per work item of the chunk kernel

// What one sub-batch's partial sums and one search tile's scratch may take.  The library always passes the defaults and has no
// switch for them; the CPU tests pass budgets of a few chunks or blocks, so that short lists are cut where they choose.
struct BankBudget {
  long long partial_bytes = 256LL << 20;  // partial sums of one sub-batch of blocks at most
  long long tile_bytes = 128LL << 20;     // per-(hypothesis, block) scratch and finished runs / maps of one tile at most
};

// ---- checks ------------------------------------------------------------------------------------------------------------------
// What gc_correlate_bank accepts (include/gnsscorr.h), for it and for the functions defined through it (`fn`: the name in the
// error texts); *arms = the most arms a channel of the list has.
inline int bank_validate(const char* fn, const gc_context* ctx, int nblocks, const gc_block* b, int ntaps, const double* off, int* arms) {
  if (ntaps < 1 || ntaps > GC_BANK_MAX_TAPS) {
    gc_set_error("%s: %d taps (1 .. %d)", fn, ntaps, GC_BANK_MAX_TAPS);
    return GC_E_INVALID;
  }
  double omax = 0.0;
  for (int j = 0; j < ntaps; ++j) {
    if (!std::isfinite(off[j])) {
      gc_set_error("%s: tap offset %d is not finite", fn, j);
      return GC_E_INVALID;
    }
    omax = std::max(omax, std::fabs(off[j]));
  }
  if (nblocks == 0) return GC_OK;  // an empty list is no call sequence error, as in gc_correlate
  if (ctx->precision != GC_PREC_F32) {
    gc_set_error("%s: float32 kernels only (gc_set_precision GC_PREC_F32)", fn);
    return GC_E_UNSUPPORTED;
  }
  if (!ctx->d_if) {
    gc_set_error("no IF buffer loaded");
    return GC_E_STATE;
  }
  if (!(ctx->fs > 0)) {
    gc_set_error("sampling frequency not set (gc_set_sampling_freq)");
    return GC_E_STATE;
  }
  *arms = 1;
  bool seen[GC_MAX_CHANNELS] = {false};
  for (int i = 0; i < nblocks; ++i) {
    const gc_block& k = b[i];
    if (k.channel < 0 || k.channel >= GC_MAX_CHANNELS || !ctx->ch[k.channel].configured) {
      gc_set_error("block %d: channel %d not configured", i, k.channel);
      return GC_E_STATE;
    }
    const HostChannel& c = ctx->ch[k.channel];
    double max_mult = 1.0;
    for (int a = 0; a < c.arms; ++a) {
      if (!c.d_tab[a]) {
        gc_set_error("block %d: channel %d arm %d has no code table", i, k.channel, a);
        return GC_E_STATE;
      }
      if (k.table_offset[a] != 0) {
        gc_set_error("block %d: %s reads whole tables periodically (table_offset must be 0)", i, fn);
        return GC_E_INVALID;
      }
      max_mult = std::max(max_mult, c.mult[a]);
    }
    if (!seen[k.channel]) {  // per channel: no window, pads that are the period, every offset within one period
      seen[k.channel] = true;
      *arms = std::max(*arms, c.arms);
      for (int a = 0; a < c.arms; ++a) {
        if (c.window[a] > 0) {
          gc_set_error("channel %d arm %d: %s does not take a code window (gc_set_code_window)", k.channel, a, fn);
          return GC_E_UNSUPPORTED;
        }
        const std::vector<int8_t>& t = c.h_tab[a];
        const int n = c.nent[a];
        if ((int)t.size() != n || n < 3 || t[0] != t[n - 2] || t[n - 1] != t[1]) {
          gc_set_error("channel %d arm %d: the table's pads are not its period ([c(end) c c(1)])", k.channel, a);
          return GC_E_INVALID;
        }
        if (!(omax * c.index_scale * c.mult[a] < (double)(n - 2))) {
          gc_set_error("channel %d arm %d: a tap offset of %g chips reaches a code period (%d entries) or more", k.channel, a, omax, n - 2);
          return GC_E_INVALID;
        }
      }
    }
    if (k.blksize <= 0 || k.first_sample < 0 || !(k.code_phase_step > 0) || !(k.rem_code_phase > -1.0) ||
        !std::isfinite(k.rem_code_phase) || !std::isfinite(k.carr_freq) || !std::isfinite(k.rem_carr_phase)) {
      gc_set_error("block %d: invalid descriptor", i);
      return GC_E_INVALID;
    }
    const double rate = k.code_phase_step * c.index_scale * max_mult;  // table entries per sample of the fastest arm
    if (rate > 1.0) {
      gc_set_error("block %d: %g table entries per sample (%s takes at most one)", i, rate, fn);
      return GC_E_UNSUPPORTED;
    }
    if (!(rate >= 1.0 / 65536.0)) {
      gc_set_error("block %d: %g table entries per sample (below 2^-16)", i, rate);
      return GC_E_INVALID;
    }
    if (!(((double)k.blksize * k.code_phase_step + std::fabs(k.rem_code_phase) + omax) * c.index_scale * max_mult < 2147483000.0)) {
      gc_set_error("block %d: the ramps' table indices leave int32", i);
      return GC_E_INVALID;
    }
    if ((uint64_t)k.first_sample + (uint64_t)k.blksize > ctx->if_nsamples) {
      gc_set_error("block %d: samples [%lld, %lld) exceed the IF buffer (%llu samples)", i, (long long)k.first_sample,
                   (long long)(k.first_sample + k.blksize), (unsigned long long)ctx->if_nsamples);
      return GC_E_RANGE;  // tracking.m:241-245
    }
  }
  return GC_OK;
}

// The argument check of the functions defined through the bank.  freq_offsets == nullptr is the bank itself.
inline int bank_check(const char* fn, const gc_context* ctx, int nblocks, const gc_block* blocks, int ntaps, const double* tap_offsets,
                      int nfreq, const double* freq_offsets, int* arms) {
  if (freq_offsets) {
    if (nfreq < 1 || nfreq > GC_DDM_MAX_FREQS) {
      gc_set_error("%s: %d frequency bins (1 .. %d)", fn, nfreq, GC_DDM_MAX_FREQS);
      return GC_E_INVALID;
    }
    for (int m = 0; m < nfreq; ++m)
      if (!std::isfinite(freq_offsets[m])) {
        gc_set_error("%s: frequency offset %d is not finite", fn, m);
        return GC_E_INVALID;
      }
  }
  int rc = bank_validate(fn, ctx, nblocks, blocks, ntaps, tap_offsets, arms);
  if (rc) return rc;
  if (freq_offsets)
    for (int i = 0; i < nblocks; ++i)
      for (int m = 0; m < nfreq; ++m)
        if (!std::isfinite(blocks[i].carr_freq + freq_offsets[m])) {  // what the bank answers to that carr_freq
          gc_set_error("block %d: invalid descriptor (carr_freq + frequency offset %d is not finite)", i, m);
          return GC_E_INVALID;
        }
  return GC_OK;
}

// Blocks in runs, runs in maps: run r is blocks run_start[r] .. run_start[r + 1] - 1 (of the list, or of a hypothesis's window), map
// q is runs map_start[q] .. map_start[q + 1] - 1.  Without maps map_start is {0}.
struct BankPartition {
  std::vector<int> run_start, map_start;
  int nruns() const { return (int)run_start.size() - 1; }
  int nmaps() const { return (int)map_start.size() - 1; }
  int nused() const { return run_start.back(); }  // blocks the runs hold
};

// run_len / map_len as a partition.  `whole_list`: the runs must hold exactly nblocks (integrate); otherwise nused() <= nblocks is
// enough and the caller checks each window (search).
inline int bank_partition(const char* fn, int nblocks, int nruns, const int32_t* run_len, int nmaps, const int32_t* map_len, bool whole_list,
                          BankPartition* p) {
  if (nmaps < 0 || (nblocks > 0 && nruns < 1)) {
    gc_set_error("%s: %d runs, %d maps for %d blocks", fn, nruns, nmaps, nblocks);
    return GC_E_INVALID;
  }
  p->run_start.assign(1, 0);
  p->map_start.assign(1, 0);
  for (int r = 0; r < nruns; ++r) {
    if (run_len[r] < 1 || run_len[r] > nblocks - p->run_start.back()) {
      gc_set_error("%s: run %d has %d blocks (1 at least, %d in all)", fn, r, (int)run_len[r], nblocks);
      return GC_E_INVALID;
    }
    p->run_start.push_back(p->run_start.back() + run_len[r]);
  }
  if (whole_list && p->nused() != nblocks) {
    gc_set_error("%s: the runs hold %d blocks of %d", fn, p->nused(), nblocks);
    return GC_E_INVALID;
  }
  for (int q = 0; q < nmaps; ++q) {
    if (map_len[q] < 1 || map_len[q] > nruns - p->map_start.back()) {
      gc_set_error("%s: map %d has %d runs (1 at least, %d in all)", fn, q, (int)map_len[q], nruns);
      return GC_E_INVALID;
    }
    p->map_start.push_back(p->map_start.back() + map_len[q]);
  }
  if (nmaps > 0 && p->map_start.back() != nruns) {
    gc_set_error("%s: the maps hold %d runs of %d", fn, p->map_start.back(), nruns);
    return GC_E_INVALID;
  }
  return GC_OK;
}

// gc_correlate_ddm_integrate's arguments: the bank's check, the partition, one channel per run, finite weights, an output.
inline int ddm_integrate_check(const char* fn, const gc_context* ctx, int nblocks, const gc_block* blocks, const double* weights, int ntaps,
                               const double* tap_offsets, int nfreq, const double* freq_offsets, int nruns, const int32_t* run_len, int nmaps,
                               const int32_t* map_len, bool want_coh, bool want_pow, int* arms, BankPartition* p) {
  int rc = bank_check(fn, ctx, nblocks, blocks, ntaps, tap_offsets, nfreq, freq_offsets, arms);
  if (rc || (rc = bank_partition(fn, nblocks, nruns, run_len, nmaps, map_len, true, p))) return rc;
  for (int r = 0; r < nruns; ++r)
    for (int b = p->run_start[r] + 1; b < p->run_start[r + 1]; ++b)
      if (blocks[b].channel != blocks[p->run_start[r]].channel) {
        gc_set_error("%s: run %d has blocks of channels %d and %d", fn, r, blocks[p->run_start[r]].channel, blocks[b].channel);
        return GC_E_INVALID;
      }
  if (weights)
    for (int b = 0; b < nblocks; ++b)
      if (!std::isfinite(weights[b])) {
        gc_set_error("%s: the weight of block %d is not finite", fn, b);
        return GC_E_INVALID;
      }
  if (nmaps > 0 ? !want_pow : !want_coh) {
    gc_set_error(nmaps > 0 ? "%s: power maps asked for without an output" : "%s: neither coherent sums nor power maps asked for", fn);
    return GC_E_INVALID;
  }
  return GC_OK;
}

// gc_correlate_ddm_search's arguments; shift[h] = block_shift[h], or 0 without shifts.
inline int ddm_search_check(const char* fn, const gc_context* ctx, int nblocks, const gc_block* blocks, int nhyp, const int32_t* block_shift,
                            const double* weights, int ntaps, const double* tap_offsets, int nfreq, const double* freq_offsets, int nruns,
                            const int32_t* run_len, int nmaps, const int32_t* map_len, bool want_coh, bool want_pow, bool want_peaks, int* arms,
                            BankPartition* p, std::vector<int>* shift) {
  if (nhyp < 1 || nhyp > GC_DDM_MAX_HYP) {
    gc_set_error("%s: %d hypotheses (1 .. %d)", fn, nhyp, GC_DDM_MAX_HYP);
    return GC_E_INVALID;
  }
  int rc = bank_check(fn, ctx, nblocks, blocks, ntaps, tap_offsets, nfreq, freq_offsets, arms);
  if (rc || (rc = bank_partition(fn, nblocks, nruns, run_len, nmaps, map_len, false, p))) return rc;
  const int nused = p->nused();
  shift->assign((size_t)nhyp, 0);
  for (int h = 0; h < nhyp; ++h) {
    int& s = (*shift)[h];
    if (block_shift) s = block_shift[h];
    if (s < 0 || s > nblocks - nused) {
      gc_set_error("%s: hypothesis %d looks at blocks %d .. %lld of %d", fn, h, s, (long long)s + nused - 1, nblocks);
      return GC_E_INVALID;
    }
  }
  for (int h = 0; h < nhyp; ++h)
    for (int r = 0; r < nruns; ++r) {
      const int b0 = (*shift)[h] + p->run_start[r];
      for (int b = b0 + 1; b < (*shift)[h] + p->run_start[r + 1]; ++b)
        if (blocks[b].channel != blocks[b0].channel) {
          gc_set_error("%s: run %d of hypothesis %d has blocks of channels %d and %d", fn, r, h, blocks[b0].channel, blocks[b].channel);
          return GC_E_INVALID;
        }
    }
  if (weights)
    for (long long i = 0; i < (long long)nhyp * nblocks; ++i)
      if (!std::isfinite(weights[i])) {
        gc_set_error("%s: the weight of block %d in hypothesis %d is not finite", fn, (int)(i % nblocks), (int)(i / nblocks));
        return GC_E_INVALID;
      }
  if (!want_coh && !want_pow && !want_peaks) {
    gc_set_error("%s: no output asked for", fn);
    return GC_E_INVALID;
  }
  if ((want_pow || want_peaks) && nmaps == 0) {
    gc_set_error("%s: power maps or peaks asked for without a map", fn);
    return GC_E_INVALID;
  }
  return GC_OK;
}

// ---- sub-batches -------------------------------------------------------------------------------------------------------------
// Chunks whose partial sums (`row` doubles each) fit the budget of one sub-batch.
inline long long bank_max_chunks(long long row, const BankBudget& budget) {
  return std::max<long long>(1, std::min<long long>(budget.partial_bytes / (row * 8), 0x40000000LL));
}

// The sub-batch that begins at block `first`: blocks while their chunks' partial sums fit (one block at least).  base[k] = chunks
// before its block k; returns the number of blocks.
inline int bank_cut(const gc_block* blocks, int nblocks, int first, long long max_chunks, std::vector<int32_t>& base) {
  base.assign(1, 0);
  int nb = 0;
  while (first + nb < nblocks) {
    const long long c = ((long long)blocks[first + nb].blksize + kBankChunk - 1) / kBankChunk;
    if (nb > 0 && base.back() + c > max_chunks) break;
    base.push_back((int32_t)(base.back() + c));
    ++nb;
  }
  return nb;
}

// ---- the integrate walk ------------------------------------------------------------------------------------------------------
struct DdmBlockAux {
  long long dn;  // first_sample - first_sample of the run's first block
  double w;      // the block's weight
};

// One sub-batch of the integrating walk: its blocks [first, first + nb), the runs r0 .. r0 + nr - 1 that have blocks in it - the
// first nfin of them end in it -, and the maps q0 .. q0 + nm - 1 those finished runs belong to, the first mfin of which end with
// them.  So the device's run rows 0 .. nfin - 1 are the caller's rows r0 .., its map rows 0 .. mfin - 1 the caller's rows q0 ...
struct DdmStep {
  int first = 0, nb = 0;
  int r0 = 0, nr = 0, nfin = 0;
  int q0 = 0, nm = 0, mfin = 0;
  std::vector<int32_t> chunk_base;  // [nb + 1]: chunks before block k of the sub-batch
};

// The step after `s` (a fresh DdmStep: the first); false: the list is done.
inline bool ddm_next_step(DdmStep& s, const gc_block* blocks, int nblocks, long long max_chunks, const BankPartition& p) {
  s.first += s.nb;
  s.r0 += s.nfin;
  s.q0 += s.mfin;
  if (s.first >= nblocks) return false;
  s.nb = bank_cut(blocks, nblocks, s.first, max_chunks, s.chunk_base);
  const int end = s.first + s.nb;
  int r1 = s.r0;
  while (p.run_start[r1 + 1] < end) ++r1;
  s.nr = r1 - s.r0 + 1;
  s.nfin = p.run_start[r1 + 1] == end ? s.nr : s.nr - 1;
  s.nm = s.mfin = 0;
  if (p.nmaps() > 0 && s.nfin > 0) {
    const int rend = s.r0 + s.nfin;
    int q1 = s.q0;
    while (p.map_start[q1 + 1] < rend) ++q1;
    s.nm = q1 - s.q0 + 1;
    s.mfin = p.map_start[q1 + 1] == rend ? s.nm : s.nm - 1;
  }
  return true;
}

// The most blocks, runs and maps a sub-batch of the walk holds.  The accumulators a cut run or map goes on from live in buffers of
// these sizes, which must not be reallocated during the walk.
struct DdmSizes {
  int nb = 0, nr = 0, nm = 0;
};
inline DdmSizes ddm_walk_sizes(const gc_block* blocks, int nblocks, long long max_chunks, const BankPartition& p) {
  DdmSizes z;
  for (DdmStep s; ddm_next_step(s, blocks, nblocks, max_chunks, p);) {
    z.nb = std::max(z.nb, s.nb);
    z.nr = std::max(z.nr, s.nr);
    z.nm = std::max(z.nm, s.nm);
  }
  return z;
}

// What the kernels and the copies of a step are given.
struct DdmLaunch {
  std::vector<DdmBlockAux> aux;   // [nb]
  std::vector<int32_t> run_base;  // [nr + 1]: the sub-batch's blocks before its run k
  std::vector<int32_t> map_base;  // [nm + 1]: the sub-batch's finished runs before its map k (nm == 0: empty)
  int carry_run = 0;              // run row 0 began in an earlier sub-batch and goes on from its accumulator
  int carry_map = 0;              // map row 0 likewise
  int keep_run = 0, keep_map = 0;  // the row of the run / map that goes on in the next sub-batch, to be moved to row 0 (0: none to move)
};
inline void ddm_plan_step(const DdmStep& s, const gc_block* blocks, const double* weights, const BankPartition& p, DdmLaunch& l) {
  const int end = s.first + s.nb;
  l.aux.resize((size_t)s.nb);
  l.run_base.resize((size_t)s.nr + 1);
  for (int k = 0; k < s.nr; ++k) {
    const int b0 = p.run_start[s.r0 + k], lo = std::max(b0, s.first), hi = std::min(p.run_start[s.r0 + k + 1], end);
    l.run_base[k] = lo - s.first;
    l.run_base[k + 1] = hi - s.first;
    for (int b = lo; b < hi; ++b) l.aux[b - s.first] = DdmBlockAux{blocks[b].first_sample - blocks[b0].first_sample, weights ? weights[b] : 1.0};
  }
  l.map_base.resize(s.nm > 0 ? (size_t)s.nm + 1 : 0);
  for (size_t k = 0; k < l.map_base.size(); ++k) l.map_base[k] = std::min(std::max(p.map_start[s.q0 + k] - s.r0, 0), s.nfin);
  l.carry_run = p.run_start[s.r0] < s.first;
  l.carry_map = s.nm > 0 && p.map_start[s.q0] < s.r0;
  l.keep_run = s.nfin < s.nr ? s.nr - 1 : 0;
  l.keep_map = s.mfin < s.nm ? s.nm - 1 : 0;
}

// ---- the search walk ---------------------------------------------------------------------------------------------------------
enum { SRCH_IN = 1, SRCH_RUN_START = 2, SRCH_RUN_END = 4, SRCH_MAP_START = 8, SRCH_MAP_END = 16 };

struct SearchAux {
  long long dn;   // first_sample - first_sample of the first block of the run this block belongs to in the hypothesis
  double w;       // the block's weight in the hypothesis
  int32_t flags;  // SRCH_*; 0: the block is outside the hypothesis's window
  int32_t pad_;
};

// Blocks per tile: what one block can cost in every hypothesis at once - its SearchAux, its rotations, and (at most one run and one
// map end with a block) a finished run if coh is asked for, a finished map with its peaks if maps are - within the tile budget.
// At the limits (128 hypotheses, 3 arms x 64 bins x 64 taps, coh and maps) a block costs 37.9 MB: one block always fits the default.
inline int search_tile_blocks(int nhyp, int nfreq, long long cells, int arms, bool want_coh, bool want_maps, const BankBudget& budget) {
  const long long per_block = (long long)nhyp * ((long long)sizeof(SearchAux) + 16LL * nfreq + (want_coh ? 16 * cells : 0) +
                                                 (want_maps ? 8 * cells + (long long)sizeof(gc_ddm_peak) * arms : 0));
  return (int)std::max<long long>(1, std::min<long long>(budget.tile_bytes / per_block, 1 << 20));
}

// The walk's state - per position of the window its run and where runs and maps begin and end, per hypothesis the runs and maps
// finished before the current tile (= the caller's row of the first one that ends in it) - and the current tile's products.
struct SearchWalk {
  std::vector<int> run_of, pos_flags;       // [nused]
  std::vector<int> runs_done, maps_done;    // [nhyp]
  std::vector<SearchAux> aux;               // [nhyp][nt]
  std::vector<int32_t> runs_now, maps_now;  // [nhyp]: runs / maps of the hypothesis that end in the tile, in device slots 0 ..
  int nslot_r = 0, nslot_m = 0;             // the most of them over the hypotheses: slots per hypothesis
};

// `want_maps` false: the open map is never stored, so no map flags and nothing kept.
inline void search_walk_begin(SearchWalk& w, const BankPartition& p, int nhyp, bool want_maps) {
  w.run_of.assign((size_t)p.nused(), 0);
  w.pos_flags.assign((size_t)p.nused(), SRCH_IN);
  for (int r = 0; r < p.nruns(); ++r) {
    for (int k = p.run_start[r]; k < p.run_start[r + 1]; ++k) w.run_of[k] = r;
    w.pos_flags[p.run_start[r]] |= SRCH_RUN_START;
    w.pos_flags[p.run_start[r + 1] - 1] |= SRCH_RUN_END;
  }
  for (int q = 0; want_maps && q < p.nmaps(); ++q) {
    w.pos_flags[p.run_start[p.map_start[q]]] |= SRCH_MAP_START;
    w.pos_flags[p.run_start[p.map_start[q + 1]] - 1] |= SRCH_MAP_END;
  }
  w.runs_done.assign((size_t)nhyp, 0);
  w.maps_done.assign((size_t)nhyp, 0);
  w.runs_now.assign((size_t)nhyp, 0);
  w.maps_now.assign((size_t)nhyp, 0);
}

// The tile of blocks [t_first, t_first + nt) of the list (weights: [nhyp][nblocks] or null); false: no hypothesis looks at it.
inline bool search_plan_tile(SearchWalk& w, const gc_block* blocks, int nblocks, const double* weights, const BankPartition& p,
                             const std::vector<int>& shift, int t_first, int nt) {
  const int nhyp = (int)shift.size();
  w.aux.assign((size_t)nhyp * nt, SearchAux{0, 0.0, 0, 0});
  w.nslot_r = w.nslot_m = 0;
  bool any = false;
  for (int h = 0; h < nhyp; ++h) {
    w.runs_done[h] += w.runs_now[h];  // the tile before
    w.maps_done[h] += w.maps_now[h];
    w.runs_now[h] = w.maps_now[h] = 0;
    const int lo = std::max(t_first, shift[h]), hi = std::min(t_first + nt, shift[h] + p.nused());
    for (int b = lo; b < hi; ++b) {
      const int k = b - shift[h];
      const int f = w.pos_flags[k];
      w.aux[(size_t)h * nt + (b - t_first)] = SearchAux{blocks[b].first_sample - blocks[shift[h] + p.run_start[w.run_of[k]]].first_sample,
                                                         weights ? weights[(size_t)h * nblocks + b] : 1.0, f, 0};
      w.runs_now[h] += (f & SRCH_RUN_END) != 0;
      w.maps_now[h] += (f & SRCH_MAP_END) != 0;
      any = true;
    }
    w.nslot_r = std::max(w.nslot_r, (int)w.runs_now[h]);
    w.nslot_m = std::max(w.nslot_m, (int)w.maps_now[h]);
  }
  return any;
}
