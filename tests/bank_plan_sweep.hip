// The integrate walk and the search walk of csrc/bank_plan.h over the lists of a file, as a program of its own: built for the host
// with the address and undefined-behaviour sanitizers by tests/test_bank_plan_cpu.py and run as a child process, so that an index the
// plan gets wrong is a report and a non-zero exit status.  No device is touched and nothing is loaded into another process.
//
// The file: whitespace-separated integers, per case
//   nblocks {blksize first_sample}[nblocks]  nruns run_len[nruns]  nmaps map_len[nmaps]  nhyp shift[nhyp]  budget_chunks tile_blocks
// (budget_chunks, tile_blocks 0: the library's budgets).  The runs hold the first sum(run_len) blocks, every shift keeps its window
// inside the list.  Exit status: 0 all walks done and their invariants held, 1 an invariant failed, 2 bad input.
#include <cstdarg>
#include <cstdio>

#include "../cu-sdr-collection_amd/csrc/bank_plan.h"

void gc_set_error(const char*, ...) {}

#define REQUIRE(cond)                                                              \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      std::fprintf(stderr, "case %d: %s (line %d)\n", g_case, #cond, __LINE__);    \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

static int g_case = 0;

static bool read_list(FILE* f, std::vector<int32_t>& v) {
  int n;
  if (std::fscanf(f, "%d", &n) != 1 || n < 0) return false;
  v.resize((size_t)n);
  for (int& x : v)
    if (std::fscanf(f, "%d", &x) != 1) return false;
  return true;
}

// every block in one sub-batch, every run and map fetched once to its own row, every index inside the buffers the pre-walk sized
static int integrate_walk(const std::vector<gc_block>& b, int nused, const std::vector<double>& weights, const BankPartition& p, long long max_chunks) {
  const DdmSizes z = ddm_walk_sizes(b.data(), nused, max_chunks, p);
  std::vector<int> coh((size_t)z.nr, -1), pow((size_t)std::max(z.nm, 1), -1);  // the run / map whose accumulator a device row holds
  DdmLaunch l;
  int next = 0, runs = 0, maps = 0;
  for (DdmStep s; ddm_next_step(s, b.data(), nused, max_chunks, p);) {
    ddm_plan_step(s, b.data(), weights.data(), p, l);
    REQUIRE(s.first == next && s.nb >= 1 && s.nb <= z.nb && s.nr >= 1 && s.nr <= z.nr && s.nm <= z.nm);
    REQUIRE(s.chunk_base.back() <= max_chunks || s.nb == 1);
    REQUIRE(l.run_base.front() == 0 && l.run_base.back() == s.nb && s.r0 == runs && s.q0 == maps);
    if (l.carry_run) REQUIRE(coh[0] == s.r0);
    for (int k = 0; k < s.nr; ++k) {
      REQUIRE(l.run_base[k] < l.run_base[k + 1]);
      for (int i = l.run_base[k]; i < l.run_base[k + 1]; ++i)
        REQUIRE(l.aux[i].dn == b[s.first + i].first_sample - b[p.run_start[s.r0 + k]].first_sample && l.aux[i].w == weights[s.first + i]);
      coh[k] = s.r0 + k;
    }
    if (s.nm > 0) {
      REQUIRE(l.map_base.front() == 0 && l.map_base.back() == s.nfin);
      if (l.carry_map) REQUIRE(pow[0] == s.q0);
      for (int k = 0; k < s.nm; ++k) pow[k] = s.q0 + k;
      if (l.keep_map) pow[0] = pow[l.keep_map];
    }
    if (l.keep_run) coh[0] = coh[l.keep_run];
    REQUIRE(l.keep_run < s.nr && l.keep_map < std::max(s.nm, 1));
    next += s.nb;
    runs += s.nfin;
    maps += s.mfin;
  }
  REQUIRE(next == nused && runs == p.nruns() && maps == p.nmaps());
  return 0;
}

// every block in one tile, per hypothesis as many run and map ends as the partition has, in slots the tile has room for
static int search_walk(const std::vector<gc_block>& b, const std::vector<double>& weights, const BankPartition& p, const std::vector<int>& shift,
                       long long max_chunks, int tile, bool want_maps) {
  const int nblocks = (int)b.size(), nhyp = (int)shift.size();
  SearchWalk w;
  search_walk_begin(w, p, nhyp, want_maps);
  std::vector<int32_t> base;
  std::vector<int> runs((size_t)nhyp, 0), maps((size_t)nhyp, 0);
  for (int first = 0, nb; first < nblocks; first += nb) {
    nb = bank_cut(b.data(), nblocks, first, max_chunks, base);
    REQUIRE(nb >= 1);
    for (int t0 = 0; t0 < nb; t0 += tile) {
      const int nt = std::min(tile, nb - t0);
      const bool any = search_plan_tile(w, b.data(), nblocks, weights.data(), p, shift, first + t0, nt);
      bool seen = false;
      for (int h = 0; h < nhyp; ++h) {
        REQUIRE(w.runs_done[h] == runs[h] && w.maps_done[h] == maps[h] && w.runs_now[h] <= w.nslot_r && w.maps_now[h] <= w.nslot_m);
        int re = 0, me = 0;
        for (int k = 0; k < nt; ++k) {
          const SearchAux& a = w.aux[(size_t)h * nt + k];
          const int pos = first + t0 + k - shift[h];
          REQUIRE(((a.flags & SRCH_IN) != 0) == (pos >= 0 && pos < p.nused()));
          if (!a.flags) continue;
          seen = true;
          REQUIRE(a.w == weights[(size_t)h * nblocks + first + t0 + k]);
          REQUIRE(a.dn == b[first + t0 + k].first_sample - b[shift[h] + p.run_start[w.run_of[pos]]].first_sample);
          re += (a.flags & SRCH_RUN_END) != 0;
          me += (a.flags & SRCH_MAP_END) != 0;
        }
        REQUIRE(re == w.runs_now[h] && me == w.maps_now[h]);
        runs[h] += re;
        maps[h] += me;
      }
      REQUIRE(seen == any);
    }
  }
  for (int h = 0; h < nhyp; ++h) REQUIRE(runs[h] == p.nruns() && maps[h] == (want_maps ? p.nmaps() : 0));
  return 0;
}

int main(int argc, char** argv) {
  FILE* f = argc == 2 ? std::fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  int nblocks;
  while (std::fscanf(f, "%d", &nblocks) == 1) {
    ++g_case;
    if (nblocks < 1) return 2;
    std::vector<gc_block> b((size_t)nblocks, gc_block());
    for (gc_block& k : b) {
      long long s0;
      if (std::fscanf(f, "%d %lld", &k.blksize, &s0) != 2 || k.blksize < 1) return 2;
      k.first_sample = s0;
    }
    std::vector<int32_t> run_len, map_len, shifts;
    int budget_chunks, tile_blocks;
    if (!read_list(f, run_len) || !read_list(f, map_len) || !read_list(f, shifts) || std::fscanf(f, "%d %d", &budget_chunks, &tile_blocks) != 2) return 2;
    const int nhyp = (int)shifts.size();
    BankPartition p;
    if (bank_partition("sweep", nblocks, (int)run_len.size(), run_len.data(), (int)map_len.size(), map_len.data(), false, &p) || nhyp < 1) return 2;
    const std::vector<int> shift(shifts.begin(), shifts.end());
    for (int s : shift)
      if (s < 0 || s > nblocks - p.nused()) return 2;
    std::vector<double> weights((size_t)nhyp * nblocks);
    for (size_t i = 0; i < weights.size(); ++i) weights[i] = (double)i + 0.5;
    BankBudget budget;  // one cell: 16 bytes of partial sums per chunk; a block of a tile costs every hypothesis 24 + 16 + 16 + 8 + 16 bytes
    if (budget_chunks > 0) budget.partial_bytes = 16LL * budget_chunks;
    if (tile_blocks > 0) budget.tile_bytes = 80LL * nhyp * tile_blocks;
    const long long max_chunks = bank_max_chunks(2, budget);
    const int tile = search_tile_blocks(nhyp, 1, 1, 1, true, true, budget);
    if (tile_blocks > 0 && tile != tile_blocks) {
      std::fprintf(stderr, "case %d: a tile of %d blocks, %d asked for\n", g_case, tile, tile_blocks);
      return 1;
    }
    if (int rc = integrate_walk(b, p.nused(), weights, p, max_chunks)) return rc;
    for (bool want_maps : {true, false})
      if (int rc = search_walk(b, weights, p, shift, max_chunks, tile, want_maps && p.nmaps() > 0)) return rc;
  }
  std::fclose(f);
  std::printf("%d cases\n", g_case);
  return g_case > 0 ? 0 : 2;
}
