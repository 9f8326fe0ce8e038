// mask_words of csrc/corr_common.h on the CPU, next to a reference that tests every sample on its own.  Built by
// tests/test_mask_words_cpu.py with the flags of corr_fast.hip; no GPU is touched.
#include <cstdint>

#include "../cu-sdr-collection_amd/csrc/corr_common.h"

using namespace gcorr;

namespace {

// sample j of the chunk is valid iff 0 <= i0 + j < N; an invalid sample's bits (8 * bytes per sample) are cleared in its word
template <int MODE, int SPL>
void reference(unsigned int* w, int i0, int N) {
  const int bits = 8 * Fmt<MODE>::bps;
  for (int j = 0; j < SPL; ++j) {
    const long long i = (long long)i0 + j;
    if (i >= 0 && i < (long long)N) continue;
    const int bit0 = j * bits;
    for (int b = bit0; b < bit0 + bits; ++b) w[b / 32] &= ~(1u << (b % 32));
  }
}

template <int MODE, int SPL>
int run(const unsigned int* in, int i0, int N, unsigned int* got, unsigned int* want) {
  constexpr int NW = SPL * Fmt<MODE>::bps / 4;
  unsigned int w[NW];
  for (int q = 0; q < NW; ++q) w[q] = want[q] = in[q];
  mask_words<MODE, SPL>(w, i0, N);
  reference<MODE, SPL>(want, i0, N);
  for (int q = 0; q < NW; ++q) got[q] = w[q];
  return NW;
}

}  // namespace

extern "C" {

// Words of a chunk after mask_words (got) and after the per-sample reference (want); returns the number of words, 0 for a
// (mode, spl) pair the kernels do not instantiate.  in / got / want hold 8 words.
int mask_shim_run(int mode, int spl, const unsigned int* in, int i0, int N, unsigned int* got, unsigned int* want) {
  if (spl == 16) {
    if (mode == I8_IQ) return run<I8_IQ, 16>(in, i0, N, got, want);
    if (mode == I8_QI) return run<I8_QI, 16>(in, i0, N, got, want);
    return 0;
  }
  if (spl != 8) return 0;
  switch (mode) {
    case I8_IQ: return run<I8_IQ, 8>(in, i0, N, got, want);
    case I8_QI: return run<I8_QI, 8>(in, i0, N, got, want);
    case I16_IQ: return run<I16_IQ, 8>(in, i0, N, got, want);
    case I16_QI: return run<I16_QI, 8>(in, i0, N, got, want);
    case I8_REAL: return run<I8_REAL, 8>(in, i0, N, got, want);
    case I16_REAL: return run<I16_REAL, 8>(in, i0, N, got, want);
    default: return 0;
  }
}

// The whole sweep of one (mode, spl) in one call: i0 in [-spl - 1, spl + 1] x N in [0, 3 spl + 1], on all-ones words and on the
// given pattern.  Returns the number of cases run; *bad counts the cases whose words differ, first_bad = {i0, N} of the first.
int mask_shim_sweep(int mode, int spl, const unsigned int* pattern, int* bad, int* first_bad) {
  unsigned int ones[8], got[8], want[8];
  for (int q = 0; q < 8; ++q) ones[q] = 0xffffffffu;
  int cases = 0;
  *bad = 0;
  for (int i0 = -spl - 1; i0 <= spl + 1; ++i0)
    for (int N = 0; N <= 3 * spl + 1; ++N)
      for (int which = 0; which < 2; ++which) {
        const int nw = mask_shim_run(mode, spl, which ? pattern : ones, i0, N, got, want);
        if (nw == 0) return 0;
        bool same = true;
        for (int q = 0; q < nw; ++q) same = same && got[q] == want[q];
        if (!same && (*bad)++ == 0) {
          first_bad[0] = i0;
          first_bad[1] = N;
        }
        ++cases;
      }
  return cases;
}

}  // extern "C"
