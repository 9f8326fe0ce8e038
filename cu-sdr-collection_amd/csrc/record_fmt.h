// record_fmt.h — the record formats, once: the six encodings of a sample (dtype x layout) as a compile-time Mode, what a kernel
// needs to know about each (Fmt), the context's Mode, the dispatch from that run-time value to a kernel instantiation, and one
// sample of a record as (re, im).  A new format, or a new per-sample kernel, starts here and nowhere else.
// (Not here on purpose: probe.hip reads a record in file order, without the swap; acq_cond.hip keeps dtype and layout run-time
// values; the vector loaders of the hot kernels - load_chunk, load_words, sample_ab - are corr_common.h's.)
#pragma once
#include <type_traits>

#include "gc_internal.h"

namespace gcorr {

enum Mode { I8_IQ = 0, I8_QI, I16_IQ, I16_QI, I8_REAL, I16_REAL };

template <int MODE>
struct Fmt {
  static constexpr int value_bytes = (MODE == I16_IQ || MODE == I16_QI || MODE == I16_REAL) ? 2 : 1;
  static constexpr int values = (MODE == I8_REAL || MODE == I16_REAL) ? 1 : 2;  // per sample
  static constexpr int bps = value_bytes * values;                             // bytes per sample
  static constexpr int per16 = 16 / bps;                                       // samples per 16 bytes
  static constexpr bool swap = (MODE == I8_QI || MODE == I16_QI);              // the record holds (Q, I)
  static constexpr double lo = value_bytes == 2 ? -32768.0 : -128.0, hi = value_bytes == 2 ? 32767.0 : 127.0;  // the integer range
};

inline int gc_record_mode(const gc_context* ctx) {
  if (ctx->if_dtype == GC_I8) return ctx->if_layout == GC_IQ ? I8_IQ : ctx->if_layout == GC_QI ? I8_QI : I8_REAL;
  return ctx->if_layout == GC_IQ ? I16_IQ : ctx->if_layout == GC_QI ? I16_QI : I16_REAL;
}

// f(std::integral_constant<int, MODE>{}) for the run-time mode: the one six-way ladder behind every kernel that is instantiated
// per record format.  (A dispatch over a subset of the formats - corr_multi.hip, corr_cboc.hip - stays a subset, where it is.)
template <typename F>
auto gc_with_mode(int mode, F&& f) {
  switch (mode) {
    case I8_IQ: return f(std::integral_constant<int, I8_IQ>{});
    case I8_QI: return f(std::integral_constant<int, I8_QI>{});
    case I16_IQ: return f(std::integral_constant<int, I16_IQ>{});
    case I16_QI: return f(std::integral_constant<int, I16_QI>{});
    case I8_REAL: return f(std::integral_constant<int, I8_REAL>{});
    default: return f(std::integral_constant<int, I16_REAL>{});
  }
}

// Sample idx of the record as (re, im) = (data1, data2) of tracking.m:233-235 (Q/I records, GLONASS: swapped, GLO_GL1
// tracking.m:227; real records: im = 0), in float or double - the integers convert exactly to either.  An int8 pair is one
// 16-bit load (the record's base is 32-byte aligned).
template <int MODE, typename T>
__device__ __forceinline__ void record_sample(const uint8_t* __restrict__ base, long long idx, T& re, T& im) {
  using F = Fmt<MODE>;
  T x0, x1 = (T)0;
  if constexpr (F::values == 2 && F::value_bytes == 1) {
    const unsigned int w = *(const unsigned short*)(base + 2 * idx);
    x0 = (T)(signed char)(w & 0xffu);
    x1 = (T)(signed char)(w >> 8);
  } else if constexpr (F::values == 2) {
    const short* s = (const short*)base + 2 * idx;
    x0 = (T)s[0];
    x1 = (T)s[1];
  } else if constexpr (F::value_bytes == 1) {
    x0 = (T)((const signed char*)base)[idx];
  } else {
    x0 = (T)((const short*)base)[idx];
  }
  re = F::swap ? x1 : x0;
  im = F::swap ? x0 : x1;
}

}  // namespace gcorr
