// record_fmt.h — the record formats, once: the six encodings of a sample (dtype x layout) as a compile-time Mode, what a kernel
// needs to know about each (Fmt), the context's Mode, the dispatch from that run-time value to a kernel instantiation, and one
// sample of a record as (re, im) or, in file order, as the integers (c0, c1); the 16-byte vector of a record (RecVec) that the
// record-to-record kernels load, change sample by sample and store; and the rounding into a format (quantise).  A new format, or a
// new per-sample kernel, starts here and nowhere else.
// (Not here on purpose: acq_cond.hip keeps dtype and layout run-time values; the vector loaders of the hot kernels - load_chunk,
// load_words, sample_ab - are corr_common.h's.)
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

// The same for kernels that take a record in file order, without the swap (the probe, the excision): the Q/I modes fold onto I/Q, so
// four instantiations remain
template <typename F>
auto gc_with_file_mode(int mode, F&& f) {
  return gc_with_mode(mode, [&](auto m) {
    constexpr int M = decltype(m)::value;
    return f(std::integral_constant<int, M == I8_QI ? I8_IQ : M == I16_QI ? I16_IQ : M>{});
  });
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

// Sample idx of the record in file order, as integers: (c0, c1), c1 = 0 for a real record, no swap
template <int MODE>
__device__ __forceinline__ void file_sample(const uint8_t* __restrict__ base, long long idx, int& c0, int& c1) {
  using F = Fmt<MODE>;
  using V = std::conditional_t<F::value_bytes == 2, int16_t, int8_t>;
  const V* v = reinterpret_cast<const V*>(base) + idx * F::values;
  c0 = (int)v[0];
  c1 = 0;
  if constexpr (F::values == 2) c1 = (int)v[1];
}

// rint and clamp of y (float or double) into the format's integer range
template <int MODE, typename T>
__device__ __forceinline__ int quantise(T y) {
  using F = Fmt<MODE>;
  if constexpr (std::is_same<T, float>::value) return (int)fminf(fmaxf(rintf(y), (float)F::lo), (float)F::hi);
  else return (int)fmin(fmax(rint(y), F::lo), F::hi);
}

// The 16 bytes at byte offset `off` (a multiple of 16, possibly negative) of a record of `nbytes` bytes, as four words: F::per16
// samples, sample s of the vector in file order at bit s * 8 * F::bps.  A vector that lies inside the record is one 16-byte load
// and one 16-byte store (the record's base is 32-byte aligned: gc_internal.h, d_if); the record's partial last vector, and one in
// front of byte 0 or behind the last byte, goes byte by byte - load gives zero for the bytes that are not the record's, store leaves
// them alone.  The four words are four scalars, picked by selects: there is no array that a run-time sample number could index
// (which would send it to scratch).  Under a fully unrolled s the selects fold, under a rolled loop over s they stay in registers.
template <int MODE>
struct RecVec {
  using F = Fmt<MODE>;
  uint32_t w0, w1, w2, w3;

  __device__ __forceinline__ void load(const uint8_t* rec, long long off, long long nbytes) {
    if (off >= 0 && off + 16 <= nbytes) {
      const uint4 q = *(const uint4*)(rec + off);
      w0 = q.x, w1 = q.y, w2 = q.z, w3 = q.w;
    } else {
      const int lo = (int)max(0LL, -off), hi = (int)min(16LL, nbytes - off);  // the record's bytes of the vector: [lo, hi)
      uint32_t t[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k >= lo && k < hi) t[k >> 2] |= (uint32_t)rec[off + k] << (8 * (k & 3));
      w0 = t[0], w1 = t[1], w2 = t[2], w3 = t[3];
    }
  }
  __device__ __forceinline__ void store(uint8_t* rec, long long off, long long nbytes) const {
    if (off >= 0 && off + 16 <= nbytes) {
      *(uint4*)(rec + off) = words();
    } else {
      const int lo = (int)max(0LL, -off), hi = (int)min(16LL, nbytes - off);
      const uint32_t t[4] = {w0, w1, w2, w3};
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k >= lo && k < hi) rec[off + k] = (uint8_t)(t[k >> 2] >> (8 * (k & 3)));
    }
  }
  __device__ __forceinline__ uint4 words() const { return make_uint4(w0, w1, w2, w3); }
  // sample s as file-order integers (c1 = 0 for a real record)
  __device__ __forceinline__ void get(int s, int& c0, int& c1) const {
    const int bit = s * F::bps * 8, k = bit >> 5;
    const uint32_t raw = (k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3) >> (bit & 31);
    c0 = F::value_bytes == 1 ? (int)(signed char)(raw & 0xffu) : (int)(short)(raw & 0xffffu);
    c1 = F::values == 1 ? 0 : F::value_bytes == 1 ? (int)(signed char)((raw >> 8) & 0xffu) : (int)(short)(raw >> 16);
  }
  // (o0, o1), already inside the format's range, at sample s
  __device__ __forceinline__ void put(int s, int o0, int o1) {
    constexpr uint32_t vmask = F::value_bytes == 1 ? 0xffu : 0xffffu;
    uint32_t bits = (uint32_t)o0 & vmask;
    if constexpr (F::values == 2) bits |= ((uint32_t)o1 & vmask) << (8 * F::value_bytes);
    replace(s, bits);
  }
  __device__ __forceinline__ void zero(int s) { replace(s, 0u); }

 private:
  __device__ __forceinline__ void replace(int s, uint32_t bits) {
    constexpr uint32_t smask = F::bps == 4 ? 0xffffffffu : (1u << (F::bps * 8 % 32)) - 1u;
    const int bit = s * F::bps * 8, k = bit >> 5, sh = bit & 31;
    const uint32_t keep = ~(smask << sh), ins = bits << sh;
    w0 = k == 0 ? (w0 & keep) | ins : w0;
    w1 = k == 1 ? (w1 & keep) | ins : w1;
    w2 = k == 2 ? (w2 & keep) | ins : w2;
    w3 = k == 3 ? (w3 & keep) | ins : w3;
  }
};

}  // namespace gcorr
