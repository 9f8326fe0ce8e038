// record_check.h — what the record-to-record calls (gc_cancel, gc_excise_pulses, gc_excise_bins, gc_downconvert, gc_resample,
// gc_array_combine) and the probe ask of their records on the host, once.  Nothing here calls HIP; the plan headers include it, and with them the CPU shims under tests/.
#pragma once
#include <cstdint>

#include "gc_internal.h"

inline int gc_record_bps(const gc_context* c) { return gc_bytes_per_sample(c->if_dtype, c->if_layout); }

// a's record is b's or shares bytes with it (both hold one)
inline bool gc_records_overlap(const gc_context* a, const gc_context* b) {
  const uint64_t abytes = a->if_nsamples * (uint64_t)gc_record_bps(a), bbytes = b->if_nsamples * (uint64_t)gc_record_bps(b);
  return a->d_if == b->d_if || (a->d_if < b->d_if + bbytes && b->d_if < a->d_if + abytes);
}

// A source and the destination that takes its place: GC_E_STATE without a record on either side, GC_E_INVALID for a destination that
// differs from the source in device, sample count, dtype or layout, or overlaps it without being it
inline int check_record_pair(const char* fn, const gc_context* src, const gc_context* dst) {
  if (!src->d_if || !dst->d_if) {
    gc_set_error("%s: no IF record loaded", fn);
    return GC_E_STATE;
  }
  if (dst->device != src->device || dst->if_nsamples != src->if_nsamples || dst->if_dtype != src->if_dtype || dst->if_layout != src->if_layout) {
    gc_set_error("%s: the destination record differs from the source's in device, sample count, dtype or layout", fn);
    return GC_E_INVALID;
  }
  if (dst->d_if != src->d_if && gc_records_overlap(dst, src)) {
    gc_set_error("%s: the destination record overlaps the source without being the same record", fn);
    return GC_E_INVALID;
  }
  return GC_OK;
}

// The samples [first, first + n) of ctx's record (first >= 0, n >= 0: the caller's argument check), without forming a sum that may
// leave int64: GC_E_RANGE
inline int check_record_range(const char* fn, const gc_context* ctx, long long first, long long n) {
  const unsigned long long have = ctx->if_nsamples;
  if ((unsigned long long)first > have || have - (unsigned long long)first < (unsigned long long)n) {
    gc_set_error("%s: %lld samples from %lld end beyond the record (%llu samples)", fn, n, first, have);
    return GC_E_RANGE;
  }
  return GC_OK;
}
