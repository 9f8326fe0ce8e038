// fft_plan.h — the plan of the four-step transform (n = n1 x n2; acq_fft.hip makes it and owns the pass kernels) and the ONE statement
// of the order its results are stored in.  For the acquisition (acq_internal.h includes this) and for the record units that transform
// segments (seg_fft.h).  The storage-order functions compile without a device pass; tests/fft_order_shim.hip runs them on the CPU.
#pragma once
#include "gc_internal.h"

#if defined(__HIPCC__)
#define GC_FFT_HD __host__ __device__
#else
#define GC_FFT_HD
#endif

namespace gcacq {

constexpr int kMaxRadices = 12;

struct SubPlan {
  int len;
  int nrad;
  int rad[kMaxRadices];
};

struct Plan {
  int n, n1, n2;  // n = n1 * n2; n1 = column length (stride n2), n2 = row length (contiguous)
  SubPlan p1, p2;
};

// Storage order [k1][k2]: position k1 n2 + k2 (k1 < n1, k2 < n2) holds natural bin k1 + n1 k2.  One division and one multiply-subtract each way.
GC_FFT_HD inline int fft_bin_at(int pos, int n1, int n2) {  // the natural bin that storage position `pos` holds
  const int k1 = pos / n2, k2 = pos - k1 * n2;
  return k1 + n1 * k2;
}
GC_FFT_HD inline int fft_pos_of(int bin, int n1, int n2) {  // the storage position that holds natural bin `bin`
  const int k2 = bin / n1, k1 = bin - k2 * n1;
  return k1 * n2 + k2;
}

// ---- acq_fft.hip ------------------------------------------------------------------------------------------------------------------
bool make_plan(int n, Plan* pl);
// make_plan for a caller that has no other length to try: GC_E_UNSUPPORTED and the planner's message where it refuses n
int plan_or_refuse(int n, Plan* pl);
// exp(-2 pi i k / n), k < n, computed in float64 and rounded once, into d_tw on the context's stream, which is waited for
int upload_twiddles(gc_context* ctx, int n, float2* d_tw);

}  // namespace gcacq
