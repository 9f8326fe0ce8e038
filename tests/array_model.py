"""The numpy model of gc_array_covariance and gc_array_combine (include/gnsscorr.h), operation by operation.  The covariance is int64
products and sums (exact; Python integers where a test asks for them).  The combine loops over the records and the taps; every numpy
operation below is vectorised over the outputs and rounds by itself.  Neither has anything that may differ from the library."""
import numpy as np

REAL, IQ, QI = 0, 1, 2


def components_int(raw, layout):
    """(re, im) as int64 of a record in file order: I/Q as stored, Q/I swapped, real records im = 0."""
    x = np.asarray(raw).astype(np.int64)
    if layout == REAL:
        return x, np.zeros_like(x)
    return (x[1::2], x[0::2]) if layout == QI else (x[0::2], x[1::2])


def _window(v, first, n, lag):
    """v[first - lag .. first - lag + n) with zeros in front of sample 0"""
    lo = first - lag
    if lo >= 0:
        return v[lo:lo + n]
    return np.concatenate([np.zeros(min(-lo, n), dtype=v.dtype), v[0:max(lo + n, 0)]])


def covariance(raws, layout, first_sample, nsamples, nlags=1):
    """gc_array_covariance of the records `raws` (file order, one integer dtype and layout): int64 [L, K, K, 2] = (re, im) of
    C[l][a][b] = sum over n of x_a[n] conj(x_b[n - l])."""
    xs = [components_int(r, layout) for r in raws]
    K = len(xs)
    out = np.zeros((nlags, K, K, 2), dtype=np.int64)
    for a in range(K):
        ar, ai = (_window(v, first_sample, nsamples, 0) for v in xs[a])
        assert ar.shape[0] == nsamples, "the range ends beyond the record"
        for l in range(nlags):
            for b in range(K):
                br, bi = (_window(v, first_sample, nsamples, l) for v in xs[b])
                out[l, a, b, 0] = np.sum(ar * br + ai * bi)
                out[l, a, b, 1] = np.sum(ai * br - ar * bi)
    return out


def weights_pair(weights, nrecords):
    """(wr, wi) as float64 [K, T] of weights given as [K] or [K, T] complex or [K, T, 2] real"""
    w = np.asarray(weights)
    if w.ndim == 3:
        return w[..., 0].astype(np.float64), w[..., 1].astype(np.float64)
    w = w.astype(np.complex128).reshape(nrecords, -1)
    return w.real.copy(), w.imag.copy()


def combine(raws, src_layout, weights, dst_dtype, dst_layout, first_sample=0, noutputs=None):
    """gc_array_combine of the records `raws`.  Returns (the stored integers in dst's file order - an array of dst_dtype, 2 per output
    for I/Q and Q/I -, clipped, sum_sq, (a_r, a_i) before rounding)."""
    xs = [tuple(v.astype(np.float64) for v in components_int(r, src_layout)) for r in raws]
    K = len(xs)
    wr, wi = weights_pair(weights, K)
    T = wr.shape[1]
    if noutputs is None:
        noutputs = min(x[0].shape[0] for x in xs) - first_sample
    n = first_sample + np.arange(noutputs, dtype=np.int64)
    a_r, a_i = np.zeros(noutputs), np.zeros(noutputs)
    for a in range(K):
        # x[n] = 0 for n < 0: T - 1 zeros in front
        xr = np.concatenate([np.zeros(T - 1), xs[a][0]])
        xi = np.concatenate([np.zeros(T - 1), xs[a][1]])
        for k in range(T):
            idx = n - k + (T - 1)
            sr, si = xr[idx], xi[idx]
            pr = wr[a, k] * sr - wi[a, k] * si
            pi = wr[a, k] * si + wi[a, k] * sr
            a_r = a_r + pr
            a_i = a_i + pi
    return quantise(a_r, a_i, dst_dtype, dst_layout) + ((a_r, a_i),)


def quantise(a_r, a_i, dst_dtype, dst_layout):
    """The store and the result: clamp(rint(.)) per component in dst's file order, clipped, sum_sq (a_i of a real dst is not counted)."""
    noutputs = a_r.shape[0]
    info = np.iinfo(dst_dtype)
    rr, ri = np.rint(a_r), np.rint(a_i)
    o_r, o_i = np.clip(rr, info.min, info.max).astype(np.int64), np.clip(ri, info.min, info.max).astype(np.int64)
    c_r, c_i = (rr < info.min) | (rr > info.max), (ri < info.min) | (ri > info.max)
    if dst_layout == REAL:
        out = o_r.astype(dst_dtype)
        clipped, sum_sq = int(c_r.sum()), int(np.sum(o_r * o_r))
    else:
        out = np.empty(2 * noutputs, dtype=dst_dtype)
        first, second = (o_i, o_r) if dst_layout == QI else (o_r, o_i)
        out[0::2], out[1::2] = first, second
        clipped, sum_sq = int(c_r.sum() + c_i.sum()), int(np.sum(o_r * o_r) + np.sum(o_i * o_i))
    return out, clipped, sum_sq
