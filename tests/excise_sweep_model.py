"""The numpy model of gc_excise_sweep's definition (include/gnsscorr.h) on top of excise_model: gc_excise_bins' segments, window and
overlap-add, with the power of every cell (segment, bin), the comparison with the limit, the circular dilation by `widen` bins and
zeros in the cut cells.  float64 throughout with np.fft - or (single=True) the same pipeline in complex64 through scipy.fft, every
operation rounded to float32: the yardstick a float32 implementation is held against.  A per-segment cut mask may be given from
outside: then the decisions are the caller's and the model answers for the arithmetic alone."""
from types import SimpleNamespace

import numpy as np

import excise_model as M


def mask_words(nfft):
    return (nfft + 63) // 64


def dilate(hot, widen):
    """hot: bool [K, nfft].  Cell (k, b) is cut iff a bin b' of row k is hot with min(|b - b'|, nfft - |b - b'|) <= widen: bin
    nfft - 1 is next to bin 0; with 2 widen + 1 >= nfft one hot bin cuts the row."""
    hot = np.asarray(hot, dtype=bool)
    nfft = hot.shape[1]
    if 2 * widen + 1 >= nfft:
        return np.repeat(hot.any(axis=1, keepdims=True), nfft, axis=1)
    out = hot.copy()
    for d in range(1, int(widen) + 1):
        out |= np.roll(hot, d, axis=1) | np.roll(hot, -d, axis=1)
    return out


def spectra(z, nfft, single=False):
    """X [K, nfft] of the range samples z (complex, file order): the windowed, zero-padded segments transformed."""
    n = z.shape[0]
    H, K = nfft // 2, M.segments(n, nfft)
    w, _ = M.window(nfft)
    ctype, rtype = (np.complex64, np.float32) if single else (np.complex128, np.float64)
    padded = np.zeros((K + 1) * H, dtype=ctype)
    padded[H:H + n] = z
    seg = np.lib.stride_tricks.as_strided(padded, shape=(K, nfft), strides=(H * padded.itemsize, padded.itemsize))
    a = seg * w.astype(rtype)
    if single:
        import scipy.fft
        X = scipy.fft.fft(a, axis=1)
    else:
        X = np.fft.fft(a, axis=1)
    assert X.dtype == ctype
    return X


def power(X):
    """re * re + im * im, each product and the sum rounded in X's own precision."""
    return X.real * X.real + X.imag * X.imag


def excise_sweep(z, limit, widen=0, gain=None, cut=None, single=False):
    """SimpleNamespace(y, power, hot, cut) of the definition for the range samples z: y the unrounded output [n], power [K, nfft],
    hot = power > limit, cut = dilate(hot, widen) - or the `cut` given from outside (bool [K, nfft]), which then decides alone."""
    limit = np.asarray(limit, dtype=np.float32)
    nfft, n = limit.shape[0], z.shape[0]
    H = nfft // 2
    _, s = M.window(nfft)
    ctype, rtype = (np.complex64, np.float32) if single else (np.complex128, np.float64)
    X = spectra(z, nfft, single)
    P = power(X)
    hot = P > limit.astype(rtype)
    cut = dilate(hot, widen) if cut is None else np.asarray(cut, dtype=bool)
    Y = X if gain is None else np.asarray(gain).astype(rtype) * X
    Y = np.where(cut, ctype(0), Y)
    if single:
        import scipy.fft
        v = scipy.fft.ifft(Y, axis=1, norm="forward")                   # the unnormalised inverse
    else:
        v = np.fft.ifft(Y, axis=1) * nfft
    c = v * s.astype(rtype)
    y = (c[:-1, H:] + c[1:, :H]).reshape(-1)[:n]
    assert y.dtype == ctype and P.dtype == rtype
    return SimpleNamespace(y=y, power=P, hot=hot, cut=cut)


def counts(hot, cut):
    """(segments, hot, cut, segments_cut, most_cut) and bin_cut [nfft] of a pair of masks."""
    per = cut.sum(axis=1)
    return (int(cut.shape[0]), int(hot.sum()), int(cut.sum()), int((per > 0).sum()), int(per.max())), cut.sum(axis=0).astype(np.int64)


def chirp(n, period, amp, f0=-0.4, f1=0.4):
    """A sawtooth chirp of `amp`: the frequency rises from f0 to f1 (of the sampling frequency) in `period` samples, then starts again."""
    t = np.arange(n) % period
    return amp * np.exp(2j * np.pi * (f0 * t + 0.5 * (f1 - f0) / period * t * t))
