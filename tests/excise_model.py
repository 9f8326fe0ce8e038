"""The numpy models of the two excision calls' definitions (include/gnsscorr.h).  gc_excise_pulses in integers: mark the hot samples
of the range, dilate them by a difference array and a cumulative sum, blank, count the runs.  gc_excise_bins in float64 throughout
(np.fft per segment, the library's w, s, K and zero padding), returning the unrounded y - and the same pipeline in complex64 through
scipy.fft, the yardstick for a float32 implementation.  Samples in file order: c0 is the first value of each pair, c1 the second,
whatever the layout is called; a real record has c0 only."""
from types import SimpleNamespace

import numpy as np

REAL, IQ, QI = 0, 1, 2


def components(layout):
    return 1 if layout == REAL else 2


def norm2(raw, layout):
    """c0^2 + c1^2 of every sample as int64 (an int16 pair (-32768, -32768) gives 2^31)."""
    x = np.asarray(raw).astype(np.int64).reshape(-1, components(layout))
    return (x * x).sum(axis=1)


def blanked_mask(hot, before, after):
    """hot: bool [n] over the range.  Sample n is blanked iff a hot sample lies in [n - after, n + before], cut at the range's
    ends: every hot h adds +1 at max(h - before, 0) and -1 behind min(h + after, n - 1)."""
    n = hot.shape[0]
    h = np.flatnonzero(hot)
    d = np.zeros(n + 1, dtype=np.int64)
    np.add.at(d, np.maximum(h - before, 0), 1)
    np.add.at(d, np.minimum(h + after, n - 1) + 1, -1)
    return np.cumsum(d[:n]) > 0


def run_stats(hot, blanked):
    b = blanked.astype(np.int8)
    edges = np.diff(np.concatenate([[0], b, [0]]))
    starts, ends = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
    return SimpleNamespace(hot=int(hot.sum()), blanked=int(blanked.sum()), runs=int(starts.shape[0]),
                           longest=int((ends - starts).max()) if starts.shape[0] else 0)


def excise_pulses(raw, layout, first_sample, nsamples, threshold2, before=0, after=0):
    """(the record after the call as a new array of raw's dtype, stats) - the samples outside the range as they were."""
    nc = components(layout)
    out = np.array(raw, copy=True)
    per = out.reshape(-1, nc)
    hot = norm2(raw, layout)[first_sample:first_sample + nsamples] > int(threshold2)
    blanked = blanked_mask(hot, int(before), int(after))
    per[first_sample:first_sample + nsamples][blanked] = 0
    return out, run_stats(hot, blanked)


# ---- gc_excise_bins -------------------------------------------------------------------------------------------------------------------
def file_order(raw, layout):
    """z = c0 + i c1 of every sample as complex128 (z = c0 for a real record)."""
    x = np.asarray(raw).astype(np.float64).reshape(-1, components(layout))
    return x[:, 0] + 1j * x[:, 1] if layout != REAL else x[:, 0] + 0j


def window(nfft):
    """(w, s) as the library holds them: w[n] = (float) sin(pi (n + 0.5) / nfft), s[n] = (float)((double) w[n] / nfft)."""
    w = np.sin(np.pi * (np.arange(nfft) + 0.5) / nfft).astype(np.float32)
    return w, (w.astype(np.float64) / nfft).astype(np.float32)


def segments(nsamples, nfft):
    return -(-nsamples // (nfft // 2)) + 1


def excise_bins(z, gain, single=False):
    """The unrounded y of the definition for the range samples z (complex, file order): float64 throughout with np.fft - or
    (single=True) the same pipeline in complex64 through scipy.fft, every operation rounded to float32: the yardstick a float32
    implementation is held against.  K = ceil(n / H) + 1 segments, zeros outside the range."""
    gain = np.asarray(gain)
    nfft, n = gain.shape[0], z.shape[0]
    H, K = nfft // 2, segments(z.shape[0], nfft)
    w, s = window(nfft)
    ctype, rtype = (np.complex64, np.float32) if single else (np.complex128, np.float64)
    padded = np.zeros((K + 1) * H, dtype=ctype)
    padded[H:H + n] = z
    seg = np.lib.stride_tricks.as_strided(padded, shape=(K, nfft), strides=(H * padded.itemsize, padded.itemsize))
    a = seg * w.astype(rtype)
    if single:
        import scipy.fft
        v = scipy.fft.ifft(gain.astype(rtype) * scipy.fft.fft(a, axis=1), axis=1, norm="forward")     # the unnormalised inverse
        assert v.dtype == np.complex64
    else:
        v = np.fft.ifft(gain.astype(rtype) * np.fft.fft(a, axis=1), axis=1) * nfft
    c = v * s.astype(rtype)
    y = (c[:-1, H:] + c[1:, :H]).reshape(-1)[:n]
    assert y.dtype == ctype
    return y


def round_clamp(y, dtype, layout):
    """clamp(rint(y)) per component as a record of `dtype` in file order; the imaginary part of a real record's y is dropped."""
    info = np.iinfo(dtype)
    parts = [y.real] if layout == REAL else [y.real, y.imag]
    return np.clip(np.rint(np.stack(parts, axis=1)), info.min, info.max).astype(dtype).reshape(-1)
