"""Thin object wrapper over the C-ABI (one context = one GPU = one host thread)."""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np

from . import _lib as L


def device_count() -> int:
    """gc_device_count: the HIP devices this process sees (valid Engine(device_id) are 0 .. n - 1); 0 without a GPU.  No context."""
    n = C.c_int(0)
    L.check(L.load().gc_device_count(C.byref(n)))
    return int(n.value)


# precision= keyword of the tracking calls -> gc_set_precision value
PRECISIONS = {"single": L.GC_PREC_F32, "double": L.GC_PREC_F64}


def precision_code(precision) -> int | None:
    """gc_set_precision value of a precision= keyword ("single" | "double"; None: the context's setting as it is).
    Raises ValueError for anything else, before any library call."""
    if precision is None:
        return None
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"precision must be 'single' or 'double', not {precision!r}")
    return PRECISIONS[precision]


class Engine:
    """Owns a gc_context on `device_id`.  Raises GnssCorrError when no MI355X is visible."""

    def __init__(self, device_id: int = 0):
        self._lib = L.load()
        self._ctx = C.c_void_p()
        L.check(self._lib.gc_create(C.byref(self._ctx), int(device_id)))
        self.device_id = device_id
        self.acq_stats = {}          # transforms of the searches since the caller last cleared it (_count_transforms)

    # ---- lifetime ------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.gc_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_info(self):
        name = C.create_string_buffer(128)
        cus = C.c_int()
        L.check(self._lib.gc_device_info(self._ctx, name, 128, C.byref(cus)))
        return name.value.decode(), cus.value

    def acq_guard_stats(self):
        """gc_acq_guard_stats of the last search: {ties, max_dev, eps} (include/gnsscorr.h)."""
        t, d, e = C.c_int32(), C.c_double(), C.c_double()
        L.check(self._lib.gc_acq_guard_stats(self._ctx, C.byref(t), C.byref(d), C.byref(e)))
        return {"ties": int(t.value), "max_dev": float(d.value), "eps": float(e.value)}

    def synchronize(self):
        L.check(self._lib.gc_synchronize(self._ctx))

    # ---- IF buffer -----------------------------------------------------------------------
    @staticmethod
    def _fmt(arr_dtype, layout):
        if arr_dtype == np.int8:
            dt = L.GC_I8
        elif arr_dtype == np.int16:
            dt = L.GC_I16
        else:
            raise TypeError("IF samples must be int8 or int16 (settings.dataType)")
        comp = 1 if layout == L.GC_REAL else 2
        return dt, comp

    def load_if(self, raw: np.ndarray, layout: int = L.GC_IQ, fs: float | None = None):
        """raw: the file content as a 1-D int8/int16 array (interleaved for IQ/QI)."""
        raw = np.ascontiguousarray(raw)
        dt, comp = self._fmt(raw.dtype, layout)
        n = raw.shape[0] // comp
        L.check(self._lib.gc_load_if(self._ctx, raw.ctypes.data_as(C.c_void_p), n, dt, layout))
        if fs is not None:
            self.set_sampling_freq(fs)

    def load_if_packed2(self, packed: np.ndarray, fs: float | None = None):
        """packed: uint8 array, two 2-bit sign-magnitude complex samples per byte (unpack_cplx.m's input format)."""
        b = np.ascontiguousarray(packed, dtype=np.uint8)
        L.check(self._lib.gc_load_if_packed2(self._ctx, b.ctypes.data_as(C.c_void_p), b.shape[0]))
        if fs is not None:
            self.set_sampling_freq(fs)

    def open_if_file(self, path: str, skip_bytes: int = 0, nsamples: int = 0, dtype=np.int8,
                     layout: int = L.GC_IQ, fs: float | None = None):
        dt, _ = self._fmt(np.dtype(dtype), layout)
        L.check(self._lib.gc_open_if_file(self._ctx, path.encode(), skip_bytes, nsamples, dt, layout))
        if fs is not None:
            self.set_sampling_freq(fs)

    def alloc_if(self, nsamples: int, dtype=np.int8, layout: int = L.GC_IQ):
        dt, _ = self._fmt(np.dtype(dtype), layout)
        L.check(self._lib.gc_alloc_if(self._ctx, nsamples, dt, layout))

    def attach_if(self, device_ptr: int, nsamples: int, dtype=np.int8, layout: int = L.GC_IQ):
        dt, _ = self._fmt(np.dtype(dtype), layout)
        L.check(self._lib.gc_attach_if(self._ctx, C.c_void_p(device_ptr), nsamples, dt, layout))

    def share_if(self, owner: "Engine"):
        """Read `owner`'s IF record from this context too (same GPU, no copy): gc_share_if."""
        L.check(self._lib.gc_share_if(self._ctx, owner._ctx))
        self._if_owner = owner  # keep the owner (and with it the device allocation) alive

    def if_buffer(self):
        p = C.c_void_p()
        n = C.c_uint64()
        L.check(self._lib.gc_if_buffer(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def if_format(self):
        """(dtype, layout) of the loaded record: GC_I8 / GC_I16, GC_IQ / GC_QI / GC_REAL."""
        dt, lay = C.c_int(), C.c_int()
        L.check(self._lib.gc_if_format(self._ctx, C.byref(dt), C.byref(lay)))
        return dt.value, lay.value

    def acq_input(self, first_sample: int, fs: float, n_long: int | None = None):
        """What an acquisition's searches read: (source, first_sample, samples available from there).  int8 I/Q records are read
        in place; any other format (int16 files, Q/I order, real samples) goes through a float copy of longSignal on the device
        (gc_acq_signal_from_record; n_long samples, by default what the record holds up to 0.3 s)."""
        dt, lay = self.if_format()
        avail = int(self.if_buffer()[1]) - int(first_sample)
        if dt == L.GC_I8 and lay == L.GC_IQ:
            return 0, int(first_sample), avail if n_long is None else min(avail, int(n_long))
        n = min(avail, int(n_long) if n_long is not None else int(0.3 * fs))
        L.check(self._lib.gc_acq_signal_from_record(self._ctx, int(first_sample), n))
        return 1, 0, n

    def acq_set_signal(self, x: np.ndarray):
        """gc_acq_set_signal: longSignal itself (any complex row) as the searches' source = 1."""
        z = np.ascontiguousarray(x, dtype=np.complex64)
        L.check(self._lib.gc_acq_set_signal(self._ctx, z.view(np.float32).ctypes.data_as(C.POINTER(C.c_float)), z.shape[0]))

    def read_if(self, first: int, n: int, dtype=np.int8, layout: int = L.GC_IQ) -> np.ndarray:
        comp = 1 if layout == L.GC_REAL else 2
        out = np.empty(n * comp, dtype=dtype)
        L.check(self._lib.gc_read_if(self._ctx, first, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def force_generic_kernel(self, on: bool):
        L.check(self._lib.gc_force_generic_kernel(self._ctx, int(bool(on))))

    def set_precision(self, precision: str):
        """gc_set_precision: "single" (float32 kernels, the default) or "double" (the float64 kernel, corr_f64.hip) for
        gc_correlate and every tracking call of this context until changed."""
        code = precision_code(precision)
        if code is None:
            raise ValueError("precision must be 'single' or 'double', not None")
        L.check(self._lib.gc_set_precision(self._ctx, code))

    @property
    def precision(self) -> str:
        """The context's setting (gc_get_precision): "single" or "double"."""
        v = C.c_int(-1)
        L.check(self._lib.gc_get_precision(self._ctx, C.byref(v)))
        return "double" if v.value == L.GC_PREC_F64 else "single"

    @contextlib.contextmanager
    def _precision_for_call(self, code):
        """The precision= keyword of one call: set, and the previous setting restored whatever happens (a session-wide engine
        must not carry one test's float64 into the next)."""
        if code is None:
            yield
            return
        prev = C.c_int(L.GC_PREC_F32)
        L.check(self._lib.gc_get_precision(self._ctx, C.byref(prev)))
        L.check(self._lib.gc_set_precision(self._ctx, code))
        try:
            yield
        finally:
            self._lib.gc_set_precision(self._ctx, prev.value)

    def set_sampling_freq(self, fs: float):
        L.check(self._lib.gc_set_sampling_freq(self._ctx, float(fs)))
        self.sampling_freq = float(fs)   # what the context holds (receiver.downconvert_band designs its filter for it)

    # ---- code tables ---------------------------------------------------------------------
    def set_channel(self, channel: int, tables, index_scale: float = 1.0, arm_mult=None, windows=None):
        """tables: list of padded code tables ([c(end) c c(1)]), one per arm."""
        arms = len(tables)
        L.check(self._lib.gc_set_channel(self._ctx, channel, arms, float(index_scale)))
        for a, t in enumerate(tables):
            t8 = np.ascontiguousarray(np.asarray(t), dtype=np.int8)
            if not np.array_equal(t8, np.asarray(t)):
                raise ValueError("code tables must hold integers in {-1,0,+1}")
            m = 1.0 if arm_mult is None else float(arm_mult[a])
            L.check(self._lib.gc_set_code(self._ctx, channel, a, t8.ctypes.data_as(C.c_void_p), t8.shape[0], m))
            if windows is not None and windows[a]:
                L.check(self._lib.gc_set_code_window(self._ctx, channel, a, int(windows[a])))

    # ---- correlator ----------------------------------------------------------------------
    @staticmethod
    def make_blocks(n: int):
        return (L.gc_block * n)()

    def correlate(self, blocks) -> np.ndarray:
        """blocks: ctypes array of gc_block.  Returns float64 [nblocks, GC_MAX_ARMS, 6]."""
        n = len(blocks)
        out = np.zeros((n, L.GC_MAX_ARMS, 6))
        L.check(self._lib.gc_correlate(self._ctx, n, blocks, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def correlate_bank(self, blocks, offsets) -> np.ndarray:
        """gc_correlate_bank: every block's correlation function at the code offsets `offsets` (chips, positive = late; at most
        GC_BANK_MAX_TAPS of them, any order), the tables read periodically; el_spacing of the blocks is ignored.
        Returns complex128 [nblocks, GC_MAX_ARMS, ntaps] = I + 1j * Q, unused arms zero."""
        n = len(blocks)
        off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        out = np.zeros((n, L.GC_MAX_ARMS, off.shape[0], 2))
        L.check(self._lib.gc_correlate_bank(self._ctx, n, blocks, off.shape[0], off.ctypes.data_as(C.POINTER(C.c_double)),
                                            out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[..., 0] + 1j * out[..., 1]

    def correlate_ddm(self, blocks, offsets, freqs) -> np.ndarray:
        """gc_correlate_ddm: every block's correlation at the code offsets `offsets` (chips, as correlate_bank) and the carrier
        offsets `freqs` (Hz, added to each block's carr_freq; at most GC_DDM_MAX_FREQS of them, any order) - bin m is
        correlate_bank on the blocks with carr_freq + freqs[m], bit for bit.
        Returns complex128 [nblocks, GC_MAX_ARMS, nfreq, ntaps] = I + 1j * Q, unused arms zero."""
        n = len(blocks)
        off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        frq = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        out = np.zeros((n, L.GC_MAX_ARMS, frq.shape[0], off.shape[0], 2))
        L.check(self._lib.gc_correlate_ddm(self._ctx, n, blocks, off.shape[0], off.ctypes.data_as(C.POINTER(C.c_double)),
                                           frq.shape[0], frq.ctypes.data_as(C.POINTER(C.c_double)),
                                           out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[..., 0] + 1j * out[..., 1]

    def correlate_ddm_integrate(self, blocks, offsets, freqs, run_len, weights=None, map_len=None, coherent=True):
        """gc_correlate_ddm_integrate: correlate_ddm's cells added coherently over runs of blocks, then as power over runs, on the
        device - only the maps come back.  run_len: the blocks of every run, in order (one channel per run); weights: one real factor per
        block (+1 / -1 wipes a data bit, 0 drops the block; None: all 1); map_len: the runs of every power map, in order (None: no power
        maps); coherent=False leaves the coherent sums on the device.  Within a run bin m of block b is rotated by
        exp(-2j pi freqs[m] (first_sample[b] - first_sample[first block of the run]) / fs) before it is added (include/gnsscorr.h).
        Returns (complex128 [nruns, GC_MAX_ARMS, nfreq, ntaps] or None, float64 [nmaps, GC_MAX_ARMS, nfreq, ntaps] or None), unused arms zero."""
        n = len(blocks)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        frq = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        runs = np.ascontiguousarray(run_len, dtype=np.int32).reshape(-1)
        maps = None if map_len is None else np.ascontiguousarray(map_len, dtype=np.int32).reshape(-1)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if w.shape[0] != n:
                raise ValueError("correlate_ddm_integrate: one weight per block")
        nmaps = 0 if maps is None else maps.shape[0]
        coh = np.zeros((runs.shape[0], L.GC_MAX_ARMS, frq.shape[0], off.shape[0], 2)) if coherent else None
        pw = np.zeros((nmaps, L.GC_MAX_ARMS, frq.shape[0], off.shape[0])) if maps is not None else None
        L.check(self._lib.gc_correlate_ddm_integrate(self._ctx, n, blocks, None if w is None else w.ctypes.data_as(dp), off.shape[0],
                                                     off.ctypes.data_as(dp), frq.shape[0], frq.ctypes.data_as(dp), runs.shape[0],
                                                     runs.ctypes.data_as(ip), nmaps, None if maps is None else maps.ctypes.data_as(ip),
                                                     None if coh is None else coh.ctypes.data_as(dp),
                                                     None if pw is None else pw.ctypes.data_as(dp)))
        return (None if coh is None else coh[..., 0] + 1j * coh[..., 1]), pw

    def correlate_ddm_search(self, blocks, offsets, freqs, run_len, map_len=None, shifts=None, weights=None, coherent=False, power=True,
                             peaks=True):
        """gc_correlate_ddm_search: correlate_ddm_integrate under many hypotheses from one pass over the samples, every power map's peak
        picked on the device.  Hypothesis h looks at the sum(run_len) blocks from block shifts[h] on (None: 0) with the weights
        weights[h, :] - [nhyp, nblocks], indexed by absolute block number (None: all 1) - and its maps are, bit for bit, those of
        correlate_ddm_integrate(blocks[shifts[h]:shifts[h] + nused], ..., weights=weights[h, shifts[h]:shifts[h] + nused]).  The number
        of hypotheses is len(shifts), else weights.shape[0], else 1.  map_len None: one power map of all the runs.
        Returns (complex128 [nhyp, nruns, GC_MAX_ARMS, nfreq, ntaps] if coherent else None,
                 float64 [nhyp, nmaps, GC_MAX_ARMS, nfreq, ntaps] if power else None,
                 structured [nhyp, nmaps, GC_MAX_ARMS] with fields power, bin, tap if peaks else None):
        a peak is the first maximum of its plane walked bin-major, {0.0, 0, 0} for an arm the channel does not have.  With peaks alone
        neither maps nor coherent sums leave the device."""
        n = len(blocks)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        frq = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        runs = np.ascontiguousarray(run_len, dtype=np.int32).reshape(-1)
        if map_len is None:
            map_len = [runs.shape[0]] if runs.shape[0] else []
        maps = np.ascontiguousarray(map_len, dtype=np.int32).reshape(-1)
        sh = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            if w.ndim != 2 or w.shape[1] != n or (sh is not None and w.shape[0] != sh.shape[0]):
                raise ValueError("correlate_ddm_search: weights are [nhyp, nblocks]")
        nhyp = sh.shape[0] if sh is not None else w.shape[0] if w is not None else 1
        nmaps = maps.shape[0]
        coh = np.zeros((nhyp, runs.shape[0], L.GC_MAX_ARMS, frq.shape[0], off.shape[0], 2)) if coherent else None
        pw = np.zeros((nhyp, nmaps, L.GC_MAX_ARMS, frq.shape[0], off.shape[0])) if power else None
        pk = np.zeros((nhyp, nmaps, L.GC_MAX_ARMS), dtype=L.DDM_PEAK_DTYPE) if peaks else None
        # without a map there is nothing for pow and peaks to hold: the library is asked for neither
        L.check(self._lib.gc_correlate_ddm_search(self._ctx, n, blocks, nhyp, None if sh is None else sh.ctypes.data_as(ip),
                                                  None if w is None else w.ctypes.data_as(dp), off.shape[0], off.ctypes.data_as(dp),
                                                  frq.shape[0], frq.ctypes.data_as(dp), runs.shape[0], runs.ctypes.data_as(ip), nmaps,
                                                  maps.ctypes.data_as(ip), None if coh is None else coh.ctypes.data_as(dp),
                                                  None if pw is None or nmaps == 0 else pw.ctypes.data_as(dp),
                                                  None if pk is None or nmaps == 0 else pk.ctypes.data_as(C.POINTER(L.gc_ddm_peak))))
        return (None if coh is None else coh[..., 0] + 1j * coh[..., 1]), pw, pk

    CANCEL_MODES = {"subtract": L.GC_CANCEL_SUBTRACT, "model": L.GC_CANCEL_MODEL}

    @classmethod
    def _cancel_args(cls, nblocks: int, amp, mode):
        """(gc_cancel_mode, amp_in as float64 [nblocks, GC_MAX_ARMS, 2] or None) of cancel()'s keywords; ValueError for a mode that is
        neither "subtract" nor "model" and for amplitudes of another shape - before any library call."""
        if not isinstance(mode, str) or mode not in cls.CANCEL_MODES:
            raise ValueError(f"mode must be one of {sorted(cls.CANCEL_MODES)}, not {mode!r}")
        if amp is None:
            return cls.CANCEL_MODES[mode], None
        a = np.asarray(amp)
        if a.shape != (nblocks, L.GC_MAX_ARMS):
            raise ValueError(f"amp must be complex [nblocks, GC_MAX_ARMS] = [{nblocks}, {L.GC_MAX_ARMS}], not {a.shape}")
        a = a.astype(np.complex128)
        return cls.CANCEL_MODES[mode], np.ascontiguousarray(np.stack([a.real, a.imag], axis=-1))

    def cancel(self, blocks, dst: "Engine | None" = None, amp=None, mode: str = "subtract") -> np.ndarray:
        """gc_cancel: the component every block describes - its prompt replica in float64 with the amplitude `amp[b, arm]`, or (None)
        the record's own projection on the replica - taken out of this engine's record sample by sample (mode "subtract") or written
        alone ("model"), into `dst`'s record (same sample count, dtype and layout; alloc_if) or (None) in place.  The blocks may come in
        any order and from up to GC_CANCEL_MAX_CHANNELS channels; el_spacing is ignored (include/gnsscorr.h).
        Returns the amplitudes used, complex128 [nblocks, GC_MAX_ARMS], unused arms zero."""
        n = len(blocks)
        code, a_in = self._cancel_args(n, amp, mode)
        out = np.zeros((n, L.GC_MAX_ARMS, 2))
        dp = C.POINTER(C.c_double)
        L.check(self._lib.gc_cancel(self._ctx, (self if dst is None else dst)._ctx, n, blocks, None if a_in is None else a_in.ctypes.data_as(dp),
                                    out.ctypes.data_as(dp), code))
        return out[..., 0] + 1j * out[..., 1]

    @staticmethod
    def _excise_pulse_args(first_sample, nsamples, threshold2, before, after):
        """gc_excise_pulse_params of excise_pulses()'s arguments; ValueError for a value that is not a whole number or does not fit
        its field - before any library call (what the library refuses is the library's to refuse)."""
        vals = []
        for name, v, bits in (("first_sample", first_sample, 64), ("nsamples", nsamples, 64), ("threshold2", threshold2, 64),
                              ("before", before, 32), ("after", after, 32)):
            if isinstance(v, (bool, str, bytes)) or v is None or v != int(v) or not -(1 << (bits - 1)) <= int(v) < 1 << (bits - 1):
                raise ValueError(f"excise_pulses(): {name} must be a whole number of {bits} bits, not {v!r}")
            vals.append(int(v))
        return L.gc_excise_pulse_params(*vals)

    def excise_pulses(self, first_sample: int, nsamples: int, threshold2: int, before: int = 0, after: int = 0, dst: "Engine | None" = None):
        """gc_excise_pulses: of the samples [first_sample, first_sample + nsamples) of this engine's record, those with
        c0^2 + c1^2 > threshold2 (file order, exact integers) and `before` samples in front of and `after` behind each of them
        (0 .. GC_EXCISE_MAX_GUARD, cut at the range's ends) written as zero, into `dst`'s record (same sample count, dtype and layout;
        alloc_if) or (None) in place.  Returns SimpleNamespace(hot, blanked, runs, longest) (include/gnsscorr.h)."""
        p = self._excise_pulse_args(first_sample, nsamples, threshold2, before, after)
        st = L.gc_excise_pulse_stats()
        L.check(self._lib.gc_excise_pulses(self._ctx, (self if dst is None else dst)._ctx, C.byref(p), C.byref(st)))
        return SimpleNamespace(hot=int(st.hot), blanked=int(st.blanked), runs=int(st.runs), longest=int(st.longest))

    @staticmethod
    def _excise_gain(gain) -> np.ndarray:
        """excise_bins()'s gain as contiguous float32 [nfft]; ValueError for anything but one real value per bin of an even transform
        of at least 4 points - before any library call."""
        g = np.asarray(gain)
        if g.ndim != 1 or g.shape[0] < 4 or g.shape[0] % 2 or not (np.issubdtype(g.dtype, np.floating) or np.issubdtype(g.dtype, np.integer)):
            raise ValueError(f"excise_bins(): gain must be one real value per bin of an even transform length >= 4, not {g.dtype} {g.shape}")
        return np.ascontiguousarray(g, dtype=np.float32)

    def excise_bins(self, first_sample: int, nsamples: int, gain, dst: "Engine | None" = None, values: bool = False):
        """gc_excise_bins: the samples [first_sample, first_sample + nsamples) of this engine's record through a gain per frequency bin
        - gain[b] is bin b of probe_psd with nfft = len(gain), bin 0 = DC, file order - by weighted overlap-add on the library's
        float32 transform (sine window, half-overlapping segments, zeros outside the range; all ones is the identity), rounded and
        clamped into `dst`'s record (same sample count, dtype and layout; alloc_if) or (None) in place.  values=True returns the
        complex64 [nsamples] values before rounding, else None (include/gnsscorr.h)."""
        g = self._excise_gain(gain)
        p = L.gc_excise_bins_params(int(first_sample), int(nsamples), g.shape[0], 0)
        out = np.zeros((max(int(nsamples), 0), 2), dtype=np.float32) if values else None
        fp = C.POINTER(C.c_float)
        L.check(self._lib.gc_excise_bins(self._ctx, (self if dst is None else dst)._ctx, C.byref(p), g.ctypes.data_as(fp),
                                         None if out is None else out.ctypes.data_as(fp)))
        return None if out is None else out.view(np.complex64)[:, 0]

    @staticmethod
    def _excise_sweep_args(first_sample, nsamples, limit, widen, gain):
        """(gc_excise_sweep_params, limit, gain or None) of excise_sweep()'s arguments: limit and gain as contiguous float32 [nfft];
        ValueError for a limit that is not one real value per bin of an even transform of at least 4 points, a gain of another
        shape than the limit, or a whole number that does not fit its field - before any library call."""
        lim = np.asarray(limit)
        if lim.ndim != 1 or lim.shape[0] < 4 or lim.shape[0] % 2 or not (np.issubdtype(lim.dtype, np.floating) or np.issubdtype(lim.dtype, np.integer)):
            raise ValueError(f"excise_sweep(): limit must be one real value per bin of an even transform length >= 4, not {lim.dtype} {lim.shape}")
        g = None
        if gain is not None:
            g = np.asarray(gain)
            if g.shape != lim.shape or not (np.issubdtype(g.dtype, np.floating) or np.issubdtype(g.dtype, np.integer)):
                raise ValueError(f"excise_sweep(): gain must be one real value per bin, as the limit ({lim.shape[0]}), not {g.dtype} {g.shape}")
            g = np.ascontiguousarray(g, dtype=np.float32)
        vals = []
        for name, v, bits in (("first_sample", first_sample, 64), ("nsamples", nsamples, 64), ("widen", widen, 32)):
            if isinstance(v, (bool, str, bytes)) or v is None or v != int(v) or not -(1 << (bits - 1)) <= int(v) < 1 << (bits - 1):
                raise ValueError(f"excise_sweep(): {name} must be a whole number of {bits} bits, not {v!r}")
            vals.append(int(v))
        with np.errstate(over="ignore"):                                                 # a float64 limit over float32's range: +inf
            lim = np.ascontiguousarray(lim, dtype=np.float32)
        return L.gc_excise_sweep_params(vals[0], vals[1], lim.shape[0], vals[2]), lim, g

    @staticmethod
    def _unpack_masks(words: np.ndarray, nfft: int) -> np.ndarray:
        """gc_excise_sweep's mask rows uint64 [K, W] as bool [K, nfft]: bin b is bit b & 63 of word b >> 6."""
        bits = np.unpackbits(np.ascontiguousarray(words).astype("<u8", copy=False).view(np.uint8), axis=1, bitorder="little")
        return bits[:, :nfft].astype(bool)

    def excise_sweep(self, first_sample: int, nsamples: int, limit, widen: int = 0, gain=None, dst: "Engine | None" = None, values: bool = False,
                     power: bool = False, masks: bool = False, bin_cut: bool = False):
        """gc_excise_sweep: excise_bins' overlap-add with a decision per segment and bin - cell (k, b) is hot iff its float32 power
        |X_k[b]|^2 > limit[b] (inf protects a bin), cut iff a hot bin of the segment lies within `widen` bins around the circle
        (0 .. GC_EXCISE_MAX_WIDEN); cut cells become 0, the others gain[b] X_k[b] (None: X_k[b]).  nfft = len(limit); bins as probe_psd's.
        Into `dst`'s record or (None) in place.  Returns SimpleNamespace(stats, values, power, hot, cut, bin_cut): stats =
        SimpleNamespace(segments, hot, cut, segments_cut, most_cut); values complex64 [nsamples], power float32 [K, nfft], hot and
        cut bool [K, nfft] (masks=True), bin_cut int64 [nfft] - None where not asked for (include/gnsscorr.h)."""
        p, lim, g = self._excise_sweep_args(first_sample, nsamples, limit, widen, gain)
        nfft, n = p.nfft, max(p.nsamples, 0)
        K, W = -(-n // (nfft // 2)) + 1, (nfft + 63) // 64
        vals = np.zeros((n, 2), dtype=np.float32) if values else None
        pw = np.zeros((K, nfft), dtype=np.float32) if power else None
        hot, cut = (np.zeros((K, W), dtype=np.uint64), np.zeros((K, W), dtype=np.uint64)) if masks else (None, None)
        bc = np.zeros(nfft, dtype=np.int64) if bin_cut else None
        fp, up, ip = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        out = L.gc_excise_sweep_out(None if vals is None else vals.ctypes.data_as(fp), None if pw is None else pw.ctypes.data_as(fp),
                                    None if hot is None else hot.ctypes.data_as(up), None if cut is None else cut.ctypes.data_as(up),
                                    None if bc is None else bc.ctypes.data_as(ip))
        st = L.gc_excise_sweep_stats()
        L.check(self._lib.gc_excise_sweep(self._ctx, (self if dst is None else dst)._ctx, C.byref(p), lim.ctypes.data_as(fp),
                                          None if g is None else g.ctypes.data_as(fp), C.byref(out), C.byref(st)))
        stats = SimpleNamespace(segments=int(st.segments), hot=int(st.hot), cut=int(st.cut), segments_cut=int(st.segments_cut), most_cut=int(st.most_cut))
        return SimpleNamespace(stats=stats, values=None if vals is None else vals.view(np.complex64)[:, 0], power=pw,
                               hot=None if hot is None else self._unpack_masks(hot, nfft), cut=None if cut is None else self._unpack_masks(cut, nfft),
                               bin_cut=bc)

    @staticmethod
    def debug_excise_tile_segments(nfft: int) -> int:
        """gc_debug_excise_tile_segments (test hook, host code only): segments of an nfft-point excise_bins the library transforms at a time."""
        return int(L.load().gc_debug_excise_tile_segments(int(nfft)))

    @staticmethod
    def _ddc_taps(taps, call="downconvert()") -> np.ndarray:
        """The taps of downconvert() or resample() (`call`, for the messages) as contiguous float64 [T, 2] = (re, im); ValueError for
        anything but a [T] real or complex array or a [T][2] real one with 1 <= T <= GC_DDC_MAX_TAPS - before any library call."""
        g = np.asarray(taps)
        numeric = np.issubdtype(g.dtype, np.floating) or np.issubdtype(g.dtype, np.integer)
        if g.ndim == 1 and (numeric or np.issubdtype(g.dtype, np.complexfloating)):
            g = g.astype(np.complex128)
            g = np.stack([g.real, g.imag], axis=-1)
        elif not (g.ndim == 2 and g.shape[1] == 2 and numeric):
            raise ValueError(f"{call}: taps must be [T] complex or [T][2] real, not {g.dtype} {g.shape}")
        if not 1 <= g.shape[0] <= L.GC_DDC_MAX_TAPS:
            raise ValueError(f"{call}: 1 .. {L.GC_DDC_MAX_TAPS} taps, not {g.shape[0]}")
        return np.ascontiguousarray(g, dtype=np.float64)

    @staticmethod
    def _whole(call, name, v, bits):
        """Argument `name` of `call` as an int; ValueError for anything but a whole number of `bits` bits - before any library call."""
        if isinstance(v, (bool, str, bytes)) or v is None or v != int(v) or not -(1 << (bits - 1)) <= int(v) < 1 << (bits - 1):
            raise ValueError(f"{call}: {name} must be a whole number of {bits} bits, not {v!r}")
        return int(v)

    def downconvert(self, dst: "Engine", taps, decim: int, carr_freq: float = 0.0, carr_phase: float = 0.0, first_sample: int = 0,
                    noutputs: int | None = None, dst_first: int = 0):
        """gc_downconvert: this engine's record through the complex FIR `taps` ([T] complex or [T][2] real), every decim-th output -
        output m sits at record sample first_sample + m * decim - rotated by an NCO of carr_freq Hz (phase carr_phase at record sample
        0) and rounded into sample dst_first + m of `dst`'s record (another engine on the same device; any sample count, dtype and
        layout).  noutputs=None: every output that still has a record sample under it, up to dst's capacity.
        Returns SimpleNamespace(phase_step, phase0, clipped, sum_sq, carr_freq, noutputs) (include/gnsscorr.h)."""
        g = self._ddc_taps(taps)
        d = self._whole("downconvert()", "decim", decim, 32)
        first = self._whole("downconvert()", "first_sample", first_sample, 64)
        dfirst = self._whole("downconvert()", "dst_first", dst_first, 64)
        if noutputs is None:
            _, have = self.if_buffer()
            _, room = dst.if_buffer()
            nout = min((int(have) + g.shape[0] - 2 - first) // max(d, 1) + 1, int(room) - dfirst)
        else:
            nout = self._whole("downconvert()", "noutputs", noutputs, 64)
        p = L.gc_ddc_params(first, nout, dfirst, d, g.shape[0], float(carr_freq), float(carr_phase))
        r = L.gc_ddc_result()
        L.check(self._lib.gc_downconvert(self._ctx, dst._ctx, C.byref(p), g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r)))
        return SimpleNamespace(phase_step=int(r.phase_step), phase0=int(r.phase0), clipped=int(r.clipped), sum_sq=int(r.sum_sq),
                               carr_freq=float(r.carr_freq), noutputs=nout)

    @staticmethod
    def debug_ddc_tile_outputs(decim: int, ntaps: int) -> int:
        """gc_debug_ddc_tile_outputs (test hook, host code only): outputs a workgroup of downconvert() takes; 0 for a refused (decim, ntaps)."""
        return int(L.load().gc_debug_ddc_tile_outputs(int(decim), int(ntaps)))

    def resample(self, dst: "Engine", taps, interp: int, decim: int, carr_freq: float = 0.0, carr_phase: float = 0.0, first_tick: int = 0,
                 noutputs: int | None = None, dst_first: int = 0):
        """gc_resample: this engine's record at interp / decim times its rate.  `taps` ([T] complex or [T][2] real) is the prototype
        at the rate fs * interp; output m sits at tick first_tick + m * decim (a tick is 1 / interp input sample), is rotated by an NCO
        of carr_freq Hz (phase carr_phase at tick 0) and rounded into sample dst_first + m of `dst`'s record (another engine on the
        same device; any sample count, dtype and layout).  noutputs=None: every output that still has a record sample under it, up to
        dst's capacity.  With interp == 1 it is downconvert().
        Returns SimpleNamespace(phase_step, phase0, clipped, sum_sq, carr_freq, out_rate, noutputs) (include/gnsscorr.h)."""
        g = self._ddc_taps(taps, "resample()")
        li = self._whole("resample()", "interp", interp, 32)
        d = self._whole("resample()", "decim", decim, 32)
        first = self._whole("resample()", "first_tick", first_tick, 64)
        dfirst = self._whole("resample()", "dst_first", dst_first, 64)
        nout = None if noutputs is None else self._whole("resample()", "noutputs", noutputs, 64)
        if not 1 <= li <= L.GC_RS_MAX_INTERP:
            raise ValueError(f"resample(): interp must lie in 1 .. {L.GC_RS_MAX_INTERP}, not {li}")
        if not 1 <= d <= L.GC_DDC_MAX_DECIM * li:
            raise ValueError(f"resample(): decim must lie in 1 .. {L.GC_DDC_MAX_DECIM} * interp = {L.GC_DDC_MAX_DECIM * li}, not {d}")
        if nout is None:
            _, have = self.if_buffer()
            _, room = dst.if_buffer()
            branches = -(-g.shape[0] // li)
            nout = min(((int(have) + branches - 1) * li - 1 - first) // d + 1, int(room) - dfirst)
        p = L.gc_rs_params(first, nout, dfirst, li, d, g.shape[0], 0, float(carr_freq), float(carr_phase))
        r = L.gc_rs_result()
        L.check(self._lib.gc_resample(self._ctx, dst._ctx, C.byref(p), g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r)))
        return SimpleNamespace(phase_step=int(r.phase_step), phase0=int(r.phase0), clipped=int(r.clipped), sum_sq=int(r.sum_sq),
                               carr_freq=float(r.carr_freq), out_rate=float(r.out_rate), noutputs=nout)

    @staticmethod
    def debug_rs_tile_outputs(interp: int, decim: int, ntaps: int) -> int:
        """gc_debug_rs_tile_outputs (test hook, host code only): outputs a workgroup of resample() takes; 0 for a refused (interp, decim, ntaps)."""
        return int(L.load().gc_debug_rs_tile_outputs(int(interp), int(decim), int(ntaps)))

    @staticmethod
    def _array_records(records):
        """The engines of an array call as a ctypes array of their contexts; ValueError for anything but 1 .. GC_ARRAY_MAX_RECORDS of them."""
        try:
            recs = list(records)
        except TypeError:
            raise ValueError(f"array: records must be a list of engines, not {records!r}") from None
        if not 1 <= len(recs) <= L.GC_ARRAY_MAX_RECORDS or not all(isinstance(r, Engine) for r in recs):
            raise ValueError(f"array: records must be 1 .. {L.GC_ARRAY_MAX_RECORDS} engines, not {len(recs)} entries of {sorted({type(r).__name__ for r in recs})}")
        return recs, (C.c_void_p * len(recs))(*[r._ctx for r in recs])

    @staticmethod
    def _array_weights(weights, nrecords) -> np.ndarray:
        """array_combine()'s weights as contiguous float64 [K, T, 2] = (re, im); ValueError for anything but a [K] or [K, T] real or
        complex array or a [K, T, 2] real one with 1 <= T <= GC_ARRAY_MAX_TAPS - before any library call."""
        w = np.asarray(weights)
        numeric = np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)
        if w.ndim in (1, 2) and (numeric or np.issubdtype(w.dtype, np.complexfloating)):
            w = w.astype(np.complex128).reshape(w.shape[0], -1)
            w = np.stack([w.real, w.imag], axis=-1)
        elif not (w.ndim == 3 and w.shape[2] == 2 and numeric):
            raise ValueError(f"array_combine(): weights must be [K] or [K, T] complex or [K, T, 2] real, not {w.dtype} {w.shape}")
        if w.shape[0] != nrecords or not 1 <= w.shape[1] <= L.GC_ARRAY_MAX_TAPS:
            raise ValueError(f"array_combine(): weights for {nrecords} records and 1 .. {L.GC_ARRAY_MAX_TAPS} taps, not {w.shape[0]} x {w.shape[1]}")
        return np.ascontiguousarray(w, dtype=np.float64)

    @staticmethod
    def array_covariance(records, first_sample: int, nsamples: int, nlags: int = 1) -> np.ndarray:
        """gc_array_covariance: C[l][a][b] = sum over the nsamples samples from first_sample of x_a[n] conj(x_b[n - l]) for the records
        of the K engines `records` (one device, one dtype and layout) and the lags 0 .. nlags-1, in exact integers.
        Returns int64 [L, K, K, 2] = (re, im) (include/gnsscorr.h)."""
        recs, ctxs = Engine._array_records(records)
        first = Engine._whole("array", "first_sample", first_sample, 64)
        n = Engine._whole("array", "nsamples", nsamples, 64)
        lags = Engine._whole("array", "nlags", nlags, 32)
        if not 1 <= lags <= L.GC_ARRAY_MAX_TAPS:
            raise ValueError(f"array_covariance(): nlags must lie in 1 .. {L.GC_ARRAY_MAX_TAPS}, not {lags}")
        p = L.gc_array_cov_params(first, n, len(recs), lags)
        cov = np.zeros((lags, len(recs), len(recs), 2), dtype=np.int64)
        L.check(recs[0]._lib.gc_array_covariance(ctxs, C.byref(p), cov.ctypes.data_as(C.POINTER(C.c_int64))))
        return cov

    @staticmethod
    def array_combine(records, dst: "Engine", weights, first_sample: int = 0, noutputs: int | None = None, dst_first: int = 0):
        """gc_array_combine: output m = sum over the K engines `records` and the taps k of weights[a][k] * x_a[first_sample + m - k], in
        float64, rounded into sample dst_first + m of `dst`'s record (another engine on the same device; any dtype and layout).
        `weights` is [K] or [K, T] complex, or [K, T, 2] real; it is applied as given (conjugate for w^H x).  noutputs=None: what both
        sides hold.  Returns SimpleNamespace(clipped, sum_sq, noutputs) (include/gnsscorr.h)."""
        recs, ctxs = Engine._array_records(records)
        w = Engine._array_weights(weights, len(recs))
        first = Engine._whole("array", "first_sample", first_sample, 64)
        dfirst = Engine._whole("array", "dst_first", dst_first, 64)
        if noutputs is None:
            nout = min(min(int(r.if_buffer()[1]) for r in recs) - first, int(dst.if_buffer()[1]) - dfirst)
        else:
            nout = Engine._whole("array", "noutputs", noutputs, 64)
        p = L.gc_array_combine_params(first, nout, dfirst, len(recs), w.shape[1])
        r = L.gc_array_combine_result()
        L.check(recs[0]._lib.gc_array_combine(ctxs, dst._ctx, C.byref(p), w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r)))
        return SimpleNamespace(clipped=int(r.clipped), sum_sq=int(r.sum_sq), noutputs=nout)

    @staticmethod
    def debug_array_tile_outputs(nrecords: int, ntaps: int) -> int:
        """gc_debug_array_tile_outputs (test hook, host code only): samples a workgroup of either array kernel takes; 0 for a refused (nrecords, ntaps)."""
        return int(L.load().gc_debug_array_tile_outputs(int(nrecords), int(ntaps)))

    def last_kernel(self) -> int:
        """gc_debug_last_kernel: 0 lane, 1 fast (one wave), 2 fast (four waves, int8 pairs), 3 fast (four waves, floats), 4 multi-transition
        (corr_multi.hip), 5 hybrid for channels with a derived six-fold arm (corr_cboc.hip), 6 float64 (corr_f64.hip), -1 mixed
        (exact per-sample kernel); -2 before the first launch."""
        return int(self._lib.gc_debug_last_kernel(self._ctx))

    def last_track_mode(self) -> int:
        """gc_debug_last_track_mode: 0 a launch per epoch, 1 persistent host-fed kernel, 2 device loop."""
        return int(self._lib.gc_debug_last_track_mode(self._ctx))

    def last_track_team(self) -> int:
        """gc_debug_last_track_team: workgroups per block of the last tracking call (team members, or splits of a launch per epoch)."""
        return int(self._lib.gc_debug_last_track_team(self._ctx))

    def debug_wave_transpose_sum(self, values: np.ndarray) -> np.ndarray:
        """gc_debug_wave_transpose_sum: values [k, 64] float32 -> the k wave sums as the lane kernel's flush forms them."""
        v = np.ascontiguousarray(values, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != 64:
            raise ValueError("debug_wave_transpose_sum: [k, 64] values")
        out = np.empty(v.shape[0], dtype=np.float32)
        L.check(self._lib.gc_debug_wave_transpose_sum(self._ctx, v.shape[0], v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def replay_prepare(self, blocks):
        self._replay_n = len(blocks)
        L.check(self._lib.gc_replay_prepare(self._ctx, len(blocks), blocks))

    def replay_launch(self):
        L.check(self._lib.gc_replay_launch(self._ctx))

    def replay_fetch(self) -> np.ndarray:
        out = np.zeros((self._replay_n, L.GC_MAX_ARMS, 6))
        L.check(self._lib.gc_replay_fetch(self._ctx, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def timer_start(self):
        L.check(self._lib.gc_timer_start(self._ctx))

    def timer_stop(self) -> float:
        ms = C.c_double()
        L.check(self._lib.gc_timer_stop(self._ctx, C.byref(ms)))
        return ms.value

    # ---- closed-loop tracking ------------------------------------------------------------
    def track(self, params: L.gc_track_params, inits, device_loop: bool = False, precision: str | None = None):
        """Runs gc_track (or gc_track_device: loop closed on the GPU, one persistent launch).
        precision: "single" | "double" for this call only (gc_set_precision, restored afterwards); None: the context's setting.
        Returns (fields dict name -> [nch, n_epochs], epochs_done, status)."""
        code = precision_code(precision)
        nch = len(inits)
        arr = (L.gc_channel_init * nch)(*inits)
        n_ep = params.n_epochs
        out = np.zeros((nch, L.GC_TRK_NFIELDS, n_ep))
        done = (C.c_int32 * nch)()
        fn = self._lib.gc_track_device if device_loop else self._lib.gc_track
        cno = self._cno_buffer(params, nch)
        try:
            with self._precision_for_call(code):
                st = fn(self._ctx, C.byref(params), nch, arr,
                                        out.ctypes.data_as(C.POINTER(C.c_double)), done)
        finally:
            if cno is not None:
                self._lib.gc_set_cno_output(self._ctx, None, 0)
        if st not in (L.GC_OK, L.GC_E_RANGE):
            L.check(st)
        fields = {name: out[:, i, :] for i, name in enumerate(L.TRK_FIELDS)}
        if cno is not None:
            # [nch, n_epochs // cno_interval], 0 where an interval was not completed; Calc_CNo_PLD modes: [nch, nk, GC_CNO_NPLD]
            fields["CNoVSM" if cno.ndim == 2 else "CNoPLD"] = cno
        return fields, np.array(list(done)), st

    def _cno_buffer(self, params, nch):
        """Registers the C/N0 output of the next tracking call when the parameters ask for it (gc_set_cno_output)."""
        k = int(params.cno_interval)
        if k <= 1 or params.n_epochs // k == 0:
            return None
        cno = np.zeros((nch, params.n_epochs // k) + ((L.GC_CNO_NPLD,) if params.cno_mode != L.GC_CNO_VSM else ()))
        L.check(self._lib.gc_set_cno_output(self._ctx, cno.ctypes.data_as(C.POINTER(C.c_double)), cno.size))
        return cno

    def track_resume(self, params: L.gc_track_params, inits, state=None, origin: int = 0, pause_at_end: bool = False,
                     device_loop: bool = False):
        """gc_track_resume on the window currently loaded (its first sample = record sample `origin`): continues from `state`
        (a ctypes array of gc_channel_state from a previous call; None starts from `inits`).
        device_loop: gc_track_device_resume - the loop closed on the GPU, every channel pausing at an epoch of its own; a state
        written by either loop continues under the other.
        Returns (fields, epochs_done, status, state, paused)."""
        nch = len(inits)
        arr = (L.gc_channel_init * nch)(*inits)
        flags = (1 if state is not None else 0) | (2 if pause_at_end else 0)
        if state is None:
            state = (L.gc_channel_state * nch)()
        out = np.zeros((nch, L.GC_TRK_NFIELDS, params.n_epochs))
        done = (C.c_int32 * nch)()
        paused = C.c_int32(0)
        fn = self._lib.gc_track_device_resume if device_loop else self._lib.gc_track_resume
        st = fn(self._ctx, C.byref(params), nch, arr, state, flags, int(origin),
                out.ctypes.data_as(C.POINTER(C.c_double)), done, C.byref(paused))
        if st not in (L.GC_OK, L.GC_E_RANGE):
            L.check(st)
        return {name: out[:, i, :] for i, name in enumerate(L.TRK_FIELDS)}, np.array(list(done)), st, state, bool(paused.value)

    def track_file(self, path: str, params: L.gc_track_params, inits, window_samples: int, dtype: int = L.GC_I8,
                   layout: int = L.GC_IQ, skip_bytes: int = 0, precision: str | None = None, device_loop: bool = False):
        """gc_track_file: tracking(fid, channel, settings) on a file of any size, at most 2 * window_samples samples resident
        (the next window is read and uploaded while the current one is tracked).  precision as track().
        device_loop: gc_track_file_device - one persistent launch per window closes the loop on the GPU (host-closed windows where
        the device loop does not cover the configuration: last_track_mode() tells).  Returns as track()."""
        code = precision_code(precision)
        nch = len(inits)
        arr = (L.gc_channel_init * nch)(*inits)
        out = np.zeros((nch, L.GC_TRK_NFIELDS, params.n_epochs))
        done = (C.c_int32 * nch)()
        cno = self._cno_buffer(params, nch)
        try:
            with self._precision_for_call(code):
                fn = self._lib.gc_track_file_device if device_loop else self._lib.gc_track_file
                st = fn(self._ctx, os.fsencode(path), int(skip_bytes), int(dtype), int(layout), int(window_samples),
                        C.byref(params), nch, arr, out.ctypes.data_as(C.POINTER(C.c_double)), done)
        finally:
            if cno is not None:
                self._lib.gc_set_cno_output(self._ctx, None, 0)
        if st not in (L.GC_OK, L.GC_E_RANGE):
            L.check(st)
        fields = {name: out[:, i, :] for i, name in enumerate(L.TRK_FIELDS)}
        if cno is not None:
            fields["CNoVSM" if cno.ndim == 2 else "CNoPLD"] = cno
        return fields, np.array(list(done)), st

    @staticmethod
    def track_multi(jobs, device_loop: bool = False, precision: str | None = None):
        """gc_track_multi: jobs = [(engine, gc_track_params, [gc_channel_init, ...]), ...], one engine (context) per job,
        all tracking loops run concurrently.  precision as track(), for every job's context.
        Returns [(fields, epochs_done, status), ...] in job order."""
        code = precision_code(precision)
        lib = L.load()
        n = len(jobs)
        arr = (L.gc_track_job * n)()
        keep = []
        for k, (eng, params, inits) in enumerate(jobs):
            nch = len(inits)
            ia = (L.gc_channel_init * nch)(*inits)
            out = np.zeros((nch, L.GC_TRK_NFIELDS, params.n_epochs))
            done = (C.c_int32 * nch)()
            keep.append((ia, out, done, params, eng._cno_buffer(params, nch), eng))
            arr[k].ctx = eng._ctx
            arr[k].params = C.pointer(params)
            arr[k].init = ia
            arr[k].out = out.ctypes.data_as(C.POINTER(C.c_double))
            arr[k].epochs_done = done
            arr[k].nch = nch
            arr[k].device_loop = int(bool(device_loop))
        try:
            with contextlib.ExitStack() as stack:
                for eng in dict.fromkeys(j[0] for j in jobs):  # each context once, in job order
                    stack.enter_context(eng._precision_for_call(code))
                st = lib.gc_track_multi(n, arr)
        finally:
            for item in keep:
                if item[4] is not None:
                    lib.gc_set_cno_output(item[5]._ctx, None, 0)
        res = []
        for k, (ia, out, done, params, cno, _) in enumerate(keep):
            if arr[k].status not in (L.GC_OK, L.GC_E_RANGE):
                raise L.GnssCorrError(arr[k].status, f"job {k}: " + arr[k].error.decode("utf-8", "replace"))
            fields = {name: out[:, i, :] for i, name in enumerate(L.TRK_FIELDS)}
            if cno is not None:
                fields["CNoVSM" if cno.ndim == 2 else "CNoPLD"] = cno
            res.append((fields, np.array(list(done)), int(arr[k].status)))
        if st not in (L.GC_OK, L.GC_E_RANGE):
            L.check(st)
        return res

    # ---- acquisition ---------------------------------------------------------------------
    def acquire_coarse(self, params: L.gc_acq_params, sampled_codes: np.ndarray, freq_offset=None):
        """sampled_codes: int8 [nprn, spc], or [nprn, narms, spc] for a data+pilot search.  freq_offset: Hz per row added to
        params.intermediate_freq (gc_acquire_coarse_offsets: GLONASS' frequency numbers in one call); raises GnssCorrError with status
        GC_E_UNSUPPORTED when an offset is not a whole number of the search's FFT bins."""
        codes = np.ascontiguousarray(sampled_codes, dtype=np.int8)
        nprn = codes.shape[0]
        narms = codes.shape[1] if codes.ndim == 3 else 1
        res = (L.gc_acq_result * nprn)()
        if freq_offset is None:
            L.check(self._lib.gc_acquire_coarse_multi(self._ctx, C.byref(params), nprn, narms,
                                                      codes.ctypes.data_as(C.c_void_p), res))
        else:
            off = np.ascontiguousarray(freq_offset, dtype=np.float64)
            if off.shape != (nprn,):
                raise ValueError("acquire_coarse: one frequency offset per row")
            L.check(self._lib.gc_acquire_coarse_offsets(self._ctx, C.byref(params), nprn, narms, codes.ctypes.data_as(C.c_void_p),
                                                        off.ctypes.data_as(C.POINTER(C.c_double)), res))
        # bench bookkeeping, after the library has accepted the parameters (it must never change the call's error behaviour)
        n = int(params.block_len) if params.block_len else 2 * codes.shape[-1]
        bins = int(params.n_bins) if params.n_bins else int(math.floor(params.search_band * 2 / params.search_step + 0.5)) + 1
        self._count_transforms(n, forward=bins * int(params.non_coh_time), code=nprn * narms, inverse=nprn * narms * bins * int(params.non_coh_time))
        return list(res)

    def acquire_fine_sums(self, params: L.gc_fine_params, code: np.ndarray) -> np.ndarray:
        """Per-code-period complex sums [nbins, ncodes] of the generic fine-frequency stage."""
        c8 = np.ascontiguousarray(code, dtype=np.int8)
        out = np.empty((params.nbins, params.ncodes, 2))
        L.check(self._lib.gc_acquire_fine_sums(self._ctx, C.byref(params), c8.ctypes.data_as(C.c_void_p),
                                               out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[..., 0] + 1j * out[..., 1]

    def acq_condition(self, sampling_freq: float, intermediate_freq: float, bandwidth: float, first_sample: int, n_samples: int,
                      fir_order: int = 700, band_margin: float = 0.0):
        """gc_acq_condition: the zero-phase band-pass + decimation front end of acquisition.m:46-111 on the record's samples
        [first_sample, first_sample + n_samples).  Returns (new sampling frequency, new IF, conditioned length); searches read
        the conditioned signal with gc_acq_params.source = 1."""
        fp = L.gc_acq_front_params(sampling_freq=sampling_freq, intermediate_freq=intermediate_freq, bandwidth=bandwidth,
                                   first_sample=int(first_sample), n_samples=int(n_samples), fir_order=int(fir_order),
                                   band_margin=float(band_margin))
        res = L.gc_acq_front_result()
        L.check(self._lib.gc_acq_condition(self._ctx, C.byref(fp), C.byref(res)))
        return res.sampling_freq, res.intermediate_freq, int(res.n_samples)

    def acq_conditioned(self, first: int, n: int) -> np.ndarray:
        """The conditioned signal back as complex64 (test hook)."""
        out = np.empty(2 * int(n), dtype=np.float32)
        L.check(self._lib.gc_acq_conditioned(self._ctx, int(first), int(n), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out[0::2] + 1j * out[1::2]

    def acquire_fine_sums_batch(self, params: L.gc_fine_params, codes: np.ndarray, first_sample, f0) -> np.ndarray:
        """The same for several detections in one launch: codes [ndet, code_len], first_sample [ndet], f0 [ndet]
        -> complex [ndet, nbins, ncodes]."""
        c8 = np.ascontiguousarray(codes, dtype=np.int8)
        ndet = c8.shape[0]
        fs = np.ascontiguousarray(first_sample, dtype=np.int64)
        ff = np.ascontiguousarray(f0, dtype=np.float64)
        if c8.ndim != 2 or c8.shape[1] != params.code_len or fs.shape != (ndet,) or ff.shape != (ndet,):
            raise ValueError("acquire_fine_sums_batch: codes [ndet, code_len], first_sample [ndet], f0 [ndet]")
        out = np.empty((ndet, params.nbins, params.ncodes, 2))
        L.check(self._lib.gc_acquire_fine_sums_batch(self._ctx, C.byref(params), ndet, c8.ctypes.data_as(C.c_void_p),
                                                     fs.ctypes.data_as(C.POINTER(C.c_int64)), ff.ctypes.data_as(C.POINTER(C.c_double)),
                                                     out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[..., 0] + 1j * out[..., 1]

    def acq_signal_stats(self, first_sample: int, n: int, source: int = 0):
        """gc_acq_signal_stats: (mean(x), var(x)) of n samples of the record (or of the conditioned signal) as MATLAB's mean / var."""
        mr, mi, v = C.c_double(), C.c_double(), C.c_double()
        L.check(self._lib.gc_acq_signal_stats(self._ctx, int(first_sample), int(n), int(source), C.byref(mr), C.byref(mi), C.byref(v)))
        return complex(mr.value, mi.value), v.value

    def _count_transforms(self, n: int, forward: int = 0, code: int = 0, inverse: int = 0):
        """Bookkeeping for bench.py (acq_stats): the transforms the SEARCH needs once the signal spectra are hoisted out of the PRN
        loop (acquisition.m:167-192 recomputes them per PRN) - n-point forward transforms of the signal, of the sampled codes,
        and inverse transforms, since the last reset.  Counts only; nothing on the device depends on it."""
        st = self.acq_stats
        st["n_fft"] = max(st.get("n_fft", 0), int(n))
        for k, v in (("forward", forward), ("code", code), ("inverse", inverse)):
            st[k] = st.get(k, 0) + int(v)

    def acq_shift_prepare(self, params: L.gc_acq_shift_params):
        self._count_transforms(int(params.n), forward=int(params.n_signals) * int(params.n_carriers))
        self._shift = params
        L.check(self._lib.gc_acq_shift_prepare(self._ctx, C.byref(params)))

    def acq_shift_search(self, codes: np.ndarray, arm_weight=None):
        """codes: int8 [narms, n].  Returns (row_max float32[rows], row_argmax int32[rows])."""
        p = self._shift
        c8 = np.ascontiguousarray(codes, dtype=np.int8).reshape(-1, p.n)
        rows = p.n_carriers * p.n_signals * p.n_bins
        self._count_transforms(int(p.n), code=c8.shape[0], inverse=c8.shape[0] * rows)
        rmax = np.empty(rows, dtype=np.float32)
        rarg = np.empty(rows, dtype=np.int32)
        w = None
        if arm_weight is not None:
            w = (C.c_double * c8.shape[0])(*[float(v) for v in arm_weight])
        L.check(self._lib.gc_acq_shift_search(self._ctx, c8.shape[0], c8.ctypes.data_as(C.c_void_p), w,
                                              rmax.ctypes.data_as(C.POINTER(C.c_float)), rarg.ctypes.data_as(C.POINTER(C.c_int32))))
        return rmax, rarg

    def acq_shift_search_batch(self, codes: np.ndarray, arm_weight, rule: int, exclude: int = 0, period: int = 1, sample_index=None):
        """gc_acq_shift_search_batch: codes int8 [nprn, narms, n] (sampled replicas) or, with sample_index (0-based, one vector for all
        codes), [nprn, narms, chips] -> ctypes array of gc_acq_shift_pick [nprn], or None when the library answers GC_E_NOMEM (the batch's buffers
        do not fit; GC_E_UNSUPPORTED is kept for older libraries): the caller searches PRN by PRN."""
        p = self._shift
        c8 = np.ascontiguousarray(codes, dtype=np.int8)
        nprn, narms = c8.shape[0], c8.shape[1]
        rows = p.n_carriers * p.n_signals * p.n_bins
        picks = (L.gc_acq_shift_pick * nprn)()
        w = None
        if arm_weight is not None:
            w = (C.c_double * narms)(*[float(v) for v in arm_weight])
        idx, nidx = None, 0
        if sample_index is not None:
            i32 = np.ascontiguousarray(sample_index, dtype=np.int32)
            idx, nidx = i32.ctypes.data_as(C.c_void_p), int(i32.shape[0])
        rc = self._lib.gc_acq_shift_search_batch(self._ctx, nprn, narms, c8.ctypes.data_as(C.c_void_p), int(c8.shape[2]), idx, nidx, w, int(rule),
                                                 int(exclude), int(period), picks)
        if rc in (L.GC_E_UNSUPPORTED, L.GC_E_NOMEM):
            # GC_E_NOMEM: the batch holds every PRN's code spectra (nprn x narms x N x 8 bytes) and winning rows at once; the PRN-by-PRN
            # path needs one PRN's and still fits on a device that is short of memory (next to gc_track_multi contexts)
            return None
        L.check(rc)
        self._count_transforms(int(p.n), code=nprn * narms,
                               inverse=nprn * narms * rows + (narms * sum(1 for k in picks if k.row >= 0) if rule != L.GC_SHIFT_PICK_GLOBAL else 0))
        return picks

    def acq_shift_row(self, row: int) -> np.ndarray:
        out = np.empty(self._shift.n, dtype=np.float32)
        L.check(self._lib.gc_acq_shift_row(self._ctx, int(row), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def sync_xcorr(self, i_p: np.ndarray, pattern: np.ndarray, zero_is_plus: bool = False) -> np.ndarray:
        """gc_sync_xcorr: the non-negative lags of xcorr(hard-limited I_P, pattern) (NAVdecoding.m of every package)."""
        x = np.ascontiguousarray(i_p, dtype=np.float64)
        pat = np.ascontiguousarray(pattern, dtype=np.int8)
        out = np.empty(x.shape[0], dtype=np.float32)
        L.check(self._lib.gc_sync_xcorr(self._ctx, x.ctypes.data_as(C.POINTER(C.c_double)), x.shape[0], pat.ctypes.data_as(C.c_void_p),
                                        pat.shape[0], L.GC_SYNC_ZERO_IS_PLUS if zero_is_plus else 0, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def preamble_xcorr(self, i_p: np.ndarray, pattern: np.ndarray) -> np.ndarray:
        return self.sync_xcorr(i_p, pattern)

    # ---- the record before acquisition (probeData.m) ----------------------------------------------
    PROBE_WINDOWS = {"rect": L.GC_WIN_RECT, "hamming": L.GC_WIN_HAMMING}

    def probe_psd(self, first_sample: int, nsamples: int, nfft: int = 32768, noverlap: int = 2048, window="hamming", nspans: int = 1):
        """gc_probe_psd: pwelch(x, hamming(nfft) | ones, noverlap, nfft, fs, 'twosided') without detrending of `nspans` consecutive spans
        of `nsamples` samples of the record, samples in file order (include/gnsscorr.h) -> (float64 [nspans, nfft], bin 0 = DC; K segments per span)."""
        if isinstance(window, str):
            if window not in self.PROBE_WINDOWS:
                raise ValueError(f"window must be one of {sorted(self.PROBE_WINDOWS)}, not {window!r}")
            window = self.PROBE_WINDOWS[window]
        p = L.gc_probe_psd_params(int(first_sample), int(nsamples), int(nfft), int(noverlap), int(window), int(nspans))
        out = np.empty((max(int(nspans), 0), max(int(nfft), 0)), dtype=np.float64)
        k = C.c_int64(0)
        L.check(self._lib.gc_probe_psd(self._ctx, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(k)))
        return out, int(k.value)

    def probe_histogram(self, first_sample: int, nsamples: int):
        """gc_probe_histogram: hist(component, -128:128) of both components in file order (row 1 all zero for a real record) ->
        (uint64 [2, 257], max(c0^2 + c1^2) as an exact integer)."""
        counts = np.zeros((2, L.GC_PROBE_HIST_BINS), dtype=np.uint64)
        m = C.c_int64(0)
        L.check(self._lib.gc_probe_histogram(self._ctx, int(first_sample), int(nsamples), counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(m)))
        return counts, int(m.value)

    @staticmethod
    def debug_probe_tile_segments(nfft: int) -> int:
        """gc_debug_probe_tile_segments (test hook, host code only): segments of an nfft-point probe_psd the library transforms at a time."""
        return int(L.load().gc_debug_probe_tile_segments(int(nfft)))

    def debug_fft(self, x: np.ndarray, inverse: bool = False) -> np.ndarray:
        """x: complex64 [nbatch, n].  The library's FFT (test hook)."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        out = np.empty_like(x)
        L.check(self._lib.gc_debug_fft(self._ctx, x.shape[1], x.shape[0], x.ctypes.data_as(C.c_void_p),
                                       out.ctypes.data_as(C.c_void_p), int(inverse)))
        return out

    def debug_acq_surface(self, params: L.gc_acq_params, codes: np.ndarray):
        """gc_debug_acq_surface (test hook): codes int8 [spc] or [narms, spc] of ONE PRN -> the search's float32 surface
        [nbins, n] as the guard's slow path writes it.  n is the transform length: the block's, or a longer one where the
        search runs inside a padded transform (only the block's lags count then)."""
        c8 = np.ascontiguousarray(codes, dtype=np.int8)
        if c8.ndim == 1:
            c8 = c8[None, :]
        nbins, n = C.c_int32(0), C.c_int32(0)
        out = np.empty(1, dtype=np.float32)
        for _ in range(2):   # the first call only tells the sizes (GC_E_RANGE before anything is searched)
            rc = self._lib.gc_debug_acq_surface(self._ctx, C.byref(params), c8.shape[0], c8.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.POINTER(C.c_float)), out.shape[0], C.byref(nbins), C.byref(n))
            if rc != L.GC_E_RANGE or nbins.value * n.value <= out.shape[0]:
                break
            out = np.empty(nbins.value * n.value, dtype=np.float32)
        L.check(rc)
        return out[:nbins.value * n.value].reshape(nbins.value, n.value)

    @staticmethod
    def debug_fft_plan(n: int):
        """gc_debug_fft_plan (test hook, host code only): {"n1", "n2", "rad1", "rad2", "cols1", "cols2"} of an n-point transform -
        the columns pass (vectors of n1, element stride n2) and the rows pass (vectors of n2), their radices in stage order and
        tile widths.  Raises GnssCorrError (GC_E_UNSUPPORTED) where the planner refuses the length."""
        n1, n2, k1, k2, c1, c2 = (C.c_int(0) for _ in range(6))
        r1, r2 = (C.c_int * 12)(), (C.c_int * 12)()
        L.check(L.load().gc_debug_fft_plan(int(n), C.byref(n1), C.byref(n2), r1, C.byref(k1), r2, C.byref(k2), C.byref(c1), C.byref(c2)))
        return {"n1": n1.value, "n2": n2.value, "rad1": list(r1[:k1.value]), "rad2": list(r2[:k2.value]), "cols1": c1.value, "cols2": c2.value}

    def acquire_fine_l1ca(self, params: L.gc_acq_params, code: np.ndarray, code_phase: int,
                          coarse_freq: float) -> float:
        c8 = np.ascontiguousarray(code, dtype=np.int8)
        f = C.c_double()
        L.check(self._lib.gc_acquire_fine_l1ca(self._ctx, C.byref(params), c8.ctypes.data_as(C.c_void_p),
                                               int(code_phase), float(coarse_freq), C.byref(f)))
        return f.value

    def acquire_fine_l1ca_batch(self, params: L.gc_acq_params, codes: np.ndarray, code_phase, coarse_freq) -> np.ndarray:
        """Fine stage of all detected PRNs in one launch: codes [ndet, code_length] -> carrFreq [ndet]."""
        c8 = np.ascontiguousarray(codes, dtype=np.int8)
        ndet = c8.shape[0]
        cp = np.ascontiguousarray(code_phase, dtype=np.int32)
        cf = np.ascontiguousarray(coarse_freq, dtype=np.float64)
        if c8.ndim != 2 or c8.shape[1] != int(params.code_length) or cp.shape != (ndet,) or cf.shape != (ndet,):
            raise ValueError("acquire_fine_l1ca_batch: codes [ndet, code_length], code_phase [ndet], coarse_freq [ndet]")
        out = np.empty(ndet)
        L.check(self._lib.gc_acquire_fine_l1ca_batch(self._ctx, C.byref(params), ndet, c8.ctypes.data_as(C.c_void_p),
                                                     cp.ctypes.data_as(C.POINTER(C.c_int32)), cf.ctypes.data_as(C.POINTER(C.c_double)),
                                                     out.ctypes.data_as(C.POINTER(C.c_double))))
        return out
