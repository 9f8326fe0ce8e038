"""The closed loops' planners (csrc/track_plan.h: gc_plan_track_host, gc_plan_track_device, the knobs, the team vocabulary) without a
GPU: tests/track_plan_shim.hip runs them on the CPU over channel FACTS (arms, table lengths, ramp multipliers, windows), a record
format, the loop's parameters and the channels' code frequencies, and returns the mode, the kernel and the teams gc_track /
gc_track_device would launch with.

Cases: what the GPU tests observe on the device, restated as such facts at 256 compute units - the teams of
tests/test_gpu_loop_epochs.py (gc_debug_last_track_team before any halving), the mode and kernel of every rig whose
last_track_mode / last_kernel a GPU test asserts, every refusal with its status and text, each knob's clamp (on the shim built with
-DGC_TUNING=1, as the knob tests run on libgnsscorr_tuning.so).  And a seeded sweep of the teams against tests/track_teams.py."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import test_launch_plan_cpu as LP
from track_teams import _fast_device_team, _fast_host_team, _halvings, _lane_device_team, _lowrate

HERE = os.path.dirname(os.path.abspath(__file__))
CUS = 256
PER_EPOCH, PERSIST_FAST, PERSIST_LANE, F64 = 0, 1, 2, 3      # TrackHostMode
GC_OK, GC_E_INVALID, GC_E_UNSUPPORTED = 0, -1, -6
MSG, DESC_WORDS, NFIELDS = 16, 10, 21                        # bytes per message, messages per descriptor, GC_TRK_NFIELDS


class Call(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("sampling_freq", "code_freq_basis", "code_length", "el_spacing")] + \
               [(n, C.c_int) for n in ("pilot_combine", "table_phase_count", "n_epochs", "nch")] + \
               [("channel", C.POINTER(C.c_int)), ("code_freq", C.POINTER(C.c_double))]


class Out(C.Structure):
    _fields_ = [("status", C.c_int), ("message", C.c_char * 160)] + \
               [(n, C.c_int) for n in ("fast_nominal", "splits", "mode", "team", "share_lane_nominal", "share_el", "derived", "poll", "async_", "nthreads",
                                       "kernel", "lowrate", "share", "share_lane", "cboc", "lane_waves", "msgs_per_member", "xcd_local")] + \
               [("grid", C.c_uint)] + [(n, C.c_longlong) for n in ("part_bytes", "desc_bytes", "rec_bytes")]

    @property
    def text(self):
        return self.message.decode()


_LIBS = {}


def _shim(tuning=False):
    if tuning in _LIBS:
        return _LIBS[tuning]
    from cu_sdr_collection_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(HERE, "track_plan_shim.hip")
    out = os.path.join(HERE, "build", "libtrack_plan_shim_tuning.so" if tuning else "libtrack_plan_shim.so")
    deps = [src, os.path.join(HERE, "launch_plan_shim.hip")] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = [f for f in B._tu_flags("track.hip") if f != "--offload-compress"] + (["-DGC_TUNING=1"] if tuning else [])
        subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.plan_shim_create.restype = C.c_void_p
    lib.plan_shim_create.argtypes = [C.c_int] * 5 + [C.c_ulonglong]
    lib.plan_shim_destroy.argtypes = [C.c_void_p]
    lib.plan_shim_set_channel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]
    lib.tplan_shim_concurrent.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.tplan_shim_host.argtypes = [C.c_void_p, C.POINTER(Call), C.c_int, C.POINTER(Out)]
    lib.tplan_shim_device.argtypes = [C.c_void_p, C.POINTER(Call), C.c_int, C.POINTER(Out)]
    lib.tplan_shim_nch_dev.argtypes = [C.c_void_p, C.c_int]
    _LIBS[tuning] = lib
    return lib


class Ctx(LP.Ctx):
    """launch_plan's context of channel facts on the track-plan shim; host() / device() = gc_track / gc_track_device up to the launch."""

    def __init__(self, fmt="i8_iq", cus=CUS, generic=False, double=False, tuning=False):
        self.lib = _shim(tuning)
        dtype, layout = LP.FORMATS[fmt]
        self.p = self.lib.plan_shim_create(cus, dtype, layout, int(generic), int(double), 1 << 40)
        self.chans = {}

    def _call(self, nch, fs, rate, chips, d, channels=None, code_freq=None, pilot=0, phases=0, n_epochs=40):
        channels = list(range(nch)) if channels is None else list(channels)
        code_freq = [rate] * nch if code_freq is None else list(code_freq)
        self._keep = ((C.c_int * nch)(*channels), (C.c_double * nch)(*code_freq))
        return Call(fs, rate, chips, d, pilot, phases, n_epochs, nch, *self._keep)

    def host(self, nch, fs, rate, chips, d, pause=False, **kw):
        o = Out()
        self.lib.tplan_shim_host(self.p, C.byref(self._call(nch, fs, rate, chips, d, **kw)), int(pause), C.byref(o))
        return o

    def device(self, nch, fs, rate, chips, d, cap=0, **kw):
        o = Out()
        self.lib.tplan_shim_device(self.p, C.byref(self._call(nch, fs, rate, chips, d, **kw)), cap, C.byref(o))
        return o

    def concurrent(self, jobs, channels):
        self.lib.tplan_shim_concurrent(self.p, int(jobs), channels)


def _l1ca(nch, **kw):
    ctx = Ctx(**kw)
    for i in range(nch):
        ctx.channel(i, nent=[1025])
    return ctx


def _l5(nch, arms=2, L=10230, **kw):
    ctx = Ctx(**kw)
    for i in range(nch):
        ctx.channel(i, nent=[L + 2] * arms)
    return ctx


L1 = dict(fs=18e6, rate=1.023e6, chips=1023.0, d=0.5)
L5 = dict(fs=18e6, rate=10.23e6, chips=10230.0, d=0.5, pilot=1)


def _settings(fs, rate, chips):
    return SimpleNamespace(samplingFreq=fs, codeFreqBasis=rate, codeLength=chips)


# ---- teams: tests/test_gpu_loop_epochs.py, section b --------------------------------------------------------------------------------
def test_fast_device_loop_teams_by_channel_count():
    S = _settings(18e6, 1.023e6, 1023.0)
    by_team = {}
    for nch in range(1, 257):
        by_team[_fast_device_team(CUS, nch, S)] = nch
    v = sorted(by_team)
    teams = sorted({v[round(i * (len(v) - 1) / 5)] for i in range(6)})                 # the GPU module's _spread(by_team, 6)
    assert teams == [4, 10, 15, 21, 26, 32]
    for team in teams:
        nch = by_team[team]
        o = _l1ca(nch).device(nch, **L1)
        assert (o.status, o.kernel, o.team, o.lowrate, o.msgs_per_member) == (0, 1, team, 2, 2), (nch, o.team)
        assert o.xcd_local == 1 and o.grid == (nch + 7) // 8 * 8 * team
        assert o.part_bytes == MSG * nch * team * 4 and o.desc_bytes == MSG * nch * DESC_WORDS and o.rec_bytes == 8 * nch * NFIELDS * 40


@pytest.mark.parametrize("spc", [16, 8])
def test_fast_loops_teams_limited_by_the_block_length(spc):
    for i, chips in enumerate((50, 80, 100, 200, 400)):
        rate, fs = chips * 1e3, float(round(spc * chips * 1e3))
        ctx = Ctx()
        for c in range(4):
            ctx.channel(c, nent=[chips + 2])
        dev, host = ctx.device(4, fs, rate, float(chips), 0.5), ctx.host(4, fs, rate, float(chips), 0.5)
        assert (dev.status, dev.kernel, dev.team, dev.lowrate) == (0, 1, (1, 2, 3, 6, 12)[i], 2 if spc == 16 else 1), (chips, spc, dev.team, dev.lowrate)
        assert (host.status, host.mode, host.team, host.fast_nominal) == (0, PERSIST_FAST, (1, 1, 2, 4, 8)[i], 2 if spc == 16 else 1), (chips, spc, host.team)
        S = _settings(fs, rate, chips)
        assert (dev.team, host.team) == (_fast_device_team(CUS, 4, S), _fast_host_team(CUS, 4, S))


def test_lane_device_loop_teams():
    for nch, team in ((256, 2), (128, 4), (102, 5), (85, 6)):                           # two arms, blksize 18 000: 2 CU / nch, the cap of 6
        o = _l5(nch).device(nch, **L5)
        assert (o.status, o.kernel, o.team, o.lane_waves, o.msgs_per_member) == (0, 0, team, 8, 12), (nch, o.team)
        assert o.team == _lane_device_team(CUS, nch, 2, 18000) and o.part_bytes == MSG * nch * team * 12
    for fs, team in ((2.5e6, 2), (4.5e6, 4), (5.5e6, 5), (18e6, 6)):                    # four channels on blocks of 2 500 .. 18 000 samples
        o = _l5(4).device(4, **dict(L5, fs=fs))
        assert (o.status, o.kernel, o.team) == (0, 0, team) and team == _lane_device_team(CUS, 4, 2, int(fs * 1e-3)), (fs, o.team)
    assert _l5(4, arms=1).device(4, **dict(L5, pilot=0)).team == 8                      # the one-arm cap
    lib = _shim()
    assert [lib.tplan_shim_lane_member_cap(a) for a in (1, 2, 3)] == [8, 6, 4]
    cb = _cboc(4).device(4, **E1C)                                                     # three arms, the third derived: the cap of 4
    assert (cb.status, cb.kernel, cb.cboc, cb.team, cb.msgs_per_member) == (0, 0, 1, 4, 18)


def test_halving_chains():
    lib = _shim()
    for start in (32, 6, 5, 1):
        chain = [start]
        while chain[-1] > 1:
            chain.append(lib.tplan_shim_team_halved(chain[-1]))
        assert chain == _halvings(start)
    assert _halvings(32) == [32, 16, 8, 4, 2, 1] and _halvings(6) == [6, 3, 2, 1]
    ctx = _l1ca(33)                                                                    # the retry's plan: the team capped, the buffers and the grid with it
    whole = ctx.device(33, **L1)
    assert whole.team == 32
    for cap in _halvings(32)[1:]:
        o = ctx.device(33, cap=cap, **L1)
        assert (o.team, o.grid, o.part_bytes, o.kernel, o.lowrate) == (cap, 40 * cap, MSG * 33 * cap * 4, 1, 2)
    assert ctx.device(33, cap=40, **L1).team == 32                                      # a cap above the formula's team changes nothing


# ---- modes and kernels: every rig whose last_track_mode / last_kernel a GPU test asserts --------------------------------------------
def _cboc(nch, **kw):
    ctx = Ctx(**kw)
    for i in range(nch):
        ctx.channel(i, six_fold=True, **LP._boc(4092))
    return ctx


E1C = dict(fs=18e6, rate=1.023e6, chips=4092.0, d=0.05, pilot=5)


def test_modes_and_kernels_of_the_gpu_rigs():
    h, d = _l1ca(4).host(4, **L1), _l1ca(4).device(4, **L1)                             # GPS L1 C/A: the fast kernel, host-fed and device loop
    assert (h.status, h.mode, h.fast_nominal, h.share_el, h.async_, h.nthreads, h.poll) == (0, PERSIST_FAST, 2, 1, 1, 1, 1)
    assert (d.status, d.kernel, d.share, d.lowrate) == (0, 1, 1, 2)
    assert _l1ca(4).host(4, pause=True, **L1).async_ == 0                               # a window of a streamed record: lock step
    h, d = _l5(4).host(4, **L5), _l5(4).device(4, **L5)                                 # GPS L5: the lane kernel, two arms
    assert (h.status, h.mode, h.team, h.share_lane_nominal, h.share_el, h.derived) == (0, PERSIST_LANE, 6, 1, 0, 0)
    assert (d.status, d.kernel, d.share_lane, d.cboc) == (0, 0, 1, 0)
    h, d = _cboc(2).host(2, **E1C), _cboc(2).device(2, **E1C)                           # Galileo E1-C CBOC: the derived arm on the lane kernel
    assert (h.status, h.mode, h.derived, h.fast_nominal, h.team, h.share_lane_nominal) == (0, PERSIST_LANE, 1, 0, 4, 0)
    assert (d.status, d.kernel, d.cboc, d.team) == (0, 0, 1, 4)
    ctx = Ctx()                                                                         # GPS L2C: CM + windowed CL, must not take the fast kernel
    ctx.channel(0, nent=[10232, 767252], window=[0, 10240])
    l2c = dict(fs=18e6, rate=0.5115e6, chips=10230.0, d=0.5, pilot=0, phases=75)
    h, d = ctx.host(1, **l2c), ctx.device(1, **l2c)
    assert (h.status, h.mode) == (0, PERSIST_LANE) and (d.status, d.kernel) == (0, 0)
    one = Ctx()                                                                         # ... nor does a one-arm channel, for its window alone
    one.channel(0, nent=[20000], window=[1040])
    one.channel(1, nent=[1025])
    assert (one.device(1, **L1).kernel, one.host(1, **L1).mode) == (0, PERSIST_LANE)
    assert (one.device(1, channels=[1], **L1).kernel, one.host(1, channels=[1], **L1).mode) == (1, PERSIST_FAST)
    h, d = _l1ca(4, double=True).host(4, **L1), _l1ca(4, double=True).device(4, **L1)   # GC_PREC_F64
    assert (h.status, h.mode, h.async_) == (0, F64, 0) and (d.status, d.kernel) == (0, 6)
    h, d = _l1ca(4, generic=True).host(4, **L1), _l1ca(4, generic=True).device(4, **L1) # gc_force_generic_kernel: the lane kernels
    assert (h.mode, h.fast_nominal, h.team) == (PERSIST_LANE, 0, 8) and (d.kernel, d.team) == (0, 8)
    for fmt in ("i16_iq", "i16_qi", "i8_real", "i16_real"):                             # 16-sample chunks are an int8 I/Q format
        h, d = _l1ca(4, fmt=fmt).host(4, **L1), _l1ca(4, fmt=fmt).device(4, **L1)
        assert (h.mode, d.kernel, d.lowrate) == (PERSIST_FAST, 1, 1)
        S = _settings(18e6, 1.023e6, 1023.0)
        assert (d.team, h.team) == (_fast_device_team(CUS, 4, S, False), _fast_host_team(CUS, 4, S)) == (32, 23)
    mixed = Ctx()                                                                       # plain mixed multipliers: a launch per epoch, the exact kernel
    mixed.channel(0, **LP._boc(1023))
    assert (mixed.host(1, **dict(E1C, chips=1023.0)).mode, mixed.host(1, **dict(E1C, chips=1023.0)).status) == (PER_EPOCH, 0)


def test_refusals_with_status_and_text():
    h = _l5(2).host(2, **dict(L5, pilot=4))
    assert (h.status, h.text) == (GC_E_INVALID, "gc_track: pilot_combine 4 / 5 need three arms {data, pilot BOC(1,1), pilot BOC(6,1)}")
    h = _l1ca(2).host(2, **dict(L1, pilot=1))
    assert (h.status, h.text) == (GC_E_INVALID, "gc_track: pilot_combine requires a pilot arm")
    uncovered = "gc_track_device: configuration not covered by the persistent kernels (use gc_track)"
    three = Ctx()                                                                       # three plain arms: max_arms > 2 without CBOC
    three.channel(0, nent=[1025] * 3)
    d = three.device(1, **dict(L1, pilot=0))
    assert (d.status, d.text) == (GC_E_UNSUPPORTED, uncovered)
    d = _cboc(2).device(2, **dict(E1C, pilot=2))                                        # ... derived, but not folded
    assert (d.status, d.text) == (GC_E_UNSUPPORTED, uncovered)
    d = _l1ca(2).device(2, **dict(L1, pilot=1))                                         # a pilot mode without a pilot arm
    assert (d.status, d.text) == (GC_E_UNSUPPORTED, uncovered)
    for fmt in ("i16_iq", "i8_real"):                                                   # CBOC on a record that is not int8 I/Q or Q/I
        d = _cboc(2, fmt=fmt).device(2, **E1C)
        assert (d.status, d.text) == (GC_E_UNSUPPORTED, uncovered), fmt
    mixed = Ctx()                                                                       # a multiplier other than a derived third arm
    mixed.channel(0, **LP._boc(1023))
    d = mixed.device(1, **dict(E1C, chips=1023.0))
    assert (d.status, d.text) == (GC_E_UNSUPPORTED, "gc_track_device: ramp multipliers other than a derived third arm are not covered (use gc_track)")
    d = _l1ca(2, double=True).device(2, **dict(L1, pilot=1))                            # float64: what gc_track refuses
    assert (d.status, d.text) == (GC_E_INVALID, "gc_track_device: pilot_combine 1 does not match the channels' arms")
    d = _l5(2, double=True).device(2, **dict(L5, pilot=5))
    assert (d.status, d.text) == (GC_E_INVALID, "gc_track_device: pilot_combine 5 does not match the channels' arms")
    mixed64 = Ctx(double=True)                                                          # ... and float64 takes any multiplier
    mixed64.channel(0, **LP._boc(1023))
    assert (mixed64.device(1, **dict(E1C, chips=1023.0)).status, mixed64.device(1, **dict(E1C, chips=1023.0)).kernel) == (0, 6)


def test_concurrent_jobs_size_the_teams_for_all_channels():
    ctx = _l1ca(12)
    lib = ctx.lib
    assert lib.tplan_shim_nch_dev(ctx.p, 12) == 12
    alone = ctx.device(12, **L1)
    assert (alone.team, alone.xcd_local, alone.grid) == (32, 1, 16 * 32)
    ctx.concurrent(True, 96)
    assert lib.tplan_shim_nch_dev(ctx.p, 12) == 96 and lib.tplan_shim_nch_dev(ctx.p, 120) == 120
    beside = ctx.device(12, **L1)
    assert (beside.team, beside.xcd_local, beside.grid) == (11, 0, 12 * 11)             # ceil(4 * 256 / 96); teams spread, no rounding to 8
    assert ctx.host(12, **L1).team == 11 and ctx.host(12, **L1).splits == min(32, (8 * CUS + 95) // 96, 8)
    lane = _l5(12)
    lane.concurrent(True, 200)
    assert lane.device(12, **L5).team == 2 and lane.host(12, **L5).team == 2            # 2 * 256 // 200


def test_grid_rounding_to_eight_channels_per_xcd():
    for nch in (1, 7, 8, 9, 33):
        o = _l1ca(nch).device(nch, **L1)
        assert o.xcd_local == 1 and o.grid == -(-nch // 8) * 8 * o.team


# ---- knobs --------------------------------------------------------------------------------------------------------------------------
def test_the_shipping_build_reads_no_tuning_knob(monkeypatch):
    for name, value in (("GC_TRACK_PERSIST", "0"), ("GC_TRACK_SPLITS", "5"), ("GC_DEVLOOP_MEMBERS", "3"), ("GC_DEVLOOP_WAVES", "4"), ("GC_DEVLOOP_SPREAD", "1"),
                        ("GC_TRACK_THREADS", "3"), ("GC_TRACK_LOCKSTEP", "1"), ("GC_TRACK_NO_POLL", "1")):
        monkeypatch.setenv(name, value)
    h, d = _l1ca(4).host(4, **L1), _l1ca(4).device(4, **L1)
    assert (h.mode, h.team, h.splits, h.async_, h.nthreads, h.poll) == (PERSIST_FAST, 23, 8, 1, 1, 1) and (d.team, d.xcd_local) == (32, 1)
    assert _l5(4).device(4, **L5).lane_waves == 8
    lib = _shim()
    assert lib.tplan_shim_poll_timeout_ms() == 2000
    monkeypatch.setenv("GC_TRACK_POLL_TIMEOUT_MS", "750")                               # the one variable the library that ships reads
    assert lib.tplan_shim_poll_timeout_ms() == 750
    monkeypatch.setenv("GC_TRACK_POLL_TIMEOUT_MS", "0")
    assert lib.tplan_shim_poll_timeout_ms() == 1


def test_knob_clamps_in_the_tuning_build(monkeypatch):
    fast, lane = _l1ca(4, tuning=True), _l5(4, tuning=True)
    assert (fast.host(4, **L1).mode, fast.host(4, **L1).team, lane.host(4, **L5).mode) == (PERSIST_FAST, 23, PERSIST_LANE)
    monkeypatch.setenv("GC_TRACK_PERSIST", "0")
    assert (fast.host(4, **L1).mode, lane.host(4, **L5).mode, fast.host(4, **L1).async_) == (PER_EPOCH, PER_EPOCH, 0)
    monkeypatch.setenv("GC_TRACK_PERSIST", "1")
    assert fast.host(4, **L1).mode == PERSIST_FAST
    monkeypatch.delenv("GC_TRACK_PERSIST")
    for value, splits, fast_team, lane_team in (("0", 1, 1, 1), ("5", 5, 5, 5), ("99", 32, 32, 6)):
        monkeypatch.setenv("GC_TRACK_SPLITS", value)
        hf, hl = fast.host(4, **L1), lane.host(4, **L5)
        assert (hf.splits, hf.team, hl.splits, hl.team) == (splits, fast_team, splits, lane_team), value
    monkeypatch.delenv("GC_TRACK_SPLITS")
    for value, fast_team, lane_team in (("0", 1, 1), ("3", 3, 3), ("99", 32, 6)):
        monkeypatch.setenv("GC_DEVLOOP_MEMBERS", value)
        assert (fast.device(4, **L1).team, lane.device(4, **L5).team) == (fast_team, lane_team), value
    assert fast.device(4, cap=2, **L1).team == 2                                        # the retry's cap holds over the knob
    monkeypatch.delenv("GC_DEVLOOP_MEMBERS")
    for value, waves, team in (("0", 1, 6), ("4", 4, 6), ("99", 8, 6)):
        monkeypatch.setenv("GC_DEVLOOP_WAVES", value)
        o = lane.device(4, **L5)
        assert (o.lane_waves, o.team) == (waves, team), value
    monkeypatch.setenv("GC_DEVLOOP_WAVES", "2")                                         # fewer waves per member: more members by the block length
    assert lane.device(4, **dict(L5, fs=2.5e6)).team == min(6, 2500 // (64 * 2 * 2))
    monkeypatch.delenv("GC_DEVLOOP_WAVES")
    many = _l1ca(200, tuning=True)
    assert many.host(200, **L1).nthreads == 4 and fast.host(4, **L1).nthreads == 1 and _l1ca(64, tuning=True).host(64, **L1).nthreads == 2
    for value, n4, n200 in (("0", 1, 1), ("3", 3, 3), ("99", 4, 16)):
        monkeypatch.setenv("GC_TRACK_THREADS", value)
        assert (fast.host(4, **L1).nthreads, many.host(200, **L1).nthreads) == (n4, n200), value
    monkeypatch.delenv("GC_TRACK_THREADS")
    monkeypatch.setenv("GC_TRACK_LOCKSTEP", "1")
    assert (fast.host(4, **L1).mode, fast.host(4, **L1).async_) == (PERSIST_FAST, 0)
    monkeypatch.delenv("GC_TRACK_LOCKSTEP")
    monkeypatch.setenv("GC_TRACK_NO_POLL", "1")
    assert (fast.host(4, **L1).mode, fast.host(4, **L1).poll, lane.host(4, **L5).mode) == (PER_EPOCH, 0, PER_EPOCH)
    monkeypatch.delenv("GC_TRACK_NO_POLL")
    monkeypatch.setenv("GC_DEVLOOP_SPREAD", "1")
    o = _l1ca(33, tuning=True).device(33, **L1)
    assert (o.xcd_local, o.grid) == (0, 33 * 32)


# ---- a seeded sweep of the teams against tests/track_teams.py ------------------------------------------------------------------------
def test_teams_of_a_seeded_sweep_equal_the_mirrors():
    rng = np.random.default_rng(20241104)
    fmts = sorted(LP.FORMATS)
    seen = {"fast_dev": 0, "fast_host": 0, "lane_dev": 0, "lane_host": 0}
    for it in range(2000):
        fmt = fmts[int(rng.integers(0, 6))]
        i8c = fmt in ("i8_iq", "i8_qi")
        cus = int(rng.integers(32, 305))
        nch = int(rng.integers(1, 257)) if it % 3 else int(rng.choice((1, 2, 4, 12, 33, 85, 128, 256)))
        arms = int(rng.integers(1, 3))
        chips = int(rng.choice((50, 100, 400, 511, 1023, 2046, 4092, 10230)))
        spc = float(rng.choice((1.3, 1.76, 2.5, 4.0, 6.9, 7.2, 8.0, 12.0, 15.0, 15.3, 17.6, 25.0)))   # samples per chip: both sides of the lowrate thresholds
        rate = chips * 1e3
        fs = float(round(spc * rate))
        ctx = Ctx(fmt, cus=cus)
        ids = list(range(min(nch, 4)))                                                  # the channels share four table sets, as the GPU rigs share four PRNs
        for c in ids:
            ctx.channel(c, nent=[chips + 2] * arms)
        channels = [ids[k % len(ids)] for k in range(nch)]
        kw = dict(fs=fs, rate=rate, chips=float(chips), d=0.5, pilot=1 if arms == 2 else 0, channels=channels)
        S = _settings(fs, rate, chips)
        dev, host = ctx.device(nch, **kw), ctx.host(nch, **kw)
        assert dev.status == 0 and host.status == 0, (it, dev.status, host.status)
        lr = _lowrate(rate * 1.001 / fs)
        tables_fit = 8 * ((chips + 2 + 8 + 15) // 16 * 16) + 512 <= 64 * 1024            # launch_plan.h gc_fast_table_mode 0, one arm
        if arms == 1 and lr > 0 and tables_fit:
            assert (dev.kernel, dev.team, dev.lowrate) == (1, _fast_device_team(cus, nch, S, i8c), lr if i8c else 1), (it, fmt, cus, nch, chips, spc, dev.team)
            assert (host.mode, host.team, host.fast_nominal) == (PERSIST_FAST, _fast_host_team(cus, nch, S), lr), (it, fmt, cus, nch, chips, spc, host.team)
            seen["fast_dev"] += 1
            seen["fast_host"] += 1
        else:
            blksize = int(np.ceil(chips / (rate / fs)))
            assert (dev.kernel, dev.team) == (0, _lane_device_team(cus, nch, arms, blksize)), (it, fmt, cus, nch, arms, chips, spc, dev.team)
            seen["lane_dev"] += 1
            approx8 = (int(chips / (rate / fs) / 8.0) + 1) * 8                          # the host's lane team: its 8-sample chunk count, not the block's length
            assert (host.mode, host.team) == (PERSIST_LANE, max(1, min({1: 8, 2: 6}[arms], approx8 // 1024, max(1, 2 * cus // nch)))), (it, host.mode, host.team)
            seen["lane_host"] += 1
        assert dev.grid == (nch + 7) // 8 * 8 * dev.team
        assert 1 <= host.splits <= 32 and (host.fast_nominal > 0 or host.splits % 16 == 0)
    print(f"\n[track plan] sweep: {seen}")
    assert min(seen.values()) >= 200, seen
