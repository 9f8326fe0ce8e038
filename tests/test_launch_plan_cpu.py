"""The launch planner (csrc/launch_plan.h: gc_scope_from_blocks, the splits policies, gc_plan_launch) without a GPU:
tests/launch_plan_shim.hip runs it on the CPU over channel FACTS (arms, table lengths, ramp multipliers), a record format and a
descriptor list, and returns the plan gc_correlate / gc_replay_launch / gc_track's launch per epoch would dispatch on.

Kernel codes: the cases of tests/test_gpu_correlator_edges.py (every rig x record format, the replay-only kernels, the step
thresholds), tests/test_gpu_variants.py, tests/test_gpu_correlator.py and tests/test_gpu_tracking_f64.py, restated as such facts;
the plan's kernel is the code those tests assert with engine.last_kernel() on the device (256 CUs).  The cases behind a tuning
switch run on the shim built with -DGC_TUNING=1, as those tests run on libgnsscorr_tuning.so.

Geometry: a seeded sweep; every plan must cover each block exactly once and keep the alignments the kernels rely on."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CUS = 256
FORMATS = {"i8_iq": (0, 1), "i8_qi": (0, 2), "i16_iq": (1, 1), "i16_qi": (1, 2), "i8_real": (0, 0), "i16_real": (1, 0)}  # (dtype, layout)
LANE_WAVES = 16


class Out(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("status", "kernel", "fast", "chunk", "bpw", "stride", "wide", "share_el", "derived", "waves",
                                       "xcd_swizzle", "splits", "period")] + [("grid", C.c_uint), ("total_wg", C.c_longlong)]

    def key(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


_LIBS = {}


def _shim(tuning=False):
    if tuning in _LIBS:
        return _LIBS[tuning]
    from cu_sdr_collection_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(HERE, "launch_plan_shim.hip")
    out = os.path.join(HERE, "build", "liblaunch_plan_shim_tuning.so" if tuning else "liblaunch_plan_shim.so")
    deps = [src] + [os.path.join(B.CSRC, h) for h in B.HEADERS]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = [f for f in B._tu_flags("corr_kernel.hip") if f != "--offload-compress"] + (["-DGC_TUNING=1"] if tuning else [])
        subprocess.run([hipcc, *flags, "-shared", src, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.plan_shim_create.restype = C.c_void_p
    lib.plan_shim_create.argtypes = [C.c_int] * 5 + [C.c_ulonglong]
    lib.plan_shim_destroy.argtypes = [C.c_void_p]
    lib.plan_shim_set_channel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]
    lib.plan_shim_plan.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Out)]
    lib.plan_shim_plan_epoch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(Out)]
    lib.plan_shim_track_splits.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_double] * 3
    _LIBS[tuning] = lib
    return lib


class Ctx:
    """Device and record facts + channels; plan() = gc_correlate's launch, plan(replay=True) = gc_replay_prepare + gc_replay_launch."""

    def __init__(self, fmt="i8_iq", cus=CUS, generic=False, double=False, nsamp=1 << 40, tuning=False):
        self.lib = _shim(tuning)
        dtype, layout = FORMATS[fmt]
        self.p = self.lib.plan_shim_create(cus, dtype, layout, int(generic), int(double), nsamp)
        self.chans = {}

    def __del__(self):
        self.lib.plan_shim_destroy(self.p)

    def channel(self, i, nent, R=1.0, mult=None, window=None, six_fold=False):
        arms = len(nent)
        mult = [1.0] * arms if mult is None else list(mult)
        window = [0] * arms if window is None else list(window)
        self.lib.plan_shim_set_channel(self.p, i, arms, R, (C.c_int * arms)(*nent), (C.c_double * arms)(*mult), (C.c_int * arms)(*window), int(six_fold))
        self.chans[i] = (list(nent), R, mult)

    def blocks(self, channel, n, step, d, rem=0.0, s0=0):
        """Descriptor list from arrays (or scalars) of equal length."""
        from cu_sdr_collection_amd import _lib as L
        channel = np.atleast_1d(channel)
        dt = np.dtype([("channel", "<i4"), ("blksize", "<i4"), ("first_sample", "<i8"), ("rem", "<f8"), ("step", "<f8"), ("d", "<f8"),
                       ("f", "<f8"), ("phi", "<f8"), ("off", "<i4", 3), ("res", "<i4")])
        assert dt.itemsize == C.sizeof(L.gc_block)
        b = np.zeros(channel.shape[0], dtype=dt)
        b["channel"], b["blksize"], b["first_sample"], b["rem"], b["step"], b["d"] = channel, n, s0, rem, step, d
        return b

    def plan(self, b, replay=False, splits=-1, polled=False):
        o = Out()
        self.lib.plan_shim_plan(self.p, b.shape[0], b.ctypes.data, int(replay), splits, int(polled), C.byref(o))
        return o

    def track_splits(self, b, fs, rate, chips):
        """The splits gc_track's planner (csrc/track_plan.h) gives the launch per epoch of these channels' first blocks."""
        return self.lib.plan_shim_track_splits(self.p, b.shape[0], b.ctypes.data, fs, rate, chips)

    def plan_epoch(self, b, splits, polled=True):
        o = Out()
        self.lib.plan_shim_plan_epoch(self.p, b.shape[0], b.ctypes.data, splits, int(polled), C.byref(o))
        return o


def _periodic(ctx, period, nb, n, step, d, rng=None):
    """An epoch-major replay list over channels 0 .. period-1; the steps scattered by 3e-6 as a tracking loop leaves them."""
    steps = step * (1 + (rng.uniform(-3e-6, 3e-6, nb) if rng is not None else 0.0))
    return ctx.blocks(np.arange(nb) % period, n, steps, d)


# ---- kernel codes: tests/test_gpu_correlator_edges.py ----------------------------------------------------------------------------
def _boc(L):  # BOC(1,1) data and pilot, BOC(6,1) pilot of an L-chip code, padded: R = 2, arm_mult = [1, 1, 6]
    return dict(nent=[2 * L + 2, 2 * L + 2, 12 * L + 2], R=2.0, mult=[1.0, 1.0, 6.0])


RIGS = {  # name: (channels, code rate at 18 Msps, spacing)
    "fast16": ([dict(nent=[1025]), dict(nent=[513])], 1.023e6, 0.5),
    "fast8": ([dict(nent=[2048]), dict(nent=[1025])], 2.046e6, 0.5),
    "lane_f32": ([dict(nent=[10232, 10232]), dict(nent=[8186, 8186])], 10.23e6, 0.5),
    "lane_f16": ([dict(nent=[16384, 16384]), dict(nent=[10232, 10232])], 10.23e6, 0.5),
    "lane_derived": ([dict(six_fold=True, **_boc(1023)), dict(six_fold=True, **_boc(511))], 1.023e6, 0.05),
    "mixed": ([_boc(1023), _boc(511)], 1.023e6, 0.05),
}
RIGS["generic"] = RIGS["double"] = RIGS["fast16"]
EDGE_FORMATS = ("i8_iq", "i8_qi", "i16_iq", "i8_real")


def _rig_kernel(name, fmt):
    """Rig.expected_kernel of the GPU module at the rig's nominal step."""
    i8c = fmt in ("i8_iq", "i8_qi")
    return {"fast16": 1, "fast8": 1, "lane_f32": 0, "lane_f16": 0, "lane_derived": 0 if i8c else -1, "mixed": -1, "generic": 0, "double": 6}[name]


@pytest.mark.parametrize("fmt", EDGE_FORMATS)
@pytest.mark.parametrize("name", sorted(RIGS))
def test_edge_rigs_plan_the_kernel_the_gpu_sweep_asserts(name, fmt):
    chans, rate, d = RIGS[name]
    ctx = Ctx(fmt, generic=name == "generic", double=name == "double")
    for i, c in enumerate(chans):
        ctx.channel(i, **c)
    step = rate / 18e6
    for nb in (1, 2, 63, 64, 65, 1040):                               # the launch sizes of the sweep
        b = ctx.blocks(np.arange(nb) % 2 if nb > 4 else np.zeros(nb, dtype=int), np.where(np.arange(nb) % 3 == 0, 1, 257), step, d)
        for replay in ((False,) if name == "double" else (False, True)):   # run_launch: gc_correlate, then the same list through replay
            o = ctx.plan(b, replay=replay)
            assert (o.status, o.kernel) == (0, _rig_kernel(name, fmt)), (name, fmt, nb, replay, o.status, o.kernel)


@pytest.mark.parametrize("fmt", EDGE_FORMATS)
@pytest.mark.parametrize("kernel", [2, 3, 4, 5])
def test_replay_only_kernels_are_planned_for_big_periodic_lists(kernel, fmt):
    i8c, real = fmt in ("i8_iq", "i8_qi"), fmt.endswith("real")
    chans, rate, d = {3: ([dict(nent=[1025])] * 2, 1.023e6, 0.5), 2: ([dict(nent=[1025, 1025])] * 2, 1.023e6, 0.5),
                      4: ([dict(nent=[2048])] * 2, 2.046e6, 0.5), 5: ([dict(six_fold=True, **_boc(1023))] * 3, 1.023e6, 0.05)}[kernel]
    want = {2: 2 if i8c else 1, 3: 3 if i8c else 1, 4: 1 if real else 4, 5: 5 if i8c else -1}[kernel]   # _replay_expected
    ctx = Ctx(fmt)
    for i, c in enumerate(chans):
        ctx.channel(i, **c)
    period = len(chans)
    nb = (16 if kernel == 5 else 8) * period * CUS + (0 if kernel == 5 else period * 37)
    for spacing in ((d, 0.3 * d) if kernel in (3, 4) else (d,)):
        b = _periodic(ctx, period, nb, np.where(np.arange(nb) % 50 == 0, 17, 4097), rate / 18e6, spacing, np.random.default_rng(kernel))
        o = ctx.plan(b, replay=True)
        assert (o.status, o.kernel, o.period) == (0, want, period), (kernel, fmt, o.kernel, want)


def test_replay_step_thresholds_select_the_kernel():
    ctx = Ctx("i8_iq")
    for i in range(2):
        ctx.channel(i, nent=[1025])
    nb = 8 * 2 * CUS + 2 * 37
    codes = {}
    for t in (0.995, 1.995, 3.995):
        for e in (-1e-9, 1e-9):
            step = (t / 15.0) * (1 + e)
            o = ctx.plan(ctx.blocks(np.arange(nb) % 2, 150, step, 0.5), replay=True)
            assert o.status == 0
            codes[(t, e < 0)] = o.kernel
    assert codes == {(0.995, True): 3, (0.995, False): 4, (1.995, True): 4, (1.995, False): 4, (3.995, True): 4, (3.995, False): 0}, codes


def test_small_launch_step_thresholds_change_the_kernel():
    ctx = Ctx("i8_iq")
    ctx.channel(0, nent=[2048])
    seen = {e < 0: ctx.plan(ctx.blocks([0], 4097, (0.995 / 7.0) * (1 + e), 0.5)).kernel for e in (-1e-9, 1e-9)}
    assert seen == {True: 1, False: 0}, seen


def test_refused_descriptors_are_refused_by_the_scope_builder():
    from cu_sdr_collection_amd import _lib as L
    ctx = Ctx("i8_iq", nsamp=40009)
    ctx.channel(0, nent=[1025])
    step = 1.023e6 / 18e6
    for kw, want in ((dict(rem=-0.9), L.GC_E_INVALID), (dict(rem=-0.4), L.GC_OK), (dict(s0=40000), L.GC_E_RANGE)):
        for replay in (False, True):
            assert ctx.plan(ctx.blocks([0], 1000, step, 0.5, **kw), replay=replay).status == want, kw
    assert ctx.plan(ctx.blocks([1], 1000, step, 0.5)).status == L.GC_E_STATE          # channel not configured
    assert ctx.plan(ctx.blocks([0], 1000, step, 1.0)).status == L.GC_E_INVALID        # d * R * mult >= 1


# ---- kernel codes: tests/test_gpu_correlator.py ----------------------------------------------------------------------------------
def _big_list(tuning, nent, rate, tail, spacing=0.5):
    ctx = Ctx("i8_iq", tuning=tuning)
    for i in range(2):
        ctx.channel(i, nent=[nent])
    nb = 64 * 2 * CUS + 2 * tail
    step = rate / 18e6
    return ctx, _periodic(ctx, 2, nb, int((nent - 2) / step), step, spacing, np.random.default_rng(77)), nb


def test_big_periodic_lists_take_the_four_wave_kernels():
    for spacing in (0.5, 0.3):
        ctx, b, nb = _big_list(False, 1025, 1.023e6, 37, spacing)
        assert ctx.plan(b, replay=True).kernel == 3
        assert ctx.plan(b[::nb // 2000].copy()).kernel == 1               # 2 000 of them through gc_correlate: the one-wave kernel
    ctx, b, _ = _big_list(False, 2048, 2.046e6, 11)
    assert ctx.plan(b, replay=True).kernel == 4


def test_big_periodic_lists_behind_the_tuning_switches(monkeypatch):
    ctx, b, _ = _big_list(True, 1025, 1.023e6, 37)
    monkeypatch.setenv("GC_NO_TABF", "1")
    assert ctx.plan(b, replay=True).kernel == 2
    monkeypatch.delenv("GC_NO_TABF")
    ctx, b, _ = _big_list(True, 2048, 2.046e6, 11)
    monkeypatch.setenv("GC_NO_MULTI", "1")
    assert ctx.plan(b, replay=True).kernel == 3
    monkeypatch.setenv("GC_NO_TABF", "1")
    assert ctx.plan(b, replay=True).kernel == 2
    ctx, b, _ = _big_list(False, 2048, 2.046e6, 11)                        # the library that ships reads no switch
    assert ctx.plan(b, replay=True).kernel == 4


# ---- kernel codes: tests/test_gpu_variants.py ------------------------------------------------------------------------------------
MULTI_CASES = {"l5_50msps_share": dict(fs=50e6, L=10230, rate=10.23e6, R=1.0, arms=2, d=0.5, fmt="i8_iq"),
               "l5_50msps_three_ramps": dict(fs=50e6, L=10230, rate=10.23e6, R=1.0, arms=2, d=0.3, fmt="i8_iq"),
               "e1_share": dict(fs=18e6, L=4092, rate=1.023e6, R=2.0, arms=2, d=0.25, fmt="i8_iq"),
               "e1_three_ramps": dict(fs=18e6, L=4092, rate=1.023e6, R=2.0, arms=2, d=0.1, fmt="i8_iq"),
               "b1i_one_arm_qi": dict(fs=18e6, L=2046, rate=2.046e6, R=1.0, arms=1, d=0.5, fmt="i8_qi"),
               "l5_50msps_int16": dict(fs=50e6, L=10230, rate=10.23e6, R=1.0, arms=2, d=0.5, fmt="i16_iq"),
               "e1_int16_qi": dict(fs=18e6, L=4092, rate=1.023e6, R=2.0, arms=2, d=0.1, fmt="i16_qi")}


@pytest.mark.parametrize("case", sorted(MULTI_CASES))
def test_multi_transition_kernel_takes_its_lists_and_its_switch_gives_them_back(case, monkeypatch):
    cfg = MULTI_CASES[case]
    monkeypatch.setenv("GC_MULTI_MIN", "1")
    ctx = Ctx(cfg["fmt"], tuning=True)
    period = 3
    for i in range(period):
        ctx.channel(i, nent=[int(cfg["L"] * cfg["R"]) + 2] * cfg["arms"], R=cfg["R"])
    epochs = max(180, (8 * CUS + period - 1) // period + 4)
    step = cfg["rate"] / cfg["fs"]
    b = _periodic(ctx, period, period * epochs, int(np.ceil(cfg["L"] / step)), step, cfg["d"], np.random.default_rng(11))
    assert ctx.plan(b, replay=True).kernel == 4
    monkeypatch.setenv("GC_NO_MULTI", "1")
    o = ctx.plan(b, replay=True)
    assert o.status == 0 and o.kernel != 4


def _hybrid(ctx, L, epochs, rng=None):
    for i in range(3):
        ctx.channel(i, six_fold=True, **_boc(L))
    step = 1.023e6 / 18e6
    return _periodic(ctx, 3, 3 * epochs, int(np.ceil(L / step)), step, 0.05, rng)


@pytest.mark.parametrize("case", [("i8_iq", 4092), ("i8_qi", 4092), ("i8_iq", 10230)])
def test_hybrid_kernel_takes_two_rounds_two_thirds_full(case, monkeypatch):
    fmt, L = case
    ctx = Ctx(fmt)
    assert ctx.plan(_hybrid(ctx, L, 16 * CUS, np.random.default_rng(23)), replay=True).kernel == 5
    gen = Ctx(fmt, generic=True)                                          # gc_force_generic_kernel: the lane kernel's derived-arm instantiation
    o = gen.plan(_hybrid(gen, L, 16 * CUS), replay=True)
    assert (o.kernel, o.derived) == (0, 1)
    assert ctx.plan(_hybrid(ctx, L, 5 * CUS), replay=True).kernel == 0   # one round at 16 waves per CU, 1.25 at 12
    assert ctx.plan(_hybrid(ctx, L, 2), replay=True).kernel == 0         # a few blocks
    tun = Ctx(fmt, tuning=True)
    b = _hybrid(tun, L, 16 * CUS)
    assert tun.plan(b, replay=True).kernel == 5
    monkeypatch.setenv("GC_NO_CBOC", "1")
    assert tun.plan(b, replay=True).kernel == 0


# ---- kernel codes: tests/test_gpu_tracking_f64.py --------------------------------------------------------------------------------
def test_float64_precision_always_plans_the_float64_kernel():
    for fmt in FORMATS:
        ctx = Ctx(fmt, double=True)
        ctx.channel(0, nent=[1025])
        ctx.channel(1, nent=[2048, 2048, 12278], R=2.0, mult=[1.0, 1.0, 6.0], six_fold=True)
        step = 1.023e6 / 18e6
        assert ctx.plan(ctx.blocks([0, 0, 0], 17000, step, 0.5)).kernel == 6                   # gc_correlate
        for b in (ctx.blocks([0], 17000, step, 0.5), ctx.blocks([1], 17000, step, 0.05)):     # gc_track's launch per epoch
            splits = ctx.track_splits(b, 18e6, 1.023e6, 1023.0)
            assert 1 <= splits <= 32
            assert ctx.plan_epoch(b, splits).kernel == 6


# ---- every plan of a sweep: coverage and alignment -------------------------------------------------------------------------------
TABLES = (300, 1025, 2010, 2040, 4050, 4070, 6100, 6140, 8100, 8130, 10100, 10120, 12250, 12300, 20000, 40000, 70000)
RATES = (0.05, 0.995 / 15 * (1 - 1e-3), 0.995 / 15 * (1 + 1e-3), 0.1, 0.13, 0.995 / 7 * (1 - 1e-3), 0.995 / 7 * (1 + 1e-3), 0.2, 0.3, 0.57)


def _each_once(idx, n):
    """idx holds every integer below n exactly once."""
    return idx.shape[0] == n and (n == 0 or (0 <= idx.min() and idx.max() < n and bool((np.bincount(idx, minlength=n) == 1).all())))


def _covered_once(o, nb):
    """Every block index below nb - every (block, split) item where blocks are split - is reached by exactly one (workgroup, slot)
    of the plan's bpw / stride / grid, enumerated the way the kernels index (corr_lane.hip, corr_fast.hip, corr_kernel.hip)."""
    b = np.arange(o.grid, dtype=np.int64)
    if o.xcd_swizzle:                                                    # workgroup b runs on XCD b % 8: every XCD a contiguous range
        b = (b & 7) * (o.grid >> 3) + (b >> 3)
        b = b[b < o.total_wg]                                            # the workgroups past total_wg go home
    if o.bpw > 1 or o.stride > 1:                                        # periodic: slot bi of workgroup w is epoch grp * bpw + bi of channel cslot
        idx = ((b // o.stride * o.bpw)[:, None] + np.arange(o.bpw, dtype=np.int64)[None, :]) * o.stride + (b % o.stride)[:, None]
        idx = idx.ravel()
        idx = idx[idx < nb]
        return _each_once(idx, nb)
    if o.kernel == 0 and o.wide:                                         # one block per workgroup, cut 16 ways over its waves in the kernel
        return _each_once(b, nb)
    # the slots of workgroup w are the `waves` consecutive items w * waves ..; item i is split i % splits of block i // splits
    waves = LANE_WAVES if o.kernel == 0 else 4 if o.kernel in (2, 3) else 1
    return o.splits % waves == 0 and b.shape[0] * waves == nb * o.splits and _each_once(b, b.shape[0])


def test_every_plan_of_a_seeded_sweep_covers_its_blocks_once_and_is_aligned():
    rng = np.random.default_rng(20240229)
    fmts = sorted(FORMATS)
    ctxs = {(f, cus, dbl): Ctx(f, cus=cus, double=dbl) for f in fmts for cus in (256, 304) for dbl in (False, True)}
    cases, skipped, kernels = 0, 0, {}
    for it in range(360):
        fmt, cus, dbl = fmts[it % 6], (256, 304)[(it // 6) % 2], it % 37 == 0
        # every fifth case each aims at the float-table WIDE and at the hybrid kernel, which take the narrowest class of lists: int8
        # I/Q or Q/I (two in three of these cases), periodic, >= 4 epochs per CU (hybrid: two rounds), one arm / a six-fold third arm
        aim = {1: 3, 3: 5}.get(it % 5, 0)
        if aim and it % 3:
            fmt = ("i8_iq", "i8_qi")[it % 2]
        ctx = ctxs[(fmt, cus, dbl)]
        period = (0, 1, 3, 8, 12)[int(rng.integers(1 if aim else 0, 5))]
        arms = 1 if it % 8 == 0 or aim == 3 else 3 if aim == 5 else int(rng.integers(1, 4))   # one-arm channels more often
        kind = "six_fold" if aim == 5 else ("plain", "six_fold", "mixed")[int(rng.integers(0, 3))] if arms == 3 else "plain"
        nchan = max(period, 1)
        if kind == "plain":
            nent, R = int(rng.choice(TABLES[:4] if aim else TABLES[:6] if it % 8 == 0 else TABLES)), float(rng.choice((1.0, 2.0)))
            for c in range(nchan):
                ctx.channel(c, nent=[nent] * arms, R=R)
        else:
            L = int(rng.choice((511, 1023, 4092, 10230)))
            nent, R = 2 * L + 2, 2.0
            for c in range(nchan):
                ctx.channel(c, six_fold=kind == "six_fold", **_boc(L))
        rate = float(rng.choice(RATES[:3] if aim == 3 else RATES[:5] if aim else RATES))   # table entries per sample
        step = rate / R
        d = float(rng.choice((0.5, 0.25, 0.3, 0.05))) / R
        if kind != "plain":
            d = min(d, 0.9 / (6 * R))
        nmax = int((nent - 3 - d * R) / rate)                            # the ramp stays inside the table
        nb = int(round(10 ** rng.uniform(0, 5)))
        if period and it % 4 == 0:                                       # lists around the launchers' own thresholds: 4, 8 and 64 epochs per CU
            nb = period * cus * int(rng.choice((4, 9, 70) if period <= 3 else (4, 9))) + int(rng.integers(-3, 40))
        elif aim:                                                        # from just below 4 epochs per CU (hybrid: per 16-wave workgroup) up
            nb = int(period * cus * rng.uniform(3.5, 12) * (1 if aim == 3 else 16 / period)) + int(rng.integers(0, 40))
        n = np.minimum(nmax, rng.integers(1, 40000, nb) if it % 3 else np.full(nb, nmax))
        chan = np.arange(nb) % period if period else rng.integers(0, nchan, nb)
        b = ctx.blocks(chan, n, step, d, rem=rng.uniform(0, step, nb))
        for replay in (False, True):
            o = ctx.plan(b, replay=replay)
            cases += 1
            if o.status != 0 and o.kernel == -2 and o.splits == 0:      # refused by the scope builder
                skipped += 1
                continue
            assert o.status == 0, (it, replay, o.key())
            plans = [o]
            if not dbl:                                                  # a caller's own splits (gc_track's: every kernel class takes a multiple of 16), polled or not
                for splits, polled in ((int(rng.choice((16, 32))), bool(it % 2)), (1, True)):
                    f = ctx.plan(b, replay=replay, splits=splits, polled=polled)
                    assert f.status == 0 and f.kernel not in (4, 5), (it, splits, polled, f.key())
                    plans.append(f)
            for q in plans:
                kernels[q.kernel] = kernels.get(q.kernel, 0) + 1
                if q.kernel == 6:                                    # corr_f64.hip lays its own grid out
                    assert dbl
                    continue
                assert not dbl and q.grid >= 1 and q.bpw >= 1 and q.stride >= 1
                if q.xcd_swizzle:
                    assert q.grid % 8 == 0 and 64 <= q.total_wg <= q.grid < q.total_wg + 8
                if q.kernel == 0 and q.splits > 1:
                    assert q.splits % 16 == 0
                if q.kernel in (2, 3) and q.bpw == 1:
                    assert q.splits % 4 == 0
                if q.kernel in (4, 5):
                    assert q.period > 0 and q.splits == 1 and q.waves >= 1 and q.bpw % q.waves == 0
                if q.bpw > 1 or q.stride > 1:
                    assert q.period > 0 and q.stride == q.period and q.splits == 1
                if q.kernel in (2, 3):
                    assert fmt in ("i8_iq", "i8_qi")
                if q.kernel == 5 or q.derived:
                    assert kind == "six_fold" and fmt in ("i8_iq", "i8_qi")
                assert _covered_once(q, nb), (it, q.key())
    print(f"\n[plan] {cases} cases, {skipped} refused by the scope builder; plans per kernel: {dict(sorted(kernels.items()))}")
    assert skipped * 10 < cases, (skipped, cases)
    assert set(kernels) == {-1, 0, 1, 2, 3, 4, 5, 6}, kernels
    assert min(kernels.values()) >= 20, kernels                          # no kernel's alignment rules rest on a handful of plans


def test_planning_is_pure():
    """The same inputs planned twice, with other plans made in between, give the same plan."""
    rng = np.random.default_rng(5)
    lists = []
    for fmt in ("i8_iq", "i16_qi", "i8_real"):
        ctx = Ctx(fmt)
        for c in range(3):
            ctx.channel(c, nent=[1025])
            ctx.channel(3 + c, nent=[8186, 8186], R=2.0)
            ctx.channel(6 + c, six_fold=True, **_boc(1023))
        for base, rate, d in ((0, 1.023e6 / 18e6, 0.5), (3, 0.13, 0.25), (6, 1.023e6 / 18e6, 0.05)):
            for nb in (1, 7, 300, 3 * 16 * CUS):
                lists.append((ctx, ctx.blocks(base + np.arange(nb) % 3, 2000, rate, d, rem=rng.uniform(0, rate, nb))))
    first = [(ctx.plan(b).key(), ctx.plan(b, replay=True).key(), ctx.plan(b, splits=16, polled=True).key()) for ctx, b in lists]
    for k in rng.permutation(len(lists)):
        ctx, b = lists[k]
        assert (ctx.plan(b).key(), ctx.plan(b, replay=True).key(), ctx.plan(b, splits=16, polled=True).key()) == first[k]
    assert len({f for f in first}) > 12
