"""The descriptors and calls of gc_cancel's edge sweep: tests/test_gpu_cancel_edges.py sends them to the device,
tests/test_cancel_edges_cpu.py checks the sweep itself (its caps, its refusal predictor, its axes, the exact class).

gc_cancel (csrc/cancel.hip) refuses two overlapping blocks of one channel, so descriptors cannot be sent one by one: the generator
classifies every descriptor first and then packs the inside ones into calls.  Every descriptor is exactly one of
  inside    check_block accepts it and MATLAB's colon of its ramp has N elements (cancel_model.oracle_ok): sent and compared
  refused   refusal() - check_block's numeric conditions restated, in its order - predicts the status: sent alone, the library
            must answer exactly that and leave dst and amp_out untouched
  outside   accepted, but MATLAB's colon has N - 1 elements: not sent (at most 1 % of a rig's descriptors)
Everything is seeded; a sweep depends on the rig, the record format's name and the record's sample count only.

Rigs: bank_edge_cases.make_rig's l1ca (R = 1), e1bc (R = 2, two arms), b1c (R = 2, multipliers 1, 1, 6) and l5, and `wide`: a ternary
table with runs of zeros (E < N, E = 0 on short blocks), a channel with a code window on one arm and a channel whose blocks carry a
table_offset per arm up to the largest one check_block lets through (table_offset + 3 == entries).  gc_set_code refuses a table
value outside {-1, 0, +1} (GC_E_INVALID, asserted by the GPU module), so a table of larger integers cannot reach gc_cancel.

Slots: slot s of the engine holds logical channel SLOT_OF[s % len] of the rig, all GC_CANCEL_MAX_CHANNELS slots configured in
descending order; the packer lays the blocks of the first PACK_SLOTS slots end to end with gaps from {0, 1, 7, 64}, a new call
where a slot's record is full; the slots overlap each other freely."""
import math

import numpy as np

import bank_edge_cases as B
import cancel_model as M
from oracle import gnss_oracle as O
from test_gpu_correlator_edges import IF, Chan

FS = 18e6
NS = 40009                                  # samples per record in every format: no format's byte count is a multiple of 16
ZERO_AT, ZERO_LEN = 34000, 100              # an all-zero stretch (samples)
FORMATS = {"i8_iq": (np.int8, M.IQ), "i8_qi": (np.int8, M.QI), "i8_real": (np.int8, M.REAL),
           "i16_iq": (np.int16, M.IQ), "i16_qi": (np.int16, M.QI), "i16_real": (np.int16, M.REAL)}
RIGS = ("l1ca", "e1bc", "b1c", "l5", "wide")
LENGTHS = B.LENGTHS + [6145]
RATES = ("one", "0.999", "0.5", "0.2", "nominal", "1/64", "2^-16", "2^-40")       # step * R * max(m); and 3.5 on short blocks
REMS = ("0", "+1e-13", "-1e-13", "-0.4", "min", "1000.25", "1000.5", "top")
F_SET = (0.0, -IF, FS / 2 - 1, -(FS / 2 - 1), 1.5 * FS)
PHI_SET = (0.0, 2 * math.pi, -2 * math.pi, 1e4, -1e4, 1e-300)
GAPS = (0, 1, 7, 64)
MAX_CHANNELS = 64                           # GC_CANCEL_MAX_CHANNELS
PACK_SLOTS = 4
OUTSIDE_CAP = 0.01
CLASSES = ("offset", "descriptor", "range", "low", "table_end")
STATUS = {"offset": "GC_E_INVALID", "descriptor": "GC_E_INVALID", "range": "GC_E_RANGE", "low": "GC_E_INVALID", "table_end": "GC_E_INVALID"}


class CancelRig:
    """chans: the logical channels (test_gpu_correlator_edges.Chan); windows[c]: code window per arm or None; slot s holds
    chans[slot_of[s % len(slot_of)]]."""

    def __init__(self, name, chans, step0, seed, windows=None, slot_of=(0, 1, 0, 0)):
        self.name, self.chans, self.step0, self.seed, self.fs = name, chans, step0, seed, FS
        self.windows = windows or [None] * len(chans)
        self.slot_of = slot_of

    def logical(self, slot):
        return self.slot_of[slot % len(self.slot_of)]

    def chan(self, slot):
        return self.chans[self.logical(slot)]

    def model_chans(self):
        return {s: {"tables": self.chan(s).tables, "r": self.chan(s).R, "mult": self.chan(s).mult} for s in range(MAX_CHANNELS)}

    def setup(self, engine):
        for s in range(MAX_CHANNELS - 1, -1, -1):           # descending: the sum must still run in ascending channel index
            ch, c = self.chan(s), self.logical(s)
            engine.set_channel(s, [t.astype(np.int8) for t in ch.tables], index_scale=ch.R,
                               arm_mult=None if set(ch.mult) == {1.0} else ch.mult, windows=self.windows[c])

    def clear_windows(self, engine):
        """A session-wide engine must not carry a code window into the next module."""
        for s in range(MAX_CHANNELS):
            ch = self.chan(s)
            engine.set_channel(s, [t.astype(np.int8) for t in ch.tables], index_scale=ch.R,
                               arm_mult=None if set(ch.mult) == {1.0} else ch.mult)


def _ternary(rng, n):
    """A padded ternary table of n chips with runs of zeros (entries 100..140 of the padded table among them)."""
    c = rng.choice(np.array([-1.0, 0.0, 1.0]), size=n, p=[0.4, 0.2, 0.4])
    for at, ln in ((99, 41), (700, 9), (1500, 3)):
        if at + ln < n:
            c[at:at + ln] = 0.0
    return O.pad_code(c)


def make_rig(name):
    if name != "wide":
        r = B.make_rig(name)
        return CancelRig(name, r.chans, r.step0, r.seed)
    rng = np.random.default_rng(sum(map(ord, name)))
    pm = lambda n: O.pad_code(rng.choice(np.array([-1.0, 1.0]), size=n))        # noqa: E731
    chans = [Chan([_ternary(rng, 2048)], 2048),
             Chan([_ternary(rng, 4092), pm(4092)], 2046, R=2.0),                # arm 1 under a window of 1 500 entries
             Chan([_ternary(rng, 2048), pm(1023)], 1023)]                       # its blocks carry table offsets
    return CancelRig(name, chans, 1.023e6 / FS, 35, windows=[None, [0, 1500], None], slot_of=(0, 1, 2, 0))


def make_record(fmt, seed=2031):
    """NS samples of full-range values: every int8 value, every int16 value that fits (a real int16 record holds 40 009 of the
    65 536: both ends of the range among them), an all-zero stretch."""
    dtype, layout = FORMATS[fmt]
    rng = np.random.default_rng(seed + list(FORMATS).index(fmt))
    info = np.iinfo(dtype)
    nval = NS * (1 if layout == M.REAL else 2)
    x = rng.integers(info.min, info.max + 1, size=nval).astype(dtype)
    every = rng.permutation(np.arange(info.min, info.max + 1))
    every = np.concatenate([[info.min, info.max], every[(every != info.min) & (every != info.max)]])[:nval]
    x[:every.shape[0]] = rng.permutation(every).astype(dtype)
    per = nval // NS
    x[per * ZERO_AT:per * (ZERO_AT + ZERO_LEN)] = 0
    return x


# ---- check_block (csrc/cancel.hip) restated -------------------------------------------------------------------------------------
def avail(chan, window, off):
    """Per arm: the entries a ramp may reach, min(window or table, entries - table_offset)."""
    out = []
    for a, t in enumerate(chan.tables):
        nent = len(t)
        stage = min(window[a], nent) if window and window[a] > 0 else nent
        out.append(min(stage, nent - off[a]))
    return out


def refusal(chan, window, nsamp, n, s0, rem, step, off=None, f=0.0, phi=0.0):
    """check_block's numeric conditions in its order: the class of the refusal (STATUS has its status), or None."""
    off = off or [0] * len(chan.tables)
    for a, t in enumerate(chan.tables):
        if off[a] < 0 or off[a] + 3 > len(t):
            return "offset"
    if n <= 0 or s0 < 0 or not step > 0 or not rem > -1.0 or not math.isfinite(f) or not math.isfinite(phi):
        return "descriptor"
    if s0 + n > nsamp:
        return "range"
    av = avail(chan, window, off)
    for a, m in enumerate(chan.mult):
        tmin = rem * chan.R * m
        if not math.ceil(tmin) >= 0.0:
            return "low"
        tmax = ((n - 1) * step + rem) * chan.R * m
        if not math.ceil(tmax) <= av[a] - 1:
            return "table_end"
    return None


def rem_min(chan):
    """The most negative rem check_block lets through: rem > -1 and ceil(rem * R * m) >= 0 for every arm."""
    ok = lambda r: r > -1.0 and all(math.ceil(r * chan.R * m) >= 0.0 for m in chan.mult)      # noqa: E731
    r = max(-1.0, -1.0 / chan.K)
    while not ok(r):
        r = float(np.nextafter(r, np.inf))
    while ok(float(np.nextafter(r, -np.inf))):
        r = float(np.nextafter(r, -np.inf))
    return r


def rem_top(chan, window, n, step, off=None):
    """The largest rem that keeps ceil(tmax) <= avail - 1 on every arm, next to this length, step and offsets."""
    off = off or [0] * len(chan.tables)
    ok = lambda r: refusal(chan, window, n, n, 0, r, step, off) is None                        # noqa: E731
    lo = 0.0 if ok(0.0) else rem_min(chan)
    hi = min((av - 1) / (chan.R * m) for av, m in zip(avail(chan, window, off), chan.mult)) - (n - 1) * step + 1.0
    assert ok(lo) and not ok(hi), (n, step, lo, hi)
    while True:                                             # tmax does not decrease with rem: bisect down to neighbouring doubles
        mid = lo + (hi - lo) / 2.0
        if not lo < mid < hi:
            break
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    assert ok(lo) and not ok(float(np.nextafter(lo, np.inf)))
    return lo


def rate_step(rig, chan, name):
    if name == "one":
        return B.step_at(chan, 1.0)
    if name == "2^-16":
        return B.step_at(chan, 2.0 ** -16)
    if name == "nominal":
        return rig.step0
    return {"0.999": 0.999, "0.5": 0.5, "0.2": 0.2, "1/64": 1.0 / 64, "2^-40": 2.0 ** -40, "3.5": 3.5}[name] / chan.K


def blocks_of(engine, descs):
    b = engine.make_blocks(len(descs))
    for k, d in enumerate(descs):
        b[k].channel, b[k].blksize, b[k].first_sample = d["ch"], d["n"], d["s0"]
        b[k].rem_code_phase, b[k].code_phase_step, b[k].el_spacing = d["rem"], d["step"], d.get("d", 0.37)    # el_spacing is ignored
        b[k].carr_freq, b[k].rem_carr_phase = d["f"], d["phi"]
        for a, o in enumerate(d.get("off") or ()):
            b[k].table_offset[a] = int(o)
    return b


# ---- generator -----------------------------------------------------------------------------------------------------------------
class CancelSweep:
    """cases: every descriptor generated; calls: [(label, [case, ...]), ...] the inside ones as they are sent (a case is also the
    model's block: keys ch, s0, n, rem, step, f, phi, off); refused: the ones sent alone; shuffled: label -> the same call in
    another order."""

    def __init__(self, rig, fmt):
        self.rig, self.fmt = rig, fmt
        self.nsamp = NS
        self.rng = np.random.default_rng(9000 + 10 * rig.seed + list(FORMATS).index(fmt))
        self.cases, self.calls, self.refused = [], [], []
        self.queue = {s: [] for s in range(PACK_SLOTS)}        # slot -> inside cases waiting for the packer
        self.turn = {}

    # -- one descriptor
    def slot_for(self, logical):
        slots = [s for s in range(PACK_SLOTS) if self.rig.logical(s) == logical]
        k = self.turn.get(logical, 0)
        self.turn[logical] = k + 1
        return slots[k % len(slots)]

    def case(self, n, chan=0, rem="0", rate="nominal", step=None, f=None, phi=None, off=None, pin=None, s0=None, slot=None, queue=True,
             **tags):
        rig, rng = self.rig, self.rng
        ch = rig.chans[chan]
        window = rig.windows[chan]
        cell = (rem if isinstance(rem, str) else "other", rate if step is None else "other")
        if step is None:
            step = rate_step(rig, ch, rate)
            if rate == "nominal":
                step *= 1 + float(rng.uniform(-3e-6, 3e-6))
        if rem == "top":
            rem = rem_top(ch, window, n, step, off)
        elif rem == "min":
            rem = rem_min(ch)
        elif isinstance(rem, str):
            rem = {"0": 0.0, "+1e-13": 1e-13, "-1e-13": -1e-13, "-0.4": -0.4, "1000.25": 1000.25, "1000.5": 1000.5}[rem]
        c = dict(id=len(self.cases), ch=self.slot_for(chan) if slot is None else slot, chan=chan, n=int(n), s0=s0, rem=float(rem),
                 step=float(step), f=IF + float(rng.uniform(-5e3, 5e3)) if f is None else float(f),
                 phi=float(rng.uniform(-3, 3)) if phi is None else float(phi), off=None if off is None else [int(o) for o in off],
                 pin=pin, cell=cell, tags=tags)
        why = refusal(ch, window, self.nsamp, c["n"], 0 if s0 is None else s0, c["rem"], c["step"], c["off"], c["f"], c["phi"])
        if why is not None:
            c["kind"], c["refuse"] = "refused", why
            if c["s0"] is None:
                c["s0"] = int(rng.integers(0, max(1, self.nsamp - max(c["n"], 0))))
            self.refused.append(c)
        elif not M.oracle_ok(c, {"r": ch.R}):
            c["kind"] = "outside"
        else:
            c["kind"] = "inside"
            if queue:
                self.queue[c["ch"]].append(c)
        self.cases.append(c)
        return c

    def fits(self, n, chan, rem, rate, off=None):
        ch = self.rig.chans[chan]
        step = rate_step(self.rig, ch, rate) * (1 + 3e-6 if rate == "nominal" else 1)
        if rem == "top":
            return refusal(ch, self.rig.windows[chan], n, n, 0, 0.0, step, off) is None
        r = rem_min(ch) if rem == "min" else float(rem.replace("+", "")) if isinstance(rem, str) else rem
        return refusal(ch, self.rig.windows[chan], n, n, 0, max(r, 0.0), step, off) is None

    # -- the packer
    def pack(self, label):
        """The queued cases as calls: per slot end to end with gaps from GAPS, a new lane where the record is full or a pinned
        position asks for one; call k is lane k of every slot."""
        lanes = {}
        for s, cases in self.queue.items():
            zero = [c for c in cases if c["pin"] == "zero"]
            last = [c for c in cases if c["pin"] == "end"]
            rest = [c for c in cases if c["pin"] not in ("zero", "end")]
            lanes[s] = []
            while zero or last or rest:
                lane, cur = [], 0
                if zero:
                    lane.append(zero.pop(0))
                    lane[0]["s0"], cur = 0, lane[0]["n"]
                end = last.pop(0) if last and cur <= self.nsamp - last[0]["n"] else None
                limit = self.nsamp - (end["n"] if end else 0)
                while rest:
                    c = rest[0]
                    s0 = cur + GAPS[int(self.rng.integers(0, 4))]
                    if c["pin"] is not None:
                        s0 += (c["pin"] - s0) % 16
                    if s0 + c["n"] > limit:
                        break
                    c["s0"], cur = int(s0), s0 + c["n"]
                    lane.append(rest.pop(0))
                if end:
                    end["s0"] = self.nsamp - end["n"]
                    lane.append(end)
                assert lane, (s, rest[0] if rest else None)
                lanes[s].append(lane)
            self.queue[s] = []
        for k in range(max(len(v) for v in lanes.values())):
            call = [c for s in sorted(lanes) if k < len(lanes[s]) for c in lanes[s][k]]
            if call:
                self.calls.append((f"{label}{k}", call))

    def build(self):
        rig, rng = self.rig, self.rng
        nlog = len(rig.chans)
        # the whole record as one block of 20 chunks, at two rates
        self.case(self.nsamp, rem=0.25, rate="1/64", pin="zero", whole=True, must=True)
        self.case(self.nsamp, rem="0", rate="2^-16", pin="zero", whole=True, must=True)
        # block length x channel, at the receiver's rate
        for i, n in enumerate(LENGTHS):
            chan = i % nlog if self.fits(n, i % nlog, 1.0, "nominal") else 0
            self.case(n, chan=chan, rem=float(rng.uniform(0, 0.9)))
        # rem class x rate class on channel 0: four lengths that fit, walking through LENGTHS.  (2^-40 entries per sample next to a
        # rem of a thousand chips is a step below rem's ulp: MATLAB's colon has N - 1 elements about as often as not, so one length.)
        at = 0
        for rem in REMS:
            for rate in RATES:
                found, want = 0, 1 if rate == "2^-40" and rem in ("1000.25", "1000.5", "top") else 4
                for j in range(len(LENGTHS)):
                    n = LENGTHS[(at + 7 * j) % len(LENGTHS)]
                    if self.fits(n, 0, rem, rate):
                        self.case(n, rem=rem, rate=rate)
                        found += 1
                        if found == want:
                            at += 7 * (j + 1)
                            break
                assert found == want, (rig.name, rem, rate)
        # more than one entry per sample: 3.5, on blocks short enough to stay inside the table
        for n in (1, 2, 17, 33, 65, 129, 257):
            for rem in ("0", "min", "top", 0.3):
                self.case(n, rem=rem, rate="3.5", fast=True)
        # a block inside one table entry at the receiver's length
        self.case(4097, rem=0.25 / rig.chans[0].K, rate="2^-16", one_entry=True, must=True)
        # carrier
        for f in F_SET:
            for phi in PHI_SET:
                self.case(65, rem=0.3, f=f, phi=phi)
            self.case(4097, rem=0.3, f=f, phi=1e4)
        # position: sample 0, the record's last sample, every residue of 16 with lengths 1..17
        for n in (1, 17, 4097):
            self.case(n, rem=float(rng.uniform(0, 0.9)), pin="zero")
            self.case(n, rem=float(rng.uniform(0, 0.9)), pin="end")
        for r in range(16):
            for n in range(1, 18):
                self.case(n, chan=(r + n) % nlog, rem=float(rng.uniform(0, 0.9)), pin=r)
        # the all-zero stretch is covered by whatever the packer puts there; E == 0: a block inside a run of zero entries
        if rig.name == "wide":
            self.wide()
        self.refusals()
        self.pack("packed")
        self.named()
        assert all(c["kind"] == "inside" for c in self.cases if c["tags"].get("must")), rig.name
        return self

    def wide(self):
        rig, rng = self.rig, self.rng
        for n in (1, 2, 3, 5, 33):                           # inside the run of zeros at entries 100..140: E == 0
            self.case(n, chan=0, rem=105.0, must=True, zeros=True)
        ch1, ch2 = rig.chans[1], rig.chans[2]
        for n in (1, 17, 65, 1025, 4097):                    # the windowed arm: up to the window's last entry
            self.case(n, chan=1, rem="top", windowed=True, must=n == 1)
            self.case(n, chan=1, rem=float(rng.uniform(0, 0.9)), windowed=True)
        n0, n1 = len(ch2.tables[0]), len(ch2.tables[1])
        for off in ([1, 1], [1023, 0], [0, 500], [n0 - 3, n1 - 3], [n0 - 3, 0], [700, 1]):
            for n in (1, 2, 17, 257):
                for rem in ("0", "top", 0.4):
                    if self.fits(n, 2, rem, "nominal", off):
                        self.case(n, chan=2, rem=rem, off=off, offset=True, largest=off[0] == n0 - 3)

    def refusals(self):
        """Either side of every limit of check_block; the accepted sides are the cells "min" and "top" and these."""
        rig = self.rig
        ch0 = rig.chans[0]
        for c, ch in enumerate(rig.chans):                  # K == 1: rem > -1 is all there is, the class "low" cannot be reached
            if ch.K > 1:
                self.case(33, chan=c, rem=float(np.nextafter(rem_min(ch), -np.inf)), side="low")
                self.case(33, chan=c, rem=-0.9, side="low")
                self.case(33, chan=c, rem="min", must=True, side_ok="low")
        self.case(33, rem=-1.0, side="descriptor")
        self.case(33, rem=-7.5, side="descriptor")
        self.case(0, rem=0.1, side="descriptor")
        self.case(33, rem=0.1, step=0.0, side="descriptor")
        self.case(33, rem=0.1, step=-rig.step0, side="descriptor")
        self.case(33, rem=0.1, f=math.inf, side="descriptor")
        self.case(33, rem=0.1, phi=math.nan, side="descriptor")
        self.case(33, rem=0.1, s0=-1, side="descriptor")
        for n, rate in ((1, "nominal"), (257, "one"), (4097, "2^-16"), (33, "3.5")):
            step = rate_step(rig, ch0, rate)
            top = rem_top(ch0, rig.windows[0], n, step)
            self.case(n, rem=float(np.nextafter(top, np.inf)), step=step, side="table_end")
            self.case(n, rem=top, step=step, side_ok="table_end")
            self.case(n, rem=2.0 * top, step=step, side="table_end")
        self.case(self.nsamp, rem=0.1, pin="zero", side="table_end" if not self.fits(self.nsamp, 0, 0.1, "nominal") else "none")
        for n, s0 in ((33, self.nsamp - 32), (1, self.nsamp), (self.nsamp, 1), (65, 2 ** 40)):
            self.case(n, rem=0.1, rate="2^-16", s0=s0, side="range")
        k = len(ch0.tables)
        self.case(33, rem=0.1, off=[-1] + [0] * (k - 1), side="offset")
        self.case(33, rem=0.1, off=[0] * (k - 1) + [len(ch0.tables[-1]) - 2], side="offset")
        self.case(1, rem=0.0, step=2.0 ** -40, off=[len(t) - 3 for t in ch0.tables], queue=False, alone=True, must=True, side_ok="offset")

    def named(self):
        """The calls the packer would not produce by chance."""
        rig, rng = self.rig, self.rng
        # 64 channels over the same 300 samples
        call = []
        for s in range(MAX_CHANNELS):
            c = self.case(300, chan=rig.logical(s), rem=float(rng.uniform(0, 0.9)), s0=20003, slot=s, queue=False, many=True)
            if c["kind"] == "inside":
                call.append(c)
        self.calls.append(("chan64", call))
        # a last offset block on its own (the largest table_offset of channel 0's tables)
        alone = [c for c in self.cases if c["tags"].get("alone") and c["kind"] == "inside"]
        for c in alone:
            c["s0"] = 77
            self.calls.append(("alone", [c]))
        # one channel of 4 100 adjacent blocks of 1..3 samples
        call, cur = [], 5
        for _ in range(4100):
            c = self.case(int(rng.integers(1, 4)), rem=float(rng.uniform(0, 0.9)), s0=cur, slot=0, queue=False, tiny=True)
            if c["kind"] == "inside":
                call.append(c)
                cur += c["n"]
        self.calls.append(("tiny4100", call))
        # 3 000 tiny blocks in the first 8 000 samples, then one block of 20 000: the mean-length guess misses
        call, cur = [], 0
        for _ in range(3000):
            c = self.case(int(rng.integers(1, 4)), rem=float(rng.uniform(0, 0.9)), s0=cur + int(rng.integers(0, 2)), slot=0, queue=False, tiny=True)
            if c["kind"] == "inside":
                call.append(c)
                cur = c["s0"] + c["n"]
        assert cur <= 8000, cur
        call.append(self.case(20000, rem=0.25, rate="1/64", s0=8000 + int(rng.integers(0, 50)), slot=0, queue=False, must=True))
        self.calls.append(("tiny3000+big", call))
        self.shuffled = {"tiny3000+big": [int(i) for i in rng.permutation(len(call))]}

    # ---- what the sweep must satisfy to prove something ------------------------------------------------------------------------
    def counts(self):
        kinds = [c["kind"] for c in self.cases]
        return {k: kinds.count(k) for k in ("inside", "refused", "outside")}

    def sent(self):
        return [c for _, call in self.calls for c in call]

    def check_caps(self):
        n = self.counts()
        assert len(self.cases) == n["inside"] + n["refused"] + n["outside"]
        assert n["outside"] <= OUTSIDE_CAP * len(self.cases), (self.rig.name, self.fmt, n)
        sent = self.sent()
        assert len({c["id"] for c in sent}) == len(sent) == n["inside"], (self.rig.name, self.fmt, len(sent), n)
        want = set(CLASSES) - (set() if any(ch.K > 1 for ch in self.rig.chans) else {"low"})
        assert {c["refuse"] for c in self.refused} == want, (self.rig.name, {c["refuse"] for c in self.refused})
        for c in self.refused:                              # a refusal meant for one class lands in it
            side = c["tags"].get("side")
            assert side is None or side == "none" or c["refuse"] == side, c
        for label, call in self.calls:                      # no two blocks of a slot overlap; everything lies in the record
            per = {}
            for c in call:
                assert 0 <= c["s0"] and c["s0"] + c["n"] <= self.nsamp, (label, c)
                per.setdefault(c["ch"], []).append((c["s0"], c["s0"] + c["n"]))
            for spans in per.values():
                spans.sort()
                assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), label


def amplitudes(sweep, call, dtype, seed):
    """Given amplitudes of a call: random doubles (not dyadic: no model value sits on a half-integer by construction), large
    enough to clip now and then, smaller where many channels overlap."""
    rng = np.random.default_rng(seed)
    scale = 25.0 * (256.0 if dtype == np.int16 else 1.0) / max(1.0, len({c["ch"] for c in call}) / 8.0)
    a = scale * (rng.uniform(-1, 1, (len(call), 3)) + 1j * rng.uniform(-1, 1, (len(call), 3)))
    for k, c in enumerate(call):
        a[k, len(sweep.rig.chans[c["chan"]].tables):] = 0.0
    return a


# ---- the exact class ------------------------------------------------------------------------------------------------------------
def exact_call(rig, fmt):
    """A call whose every product and sum is exact in float64: carr_freq = 0 and rem_carr_phase = 0 (sincos exact), amplitudes
    multiples of 1/4, tables of -1, 0, +1.  Four slots cover the record with blocks of many lengths; the amplitudes of every eighth
    block are large enough to clamp at either end of the dtype.  Returns (blocks, given amplitudes complex [nblocks, 3])."""
    dtype, _ = FORMATS[fmt]
    rng = np.random.default_rng(5000 + rig.seed + list(FORMATS).index(fmt))
    big = float(np.iinfo(dtype).max)
    blocks, amps = [], []
    for s in range(PACK_SLOTS):
        ch, cur = rig.chan(s), int(rng.integers(0, 3)) if s else 0
        while cur < NS:
            n = min(int(rng.choice([1, 2, 3, 16, 17, 64, 255, 1024, 2049])), NS - cur)
            step = rig.step0
            blk = dict(ch=s, chan=rig.logical(s), s0=cur, n=n, rem=float(rng.integers(0, 4)) / 4.0, step=step, f=0.0, phi=0.0, off=None)
            assert refusal(ch, rig.windows[rig.logical(s)], NS, n, cur, blk["rem"], step) is None
            if M.oracle_ok(blk, {"r": ch.R}):
                a = np.zeros(3, dtype=np.complex128)
                mag = 2.5 * big if len(blocks) % 8 == 7 else 12.0 * (256.0 if dtype == np.int16 else 1.0)
                arms = len(ch.tables)
                a[:arms] = (np.rint(4 * rng.uniform(-mag, mag, arms)) + 1j * np.rint(4 * rng.uniform(-mag, mag, arms))) / 4.0
                blocks.append(blk)
                amps.append(a)
            cur += n + int(rng.integers(0, 2))
    return blocks, np.array(amps)


def exact_values(raw, dtype, layout, blocks, chans, amp, mode):
    """The exact class's values before rounding, per component [NS, 1 or 2] in file order - exact, so computed here in float64
    with nothing left to round: y = x - M or M."""
    re, im = M.components(raw, layout)
    m_re, m_im = np.zeros(NS), np.zeros(NS)
    for k, blk in enumerate(blocks):
        _, _, c = M.replica(blk, chans[blk["ch"]], FS)
        sl = slice(blk["s0"], blk["s0"] + blk["n"])
        for a in range(c.shape[0]):
            m_re[sl] += c[a] * amp[k, a].real * (2.0 if layout == M.REAL else 1.0)
            m_im[sl] += c[a] * amp[k, a].imag
    y_re, y_im = (m_re, m_im) if mode == "model" else (re - m_re, im - m_im)
    if layout == M.REAL:
        return y_re[:, None]
    return np.stack([y_im, y_re] if layout == M.QI else [y_re, y_im], axis=1)
