"""Every epoch of the closed loops (gc_track, gc_track_device) against the float64 oracle of its own block: tests/loop_epochs.py.

The closed loops run their own instantiations of the fast, lane, multi-transition, CBOC and mixed kernels, cut every block over a
team of workgroups and add the partial sums in double in a fixed order (csrc/devloop.h); gc_correlate and replay reach none of it.
The trajectory tests (test_gpu_ref_vectors.py, test_gpu_tracking.py) bound these loops with room for drift; here the oracle is
teacher-forced with the loop's own recorded sums, so each epoch is judged on the descriptor the loop really used:

  sums    |recorded - float64| <= 2e-6 * sum(|I_n| + |Q_n|) of the block, per output (test_gpu_correlator.py TOL; a folded pilot:
          times the sum of the fold's absolute coefficients)
  state   absoluteSample equal (GPS L2C < 1e-6), the eight fields of test_loop_closure_cpu._CHECKED within 1e-10 of max|want|
  nothing sampled, nothing skipped: compared == the epochs_done the library reports, summed over the channels

a. all 16 scenes of ref_scenes.TRACK_SCENES on the host loop and the device loop; GPS L1 C/A also with a launch per epoch and with
   three host threads (tuning build); the Galileo E1-C CBOC pilot (fold 5) across one C/N0 interval.
b. the team sizes the shipping library picks.  Two levers only, channel count and block length; the compute-unit count comes from
   engine.device_info() and the expected team from the formulae of csrc/track_plan.h, mirrored in tests/track_teams.py and held against
   gc_debug_last_track_team.  Fast device loop: ceil(4 CU / nch) over six values from 256 channels (4 on 256 CUs) to 32; blocks so
   short that chunks / 32 limits the team to 1, 2, 3, 6, 12.  The fast kernel needs more than 7 samples per chip, so a 1023-chip
   block never has fewer than 28 teams' worth of chunks: the short blocks are the first 50 .. 400 chips of the C/A code at 16 and
   at 8 samples per chip (16- and 8-sample lane-chunks).  Lane device loop: the channel counts where 2 CU / nch = 2, 4, 5 and the
   cap of 6 (256 channels among them; a grid that is not resident whole is halved, the team that ran is what the accessor tells)
   and four channels on blocks of blksize / 1024 = 2, 4, 5 and 6 members.  Host persistent loop: chunks_nominal / 48 = 1, 2, 4, 8
   on the same short blocks.
c. one fast rig and one lane rig on the six encodings of one record (int8 / int16 x I/Q, Q/I, real; int16 values x 37).

Measured on the MI355X (256 CUs), worst error / bound of the sums and worst state difference (relative to max|want|, bound 1e-10),
every case also printed by test_zz_worst_ratios:
  16 scenes, host loops (teams 4 .. 32)         sums 0.006 (GPS_L1CA_real, BDS_B1I, GLO_GL1)   state 5.5e-16
  16 scenes, device loops (teams 4 .. 32)       sums 0.007 (GPS_L1CA_real)                     state 5.5e-16
  CBOC pilot, host and device (team 4)          sums 0.001                                     state < 1e-15
  fast device loop, 256 .. 33 channels          sums 0.004; teams 4, 5, 8, 11, 13, 16 ran (formula 4, 10, 15, 21, 26, 32, halved to fit); state 5.3e-15
  fast device loop, short blocks                sums 0.011 (50 chips x 16); teams 1, 2, 3, 6, 12
  fast host loop, short blocks                  sums 0.011 (50 chips x 16); teams 1, 1, 2, 4, 8
  lane device loop, 256 .. 85 channels          sums 0.002; teams 1, 2, 2, 2 ran (formula 2, 4, 5, 6, halved to fit)
  lane device loop, blocks of 2 500 .. 18 000   sums 0.003; teams 2, 4, 5, 6
  six encodings, lane host / device, fast device   sums 0.002
  six encodings, fast host loop                 sums 0.002.  Before the fix that came with this module the int16 I/Q, int16 Q/I, int8 real
      and int16 real runs were wrong in ONE epoch: epoch 0 of channel 0 (block at sample 0 of the record, rem 0, team 23, 8-sample
      lane-chunks), I_P 47.04 x and Q_P 17.42 x the bound (int16), I_P 94.05 x (real) - one sample's worth on the prompt pair.  With
      rem = 0 the prompt ramp is exactly 341 at sample 6000, the first sample of a lane-chunk that lane reaches in its second
      iteration; the 64-bit ramp sat a hair above the edge there, the reference's rounded double on it, and the fast kernel's near-tie
      filter (csrc/corr_fast.hip) looked at transitions ahead of the chunk's first sample only.  It now also sends a chunk whose first
      sample lies within its tolerance BEHIND an edge to the exact path."""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import loop_epochs as LE
import ref_scenes as RS
import test_gpu_ref_vectors as TRV
from track_teams import _fast_device_team, _fast_host_team, _halvings, _lane_device_team, _lowrate
from oracle import gnss_oracle as O

pytestmark = pytest.mark.gpu

WORST = {}          # case -> (team, compared, worst sum ratio, worst state ratio)
PRNS = (7, 14, 22, 31)


def _run(engine, ch, S, signal, device_loop):
    """receiver.tracking with all six pilot sums recorded, plus the epochs_done of every entry of `ch`."""
    from cu_sdr_collection_amd import receiver as R
    job = R._tracking_prepare(engine, ch, S, signal, "all")
    fields, done, st = engine.track(job.p, job.inits, device_loop=device_loop)
    tr, _ = R._tracking_finish(job, fields, done, st)
    n_done = [0] * len(ch)
    for k, i in enumerate(job.active):
        n_done[i] = int(done[k])
    return tr, n_done, st, job


def _judge(name, engine, spec, rec, layout, ch, S, tr, n_done, n_ep):
    active = [i for i, c in enumerate(ch) if c.status != "-"]
    assert [n_done[i] for i in active] == [n_ep] * len(active) and all(tr[i].status == "T" for i in active), (name, n_done)
    res = LE.check(spec, rec, layout, ch, S, tr, done=n_done)
    WORST[name] = (engine.last_track_team(), res.compared, res.worst_sum, res.worst_state)
    print(f"\n[loop epochs] {name}: mode {engine.last_track_mode()}, kernel {engine.last_kernel()}, team {engine.last_track_team()}; {LE.describe(res)}")
    assert res.compared == sum(n_done) == n_ep * len(active) > 0, (name, res.compared, n_done)
    assert res.failures == [], (name, res.failures[:8], len(res.failures))
    return res


# ---- a. every scene, every loop, every epoch ---------------------------------------------------------------------------------------
_CASES = [(sc, dl) for sc in RS.TRACK_SCENES for dl in (False, True) if not dl or sc.name in TRV._DEVICE_LOOP_SCENES]


@pytest.mark.parametrize("sc,device_loop", _CASES, ids=[f"{sc.name}-{'device' if dl else 'host'}" for sc, dl in _CASES])
def test_every_epoch_of_every_scene(engine, sc, device_loop):
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import signals
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    tr, n_done, st, job = _run(engine, ch, S, sc.signal, device_loop)
    assert st == 0
    if device_loop:
        assert engine.last_track_mode() == 2
    elif sc.name == "GPS_L1CA":
        assert engine.last_track_mode() == 1 and engine.last_kernel() == 1
    _judge(f"{sc.name} {'device' if device_loop else 'host'}", engine, sc, rec, layout, ch, S, tr, n_done, signals.epochs_to_process(S))


@pytest.mark.tuning
@pytest.mark.parametrize("knob", [("GC_TRACK_PERSIST", "0", 0), ("GC_TRACK_THREADS", "3", 1), ("GC_TRACK_LOCKSTEP", "1", 1)], ids=lambda k: k[0])
def test_every_epoch_of_the_other_host_loops(engine, monkeypatch, knob):
    """GPS L1 C/A with a correlator launch per epoch, with the channels dealt out to three host threads, and in lock step."""
    import cu_sdr_collection_amd as P
    sc = RS.TRACK_SCENES[0]
    S, rec, layout, ch = RS.scene_inputs(P, sc)
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    monkeypatch.setenv(knob[0], knob[1])
    tr, n_done, st, _ = _run(engine, ch, S, sc.signal, False)
    monkeypatch.delenv(knob[0])
    assert st == 0 and engine.last_track_mode() == knob[2]
    _judge(f"GPS_L1CA host {knob[0]}={knob[1]}", engine, sc, rec, layout, ch, S, tr, n_done, int(S.msToProcess))


@functools.lru_cache(maxsize=None)
def _cboc_rig():
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd.settings import initSettings_GAL_E1C
    S = initSettings_GAL_E1C()
    S.pilotTRKflag = 1
    S.dllCorrelatorSpacing = 0.05   # narrow correlator: spacing * 12 table entries per chip must stay below one entry
    S.CNo.VSMinterval = 4           # one C/N0 record inside ...
    S.msToProcess = 20              # ... 5 epochs of 4 ms
    S.numberOfChannels = 2
    fs = S.samplingFreq
    rng = np.random.default_rng(18)
    sats = [P.synth.SatSpec(prn=p, doppler=float(rng.uniform(-3e3, 3e3)), code_phase_samples=float(rng.uniform(0, 72000)),
                            carrier_phase=float(rng.uniform(0, 6.28)), cn0_dbhz=48.0) for p in (7, 23)]
    iq = P.synth.generate_if(sats, int(0.030 * fs), fs, S.IF, P.codes.generateE1Bcode, 2 * S.codeFreqBasis, 8184, seed=22,
                             bit_periods=1, pilot_fn=P.codes.generateE1Ccode)
    ch = [SimpleNamespace(PRN=s.prn, acquiredFreq=S.IF + s.doppler + 2.0, status="T", codePhase=int(np.ceil(s.code_phase_samples)) + 1) for s in sats]

    def tables(prn):
        c11 = O.generate_e1_code(prn, "C")                      # chip x [+1, -1]
        c61 = (c11[0::2][:, None] * np.tile(np.array([1, -1], dtype=np.int8), 6)[None, :]).reshape(-1)
        return [O.pad_code(O.generate_e1_code(prn, "B")), O.pad_code(c11), O.pad_code(c61)]
    spec = LE.generic_spec(tables=tables, r=2.0, pll="3state", coef_variant="a", pilot_combine=5, code_freq_from_channel=False, arm_mult=[1.0, 1.0, 6.0])
    return S, iq, ch, spec


@pytest.mark.parametrize("device_loop", [False, True], ids=["host", "device"])
def test_every_epoch_of_the_cboc_pilot_loop(engine, device_loop):
    """Galileo E1-C with its CBOC(6,1,1/11) subcarrier: three arms, the third derived in the lane kernel, the pilot folded (mode 5)."""
    S, iq, ch, spec = _cboc_rig()
    engine.load_if(iq, fs=S.samplingFreq)
    tr, n_done, st, _ = _run(engine, ch, S, "GAL_E1C_CBOC", device_loop)
    assert st == 0 and engine.last_kernel() == 0 and engine.last_track_mode() == (2 if device_loop else 1)
    assert all(len(t.CNo.VSMValue) == 1 and t.CNo.VSMIndex == [4] for t in tr)
    _judge(f"GAL_E1C_CBOC {'device' if device_loop else 'host'}", engine, spec, iq, RS.GC_IQ, ch, S, tr, n_done, 5)


# ---- b. team sizes -----------------------------------------------------------------------------------------------------------------
# csrc/launch_plan.h gc_block_lowrate_level and csrc/track_plan.h's team formulae, restated in tests/track_teams.py: what the accessor
# must report
def _channels(S, nch, span, code_freq=False):
    """nch channels over four PRNs, first blocks on every residue mod 16, acquiredFreq spread over +-5 kHz."""
    ch = []
    for k in range(nch):
        cp = 1 + ((k * 1129) % span) // 16 * 16 + k % 16
        f = S.IF + (-5e3 + 1e4 * k / max(1, nch - 1))
        c = SimpleNamespace(PRN=PRNS[k % 4], acquiredFreq=f, codePhase=cp, status="T")
        if code_freq:
            c.codeFreq = S.codeFreqBasis + (f - S.IF) / S.carrFreqBasis * S.codeFreqBasis
        ch.append(c)
    assert nch < 16 or {(c.codePhase - 1) % 16 for c in ch} == set(range(16))
    return ch


@functools.lru_cache(maxsize=None)
def _ca_rig(chips, spc, n_ep):
    """The first `chips` chips of the C/A codes at `spc` samples per chip, one block per millisecond: (settings, int8 I/Q record)."""
    import cu_sdr_collection_amd as P
    S = P.initSettings()
    S.codeLength, S.codeFreqBasis = chips, chips * 1e3
    S.samplingFreq = float(round(spc * chips * 1e3))
    S.msToProcess = n_ep
    fs = S.samplingFreq
    rng = np.random.default_rng(100 + chips)
    sats = [P.synth.SatSpec(prn=p, doppler=float(rng.uniform(-4e3, 4e3)), code_phase_samples=float(rng.uniform(0, fs * 1e-3)),
                            carrier_phase=float(rng.uniform(0, 6.28)), cn0_dbhz=47.0) for p in PRNS]
    iq = P.synth.generate_if(sats, int((n_ep + 2.5) * 1e-3 * fs), fs, S.IF, lambda prn: P.codes.generateCAcode(prn)[:chips], S.codeFreqBasis, chips, seed=7)
    return S, iq


def _team_case(engine, name, S, rec, ch, signal, spec, device_loop, want_team, want_kernel, layout=RS.GC_IQ):
    """`want_team`: the team that must have run, or a list of which it must be one."""
    S = copy.copy(S)
    S.numberOfChannels = len(ch)
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    tr, n_done, st, _ = _run(engine, ch, S, signal, device_loop)
    assert st == 0 and engine.last_track_mode() == (2 if device_loop else 1), (name, st, engine.last_track_mode())
    team = engine.last_track_team()
    assert engine.last_kernel() == want_kernel and team in (want_team if isinstance(want_team, list) else [want_team]), (name, engine.last_kernel(), team, want_team)
    from cu_sdr_collection_amd import signals
    _judge(name, engine, spec, rec, layout, ch, S, tr, n_done, signals.epochs_to_process(S))
    return team


def _spread(values, count):
    """`count` of the sorted distinct values, the ends included."""
    v = sorted(set(values))
    return sorted({v[round(i * (len(v) - 1) / (count - 1))] for i in range(count)}) if len(v) > count else v


@pytest.mark.parametrize("slot", range(6))
def test_fast_device_loop_teams_by_channel_count(engine, slot):
    """L1 C/A at 18 Msps, 12 epochs: team = ceil(4 CU / nch), from GC_MAX_CHANNELS = 256 channels (the smallest team) up to the cap of 32.
    Teams are laid out eight channels to an XCD, so ceil(nch / 8) * 8 * team one-wave workgroups must be resident at once: on 256 CUs
    256 x 4 are, 113 x 10 .. 33 x 32 are not and run halved (5, 8, 11, 13, 16 - six distinct team sizes all the same; the scenes above run
    two channels on teams of 32).  The team that ran must lie on the formula's halving chain, and be the formula's own at 256 channels."""
    cu = engine.device_info()[1]
    S, iq = _ca_rig(1023, 18e6 / 1.023e6, 12)
    by_team = {}
    for nch in range(1, 257):
        by_team[_fast_device_team(cu, nch, S)] = nch                       # the largest channel count of every team size
    teams = _spread(by_team, 6)
    assert len(teams) == 6 and teams[0] == _fast_device_team(cu, 256, S) >= 1 and teams[-1] == 32, (cu, teams)
    team = teams[slot]
    ran = _team_case(engine, f"fast device loop, {by_team[team]} channels", S, iq, _channels(S, by_team[team], 17000), "GPS_L1CA", LE.l1ca_spec(), True,
                     [team] if slot == 0 else _halvings(team), 1)
    assert ran >= 4


_SHORT = [(chips, spc) for chips in (50, 80, 100, 200, 400) for spc in (16, 8)]


@pytest.mark.parametrize("chips,spc", _SHORT, ids=[f"{c}chips-{s}spc" for c, s in _SHORT])
def test_fast_loops_teams_limited_by_the_block_length(engine, chips, spc):
    """Four channels on blocks of 16 (8) x 50 .. 400 samples: the device loop's team is chunks / 32 = 1, 2, 3, 6, 12, the persistent
    host-fed kernel's chunks_nominal / 48 = 1, 1, 2, 4, 8 - on 16-sample lane-chunks (16 samples per chip) and on 8-sample ones."""
    cu = engine.device_info()[1]
    S, iq = _ca_rig(chips, spc, 12)
    ch = _channels(S, 4, int(S.samplingFreq * 1e-3) - 16)
    i = (50, 80, 100, 200, 400).index(chips)
    dev, host = _fast_device_team(cu, 4, S), _fast_host_team(cu, 4, S)
    assert (dev, host) == ((1, 2, 3, 6, 12)[i], (1, 1, 2, 4, 8)[i]) and _lowrate(S.codeFreqBasis * 1.001 / S.samplingFreq) == (2 if spc == 16 else 1)
    _team_case(engine, f"fast device loop, {chips} chips x {spc}", S, iq, ch, "GPS_L1CA", LE.l1ca_spec(), True, dev, 1)
    _team_case(engine, f"fast host loop, {chips} chips x {spc}", S, iq, ch, "GPS_L1CA", LE.l1ca_spec(), False, host, 1)


@functools.lru_cache(maxsize=None)
def _l5_record(n_ep, fs=None):
    """The GPS_L5C scene's signal (I5 + Q5, pilot in quadrature; 18 Msps unless `fs`) with four satellites, n_ep + 2.5 ms long."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import settings as SET
    sc = next(s for s in RS.TRACK_SCENES if s.name == "GPS_L5C")
    S = getattr(SET, sc.settings_fn)()
    for k, v in sc.overrides.items():
        setattr(S, k, v)
    S.msToProcess = n_ep
    if fs is not None:
        S.samplingFreq = fs
    fs = S.samplingFreq
    rng = np.random.default_rng(1031)
    sats = [P.synth.SatSpec(prn=p, doppler=float(rng.uniform(-3e3, 3e3)), code_phase_samples=float(rng.uniform(0, fs * 1e-3)),
                            carrier_phase=float(rng.uniform(0, 6.28)), cn0_dbhz=50.0) for p in PRNS]
    iq = P.synth.generate_if(sats, int((n_ep + 2.5) * 1e-3 * fs), fs, S.IF, P.codes.generateL5Icode, S.codeFreqBasis, 10230, seed=1032,
                             carrier_ratio=1150.0, bit_periods=10, pilot_fn=P.codes.generateL5Qcode, pilot_phase=np.pi / 2)
    return S, iq


@functools.lru_cache(maxsize=None)
def _l5_tables(prn):           # the oracle's loop asks once per channel: 256 channels share four satellites
    return [O.pad_code(O.generate_l5_code(prn, "I")), O.pad_code(O.generate_l5_code(prn, "Q"))]


def _l5_spec(**kw):
    return LE.generic_spec(tables=_l5_tables, r=1.0, pll="3state", coef_variant="a", pilot_combine=1, code_freq_from_channel=True, **kw)


def _lane_case(engine, name, S, iq, ch, teams):
    """One lane device-loop run whose team must be one of `teams`; returns the team that ran."""
    S = copy.copy(S)
    S.numberOfChannels = len(ch)
    engine.load_if(iq, fs=S.samplingFreq)
    tr, n_done, st, _ = _run(engine, ch, S, "GPS_L5C", True)
    assert st == 0 and engine.last_track_mode() == 2 and engine.last_kernel() == 0, (name, st, engine.last_track_mode(), engine.last_kernel())
    team = engine.last_track_team()
    assert team in teams, (name, team, teams)
    _judge(f"{name}, team {team}", engine, _l5_spec(), iq, RS.GC_IQ, ch, S, tr, n_done, 10)
    return team


@pytest.mark.parametrize("slot", range(4))
def test_lane_device_loop_teams_by_channel_count(engine, slot):
    """GPS L5 I5 + Q5 at 18 Msps, 10 epochs, the channel counts at which 2 CU / nch gives 2, 4, 5 and the two-arm cap of 6 members
    (256, 128, 102 and 85 channels on 256 CUs).  A member workgroup holds two 10 232-entry float tables in LDS, so a grid of 2 CU
    workgroups may not be resident at once; gc_track_device then halves the team until the grid fits, and the accessor reports the
    team that ran: it must lie on the formula's halving chain."""
    cu = engine.device_info()[1]
    S, iq = _l5_record(10)
    by_team = {}
    for nch in range(1, 257):
        by_team[_lane_device_team(cu, nch, 2, 18000)] = nch
    assert [t for t in (2, 4, 5, 6) if t in by_team] == [2, 4, 5, 6], (cu, sorted(by_team))
    team = (2, 4, 5, 6)[slot]
    _lane_case(engine, f"lane device loop, {by_team[team]} channels (2 CU / nch = {team})", S, iq, _channels(S, by_team[team], 17000, code_freq=True), _halvings(team))


@pytest.mark.parametrize("fs,team", [(2.5e6, 2), (4.5e6, 4), (5.5e6, 5), (18e6, 6)], ids=["2.5Msps", "4.5Msps", "5.5Msps", "18Msps"])
def test_lane_device_loop_teams_by_block_length(engine, fs, team):
    """Four channels of the same signal on blocks of 2 500, 4 500, 5 500 and 18 000 samples: members = blksize / 1024 = 2, 4, 5 and the
    cap of 6 - teams small grids run as the formula says."""
    cu = engine.device_info()[1]
    S, iq = _l5_record(10, fs)
    assert _lane_device_team(cu, 4, 2, int(fs * 1e-3)) == team
    _lane_case(engine, f"lane device loop, blocks of {int(fs * 1e-3)}", S, iq, _channels(S, 4, int(fs * 1e-3) - 1000, code_freq=True), [team])


def test_more_channels_than_the_library_holds_are_refused(engine):
    """nch = GC_MAX_CHANNELS + 1 is GC_E_INVALID from both loops, and the context then tracks two channels as before."""
    import cu_sdr_collection_amd as P
    from cu_sdr_collection_amd import _lib as L
    from cu_sdr_collection_amd import receiver as R
    S, iq = _ca_rig(1023, 18e6 / 1.023e6, 12)
    S = copy.copy(S)
    S.numberOfChannels = 2
    ch = _channels(S, 2, 17000)
    engine.load_if(iq, fs=S.samplingFreq)
    job = R._tracking_prepare(engine, ch, S, "GPS_L1CA", "all")
    too_many = [job.inits[k % 2] for k in range(257)]          # GC_MAX_CHANNELS + 1 (include/gnsscorr.h)
    for device_loop in (False, True):
        with pytest.raises(P.GnssCorrError) as err:
            engine.track(job.p, too_many, device_loop=device_loop)
        assert err.value.status == L.GC_E_INVALID
        tr, n_done, st, _ = _run(engine, ch, S, "GPS_L1CA", device_loop)
        assert st == 0
        _judge(f"two channels after a refusal, {'device' if device_loop else 'host'}", engine, LE.l1ca_spec(), iq, RS.GC_IQ, ch, S, tr, n_done, 12)


# ---- c. formats in the loop --------------------------------------------------------------------------------------------------------
FORMATS = ("i8_iq", "i8_qi", "i16_iq", "i16_qi", "i8_real", "i16_real")


def _encode(iq, fmt):
    """tests/test_gpu_record_formats.py's six encodings of an int8 I/Q record; int16 values beyond the int8 range (x 37, test_gpu_variants.py)."""
    if fmt.endswith("real"):
        x, layout = iq[0::2].copy(), RS.GC_REAL
    elif fmt.endswith("qi"):
        x, layout = np.empty_like(iq), RS.GC_QI
        x[0::2], x[1::2] = iq[1::2], iq[0::2]
    else:
        x, layout = iq, RS.GC_IQ
    return (x.astype(np.int16) * np.int16(37) if fmt.startswith("i16") else x), layout


@pytest.mark.parametrize("device_loop", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_fast_loops_on_the_six_encodings(engine, fmt, device_loop):
    cu = engine.device_info()[1]
    S, iq = _ca_rig(1023, 18e6 / 1.023e6, 12)
    S = copy.copy(S)
    S.msToProcess = 10
    rec, layout = _encode(iq, fmt)
    if layout == RS.GC_REAL:
        S.fileType = 1
    ch = _channels(S, 4, 17000)
    i8c = fmt in ("i8_iq", "i8_qi")
    spec = LE.l1ca_spec() if layout != RS.GC_QI else LE.generic_spec(tables=lambda prn: [O.pad_code(O.generate_ca_code(prn))], r=1.0, pll="2nd", pilot_combine=0,
                                                                       code_freq_from_channel=False, swap_iq=True, int16_branch=True)
    team = _fast_device_team(cu, 4, S, i8c) if device_loop else _fast_host_team(cu, 4, S)
    _team_case(engine, f"fast {'device' if device_loop else 'host'} loop, {fmt}", S, rec, ch, "GPS_L1CA", spec, device_loop, team, 1, layout=layout)


@pytest.mark.parametrize("device_loop", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_lane_loops_on_the_six_encodings(engine, fmt, device_loop):
    S, iq = _l5_record(10)
    S = copy.copy(S)
    rec, layout = _encode(iq, fmt)
    if layout == RS.GC_REAL:
        S.fileType = 1
    ch = _channels(S, 4, 17000, code_freq=True)
    spec = _l5_spec(swap_iq=layout == RS.GC_QI, file_type=1 if layout == RS.GC_REAL else 2)
    S.numberOfChannels = 4
    engine.load_if(rec, layout=layout, fs=S.samplingFreq)
    tr, n_done, st, _ = _run(engine, ch, S, "GPS_L5C", device_loop)
    assert st == 0 and engine.last_kernel() == 0 and engine.last_track_mode() == (2 if device_loop else 1)
    _judge(f"lane {'device' if device_loop else 'host'} loop, {fmt}", engine, spec, rec, layout, ch, S, tr, n_done, 10)


def test_zz_worst_ratios():
    """The measured worst error / bound of every case above that ran in this process, one line each."""
    print("\n[loop epochs] case | team | epochs | worst sum ratio (epoch, channel, field) | worst state difference / 1e-10 (epoch, channel, field)")
    for name, (team, n, ws, wt) in WORST.items():
        print(f"[loop epochs] {name} | {team} | {n} | {ws[0]:.3f} ({ws[1]}, {ws[2]}, {ws[3]}) | {wt[0]:.2e} ({wt[1]}, {wt[2]}, {wt[3]})")
    assert WORST
