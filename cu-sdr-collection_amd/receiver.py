"""Host-side mirror of the reference's operator interface for the hot path (GPS L1 C/A package):

    acqResults            = acquisition(longSignal, settings)       GPS/GPS_L1CA/include/acquisition.m:1
    channel               = preRun(acqResults, settings)            GPS/GPS_L1CA/include/preRun.m:1
    [trackResults, chan]  = tracking(fid, channel, settings)        GPS/GPS_L1CA/include/tracking.m:1

Same names, argument meaning, struct fields and error behaviour; the heavy lifting is done by
libgnsscorr.so on the GPU (no CPU path exists here).  `fid` is an Engine whose IF buffer plays
the role of the open file; `longSignal` is identified by its position in that buffer.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from . import _lib as L
from .settings import skip_samples
from . import codes
from .engine import Engine, precision_code


def _round(x: float) -> int:
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


# ---------------------------------------------------------------------------------------------
# C/N0 estimator (host side, Common/CNoVSM.m:38-47)
# ---------------------------------------------------------------------------------------------
def CNoVSM(I, Q, T):
    Z = np.asarray(I) ** 2 + np.asarray(Q) ** 2
    Zm = np.mean(Z)
    Zv = np.var(Z, ddof=1)
    Pav = np.sqrt(complex(Zm ** 2 - Zv))
    Nv = 0.5 * (Zm - Pav)
    return float(10 * np.log10(abs((1 / T) * Pav / (2 * Nv))))


def Calc_CNo_PLD(trackResults, settings, loopCnt, straight_pilot: bool = False):
    """[CNo, PllDetector] = Calc_CNo_PLD(trackResults, settings, loopCnt) of BDS/B2a and BDS/B1C (host side, like CNoVSM):
    variance-summing C/N0 of the data arm, of the pilot arm and of their sum over the last settings.CNoInterval epochs, and
    the narrow-band PLL lock detector NBD/NBP of each arm with the data bits wiped by sign (B2a Calc_CNo_PLD.m:35-97).  The
    pilot prompt pair is read swapped (the pilot is tracked in quadrature) except for the B1C wide-band loop
    (`straight_pilot`; pilotTRKflag == 2 in BDS/B1C/include/Calc_CNo_PLD.m).  CNo[1], PllDetector[1] stay 0 without a pilot."""
    n = int(settings.CNoInterval)
    T = settings.intTime
    sl = slice(loopCnt - n, loopCnt)

    def arm(I, Q):
        Z = I ** 2 + Q ** 2
        Zm = np.mean(Z)
        Zv = np.var(Z, ddof=1)
        Pav = np.sqrt(complex(Zm ** 2 - Zv))          # MATLAB's sqrt of a negative number is complex; abs() below
        Nv = 0.5 * (Zm - Pav)
        lin = abs((1 / T) * Pav / (2 * Nv))
        wiped = np.sum(I[I > 0]) - np.sum(I[I < 0])
        nbp = wiped ** 2 + np.sum(Q) ** 2
        nbd = wiped ** 2 - np.sum(Q) ** 2
        return lin, nbd / nbp

    CNo = np.zeros(3)
    PllDetector = np.zeros(2)
    data, PllDetector[0] = arm(np.asarray(trackResults.I_P[sl], dtype=np.float64), np.asarray(trackResults.Q_P[sl], dtype=np.float64))
    CNo[0] = 10 * np.log10(data)
    pilot = 0.0
    if getattr(settings, "pilotTRKflag", 0) in (1, 2) and hasattr(trackResults, "Pilot_I_P"):
        pi = np.asarray(trackResults.Pilot_I_P[sl], dtype=np.float64)
        pq = np.asarray(trackResults.Pilot_Q_P[sl], dtype=np.float64)
        pilot, PllDetector[1] = arm(pi, pq) if straight_pilot else arm(pq, pi)
        CNo[1] = 10 * np.log10(pilot)
    with np.errstate(divide="ignore"):
        CNo[2] = 10 * np.log10(data + pilot)
    return CNo, PllDetector


# ---------------------------------------------------------------------------------------------
# acquisition
# ---------------------------------------------------------------------------------------------
def _acq_params(settings, first_sample: int) -> L.gc_acq_params:
    p = L.gc_acq_params()
    p.sampling_freq = settings.samplingFreq
    p.code_freq_basis = settings.codeFreqBasis
    p.code_length = settings.codeLength
    p.intermediate_freq = settings.IF
    p.search_band = settings.acqSearchBand
    p.search_step = settings.acqSearchStep
    p.non_coh_time = int(settings.acqNonCohTime)
    p.first_sample = int(first_sample)
    return p


def probeData(fid: Engine, settings, first_sample: int = 0):
    """probeData.m without the figure: the numbers behind its four plots for the 100 code periods from `first_sample` of the loaded
    record (probeData.m:66-76), computed on the device (gc_probe_psd, gc_probe_histogram) - samples in file order as :104 takes them.
      freq, psd      what pwelch(data, 32768, 2048, 32768, fs) returns: fileType 2 the two-sided spectrum over 0 .. fs in Hz (:131);
                     fileType 1 the one-sided one, called with fs / 1e6 (:128) - nfft/2 + 1 bins over 0 .. fs/2 in MHz, density per MHz
      nsegments      the Welch segments behind it
      timeScale, data   timeScale(1:round(samplesPerCode/2)) in seconds and those samples (:90,96-97,106-115; complex for fileType 2)
      histCenters, histI, histQ   hist(real(data), -128:128), hist(imag(data), -128:128) (:146,155,163; histQ None for fileType 1)
      dmax           max(abs(data)) + 1 (:148)"""
    if settings.fileType not in (1, 2):
        raise ValueError("probeData(): settings.fileType must be 1 (real) or 2 (I/Q)")
    fs = float(settings.samplingFreq)
    spc = _round(fs / (settings.codeFreqBasis / settings.codeLength))                  # :66-67
    n = 100 * spc                                                                      # :76
    dt, layout = fid.if_format()
    if (layout == L.GC_REAL) != (settings.fileType == 1):
        raise ValueError("probeData(): settings.fileType does not match the loaded record's layout")
    fid.set_sampling_freq(fs)
    nfft, noverlap = 32768, 2048
    psd, k = fid.probe_psd(first_sample, n, nfft, noverlap, "hamming")                 # :128-131
    psd = psd[0]
    counts, norm2 = fid.probe_histogram(first_sample, n)                               # :146-163
    half = _round(spc / 2)
    raw = fid.read_if(first_sample, half, dtype=np.int16 if dt == L.GC_I16 else np.int8, layout=layout).astype(np.float64)
    if settings.fileType == 1:
        fsm = fs / 1e6
        one = psd[:nfft // 2 + 1] * 1e6                                                # density per MHz
        one[1:nfft // 2] *= 2.0                                                        # one-sided: every bin but DC and Nyquist holds both sides
        freq, spec, data = np.arange(nfft // 2 + 1) * (fsm / nfft), one, raw
    else:
        freq, spec, data = np.arange(nfft) * (fs / nfft), psd, raw[0::2] + 1j * raw[1::2]   # :104
    return SimpleNamespace(freq=freq, psd=spec, nsegments=k, timeScale=np.arange(half) / fs, data=data,
                           histCenters=np.arange(-128, 129), histI=counts[0].copy(),
                           histQ=counts[1].copy() if settings.fileType == 2 else None, dmax=math.sqrt(norm2) + 1.0)


def acquisition(engine: Engine, settings, first_sample: int | None = None, n_long: int | None = None):
    """acqResults = acquisition(longSignal, settings) with longSignal = the IF buffer from
    `first_sample` (default settings.skipNumberOfBytes, as postProcessing.m:74-96 reads it).

    With settings.resamplingflag == 1 and samplingFreq above settings.resamplingThreshold the search runs on the conditioned
    signal of acquisition.m:46-111 (zero-phase FIR(700) band-pass + band-pass-sampling decimation, Engine.acq_condition) and the
    results are mapped back to the record's sampling rate and IF (:264-276).  `n_long` = length(longSignal) for that case
    (default: max(42, acqNonCohTime + 2) code periods, postProcessing.m:82-83, or what the buffer holds).
    """
    import copy
    import math
    if first_sample is None:
        first_sample = skip_samples(settings)
    flag = getattr(settings, "resamplingflag", getattr(settings, "resamplingFlag", 0))
    resampled = settings.samplingFreq > settings.resamplingThreshold and flag == 1
    S = settings
    if resampled:
        if n_long is None:
            n_long = min(int(engine.if_buffer()[1]) - int(first_sample), max(42, int(settings.acqNonCohTime) + 2) * codes.samplesPerCode(settings))
        bw = settings.codeFreqBasis * 2 + 0.5e6                      # acquisition.m:58
        new_fs, new_if, _ = engine.acq_condition(settings.samplingFreq, settings.IF, bw, first_sample, n_long)
        S = copy.copy(settings)
        S.samplingFreq, S.IF = new_fs, new_if                        # :81,95
    prns = list(S.acqSatelliteList)
    acq = SimpleNamespace(carrFreq=np.zeros(32), codePhase=np.zeros(32), peakMetric=np.zeros(32))
    src, first = (1, 0) if resampled else engine.acq_input(first_sample, settings.samplingFreq, n_long)[:2]   # int16 / Q-I / real records: float copy
    p = _acq_params(S, first)
    p.source = src
    tables = np.stack([codes.makeCaTable(prn, S) for prn in prns])
    res = engine.acquire_coarse(p, tables)
    found = []
    for prn, r in zip(prns, res):
        acq.peakMetric[prn - 1] = r.peak_metric                      # acquisition.m:200
        if r.peak_metric > S.acqThreshold:                           # :206
            found.append((prn, r))
    if found:                                                        # the fine stage of every detection in one launch
        f = engine.acquire_fine_l1ca_batch(p, np.stack([codes.generateCAcode(prn) for prn, _ in found]),
                                           [r.code_phase for _, r in found], [r.coarse_freq for _, r in found])
        for (prn, r), fk in zip(found, f):
            acq.carrFreq[prn - 1] = fk                               # :254-260
            acq.codePhase[prn - 1] = r.code_phase                    # :256
            if resampled:                                            # :264-276: back to the record's rate and IF
                acq.codePhase[prn - 1] = math.floor((r.code_phase - 1) / S.samplingFreq * settings.samplingFreq) + 1
                if S.IF >= S.samplingFreq / 2:
                    doppler = (S.samplingFreq - S.IF) - fk
                else:
                    doppler = fk - S.IF
                acq.carrFreq[prn - 1] = doppler + settings.IF
    return acq


# ---------------------------------------------------------------------------------------------
# preRun
# ---------------------------------------------------------------------------------------------
def preRun(acqResults, settings, signal: str = "GPS_L1CA"):
    """channel = preRun(acqResults, settings) of package `signal` (include/preRun.m of each package): the strongest
    detections first, one struct per channel.  Per-package fields: `codeFreq` for the packages whose tracking.m starts the code
    NCO from it (GPS_L5C preRun.m:69-71: codeFreqBasis + (acquiredFreq - IF)/carrFreqBasis*codeFreqBasis; also GAL_E5a / E5b,
    BDS B1C / B2a / B3I), `CLCodePhase` for GPS L2C with the pilot on (GPS_L2C preRun.m:70-72), `K = index - 8` instead of
    `PRN` for GLONASS (GLO_GL1 preRun.m:66).  Indices run over the whole acqResults arrays, whatever their length (32, 50, 63
    PRNs; 14 frequency numbers at K + 8)."""
    from . import signals
    spec = signals.SIGNALS[signal]
    n_ch = int(settings.numberOfChannels)
    glo = spec.id_field == "K"
    channel = []
    for _ in range(n_ch):
        ch = SimpleNamespace(acquiredFreq=0.0, codePhase=0, status="-")
        setattr(ch, spec.id_field, 0)
        if spec.code_freq_from_channel:
            ch.codeFreq = 0.0
        channel.append(ch)
    order = np.argsort(-np.asarray(acqResults.peakMetric, dtype=np.float64), kind="stable")   # preRun.m:60 (sort ... 'descend' is stable)
    n_found = int(np.sum(np.asarray(acqResults.carrFreq) != 0))
    for ii in range(min(n_ch, n_found)):                                      # :65
        p = int(order[ii])
        ch = channel[ii]
        setattr(ch, spec.id_field, p + 1 - 8 if glo else p + 1)
        ch.acquiredFreq = float(acqResults.carrFreq[p])
        ch.codePhase = int(acqResults.codePhase[p])
        if spec.code_freq_from_channel:
            ch.codeFreq = settings.codeFreqBasis + (ch.acquiredFreq - settings.IF) / settings.carrFreqBasis * settings.codeFreqBasis
        if spec.doubled_code and getattr(settings, "pilotTRKflag", 0):
            ch.CLCodePhase = int(acqResults.CLCodePhase[p])
        ch.status = "T"
    return channel


# ---------------------------------------------------------------------------------------------
# tracking
# ---------------------------------------------------------------------------------------------
_REC_FIELDS = ("absoluteSample", "codeFreq", "carrFreq", "I_P", "I_E", "I_L", "Q_E", "Q_P", "Q_L",
               "dllDiscr", "dllDiscrFilt", "pllDiscr", "pllDiscrFilt", "remCodePhase", "remCarrPhase")
_PILOT_FIELDS = ("Pilot_I_E", "Pilot_Q_E", "Pilot_I_P", "Pilot_Q_P", "Pilot_I_L", "Pilot_Q_L")
# tracking.m:47-86: these eight are created with inf(1, n), the others with zeros(1, n); epochs a channel never reaches keep them
_INF_FIELDS = ("codeFreq", "carrFreq", "dllDiscr", "dllDiscrFilt", "pllDiscr", "pllDiscrFilt", "remCodePhase", "remCarrPhase")
# "reference": trackResults carries exactly the Pilot_* fields the package's tracking.m records (signals.SignalSpec.recorded_pilot);
# "all": all six pilot sums whenever a pilot arm is correlated (the reference computes the early / late ones but drops them)
DEFAULT_PILOT_FIELDS = "reference"


def _recorded_pilot_fields(spec, pilot: bool, mode: str | None):
    if not pilot:
        return ()
    mode = mode or DEFAULT_PILOT_FIELDS
    if mode == "all" or spec.recorded_pilot == "all":
        return _PILOT_FIELDS
    return ("Pilot_I_P", "Pilot_Q_P") if spec.recorded_pilot == "prompt" else ()


def track_params(settings, signal: str = "GPS_L1CA") -> L.gc_track_params:
    from . import signals
    spec = signals.SIGNALS[signal]
    p = L.gc_track_params()
    p.sampling_freq = settings.samplingFreq
    p.code_freq_basis = settings.codeFreqBasis
    p.code_length = settings.codeLength
    p.el_spacing = settings.dllCorrelatorSpacing
    p.int_time = settings.intTime
    p.dll_noise_bw = settings.dllNoiseBandwidth
    p.dll_damping = settings.dllDampingRatio
    p.pll_noise_bw = settings.pllNoiseBandwidth
    p.pll_damping = settings.pllDampingRatio
    cno = getattr(settings, "CNo", None)
    if cno is not None and not int(getattr(settings, "CNoInterval", 0)) and int(getattr(cno, "VSMinterval", 0)) > 1:
        p.cno_interval = int(cno.VSMinterval)          # tracking.m:351-358: CNoVSM every VSMinterval epochs, inside the loop
        p.cno_acc_time = float(cno.accTime)
    p.pll_kind = spec.pll_kind
    flag = getattr(settings, "pilotTRKflag", 0)
    # BDS/B1C/include/postProcessing.m:69-74: pilotTRKflag 1 runs NB_tracking, 2 runs WB_tracking (both track the pilot)
    pilot = spec.pilot_combine if (flag == 1 or (flag == 2 and signal == "BDS_B1C_WB")) else 0
    p.pilot_combine = pilot
    if int(getattr(settings, "CNoInterval", 0)) > 1:
        # BDS/B2a tracking.m:409-432, B1C NB_tracking.m:397-418, WB_tracking.m:441-461: Calc_CNo_PLD every CNoInterval epochs; the
        # pilot prompt pair is read swapped (pilotTRKflag == 1, Calc_CNo_PLD.m:72-75) or straight (== 2, the B1C wide-band loop)
        p.cno_interval = int(settings.CNoInterval)
        p.cno_acc_time = float(settings.intTime)
        p.cno_mode = L.GC_CNO_PLD if not pilot else (L.GC_CNO_PLD_PILOT if signal.endswith("_WB") else L.GC_CNO_PLD_PILOT_SWAPPED)
    if spec.pll_kind == L.GC_PLL_3_STATE:
        p.pf3, p.pf2, p.pf1 = signals.calcLoopCoefCarr(settings, spec.coef_variant)
    if pilot:
        for name in ("pll_weight", "dll_weight"):
            w = getattr(spec, name)
            if callable(w):
                w = w(settings)
            if w is not None:
                getattr(p, name)[0], getattr(p, name)[1] = float(w[0]), float(w[1])
        if spec.dll_scale_spacing:
            p.dll_scale = 1.0 - settings.dllCorrelatorSpacing
    # tracking.m:145-153: dataAdaptCoeff*(skipNumberOfBytes + codePhase-1) bytes of schar components, or
    # dataAdaptCoeff*(skipNumberOfBytes + (codePhase-1)*2) bytes of int16 components = skipNumberOfBytes/2 + codePhase-1 samples
    if str(getattr(settings, "dataType", "schar")) == "int16" and not spec.int16_branch:
        raise NotImplementedError(f"{signal}: the reference's tracking.m has no int16 branch (its fseek assumes one byte per "
                                  "component and would start at half the code phase); convert the record to schar")
    p.skip_samples = skip_samples(settings)
    p.n_epochs = signals.epochs_to_process(settings)
    if spec.doubled_code:
        # GPS_L2C/include/tracking.m:107-109: spacing and code length in units of the RZ-doubled code; :153 seeks to
        # skipNumberOfBytes + codePhase WITHOUT the usual -1; :261,357-360 CL window bookkeeping
        p.el_spacing = settings.dllCorrelatorSpacing * 2
        p.code_length = settings.codeLength * 2
        p.code_freq_basis = settings.codeFreqBasis * 2
        p.skip_samples = skip_samples(settings) + 1
        p.table_phase_count = 75 if pilot else 0
    return p


def _tracking_prepare(fid: Engine, channel, settings, signal: str, pilot_fields: str | None = None):
    """The part of tracking() in front of the loops: result structs (tracking.m:47-86), code tables (:156-158), per-channel
    start state (:145-170).  Returns a job record for _tracking_finish."""
    from . import signals
    spec = signals.SIGNALS[signal]
    if settings.fileType not in (1, 2) or settings.dataType not in ("schar", "int8", "int16"):
        raise ValueError("tracking(): settings.fileType must be 1 (real) or 2 (I/Q), settings.dataType 'schar' or 'int16'")
    # fileType 1 (real samples, tracking.m:126-130,232-236): the record must have been loaded with layout GC_REAL
    n_ep = signals.epochs_to_process(settings)
    p = track_params(settings, signal)
    pilot = p.pilot_combine != 0
    rec_pilot = _recorded_pilot_fields(spec, pilot, pilot_fields)
    results = []
    active = []
    for i, ch in enumerate(channel):
        tr = SimpleNamespace(status="-", PRN=0)
        for f in _REC_FIELDS + rec_pilot:
            setattr(tr, f, np.full(n_ep, np.inf) if f in _INF_FIELDS else np.zeros(n_ep))
        tr.CNo = SimpleNamespace(VSMValue=[], VSMIndex=[])
        pld_n = int(getattr(settings, "CNoInterval", 0))
        if pld_n:   # BDS/B2a tracking.m:85-92, B1C NB_tracking.m:92-98: created for every channel, zeros until a record is due
            combined = "B2a_CNo" if signal.startswith("BDS_B2a") else "B1C_CNo"
            for f in ("DataCNo", "DataPLD") + (("PilotCNo", "PilotPLD", combined) if pilot else ()):
                setattr(tr, f, np.zeros(n_ep // pld_n))
        results.append(tr)
        sat = getattr(ch, spec.id_field, getattr(ch, "PRN", 0))
        if (ch.status != "-") if spec.id_field == "K" else (sat != 0):                # tracking.m:136 / GLO_GL1 tracking.m:138
            tr.PRN = sat                                                               # :138 / GLO :141
            fid.set_channel(i, spec.tables(sat, settings), index_scale=spec.index_scale, arm_mult=spec.arm_mult,
                            windows=spec.windows)
            active.append(i)
    inits = []
    for i in active:
        ch = channel[i]
        cf = ch.codeFreq if spec.code_freq_from_channel else settings.codeFreqBasis
        if spec.doubled_code:
            cf = settings.codeFreqBasis * 2                                           # GPS_L2C tracking.m:171
        inits.append(L.gc_channel_init(channel=i, prn=int(results[i].PRN), acquired_freq=ch.acquiredFreq,
                                       code_freq=cf, code_phase=int(ch.codePhase),
                                       table_phase=int(getattr(ch, "CLCodePhase", 0)) if (spec.doubled_code and pilot) else 0))
    return SimpleNamespace(fid=fid, channel=channel, settings=settings, signal=signal, spec=spec, n_ep=n_ep, p=p, pilot=pilot,
                           rec_pilot=rec_pilot, results=results, active=active, inits=inits)


def _tracking_finish(job, fields, done, status):
    """The part of tracking() behind the loops: records into the trackResults structs, C/N0 (tracking.m:351-358), status."""
    settings, signal, spec, pilot, n_ep, results, channel = job.settings, job.signal, job.spec, job.pilot, job.n_ep, job.results, job.channel
    # B2a / B1C estimate C/N0 with Calc_CNo_PLD every settings.CNoInterval epochs (below); the other packages with CNoVSM
    pld = int(getattr(settings, "CNoInterval", 0))
    cno = None if pld else getattr(settings, "CNo", None)
    vsm = int(cno.VSMinterval) if cno is not None else 0
    for k, i in enumerate(job.active):
        tr = results[i]
        n_done = int(done[k])
        for f in _REC_FIELDS + job.rec_pilot:
            getattr(tr, f)[:n_done] = fields[f][k][:n_done]          # epochs never reached keep their inf / 0 (tracking.m:47-86)
        if spec.doubled_code:
            # GPS_L2C tracking.m:226,250,376,382-383: what the reference RECORDS is in single-code units, and
            # absoluteSample is pushed back by the code-phase remainder expressed in samples
            step = tr.codeFreq[:n_done] / settings.samplingFreq
            tr.absoluteSample[:n_done] = tr.absoluteSample[:n_done] + 1 - tr.remCodePhase[:n_done] / step
            for f in ("remCodePhase", "codeFreq", "dllDiscr", "dllDiscrFilt"):
                getattr(tr, f)[:n_done] /= 2
        lib_cno = fields.get("CNoVSM")                                                # computed inside the loop (gc_track_params.cno_interval)
        for loop in (range(vsm, n_done + 1, vsm) if vsm else ()):                     # tracking.m:351-358
            if lib_cno is not None:
                tr.CNo.VSMValue.append(float(lib_cno[k][loop // vsm - 1]))
            else:
                tr.CNo.VSMValue.append(CNoVSM(tr.I_P[loop - vsm:loop], tr.Q_P[loop - vsm:loop], settings.CNo.accTime))
            tr.CNo.VSMIndex.append(loop)
        if pld:
            # BDS/B2a/include/tracking.m:85-92,191-192,409-432 (B1C NB_tracking.m:92-98,397-418, WB_tracking.m:443-461):
            # every CNoInterval epochs, the estimate averaged 0.5/0.5 with the previous one (zeros before the first)
            combined = "B2a_CNo" if signal.startswith("BDS_B2a") else "B1C_CNo"
            prev = np.zeros(3)
            lib_pld = fields.get("CNoPLD")                                            # [nch, nk, 5], evaluated by the library (gc_cno_mode)
            for loop in range(pld, n_done + 1, pld):
                kk = loop // pld - 1
                if lib_pld is not None:
                    v = lib_pld[k][kk]
                    tr.DataCNo[kk], tr.DataPLD[kk] = v[0], v[3]
                    if pilot:
                        tr.PilotCNo[kk], tr.PilotPLD[kk] = v[1], v[4]
                        getattr(tr, combined)[kk] = v[2]
                    continue
                c, d = Calc_CNo_PLD(tr, settings, loop, straight_pilot=signal.endswith("_WB"))
                tr.DataCNo[kk] = c[0] * 0.5 + prev[0] * 0.5
                tr.DataPLD[kk] = d[0]
                if pilot:
                    tr.PilotCNo[kk] = c[1] * 0.5 + prev[1] * 0.5
                    getattr(tr, combined)[kk] = c[2] * 0.5 + prev[2] * 0.5
                    tr.PilotPLD[kk] = d[1]
                prev = c
        if n_done == n_ep:
            tr.status = channel[i].status                                             # tracking.m:365
    if status == L.GC_E_RANGE:
        print("Not able to read the specified number of samples  for tracking, exiting!")
    return results, channel


def tracking(fid: Engine, channel, settings, signal: str = "GPS_L1CA", device_loop: bool = False, pilot_fields: str | None = None,
             precision: str | None = None):
    """[trackResults, channel] = tracking(fid, channel, settings) — `signal` selects the reference
    package whose tracking.m is mirrored ("GPS_L1CA": GPS/GPS_L1CA/include/tracking.m;
    "GAL_E1C": GAL/GAL_E1C/include/tracking.m, data + pilot arms, BOC(1,1) half-chip tables; ... signals.SIGNALS).

    Returns (trackResults, channel).  On a short read the reference prints a message and
    returns what it has (tracking.m:241-245); here the partially filled results are returned
    the same way and `trackResults[i].status` stays '-' for channels that did not finish.

    precision: "double" runs the correlations in float64 (include/gnsscorr.h gc_set_precision) - trackResults then follow a
    MATLAB run of tracking.m epoch for epoch; "single" the float32 kernels; None (default) the engine's setting.  Set for this
    call only.
    """
    precision_code(precision)  # ValueError before anything runs
    job = _tracking_prepare(fid, channel, settings, signal, pilot_fields)
    if not job.active:
        return job.results, channel
    fields, done, status = fid.track(job.p, job.inits, device_loop=device_loop,   # device_loop: gc_track_device (include/gnsscorr.h)
                                     precision=precision)
    return _tracking_finish(job, fields, done, status)


BANK_CHANNEL = 255   # the engine's channel slot correlation_function() configures (the last one: tracking() fills from 0)


def _tracked_blocks(fid: Engine, trackResults_k, channel_k, settings, signal: str, epochs, slot: int = BANK_CHANNEL):
    """The descriptors of the blocks a tracked channel's loop cut, from the state tracking.m records per epoch, on the engine's
    channel slot `slot` (BANK_CHANNEL unless given; configured here with the signal's tables; the sampling frequency is set too).
    Returns (blocks, arms)."""
    from . import signals
    spec = signals.SIGNALS[signal]
    sat = getattr(channel_k, spec.id_field, trackResults_k.PRN)                       # as _tracking_prepare: 'K' for GLONASS
    tables = spec.tables(sat, settings)
    fid.set_channel(slot, tables, index_scale=spec.index_scale, arm_mult=spec.arm_mult, windows=spec.windows)
    fid.set_sampling_freq(settings.samplingFreq)
    pos_all = np.asarray(trackResults_k.absoluteSample, dtype=np.float64)
    if epochs is None:
        # epochs never reached keep codeFreq = remCodePhase = inf and absoluteSample = 0 (tracking.m:47-86)
        epochs = np.nonzero(np.isfinite(np.asarray(trackResults_k.codeFreq, dtype=np.float64)) &
                            np.isfinite(np.asarray(trackResults_k.remCodePhase, dtype=np.float64)))[0]
    epochs = np.atleast_1d(np.asarray(epochs, dtype=np.int64))
    blocks = fid.make_blocks(len(epochs))
    fs = settings.samplingFreq
    for n, e in enumerate(epochs):
        b = blocks[n]
        step = float(trackResults_k.codeFreq[e]) / fs
        rem = float(trackResults_k.remCodePhase[e])
        pos = float(pos_all[e])
        length = settings.codeLength
        if spec.doubled_code:
            # GPS L2C records in single-code units with the position pushed back by the remainder (GPS_L2C tracking.m:223,250,376,382-383);
            # with pilotTRKflag = 0 the channel has the CM table alone, no window, and the library takes it
            step, rem, length = 2 * step, 2 * rem, 2 * settings.codeLength
            pos = float(np.rint(pos - 1 + rem / step))
        b.channel = slot
        b.first_sample = int(pos)
        b.rem_code_phase = rem
        b.code_phase_step = step
        b.blksize = int(math.ceil((length - rem) / step))                                      # tracking.m:219-222
        b.el_spacing = 0.0
        b.carr_freq = float(trackResults_k.carrFreq[e])
        b.rem_carr_phase = float(trackResults_k.remCarrPhase[e])
    return blocks, len(tables)


def correlation_function(fid: Engine, trackResults_k, channel_k, settings, offsets, signal: str = "GPS_L1CA", epochs=None):
    """The correlation function a tracked channel saw: R(o) at the code offsets `offsets` (chips, positive = late) on the blocks the
    loop cut, rebuilt from the state tracking.m records per epoch (absoluteSample, remCodePhase, codeFreq, carrFreq, remCarrPhase:
    tracking.m:212-216,249,277,314,332) - where on a BOC(1,1) peak the channel sits, what multipath does to the peak, a
    discriminator's S-curve at another spacing.  One gc_correlate_bank call (include/gnsscorr.h).

    trackResults_k, channel_k: one channel's entry of what tracking() returned / was given; the record must be loaded in `fid`.
    epochs: indices of the epochs to evaluate (None: every epoch the channel completed - a channel that stopped early on a short
    read, tracking.m:241-245, or was never tracked keeps codeFreq = inf in the epochs it did not reach: those are left out).
    Returns complex128 [n_epochs, arms, ntaps], arms as the signal's tables (data, pilot, ...).
    GPS L2C with its pilot (windowed CL table) is refused by the library: GnssCorrError with status GC_E_UNSUPPORTED.
    Side effects on `fid`: the signal's tables go to the engine's LAST channel slot (BANK_CHANNEL = 255 - whatever a caller keeps
    there is replaced; tracking() fills slots from 0) and the sampling frequency is set to settings.samplingFreq."""
    blocks, arms = _tracked_blocks(fid, trackResults_k, channel_k, settings, signal, epochs)
    return fid.correlate_bank(blocks, offsets)[:, :arms, :]


def excise_pulse_threshold(counts, pulse_sigmas: float, ncomponents: int):
    """(threshold2, sigma) of excise_interference()'s pulse rule from gc_probe_histogram's counts: sigma = 1.4826 x the median of |c0|
    (row 0: the first value of each pair), threshold2 = (pulse_sigmas sigma)^2 ncomponents.  A median in an end bin (|c0| >= 128:
    an int16 record whose levels the histogram does not resolve) raises ValueError."""
    row = np.asarray(counts)[0].astype(np.int64)
    mag = row[128:].copy()                                                              # |v| = 0 .. 128
    mag[1:] += row[127::-1]
    total = int(mag.sum())
    if total == 0:
        raise ValueError("excise_interference(): the histogram is empty")
    cum = np.cumsum(mag)
    lo, hi = int(np.searchsorted(cum, (total + 1) // 2)), int(np.searchsorted(cum, total // 2 + 1))   # the middle sample(s)
    if hi >= 128:
        raise ValueError("excise_interference(): the median level lies in the histogram's end bin (|c0| >= 128): give threshold2 to Engine.excise_pulses yourself")
    sigma = 1.4826 * 0.5 * (lo + hi)
    return int((float(pulse_sigmas) * sigma) ** 2 * ncomponents), sigma


def excise_bin_gain(psd, bin_factor: float, widen: int = 1) -> np.ndarray:
    """excise_interference()'s gain rule from one row of gc_probe_psd: 0 on the bins above bin_factor x the median bin and on `widen`
    neighbours each side of them (around the ends: bin nfft - 1 is next to bin 0), 1 elsewhere."""
    p = np.asarray(psd, dtype=np.float64).reshape(-1)
    hot = p > float(bin_factor) * float(np.median(p))
    out = hot.copy()
    for k in range(1, int(widen) + 1):
        out |= np.roll(hot, k) | np.roll(hot, -k)
    return np.where(out, 0.0, 1.0).astype(np.float32)


def excise_interference(fid: Engine, settings, first_sample: int = 0, nsamples: int | None = None, pulse_sigmas: float | None = None,
                        guard_us=(4.0, 4.0), bin_factor: float | None = None, nfft: int = 4096, widen: int = 1, dst: Engine | None = None):
    """Interference the receiver does not know taken out of [first_sample, first_sample + nsamples) of the loaded record (None: to its
    end) before acquisition(): pulses first (pulse_sigmas not None: gc_excise_pulses), then carriers (bin_factor not None:
    gc_excise_bins), from what the probe shows.  Into `dst`'s record (same sample count, dtype and layout) or (None) in place.
      pulses   threshold2 from gc_probe_histogram of the range (excise_pulse_threshold); guard_us = (before, after) in microseconds
               at settings.samplingFreq, at most GC_EXCISE_MAX_GUARD samples.
      bins     gain from gc_probe_psd of the range AFTER blanking - Hamming window, nfft, noverlap = nfft / 2 - by excise_bin_gain.
    Returns SimpleNamespace(holder, threshold2, sigma, before, after, stats, gain, psd_before, psd_after): the engine that holds the
    cleaned record, what the pulse stage used and counted (None where it did not run), the gain and the spectra in front of and
    behind the bin stage (None where it did not run)."""
    if pulse_sigmas is None and bin_factor is None:
        raise ValueError("excise_interference(): give pulse_sigmas, bin_factor or both")
    fs = float(settings.samplingFreq)
    first_sample = int(first_sample)
    n = int(fid.if_buffer()[1]) - first_sample if nsamples is None else int(nsamples)
    dt, layout = fid.if_format()
    res = SimpleNamespace(holder=fid, threshold2=None, sigma=None, before=None, after=None, stats=None, gain=None, psd_before=None, psd_after=None)
    if pulse_sigmas is not None:
        counts, _ = fid.probe_histogram(first_sample, n)
        res.threshold2, res.sigma = excise_pulse_threshold(counts, pulse_sigmas, 1 if layout == L.GC_REAL else 2)
        res.before, res.after = (min(L.GC_EXCISE_MAX_GUARD, _round(float(g) * 1e-6 * fs)) for g in guard_us)
        res.stats = fid.excise_pulses(first_sample, n, res.threshold2, res.before, res.after, dst=dst)
        if dst is not None:
            res.holder = dst
    if bin_factor is not None:
        src = res.holder                                                                # after blanking: in place on what holds it
        src.set_sampling_freq(fs)
        res.psd_before = src.probe_psd(first_sample, n, nfft, nfft // 2, "hamming")[0][0]
        res.gain = excise_bin_gain(res.psd_before, bin_factor, widen)
        src.excise_bins(first_sample, n, res.gain, dst=dst if (dst is not None and src is fid) else None)
        if dst is not None:
            res.holder = dst
            dst.set_sampling_freq(fs)
        res.psd_after = res.holder.probe_psd(first_sample, n, nfft, nfft // 2, "hamming")[0][0]
    return res


def excise_sweep_limit(power, factor: float) -> np.ndarray:
    """excise_swept()'s limit from the power rows [segments, nfft] of a gc_excise_sweep call: float32(factor * median over the
    segments / ln 2) per bin.  The median of a bin over the segments barely moves under a jammer that visits the bin a small share
    of the time, and the median of an exponential variable - a noise bin's power - is ln 2 times its mean: the limit is `factor`
    times the jam-free mean bin power."""
    p = np.asarray(power, dtype=np.float64)
    if p.ndim != 2 or p.shape[0] < 1:
        raise ValueError(f"excise_sweep_limit(): power must be [segments, nfft], not {p.shape}")
    return (float(factor) * np.median(p, axis=0) / math.log(2.0)).astype(np.float32)


def excise_swept(fid: Engine, settings, first_sample: int = 0, nsamples: int | None = None, nfft: int = 64, factor: float = 6.0, widen: int = 1,
                 train_segments: int = 4096, dst: Engine | None = None):
    """Swept interference - a chirp jammer that crosses the band many times per millisecond - taken out of [first_sample, first_sample
    + nsamples) of the loaded record (None: to its end) before acquisition(), by gc_excise_sweep: the time-frequency cells of
    half-overlapping nfft-sample segments that stand over a limit, and `widen` bins either side of them, are cut.  The limit is
    trained on the first `train_segments` segments of the range: one call with limit = +inf (nothing is cut) and power=True into a
    scratch record (`dst`, which the cleaning overwrites, or a temporary one) gives their power, excise_sweep_limit(power, factor)
    the limit.  Into `dst`'s record (same sample count, dtype and layout) or (None) in place.
    Returns (holder, limit, stats, bin_cut): the engine that holds the cleaned record, the float32 [nfft] limit, gc_excise_sweep's
    statistics and the segments in which each bin was cut."""
    first_sample, nfft, train_segments = int(first_sample), int(nfft), int(train_segments)
    if train_segments < 1:
        raise ValueError(f"excise_swept(): train_segments must be at least 1, not {train_segments}")
    total = int(fid.if_buffer()[1])
    n = total - first_sample if nsamples is None else int(nsamples)
    n_train = min(n, train_segments * (nfft // 2))                      # segments 0 .. train_segments - 1 lie in these samples
    inf = np.full(nfft, np.inf, dtype=np.float32)
    scratch = dst
    try:
        if scratch is None:
            dt, layout = fid.if_format()
            scratch = Engine(fid.device_id)
            scratch.alloc_if(total, np.int16 if dt == L.GC_I16 else np.int8, layout)
        power = fid.excise_sweep(first_sample, n_train, inf, 0, dst=scratch, power=True).power
    finally:
        if dst is None and scratch is not None:
            scratch.close()
    limit = excise_sweep_limit(power[:train_segments], factor)
    res = fid.excise_sweep(first_sample, n, limit, widen, dst=dst, bin_cut=True)
    holder = fid if dst is None else dst
    if dst is not None:
        dst.set_sampling_freq(float(settings.samplingFreq))
    return holder, limit, res.stats, res.bin_cut


def ddc_nco_step(freq: float, fs: float) -> int:
    """gc_downconvert's phase_step for `freq` at `fs` as a signed Python integer: ldexp(freq / fs, 64) rounded to the nearest integer,
    ties to even (what llrint gives the library)."""
    from fractions import Fraction
    return int(round(Fraction(math.ldexp(float(freq) / float(fs), 64))))


def ddc_nco_freq(step: int, fs: float) -> float:
    """The frequency an NCO of phase_step `step` (signed) runs at: gc_ddc_result.carr_freq."""
    return math.ldexp(float(int(step)), -64) * float(fs)


def ddc_band_taps(fs: float, center_freq: float, bandwidth: float, ntaps: int, window="hamming"):
    """(g, f_used, h) of downconvert_band(): h = scipy.signal.firwin(ntaps, bandwidth / 2, fs=fs) low-pass of gain 1 at DC,
    g[k] = h[k] exp(+j 2 pi f_used k / fs) the same filter around f_used, the frequency gc_downconvert's NCO runs at for center_freq."""
    from scipy.signal import firwin
    h = np.asarray(firwin(int(ntaps), float(bandwidth) / 2.0, window=window, fs=float(fs)), dtype=np.float64) if ntaps > 1 else np.ones(1)
    f_used = ddc_nco_freq(ddc_nco_step(center_freq, fs), fs)
    return ddc_modulate(h, f_used, fs), f_used, h


def ddc_modulate(h, f_used: float, fs: float) -> np.ndarray:
    """g[k] = h[k] exp(+j 2 pi f_used k / fs), operation by operation as matlab/gnsscorr_downconvert.m writes it."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    ang = 2.0 * np.pi * f_used * np.arange(h.shape[0], dtype=np.float64) / float(fs)
    return h * np.cos(ang) + 1j * (h * np.sin(ang))


def downconvert_band(engine: Engine, dst: Engine, center_freq: float, bandwidth: float, decim: int, ntaps: int | None = None,
                     target_rms: float | None = None, window="hamming", h=None):
    """The band of `bandwidth` Hz around center_freq of `engine`'s record as a record at samplingFreq / decim in `dst` (another engine
    on the same device with a record from alloc_if; any dtype and layout): one gc_downconvert with a windowed-sinc low-pass moved to
    the band, the NCO taking the band's centre to DC.  engine's sampling frequency must be set (set_sampling_freq / load_if(fs=)).
      ntaps       None: the odd number 8 decim + 1 (at most GC_DDC_MAX_TAPS - 1).
      h           a real low-pass of the caller's to use instead of the designed one (bandwidth, ntaps and window are then ignored):
                  what matlab/gnsscorr_downconvert.m does with fir1's.
      target_rms  None: gain 1.  Else the rms a stored component should have: the call runs on the first min(noutputs, 65536)
                  outputs, the taps are scaled by target_rms / the rms sum_sq gives, and the whole range runs with them.
    first_sample = (ntaps - 1) // 2, so that output m lines up with input sample m * decim.
    Returns (result of Engine.downconvert, SimpleNamespace(samplingFreq = fs / decim, IF = center_freq - f_used: what the NCO's
    quantised frequency leaves of the centre, f_used, gain, delay: the filter's residual delay in INPUT samples (0 for odd ntaps, 0.5
    for even), decim)) - code phases found on dst map back as sample * decim + delay.  dst's sampling frequency is set."""
    fs = getattr(engine, "sampling_freq", None)
    if fs is None:
        raise ValueError("downconvert_band(): set the engine's sampling frequency first")
    d = int(decim)
    if d != decim or not 1 <= d <= L.GC_DDC_MAX_DECIM:
        raise ValueError(f"downconvert_band(): decim must be a whole number in 1 .. {L.GC_DDC_MAX_DECIM}, not {decim!r}")
    if h is None:
        T = min(8 * d + 1, L.GC_DDC_MAX_TAPS - 1) if ntaps is None else int(ntaps)
        g, f_used, _ = ddc_band_taps(fs, center_freq, bandwidth, T, window)
    else:
        f_used = ddc_nco_freq(ddc_nco_step(center_freq, fs), fs)
        g = ddc_modulate(h, f_used, fs)
        T = g.shape[0]
    first = (T - 1) // 2
    gain = 1.0
    comps = 1 if dst.if_format()[1] == L.GC_REAL else 2
    if target_rms is not None:
        full = min((int(engine.if_buffer()[1]) + T - 2 - first) // d + 1, int(dst.if_buffer()[1]))
        trial = engine.downconvert(dst, g, d, carr_freq=center_freq, first_sample=first, noutputs=min(full, 65536))
        rms = math.sqrt(trial.sum_sq / (comps * trial.noutputs))
        if not rms > 0.0:
            raise ValueError("downconvert_band(): the band holds nothing to scale (every stored component of the trial is zero)")
        gain = float(target_rms) / rms
    res = engine.downconvert(dst, gain * g, d, carr_freq=center_freq, first_sample=first)
    dst.set_sampling_freq(fs / d)
    return res, SimpleNamespace(samplingFreq=fs / d, IF=float(center_freq) - f_used, f_used=f_used, gain=gain,
                                delay=(T - 1) / 2.0 - first, decim=d)


def resample_ratio(fs: float, fs_out: float) -> tuple[int, int]:
    """(L, M) of resample_record(fs_out=): fs_out / fs as the fraction L / M in lowest terms with M <= GC_DDC_MAX_DECIM *
    GC_RS_MAX_INTERP.  ValueError where no such fraction gives fs_out to 1e-9 of it, or where gc_resample refuses it (L > 64, M > 64 L)."""
    from fractions import Fraction
    if not (fs > 0.0 and fs_out > 0.0):
        raise ValueError(f"resample_record(): the rates must be positive, not {fs!r} -> {fs_out!r}")
    r = Fraction(float(fs_out) / float(fs)).limit_denominator(L.GC_DDC_MAX_DECIM * L.GC_RS_MAX_INTERP)
    li, m = r.numerator, r.denominator
    if li < 1 or abs(float(fs) * li / m - float(fs_out)) > 1e-9 * float(fs_out):
        raise ValueError(f"resample_record(): {fs_out!r} / {fs!r} is no fraction L / M with M <= {L.GC_DDC_MAX_DECIM * L.GC_RS_MAX_INTERP} (the nearest is {li} / {m})")
    _resample_ratio_check(li, m)
    return li, m


def _resample_ratio_check(li: int, m: int):
    if not 1 <= li <= L.GC_RS_MAX_INTERP:
        raise ValueError(f"resample_record(): the rate change {li} / {m} needs L = {li}; gc_resample takes L in 1 .. {L.GC_RS_MAX_INTERP}")
    if not 1 <= m <= L.GC_DDC_MAX_DECIM * li:
        raise ValueError(f"resample_record(): the rate change {li} / {m} lowers the rate by more than {L.GC_DDC_MAX_DECIM} (M in 1 .. {L.GC_DDC_MAX_DECIM} L)")


def resample_taps(fs: float, interp: int, decim: int, center_freq: float = 0.0, bandwidth: float | None = None, ntaps: int | None = None,
                  window="hamming"):
    """(g, f_used, h) of resample_record(): the prototype at the rate fs * L.  h = L * scipy.signal.firwin(T, cut, fs=fs * L) - a
    low-pass of gain L at DC, which the L - 1 zeros between the samples bring back to 1 - with cut = bandwidth / 2, or
    0.4 * fs * min(1, L / M): inside the narrower of the two Nyquist bands.  T = ntaps, or the odd number 16 max(L, M) + 1, at most
    GC_RS_MAX_TAPS - 1.  g[k] = h[k] exp(+j 2 pi f_used k / (fs L)) is the filter around f_used, the frequency gc_resample's NCO runs
    at for center_freq."""
    from scipy.signal import firwin
    li, m = int(interp), int(decim)
    rate = float(fs) * float(li)
    T = min(16 * max(li, m) + 1, L.GC_RS_MAX_TAPS - 1) if ntaps is None else int(ntaps)
    cut = float(bandwidth) / 2.0 if bandwidth is not None else 0.4 * float(fs) * min(1.0, li / m)
    h = float(li) * np.asarray(firwin(T, cut, window=window, fs=rate), dtype=np.float64) if T > 1 else np.full(1, float(li))
    f_used = ddc_nco_freq(ddc_nco_step(center_freq, rate), rate)
    return ddc_modulate(h, f_used, rate), f_used, h


def resample_record(engine: Engine, dst: Engine, fs_out: float | None = None, ratio=None, center_freq: float = 0.0,
                    bandwidth: float | None = None, ntaps: int | None = None, target_rms: float | None = None, h=None, window="hamming"):
    """`engine`'s record at another rate in `dst` (another engine on the same device with a record from alloc_if; any dtype and
    layout): one gc_resample at the rate change L / M with a windowed-sinc low-pass (resample_taps) moved to center_freq, the NCO
    taking center_freq to DC.  engine's sampling frequency must be set.
      fs_out      the rate wanted: L / M = fs_out / fs in lowest terms (resample_ratio); or
      ratio       (L, M) as given.  Exactly one of the two.
      bandwidth, ntaps   of the low-pass: see resample_taps.
      h           a real prototype of the caller's at the rate fs * L, gain L at DC (bandwidth, ntaps and window are then ignored).
      target_rms  None: gain 1.  Else the rms a stored component should have, in two passes as downconvert_band() does.
    first_tick = (T - 1) // 2, so that output m lines up with tick m * M, input sample m * M / L.
    Returns (result of Engine.resample, SimpleNamespace(samplingFreq = fs * L / M, IF = center_freq - f_used, f_used, gain, interp,
    decim, delay: the filter's residual delay in TICKS, 0 for odd T)) - a code phase found on dst maps back as sample * M / L.  dst's
    sampling frequency is set."""
    fs = getattr(engine, "sampling_freq", None)
    if fs is None:
        raise ValueError("resample_record(): set the engine's sampling frequency first")
    if (fs_out is None) == (ratio is None):
        raise ValueError("resample_record(): give fs_out or ratio=(L, M), one of the two")
    if ratio is not None:
        try:
            li, m = ratio
            if li != int(li) or m != int(m) or isinstance(li, bool) or isinstance(m, bool):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"resample_record(): ratio must be two whole numbers (L, M), not {ratio!r}") from None
        li, m = int(li), int(m)
        _resample_ratio_check(li, m)
    else:
        li, m = resample_ratio(fs, fs_out)
    rate = float(fs) * float(li)
    if h is None:
        g, f_used, _ = resample_taps(fs, li, m, center_freq, bandwidth, ntaps, window)
    else:
        f_used = ddc_nco_freq(ddc_nco_step(center_freq, rate), rate)
        g = ddc_modulate(h, f_used, rate)
    T = g.shape[0]
    first = (T - 1) // 2
    gain = 1.0
    comps = 1 if dst.if_format()[1] == L.GC_REAL else 2
    if target_rms is not None:
        branches = -(-T // li)
        full = min(((int(engine.if_buffer()[1]) + branches - 1) * li - 1 - first) // m + 1, int(dst.if_buffer()[1]))
        trial = engine.resample(dst, g, li, m, carr_freq=center_freq, first_tick=first, noutputs=min(full, 65536))
        rms = math.sqrt(trial.sum_sq / (comps * trial.noutputs))
        if not rms > 0.0:
            raise ValueError("resample_record(): the band holds nothing to scale (every stored component of the trial is zero)")
        gain = float(target_rms) / rms
    res = engine.resample(dst, gain * g, li, m, carr_freq=center_freq, first_tick=first)
    dst.set_sampling_freq(res.out_rate)
    return res, SimpleNamespace(samplingFreq=res.out_rate, IF=float(center_freq) - f_used, f_used=f_used, gain=gain, interp=li, decim=m,
                                delay=(T - 1) / 2.0 - first)


def array_covariance_matrix(cov, ntaps: int) -> np.ndarray:
    """The Hermitian K T x K T complex128 covariance of the stacked snapshot z[n] = (x_a[n - s]), a = 0 .. K-1, s = 0 .. T-1 (index
    a T + s), from Engine.array_covariance's int64 [L, K, K, 2] with L >= T: block-Toeplitz,
        R[(a, s), (b, t)] = C[t - s][a][b]  for t >= s,   conj(C[s - t][b][a])  otherwise.
    This is the range-shift approximation: the exact sum over n of x_a[n - s] conj(x_b[n - t]) runs over a range moved back by s
    samples, so each entry differs from it by edge terms of at most T - 1 samples at either end of the range (none for T = 1)."""
    c = np.asarray(cov)
    T = int(ntaps)
    if c.ndim != 4 or c.shape[1] != c.shape[2] or c.shape[3] != 2 or not 1 <= T <= c.shape[0]:
        raise ValueError(f"array_covariance_matrix(): cov must be [L, K, K, 2] with L >= ntaps = {ntaps!r}, not {c.shape}")
    K = c.shape[1]
    z = c[..., 0].astype(np.float64) + 1j * c[..., 1].astype(np.float64)
    R = np.empty((K, T, K, T), dtype=np.complex128)
    for s in range(T):
        for t in range(T):
            R[:, s, :, t] = z[t - s] if t >= s else np.conj(z[s - t].T)
    return R.reshape(K * T, K * T)


def _array_loaded(R, loading: float) -> np.ndarray:
    R = np.asarray(R, dtype=np.complex128)
    if R.ndim != 2 or R.shape[0] != R.shape[1]:
        raise ValueError(f"array weights: R must be a square matrix, not {R.shape}")
    return R + float(loading) * np.eye(R.shape[0])


def power_inversion_weights(R, nrecords: int, ntaps: int, ref: int = 0, loading: float = 0.0) -> np.ndarray:
    """w = (R + loading I)^-1 e / (e^H (R + loading I)^-1 e) with e the unit vector at (record ref, tap 0): the output power w^H R w
    is least among the weights with w[ref, tap 0] = 1.  Returns w as complex128 [K T]; Engine.array_combine takes
    conj(w).reshape(K, T)."""
    K, T, r = int(nrecords), int(ntaps), int(ref)
    A = _array_loaded(R, loading)
    if A.shape[0] != K * T or not 0 <= r < K:
        raise ValueError(f"power_inversion_weights(): R must be {K * T} x {K * T} and ref in 0 .. {K - 1}, not {A.shape} and {ref!r}")
    e = np.zeros(K * T, dtype=np.complex128)
    e[r * T] = 1.0
    u = np.linalg.solve(A, e)
    return u / np.vdot(e, u)


def mvdr_weights(R, steering, loading: float = 0.0) -> np.ndarray:
    """w = (R + loading I)^-1 v / (v^H (R + loading I)^-1 v): least output power among the weights with w^H v = 1."""
    A = _array_loaded(R, loading)
    v = np.asarray(steering, dtype=np.complex128).reshape(-1)
    if v.shape[0] != A.shape[0]:
        raise ValueError(f"mvdr_weights(): a steering vector of {A.shape[0]} entries, not {v.shape[0]}")
    u = np.linalg.solve(A, v)
    return u / np.vdot(v, u)


def null_steer(records, dst: Engine, settings, ntaps: int = 1, ref: int = 0, first_sample: int = 0, nsamples: int | None = None,
               loading: float = 0.0, target_rms: float | None = None):
    """Wide-band interference out of the records of an antenna array: one gc_array_covariance over the K engines `records`
    (nsamples=None: what every record and dst hold from first_sample), the power-inversion weights for the reference element `ref`
    over ntaps taps per element, and one gc_array_combine of conj(w) into `dst` (another engine on the same device with a record from
    alloc_if; any dtype and layout) from its sample 0.
      loading     added to R's diagonal, in the covariance's units (squared counts summed over the range).
      target_rms  None: gain 1.  Else the rms a stored component should have: a trial combine on the first min(nsamples, 65536)
                  outputs, the weights scaled by target_rms / the rms sum_sq gives, then the whole range - as downconvert_band() scales.
    The reference tap is tap 0, so the delay is 0: sample indices, samplingFreq and IF of `settings` hold for dst, whose sampling
    frequency is set to settings.samplingFreq.
    Returns (result of Engine.array_combine, w: complex128 [K, T] before the gain, gain, cov: int64 [T, K, K, 2])."""
    recs = list(records)
    K, T = len(recs), int(ntaps)
    first = int(first_sample)
    if nsamples is None:
        n = min(min(int(r.if_buffer()[1]) for r in recs) - first, int(dst.if_buffer()[1]))
    else:
        n = int(nsamples)
    cov = Engine.array_covariance(recs, first, n, T)
    w = power_inversion_weights(array_covariance_matrix(cov, T), K, T, ref, loading).reshape(K, T)
    gain = 1.0
    comps = 1 if dst.if_format()[1] == L.GC_REAL else 2
    if target_rms is not None:
        trial = Engine.array_combine(recs, dst, np.conj(w), first_sample=first, noutputs=min(n, 65536))
        rms = math.sqrt(trial.sum_sq / (comps * trial.noutputs))
        if not rms > 0.0:
            raise ValueError("null_steer(): the records hold nothing to scale (every stored component of the trial is zero)")
        gain = float(target_rms) / rms
    res = Engine.array_combine(recs, dst, gain * np.conj(w), first_sample=first, noutputs=n)
    dst.set_sampling_freq(settings.samplingFreq)
    return res, w, gain, cov


def cancel_tracked(fid: Engine, trackResults, channel, settings, which=None, signal: str = "GPS_L1CA", epochs=None, dst: Engine | None = None,
                   mode: str = "subtract", amp=None):
    """What lies under the signals a tracking run followed: every chosen channel's tracked component rebuilt from the state tracking.m
    records per epoch (the blocks of correlation_function()) and taken out of the record sample by sample - a reflection next to the
    peak, a weak satellite under a strong one's cross-correlation floor, the direct signal's leak into a down-looking record.  One
    gc_cancel call for all channels (include/gnsscorr.h); the bank, the maps, acquisition() and tracking() then run on the residual.

    trackResults, channel: what tracking() returned / was given; the record must be loaded in `fid`.
    which: indices of the channels to cancel (None: every channel that was tracked, PRN != 0), at most GC_CANCEL_MAX_CHANNELS.
    epochs: indices of the epochs to cancel, for every chosen channel (None: every epoch a channel completed).
    dst: the engine whose record receives the result (same sample count, dtype and layout: alloc_if); None works in place.
    mode: "subtract" leaves the residual, "model" writes the rebuilt components alone.
    amp: None projects every block on its replica; else one complex array [n_epochs, arms] per chosen channel.
    Returns (the engine that holds the result, [complex128 [n_epochs, arms] per chosen channel]: the amplitudes used).
    Side effects on `fid`: the chosen channels' tables go to the engine's last channel slots, counting down from BANK_CHANNEL, one per
    channel (whatever a caller keeps there is replaced), and the sampling frequency is set to settings.samplingFreq."""
    Engine._cancel_args(0, None, mode)                                                # ValueError before anything runs
    if which is None:
        which = [i for i, tr in enumerate(trackResults) if getattr(tr, "PRN", 0) != 0]
    which = [int(i) for i in which]
    if len(which) > L.GC_CANCEL_MAX_CHANNELS:
        raise ValueError(f"cancel_tracked(): at most {L.GC_CANCEL_MAX_CHANNELS} channels per call, not {len(which)}")
    if amp is not None:
        amp = [np.asarray(a) for a in amp]
        if len(amp) != len(which) or any(a.ndim != 2 or not 1 <= a.shape[1] <= L.GC_MAX_ARMS for a in amp):
            raise ValueError("cancel_tracked(): amp holds one complex array [n_epochs, arms] per chosen channel")
    parts = [_tracked_blocks(fid, trackResults[i], channel[i], settings, signal, epochs, slot=BANK_CHANNEL - k) for k, i in enumerate(which)]
    blocks = fid.make_blocks(sum(len(b) for b, _ in parts))
    amp_in = None if amp is None else np.zeros((len(blocks), L.GC_MAX_ARMS), dtype=np.complex128)
    n = 0
    for k, (b, arms) in enumerate(parts):
        if amp is not None:
            if amp[k].shape != (len(b), arms):
                raise ValueError(f"cancel_tracked(): amp[{k}] must be [{len(b)}, {arms}], not {amp[k].shape}")
            amp_in[n:n + len(b), :arms] = amp[k]
        for x in b:
            blocks[n] = x
            n += 1
    used = fid.cancel(blocks, dst=dst, amp=amp_in, mode=mode)
    out, n = [], 0
    for b, arms in parts:
        out.append(used[n:n + len(b), :arms])
        n += len(b)
    return (fid if dst is None else dst), out


def delay_doppler_map(fid: Engine, trackResults_k, channel_k, settings, offsets, freqs, signal: str = "GPS_L1CA", epochs=None):
    """The delay-Doppler map a tracked channel saw: R(o, f) at the code offsets `offsets` (chips, positive = late) and the carrier
    offsets `freqs` (Hz, added to the carrFreq the loop recorded for the epoch) on the blocks the loop cut - whether the PLL sits on
    the main lobe or a side lobe, how good the acquisition's carrFreq was, what sits next to the peak.  The carrier phase of every
    bin is remCarrPhase at the block's first sample: bins differ in frequency only.  The bin at 0 Hz is correlation_function()
    bit for bit.  One gc_correlate_ddm call (include/gnsscorr.h).

    Arguments, refusals and side effects as correlation_function().  Returns complex128 [n_epochs, arms, nfreq, ntaps]."""
    blocks, arms = _tracked_blocks(fid, trackResults_k, channel_k, settings, signal, epochs)
    return fid.correlate_ddm(blocks, offsets, freqs)[:, :arms]


def integrated_delay_doppler_map(fid: Engine, trackResults_k, channel_k, settings, offsets, freqs, coherent, noncoherent=None, wipe="prompt",
                                 signal: str = "GPS_L1CA", epochs=None):
    """delay_doppler_map() integrated over epochs on the device: the evaluated epochs, in order, form runs of `coherent` consecutive
    epochs whose maps are added coherently - every bin rotated to the carrier phase at the run's first block, which is what makes bins
    closer than 1 / (block length) resolvable - and, with `noncoherent` = M, the powers |.|^2 of M consecutive runs are added to one map.
    A trailing incomplete run (and a trailing incomplete map) is dropped.  One gc_correlate_ddm_integrate call (include/gnsscorr.h): the
    per-epoch maps never leave the device.

    wipe: the data-bit or secondary-code wipe-off, one weight per evaluated epoch - "prompt": +1 where the recorded I_P of the epoch is
    >= 0, else -1; None: no weights; an array: the caller's own (one per evaluated epoch, any finite value; 0 drops an epoch).
    Returns complex128 [n_runs, arms, nfreq, ntaps] (noncoherent=None) or float64 [n_maps, arms, nfreq, ntaps].
    Other arguments, refusals and side effects as correlation_function()."""
    blocks, arms = _tracked_blocks(fid, trackResults_k, channel_k, settings, signal, epochs)
    coherent = int(coherent)
    if coherent < 1 or (noncoherent is not None and int(noncoherent) < 1):
        raise ValueError("integrated_delay_doppler_map: coherent and noncoherent count epochs and runs (1 at least)")
    nruns = len(blocks) // coherent
    if noncoherent is not None:
        nruns -= nruns % int(noncoherent)
    nblk = nruns * coherent
    if isinstance(wipe, str) and wipe == "prompt":
        if epochs is None:           # the epochs _tracked_blocks evaluated
            epochs = np.nonzero(np.isfinite(np.asarray(trackResults_k.codeFreq, dtype=np.float64)) &
                                np.isfinite(np.asarray(trackResults_k.remCodePhase, dtype=np.float64)))[0]
        ip = np.asarray(trackResults_k.I_P, dtype=np.float64)[np.atleast_1d(np.asarray(epochs, dtype=np.int64))]
        weights = np.where(ip >= 0, 1.0, -1.0)
    elif wipe is None:
        weights = None
    else:
        weights = np.asarray(wipe, dtype=np.float64).reshape(-1)
        if weights.shape[0] != len(blocks):
            raise ValueError("integrated_delay_doppler_map: one weight per evaluated epoch")
    used = fid.make_blocks(nblk)
    for n in range(nblk):
        used[n] = blocks[n]
    if weights is not None:
        weights = weights[:nblk]
    if noncoherent is None:
        coh, _ = fid.correlate_ddm_integrate(used, offsets, freqs, [coherent] * nruns, weights=weights)
        return coh[:, :arms]
    if nruns == 0:                   # not one complete map: nothing to ask the library for
        return np.zeros((0, arms, np.asarray(freqs).size, np.asarray(offsets).size))
    _, pw = fid.correlate_ddm_integrate(used, offsets, freqs, [coherent] * nruns, weights=weights,
                                        map_len=[int(noncoherent)] * (nruns // int(noncoherent)), coherent=False)
    return pw[:, :arms]


def _search_grid(name, nblocks, run, lead, noncoherent):
    """run_len and map_len of a search whose runs are `run` epochs long and whose hypotheses need `lead` further epochs: the complete
    runs every hypothesis has, in one map or in maps of `noncoherent` runs (a trailing incomplete map is dropped)."""
    if run < 1 or (noncoherent is not None and int(noncoherent) < 1):
        raise ValueError(f"{name}: the run length and noncoherent count epochs and runs (1 at least)")
    nruns = max(nblocks - lead, 0) // run
    if noncoherent is not None:
        nruns -= nruns % int(noncoherent)
    if nruns < 1:
        raise ValueError(f"{name}: {nblocks} evaluated epochs do not hold one complete map of runs of {run} epochs for every hypothesis")
    return [run] * nruns, [nruns] if noncoherent is None else [int(noncoherent)] * (nruns // int(noncoherent))


def _search_winner(peaks):
    """The first maximum over the hypotheses of the first arm's peak power summed over the maps."""
    return int(np.argmax(peaks["power"][:, :, 0].sum(axis=1)))


def bit_edge_search(fid: Engine, trackResults_k, channel_k, settings, offsets, freqs, period, noncoherent=None, signal: str = "GPS_L1CA",
                    epochs=None):
    """Where the data-bit edges fall on a channel whose prompt signs cannot be trusted: integrated_delay_doppler_map()'s power maps
    without a wipe-off, under the `period` alignments of a grid of runs of `period` consecutive evaluated epochs (20 for GPS L1 C/A).
    Hypothesis h starts its runs at evaluated epoch h; only the alignment at which no run straddles a bit edge adds every run
    coherently.  Every hypothesis integrates the same number of runs: the complete runs common to all shifts, in one power map, or in
    maps of `noncoherent` runs each (a trailing incomplete map is dropped).  One gc_correlate_ddm_search call (include/gnsscorr.h): the
    epochs are correlated once for all alignments, the peaks are picked on the device and nothing else comes back.

    Returns (peaks, shift): peaks a structured array [period, n_maps, arms] with fields power, bin, tap - the first maximum of every
    map, bin indexing `freqs` and tap `offsets` -, shift the first maximum over the alignments of the first arm's peak power summed
    over the maps.  ValueError when the evaluated epochs do not hold one complete map for every alignment.
    Other arguments, refusals and side effects (the engine's slot 255, the sampling frequency) as correlation_function()."""
    blocks, arms = _tracked_blocks(fid, trackResults_k, channel_k, settings, signal, epochs)
    period = int(period)
    run_len, map_len = _search_grid("bit_edge_search", len(blocks), period, period - 1, noncoherent)
    _, _, peaks = fid.correlate_ddm_search(blocks, offsets, freqs, run_len, map_len=map_len, shifts=np.arange(period), power=False)
    peaks = peaks[:, :, :arms]
    return peaks, _search_winner(peaks)


def secondary_code_search(fid: Engine, trackResults_k, channel_k, settings, offsets, freqs, code, noncoherent=None,
                          signal: str = "GPS_L1CA", epochs=None):
    """The phase of a known secondary code (`code`: its chips as +1 / -1, one per code period - NH10, NH20, CS25, CS100) on a channel
    whose prompt signs cannot be trusted: integrated_delay_doppler_map()'s power maps over runs of len(code) evaluated epochs, under
    the len(code) phases of the pattern.  Hypothesis h weights evaluated epoch n with code[(n + h) % len(code)]; only the true phase
    wipes every chip and adds the whole run coherently.  One power map of all complete runs, or maps of `noncoherent` runs each.
    One gc_correlate_ddm_search call (include/gnsscorr.h; at most GC_DDM_MAX_HYP chips per call).

    Returns (peaks, phase): peaks a structured array [len(code), n_maps, arms] as bit_edge_search(), phase the first maximum over
    the hypotheses of the first arm's peak power summed over the maps.
    Other arguments, refusals and side effects (the engine's slot 255, the sampling frequency) as correlation_function()."""
    blocks, arms = _tracked_blocks(fid, trackResults_k, channel_k, settings, signal, epochs)
    chips = np.asarray(code, dtype=np.float64).reshape(-1)
    if chips.size < 1 or not np.all(np.abs(chips) == 1.0):
        raise ValueError("secondary_code_search: the code's chips are +1 / -1")
    nchip = chips.size
    run_len, map_len = _search_grid("secondary_code_search", len(blocks), nchip, 0, noncoherent)
    n = np.arange(len(blocks))
    weights = chips[(n[None, :] + np.arange(nchip)[:, None]) % nchip]
    _, _, peaks = fid.correlate_ddm_search(blocks, offsets, freqs, run_len, map_len=map_len, weights=weights, power=False)
    peaks = peaks[:, :, :arms]
    return peaks, _search_winner(peaks)


def tracking_file(fid: Engine, path: str, channel, settings, window_samples: int, signal: str = "GPS_L1CA", pilot_fields: str | None = None,
                  precision: str | None = None, device_loop: bool = False):
    """tracking(fid, channel, settings) on a record FILE that need not fit the device: at most 2 * window_samples samples are
    resident at any time (include/gnsscorr.h gc_track_file: two alternating device windows, the next one read and uploaded
    while the current one is tracked).  The reference freads block by block (tracking.m:226-245) and so handles any file
    length; results are identical to tracking() on the fully loaded record.  settings.fileType / dataType / the package's
    sample order say how the file is laid out, as in postProcessing.m:59-96.  precision as tracking().  device_loop: the loop of
    every window closed on the GPU (gc_track_file_device), results identical to tracking(..., device_loop=True)."""
    precision_code(precision)
    job = _tracking_prepare(fid, channel, settings, signal, pilot_fields)
    if not job.active:
        return job.results, channel
    dtype = L.GC_I16 if str(settings.dataType) == "int16" else L.GC_I8
    # GLONASS front ends deliver Q first (GLO_GL1/include/tracking.m:227)
    layout = L.GC_REAL if settings.fileType == 1 else (L.GC_QI if signal.startswith("GLO_") else L.GC_IQ)
    fid.set_sampling_freq(settings.samplingFreq)
    fields, done, status = fid.track_file(path, job.p, job.inits, int(window_samples), dtype=dtype, layout=layout, precision=precision,
                                         device_loop=device_loop)
    return _tracking_finish(job, fields, done, status)


def tracking_multi(calls, device_loop: bool = False, pilot_fields: str | None = None, precision: str | None = None):
    """Several packages' tracking() at once (BASELINE config 5, include/gnsscorr.h gc_track_multi):
    calls = [(fid, channel, settings, signal), ...] with one Engine per call - engines that read the same record share it
    with Engine.share_if.  precision as tracking(), for every call.  Returns [(trackResults, channel), ...] in call order,
    each exactly what tracking() returns."""
    precision_code(precision)
    jobs = [_tracking_prepare(*c, pilot_fields=pilot_fields) for c in calls]
    live = [j for j in jobs if j.active]
    got = Engine.track_multi([(j.fid, j.p, j.inits) for j in live], device_loop=device_loop, precision=precision) if live else []
    out = []
    it = iter(got)
    for j in jobs:
        out.append(_tracking_finish(j, *next(it)) if j.active else (j.results, j.channel))
    return out
