"""A float64 model of what gc_acq_shift_search_batch returns per PRN (numpy, float64 / complex128): the surface of the circshift
searches and the three packages' rules on it, restated from the reference line by line.

Surface: row ((carrier * n_signals + signal) * n_bins + bin) = sum_arm w * |ifft(roll(fft(x_signal * carrier), bin) * conj(fft(code_arm)))|
(BDS/B1I/include/acquisition.m:76-123, GPS/GPS_L2C/include/acquisition.m:40-75, BDS/B1C/include/acquisition.m:137-192).

Rules:
  SEQUENTIAL        GPS_L2C acquisition.m:46-66: the (carrier, bin) grid in order, a row taken when its maximum EXCEEDS the largest so
                    far (from 0), the last bin of every carrier but the first not looked at; :72 the row's first maximum; :77-91 the
                    second peak.
  SEQUENTIAL_PAIRS  BDS/B1I acquisition.m:87-122: two signal blocks per (carrier, bin); taken when either block's maximum exceeds the
                    largest so far, and then block 1 only if it is the larger of the two; :126, :141-156 as above.
  GLOBAL            BDS/B1C acquisition.m:193-197: the first row holding max(max(results, [], 2)), the first column holding
                    max(max(results)); no second peak.

Two places where the reference has no answer and the library has one are the library's here: a second-peak range that is empty
(MATLAB: max([]) = []) gives 0, and range positions beyond the row (MATLAB: an index error) are not looked at.  A surface without a
value above 0 under the sequential rules leaves the PRN alone (row -1, everything 0); GLOBAL takes row 0, column 0, peak 0 there, as
max does."""
import numpy as np

GLOBAL, SEQUENTIAL, SEQUENTIAL_PAIRS = 0, 1, 2


def surface(x, fs, n, n_signals, carriers, n_bins, codes, weights=None, first_sample=0):
    """x: complex samples; signal block s starts at first_sample + s * n; carriers: wipe-off frequencies in Hz; codes [narms, n]
    (zero-padded replicas).  -> float64 [len(carriers) * n_signals * n_bins, n]."""
    x = np.asarray(x, dtype=np.complex128)
    codes = np.asarray(codes, dtype=np.float64).reshape(-1, n)
    w = [1.0] * codes.shape[0] if weights is None else [float(v) for v in weights]
    k = np.arange(n)
    cspec = [np.conj(np.fft.fft(c)) for c in codes]
    rows = []
    for f in carriers:
        wipe = np.exp(-2j * np.pi * ((f * k / fs) % 1.0))
        for s in range(n_signals):
            spec = np.fft.fft(x[first_sample + s * n:first_sample + (s + 1) * n] * wipe)
            for b in range(n_bins):
                rows.append(sum(wa * np.abs(np.fft.ifft(np.roll(spec, b) * cs)) for wa, cs in zip(w, cspec)))
    return np.stack(rows)


def second_range(code_phase, exclude, period):
    """1-based positions where the second peak is looked for (B1I :141-156, L2C :77-91), code_phase 1-based."""
    e1, e2 = code_phase - exclude, code_phase + exclude
    if e1 < 2:
        return np.arange(e2, period + e1 + 1)
    if e2 >= period:
        return np.arange(e2 - period + 1, e1 + 1)
    return np.concatenate([np.arange(1, e1 + 1), np.arange(e2, period + 1)])


def second_peak(corr, code_phase, exclude, period):
    """(value, 0-based first position) of the second peak; (0.0, -1) where the range is empty."""
    rng = second_range(code_phase, exclude, period)
    rng = rng[(rng >= 1) & (rng <= len(corr))]
    if rng.size == 0:
        return 0.0, -1
    v = np.asarray(corr)[rng - 1]
    m = v.max()
    return float(m), int(np.min(rng[v == m])) - 1


def sequential_row(rowmax, n_carriers, n_signals, n_bins):
    """The reference's loop over (carrier, bin) on the row maxima [rows] -> public row or -1."""
    rm = np.asarray(rowmax, dtype=np.float64).reshape(n_carriers, n_signals, n_bins)
    prevmax, row = 0.0, -1
    for it in range(n_carriers):
        for b in range(n_bins):
            if b == n_bins - 1 and it > 0:
                continue
            if n_signals == 1:
                if rm[it, 0, b] > prevmax:
                    prevmax, row = rm[it, 0, b], it * n_bins + b
            else:
                p1, p2 = rm[it, 0, b], rm[it, 1, b]
                if p1 > prevmax or p2 > prevmax:
                    if p1 > p2:
                        prevmax, row = p1, (it * 2 + 0) * n_bins + b
                    else:
                        prevmax, row = p2, (it * 2 + 1) * n_bins + b
    return row


def pick(surf, n_carriers, n_signals, n_bins, rule, exclude=0, period=0):
    """-> dict(row, code_phase (0-based), peak, second_peak, second_col) of the rule on the float64 surface [rows, n]."""
    surf = np.asarray(surf, dtype=np.float64)
    assert surf.shape[0] == n_carriers * n_signals * n_bins
    if rule == GLOBAL:
        row = int(np.argmax(surf.max(axis=1)))
        col = int(np.argmax(surf.max(axis=0)))
        return dict(row=row, code_phase=col, peak=float(surf.max()), second_peak=0.0, second_col=-1)
    assert n_signals == (2 if rule == SEQUENTIAL_PAIRS else 1)
    row = sequential_row(surf.max(axis=1), n_carriers, n_signals, n_bins)
    if row < 0:
        return dict(row=-1, code_phase=0, peak=0.0, second_peak=0.0, second_col=-1)
    corr = surf[row]
    cp = int(np.argmax(corr))
    sec, sc = second_peak(corr, cp + 1, exclude, period)
    return dict(row=row, code_phase=cp, peak=float(corr[cp]), second_peak=sec, second_col=sc)


def decision_cells(surf, n_carriers, n_signals, n_bins, rule, exclude=0, period=0):
    """The candidates of the decisions behind pick(): (rows' maxima that the rule compares with the chosen row's - the eligible
    rows -, the chosen row, the cells of its second-peak range).  For the clearness checks of the scenes."""
    surf = np.asarray(surf, dtype=np.float64)
    p = pick(surf, n_carriers, n_signals, n_bins, rule, exclude, period)
    rm = surf.max(axis=1).reshape(n_carriers, n_signals, n_bins).copy()
    if rule != GLOBAL:
        rm[1:, :, -1] = -np.inf
    window = np.zeros(0)
    if rule != GLOBAL and p["row"] >= 0:
        rng = second_range(p["code_phase"] + 1, exclude, period)
        window = surf[p["row"]][rng[(rng >= 1) & (rng <= surf.shape[1])] - 1]
    return p, rm.reshape(-1), window


def clear(surf, n_carriers, n_signals, n_bins, rule, exclude, period, eps):
    """True when no other candidate lies within eps * (the decided value) of any decided cell: the runner-up among the eligible rows'
    maxima, among the chosen row's cells (GLOBAL: among all cells), and inside the second-peak range."""
    p, rm, window = decision_cells(surf, n_carriers, n_signals, n_bins, rule, exclude, period)
    if p["row"] < 0:
        return False
    peak = p["peak"]
    if np.sum(rm >= peak * (1.0 - eps)) != 1:
        return False
    cells = surf if rule == GLOBAL else surf[p["row"]]
    if np.sum(cells >= peak * (1.0 - eps)) != 1:
        return False
    return rule == GLOBAL or (window.size > 0 and np.sum(window >= p["second_peak"] * (1.0 - eps)) == 1)
