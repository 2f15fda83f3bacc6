# -*- coding: utf-8 -*-
"""
NumPy restatement of the amplitude stage (include/qmhip.h: qm_engine_measure_amplitudes) and of the host rules of
``quakemigrate_amd.amplitudes.DeviceAmplitude`` -- the specification the GPU tests compare against, written from the
reference's text (quakemigrate/signal/local_mag/amplitude.py).  tests/test_amplitudes_host.py pins the extrema to
``scipy.signal.find_peaks``, the pairing to a literal transcription of amplitude.py:858-901, the filter to
``scipy.signal.sosfilt`` and the window detrend to ``scipy.signal.detrend``.
"""

import math

import numpy as np

import preprocess_ref as pp

MEASURED, EMPTY_OR_FLAT, NO_EXTREMUM, CONSECUTIVE, EQUAL_PAIR, NON_FINITE = range(6)


# ---- stage A -----------------------------------------------------------------------------------------------------
def line_detrend(x):
    """The least-squares line over i = 0..n-1 subtracted in its centred form; no second demean."""
    return pp.detrend(x, also_mean=False)


def filter_trace(x, sos, weights=None):
    """Line detrend, the taper's two ramps (``weights``: left ramp then right ramp, or None), one forward pass."""
    y = line_detrend(x)
    if weights is not None and len(weights):
        m = len(weights) // 2
        y = pp.taper(y, weights[:m], weights[m:])
    return pp.sosfilt(sos, y)


# ---- stage B -----------------------------------------------------------------------------------------------------
def local_maxima(y):
    """SciPy's ``_local_maxima_1d``: the midpoints of the samples or plateaus strictly above both neighbours."""
    found = []
    n = len(y)
    i = 1
    while i < n - 1:
        if y[i - 1] < y[i]:
            ahead = i + 1
            while ahead < n - 1 and y[ahead] == y[i]:
                ahead += 1
            if y[ahead] < y[i]:
                found.append((i + ahead - 1) // 2)
                i = ahead
        i += 1
    return np.array(found, dtype=np.int64)


def prominence(y, peak):
    """SciPy's ``_peak_prominences`` without ``wlen`` for one peak."""
    left = right = y[peak]
    i = peak
    while i >= 0 and y[i] <= y[peak]:
        left = min(left, y[i])
        i -= 1
    i = peak
    while i < len(y) and y[i] <= y[peak]:
        right = min(right, y[i])
        i += 1
    return y[peak] - max(left, right)


def extrema(y, need=0.0):
    """(peaks, troughs) of ``find_peaks(y, prominence=need)`` and ``find_peaks(-y, prominence=need)``; ``need`` 0:
    nothing is filtered."""
    out = []
    for v in (y, -y):
        found = local_maxima(v)
        if need > 0.0:
            found = np.array([p for p in found if prominence(v, p) >= need], dtype=np.int64)
        out.append(found)
    return out


def pair(y, peaks, troughs):
    """amplitude.py:862-901 on the two lists: (status, full_amp, peak, trough)."""
    n_p, n_t = len(peaks), len(troughs)
    if n_p == 0 or n_t == 0:
        return NO_EXTREMUM, 0.0, -1, -1
    if n_p == 1 and n_t == 1:
        full = abs(y[peaks[0]] - y[troughs[0]])
        if not full:
            return EQUAL_PAIR, 0.0, -1, -1
        return MEASURED, full, int(peaks[0]), int(troughs[0])
    if n_p == n_t:
        if peaks[0] < troughs[0]:
            a, b, c, d = peaks, troughs, peaks[1:], troughs[:-1]
        else:
            a, b, c, d = peaks, troughs, peaks[:-1], troughs[1:]
    elif abs(n_p - n_t) != 1:
        return CONSECUTIVE, 0.0, -1, -1
    elif n_p > n_t:
        if not peaks[0] < troughs[0]:
            return CONSECUTIVE, 0.0, -1, -1
        a, b, c, d = peaks[:-1], troughs, peaks[1:], troughs
    else:
        if not peaks[0] > troughs[0]:
            return CONSECUTIVE, 0.0, -1, -1
        a, b, c, d = peaks, troughs[1:], peaks, troughs[:-1]
    fp1, fp2 = np.abs(y[a] - y[b]), np.abs(y[c] - y[d])
    if np.max(fp1) >= np.max(fp2):
        pos = int(np.argmax(fp1))
        return MEASURED, float(fp1[pos]), int(a[pos]), int(b[pos])
    pos = int(np.argmax(fp2))
    return MEASURED, float(fp2[pos]), int(c[pos]), int(d[pos])


def average(y, method):
    if method == "RMS":
        return float(np.sqrt(np.mean(np.square(y))))
    return float(np.std(y))


def measure_window(x, kind, detrend=True, method="RMS", multiplier=0.0, lo=0):
    """One window record: (values (4,), index (4,)); ``lo`` is added to the two sample indices."""
    x = np.asarray(x, dtype=np.float64)
    values, index = np.zeros(4), np.array([MEASURED, -1, -1, 0], dtype=np.int32)
    if len(x) == 0:
        index[0] = EMPTY_OR_FLAT
        return values, index
    if not np.all(np.isfinite(x)):
        index[0] = NON_FINITE
        return values, index
    if kind == 0 and x.max() == x.min():
        index[0] = EMPTY_OR_FLAT
        return values, index
    y = line_detrend(x) if detrend else x
    if kind == 1 and y.max() == y.min():
        index[0] = EMPTY_OR_FLAT
        return values, index
    values[1], values[2] = average(y, method), np.max(np.abs(y))
    if kind == 1:
        peaks, troughs = extrema(y, multiplier * values[2] if multiplier > 0.0 else 0.0)
        status, full, p, t = pair(y, peaks, troughs)
        values[0] = full
        index[:] = status, (lo + p if p >= 0 else -1), (lo + t if t >= 0 else -1), len(peaks)
    return values, index


def measure(traces, trace_records, window_records, sos=None, taper_table=None, taper_weights=None, detrend=True,
            method="RMS", multiplier=0.0):
    """``qm_engine_measure_amplitudes``: ``traces`` a list of 1-D arrays in the records' order.  Returns (values
    (n_windows, 4), index (n_windows, 4), the traces as stage B saw them)."""
    seen = []
    for x, (_, n, f, t) in zip(traces, trace_records):
        x = np.asarray(x, dtype=np.float64)
        assert len(x) == n
        if f >= 0:
            w = None
            if t >= 0:
                off, m = taper_table[t]
                w = np.asarray(taper_weights)[off:off + 2 * m]
            x = filter_trace(x, sos[f], w)
        seen.append(x)
    values = np.zeros((len(window_records), 4))
    index = np.zeros((len(window_records), 4), dtype=np.int32)
    for k, (tr, lo, hi, kind) in enumerate(window_records):
        values[k], index[k] = measure_window(seen[tr][lo:hi], kind, detrend, method, multiplier, lo)
    return values, index, seen


def pack(traces):
    """(packed 1-D array, offsets) of a list of traces laid end to end."""
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in traces])])[:-1]
    return np.concatenate([np.asarray(x, dtype=np.float64) for x in traces]), offsets.astype(np.int64)


# ---- designed rows: one window per pairing case ----------------------------------------------------------------------
def designed_rows():
    """name -> (samples, multiplier, expected status): every branch of amplitude.py:862-901, multiplier 0 and 0.3."""
    rows = {
        # P == T == 1
        "one_pair": ([0, 3, 1, -2, 0], 0.0, MEASURED),
        # P == T, peak first / trough first; the winner from fp2
        "equal_peak_first": ([0, 2, -1, 5, -4, 0], 0.0, MEASURED),           # fp1: 3, 9; fp2: |5 - -1| = 6
        "equal_trough_first": ([0, -2, 1, -5, 4, 0], 0.0, MEASURED),
        "winner_fp2": ([0, 1, -8, 7, 5, 6, 0, 3], 0.0, MEASURED),                # fp1: 9, 2, 6; fp2: 15, 1
        # P == T + 1, T == P + 1
        "more_peaks": ([0, 2, -3, 4, 0], 0.0, MEASURED),
        "more_troughs": ([0, -2, 3, -4, 0], 0.0, MEASURED),
        # fp1 == fp2 exactly: fp1 wins, first argmax
        "tie": ([0, 4, -4, 4, -4, 0], 0.0, MEASURED),
        # no extremum: monotone
        "monotone": ([0, 1, 2, 3, 4], 0.0, NO_EXTREMUM),
        # consecutive: three prominent peaks of EQUAL height over one prominent trough (a prominence walk passes
        # samples as high as its peak, so the shallow dips between them are filtered out and the peaks are not)
        "three_over_one": ([0, 10, 9, 10, 9, 10, -12, 0, -0.1, 0], 0.3, CONSECUTIVE),
        # consecutive: two peaks, one trough, the trough first
        "trough_first_two_peaks": ([5, -12, 9, 8, 9, 0], 0.3, CONSECUTIVE),
        "empty": ([], 0.0, EMPTY_OR_FLAT),
        "flat": ([2, 2, 2, 2], 0.0, EMPTY_OR_FLAT),
        "non_finite": ([0, 1, np.nan, 2, 0], 0.0, NON_FINITE),
    }
    return {k: (np.array(v[0], dtype=np.float64), v[1], v[2]) for k, v in rows.items()}


# ---- DeviceAmplitude's host rules -----------------------------------------------------------------------------------
def round_half_away(x):
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def window_samples(start, end, t0, rate, npts):
    lo = min(max(0, round_half_away((start - t0) * rate)), npts)
    hi = min(npts, round_half_away((end - t0) * rate) + 1)
    return lo, max(lo, hi)


def amplitude_windows(p_pick, s_pick, p_tt, s_tt, mw, fraction_tt, signal_window):
    """amplitude.py:590-639 in seconds after the origin time; picks as numbers, "-1" or "No <phase> onset"."""
    if "No P onset" == p_pick or "No S onset" == s_pick:
        # (the loop breaks at the first missing onset; a "-1" P before a missing S onset is replaced either way)
        p_pick, s_pick = p_tt, s_tt
    else:
        p_pick = p_tt if isinstance(p_pick, str) else p_pick
        s_pick = s_tt if isinstance(s_pick, str) else s_pick
    if not p_pick < s_pick:
        return 1, None
    p_start, p_end = p_pick - mw - p_tt * fraction_tt, p_pick + mw + p_tt * fraction_tt
    s_start, s_end = s_pick - mw - s_tt * fraction_tt, s_pick + mw + s_tt * fraction_tt + signal_window
    if s_start < p_end:
        mid = p_end + (s_start - p_end) / 2
        return 0, [[p_start, mid], [mid, s_end]]
    if s_start - p_end < signal_window:
        return 0, [[p_start, s_start], [s_start, s_end]]
    return 0, [[p_start, p_end + signal_window], [s_start, s_end]]


def trace_table_row(x, rate, since, windows, noise_window, sos=None, weights=None, method="RMS", multiplier=0.0):
    """One measured trace (``since``: its first sample in seconds after the origin time; ``windows`` from
    amplitude_windows): a dict of the row's P_*, S_* and Noise_amp entries -- times as seconds after the trace's first
    sample -- and the three statuses."""
    from scipy.signal import sosfreqz

    y = filter_trace(x, sos, weights) if sos is not None else np.asarray(x, dtype=np.float64)
    n = len(y)
    row = {"status": [], "bounds": []}
    bounds = [window_samples(windows[0][0] - noise_window, windows[0][0], since, rate, n),
              window_samples(windows[0][0], windows[0][1], since, rate, n),
              window_samples(windows[1][0], windows[1][1], since, rate, n)]
    for (lo, hi), name in zip(bounds, ("Noise", "P", "S")):
        values, index = measure_window(y[lo:hi], 0 if name == "Noise" else 1, True, method, multiplier, lo)
        row["status"].append(int(index[0]))
        row["bounds"].append((lo, hi))
        if index[0] != MEASURED:
            continue
        if name == "Noise":
            row["Noise_amp"] = values[1] * 1000.0
            continue
        half, avg = values[0] * 1000 / 2, values[1] * 1000.0
        freq = 1.0 / (abs(int(index[1]) - int(index[2])) / rate * 2.0)
        gain = np.nan
        if sos is not None:
            gain = float(np.abs(sosfreqz(sos, worN=[freq], fs=rate)[1][0]))
            if not gain:
                continue
            half, avg = half / gain, avg / gain
        row.update({f"{name}_amp": half, f"{name}_freq": freq, f"{name}_avg_amp": avg, f"{name}_filter_gain": gain,
                    f"{name}_time": (index[1] + (int(index[2]) - int(index[1])) / 2) / rate})
    return row


# ---- test families ---------------------------------------------------------------------------------------------------
def family(seed=5, n_traces=12):
    """Traces of unequal lengths between 300 and 2000 at two rates, three windows each (noise, P, S)."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(300, 2001, size=n_traces)
    lengths[0], lengths[1] = 300, 2000
    traces, windows = [], []
    for k, n in enumerate(lengths):
        t = np.arange(n, dtype=np.float64)
        x = 1e-3 * rng.standard_normal(n) + 3e-7 * t + 2e-4
        centre = n // 2
        x += 5e-3 * np.exp(-0.5 * ((t - centre) / 20.0) ** 2) * np.sin(0.7 * (t - centre))
        traces.append(x)
        a, b, c = sorted(rng.integers(1, n - 1, size=3))
        windows += [[k, 0, a, 0], [k, a, b, 1], [k, b, n, 1]]
    packed, offsets = pack(traces)
    records = np.stack([offsets, lengths, np.full(n_traces, -1), np.full(n_traces, -1)], axis=1).astype(np.int64)
    rates = np.where(np.arange(n_traces) % 2 == 0, 100.0, 50.0)
    return dict(traces=traces, packed=packed, trace_records=records,
                window_records=np.array(windows, dtype=np.int64), rates=rates)


# ---- a synthetic event for DeviceAmplitude ---------------------------------------------------------------------------
def synthetic_event(seed=11):
    """Three stations around an origin time: A picked on both phases, B not picked (its N component has a gap: two
    traces; its Z component runs at 40 Hz), C with its P pick after its S pick (components named 2, 1, Z).  Traces as
    dicts; picks as a picker's table."""
    import datetime as dt

    rng = np.random.default_rng(seed)
    t0 = dt.datetime(2024, 5, 17, 10, 0, 0)
    otime = t0 + dt.timedelta(seconds=20)
    stations = ["A", "B", "C"]
    p_tt, s_tt = [2.0, 3.0, 2.5], [3.6, 5.4, 4.5]
    picks = {"Station": np.array(["A", "A", "C", "C"], dtype=object), "Phase": np.array(["P", "S", "P", "S"], dtype=object),
             "PickTime": np.array([otime + dt.timedelta(seconds=2.1), otime + dt.timedelta(seconds=3.5),
                                   otime + dt.timedelta(seconds=4.6), otime + dt.timedelta(seconds=4.4)], dtype=object)}
    traces = []

    def add(station, comp, rate, start_s, seconds, k):
        n = int(seconds * rate) + 1
        t = np.arange(n) / rate + start_s                   # seconds after the origin time
        x = 3e-7 * rng.standard_normal(n) + 1e-8 * t + 2e-7
        for j, at in enumerate((p_tt[k], s_tt[k])):
            since = np.clip(t - at, 0.0, None)
            x += (1 + 2 * j) * 2e-5 * since * np.exp(-2.5 * since) * np.sin(2 * np.pi * (5.0 - j) * since)
        traces.append(dict(id=f"XX.{station}..HH{comp}", station=station, component=comp,
                           starttime=otime + dt.timedelta(seconds=start_s), sampling_rate=float(rate), data=x))

    for k, station in enumerate(stations):
        names = ("2", "1", "Z") if station == "C" else ("E", "N", "Z")
        for comp in names:
            rate = 40 if (station, comp) == ("B", "Z") else 100
            if (station, comp) == ("B", "N"):
                add(station, comp, rate, -9.0, 10.0, k)
                add(station, comp, rate, 2.0, 20.0, k)
            else:
                add(station, comp, rate, -9.0 - 0.003 * k, 31.0, k)
    return dict(stations=stations, p_tt=p_tt, s_tt=s_tt, picks=picks, traces=traces, otime=otime, mw=0.5,
                fraction_tt=0.1, pick_offsets={"A": (2.1, 3.5), "B": ("-1", "-1"), "C": (4.6, 4.4)})


def expected_rows(ev, sos_of_rate, noise_window=5.0, signal_window=0.0, method="RMS", multiplier=0.0, trim=None):
    """The table of ``DeviceAmplitude.get_amplitudes`` over ``synthetic_event`` by the restatement: a list of 9 rows
    (dicts; ``id``, ``is_picked``, ``status`` and, where measured, the columns of ``trace_table_row`` with times as
    seconds after the origin time).  ``sos_of_rate(rate)``: the filter or None; ``trim``: (start, end) in seconds after
    the origin time."""
    from quakemigrate_amd.preprocess import cosine_taper_sides

    rows = []
    for k, station in enumerate(ev["stations"]):
        status, windows = amplitude_windows(*ev["pick_offsets"][station], ev["p_tt"][k], ev["s_tt"][k], ev["mw"],
                                            ev["fraction_tt"], signal_window)
        for pattern in ("E2", "N1", "Z"):
            found = [tr for tr in ev["traces"] if tr["station"] == station and tr["component"] in pattern]
            if len(found) != 1:
                rows.append(dict(id=f".{station}..[{pattern[0]},{pattern[1]}]" if len(pattern) == 2
                                 else f".{station}..{pattern}", is_picked=False, status=[-1, -1, -1]))
                continue
            tr = found[0]
            if status:
                rows.append(dict(id=tr["id"], is_picked=False, status=[-2, -2, -2]))
                continue
            rate, x = tr["sampling_rate"], tr["data"]
            since = (tr["starttime"] - ev["otime"]).total_seconds()
            if trim is not None:
                lo, hi = window_samples(trim[0], trim[1], since, rate, len(x))
                x, since = x[lo:hi], since + lo / rate
            sos = sos_of_rate(rate)
            weights = np.concatenate(cosine_taper_sides(len(x))) if sos is not None else None
            row = trace_table_row(x, rate, since, windows, noise_window, sos, weights, method, multiplier)
            for name in ("P_time", "S_time"):
                if name in row:
                    row[name] += since
            row.update(id=tr["id"], is_picked=station == "A", start=since, rate=rate)
            rows.append(row)
    return rows


class RestatedEngine:
    """``Engine.measure_amplitudes`` answered by the restatement."""

    def measure_amplitudes(self, traces, trace_records, window_records, sos=None, taper_table=None,
                           taper_weights=None, detrend_windows=True, average_method="RMS", prominence_multiplier=0.0,
                           want_filtered=False):
        values, index, seen = measure(traces, trace_records, window_records, sos, taper_table, taper_weights,
                                      detrend_windows, average_method, prominence_multiplier)
        if not want_filtered:
            return values, index
        packed = np.zeros(int(max(r[0] + r[1] for r in trace_records)))
        for r, x in zip(trace_records, seen):
            packed[r[0]:r[0] + r[1]] = x
        return values, index, packed


def compare_table(table, rows, otime, rel=0.0):
    """``DeviceAmplitude.get_amplitudes``' table against ``expected_rows``: ids, picked flags, statuses, the NaN pattern,
    frequencies and times equal; amplitudes within ``rel`` (relative; None: only their NaN pattern).  Returns the number of measured P / S entries."""
    assert len(table["id"]) == len(rows)
    measured = 0
    for r, want in enumerate(rows):
        assert table["id"][r] == want["id"] and bool(table["is_picked"][r]) == want["is_picked"], r
        assert list(table["status"][r]) == list(want["status"]), (r, table["status"][r], want["status"])
        for name in ("Noise_amp", "P_amp", "P_freq", "P_avg_amp", "P_filter_gain", "S_amp", "S_freq", "S_avg_amp",
                     "S_filter_gain"):
            got, exp = float(table[name][r]), float(want.get(name, np.nan))
            assert np.isnan(got) == np.isnan(exp), (r, name, got, exp)
            if np.isnan(exp):
                continue
            if name.endswith("_freq") or name.endswith("_gain"):
                assert got == exp, (r, name, got, exp)
            elif rel is not None:
                assert abs(got - exp) <= rel * abs(exp), (r, name, got, exp)
        for name in ("P_time", "S_time"):
            if name in want:
                measured += 1
                assert abs((table[name][r] - otime).total_seconds() - want[name]) < 2e-6, (r, name)
            else:
                assert isinstance(table[name][r], float) and np.isnan(table[name][r]), (r, name)
        assert np.isnan(table["epi_dist"][r]) and np.isnan(table["z_dist"][r])
    return measured


# ---- error bounds of the table's amplitudes --------------------------------------------------------------------------
U = 2.0 ** -53
_L1 = {}


def row_bounds(x, sos, bounds):
    """
    Per window of one trace the bounds (peak-to-trough, RMS average) in input units on what two evaluations of the
    stage may differ by when they add the detrends' sums in different orders.  ``x``: the trace as given; ``sos``: its
    filter or None; ``bounds``: the windows' ``(lo, hi)``.
      * the filtered samples differ by at most d = |h|_1 4 n 2^-53 max|x| (the filter stage's bound; 0 without a
        filter);
      * the window detrend of samples that differ by d: the mean moves by at most d and the line's slope term by at
        most 3 n / (2 (n + 1)) d < 1.5 d (sum |i - tbar| <= n^2 / 4 over sum (i - tbar)^2 = n (n^2 - 1) / 12, times
        (n - 1) / 2), so the detrended samples differ by at most 3.5 d, plus the detrend's own bound
        4 n_w 2^-53 max|y_w|: e;
      * the peak-to-trough is a difference of two such samples: 2 e; the RMS moves by at most e and pays
        2 n_w 2^-53 of itself for the order of its own sum.
    """
    from quakemigrate_amd.preprocess import cosine_taper_sides

    x = np.asarray(x, dtype=np.float64)
    n, d, y = len(x), 0.0, x
    if sos is not None:
        key = (np.asarray(sos).tobytes(), n)
        if key not in _L1:
            _L1[key] = pp.impulse_l1(sos, n)
        d = _L1[key] * 4 * n * U * np.max(np.abs(x))
        y = filter_trace(x, sos, np.concatenate(cosine_taper_sides(n)))
    out = []
    for lo, hi in bounds:
        w = y[lo:hi]
        if len(w) == 0:
            out.append((0.0, 0.0))
            continue
        e = 3.5 * d + 4 * len(w) * U * np.max(np.abs(w))
        out.append((2 * e, e + 2 * len(w) * U * average(line_detrend(w), "RMS")))
    return out


def table_within_bounds(amp, plan, table, want):
    """``table`` (the device's) against ``want`` (the same host code over the restatement) entry by entry within
    ``row_bounds`` -- in millimetres, halved for the amplitudes, over the filter gain where there is one.  RMS
    averages only.  Returns (entries checked, worst error / bound)."""
    checked, worst = 0, 0.0
    for r, k in enumerate(plan["rows"]):
        if k is None:
            continue
        f = int(plan["trace_records"][k][2])
        limits = row_bounds(plan["data"][k], plan["gain_sos"][f] if f >= 0 else None, plan["windows"][r])
        for (b_amp, b_avg), name in zip(limits, ("Noise", "P", "S")):
            entries = [("Noise_amp", b_avg * 1000.0)] if name == "Noise" else \
                [(f"{name}_amp", b_amp * 1000.0 / 2), (f"{name}_avg_amp", b_avg * 1000.0)]
            gain = 1.0 if name == "Noise" or f < 0 else float(want[f"{name}_filter_gain"][r])
            for column, bound in entries:
                got, exp = float(table[column][r]), float(want[column][r])
                assert np.isnan(got) == np.isnan(exp), (r, column)
                if np.isnan(exp):
                    continue
                err = abs(got - exp)
                assert err <= bound / gain, (r, column, got, exp, err, bound / gain)
                checked += 1
                worst = max(worst, err * gain / bound)
    return checked, worst
