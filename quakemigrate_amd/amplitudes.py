# -*- coding: utf-8 -*-
"""
Local-magnitude amplitudes for located events on the GPU -- the counterpart of ``Amplitude.get_amplitudes``
(quakemigrate/signal/local_mag/amplitude.py:174-371).

The reference walks the Wood-Anderson traces of an event station by station and component by component: an optional
causal Butterworth filter behind a detrend and a taper (``_filter_trace``), three time windows -- noise, P, S
(``_get_amplitude_windows``, ``_measure_noise_amp``) --, each cut, detrended and searched with
``scipy.signal.find_peaks`` for the largest peak-to-trough swing (``_peak_to_trough_amplitude``), an average amplitude
and the filter's gain at the measured frequency.  Here the windows are arithmetic on the host
(:func:`amplitude_windows`, :func:`window_samples`), everything from the filter to the peak/trough pair is ONE call over
all traces (``Engine.measure_amplitudes``, csrc/qm_amplitudes.hpp), and units, frequencies, times and gains follow on
the host.  :class:`DeviceAmplitude` carries the reference's parameter names and returns its table.

Not here: response removal (``Archive.get_wa_waveform``) -- the traces come in as Wood-Anderson displacement in metres
--, ``Magnitude`` (pandas algebra over the table: ``pandas.DataFrame(table_columns).set_index("id")`` is what it takes)
and geodesic distances (an optional ``distance_fn``).
"""

from __future__ import annotations

import fnmatch
import math

import numpy as np

from quakemigrate_amd import preprocess
from quakemigrate_amd.picks import _seconds_since
from quakemigrate_amd.scan import _shift

COLUMNS = ("id", "epi_dist", "z_dist", "P_amp", "P_freq", "P_time", "P_avg_amp", "P_filter_gain", "S_amp", "S_freq",
           "S_time", "S_avg_amp", "S_filter_gain", "Noise_amp", "is_picked")
COMPONENTS = ("[E,2]", "[N,1]", "Z")
NOT_MEASURED, PICK_ORDER = -1, -2           # row-level entries of the table's ``status``


def round_half_away(x):
    """Nearest integer, halves away from zero."""
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def window_samples(start, end, t0, rate, npts):
    """
    Samples ``[lo, hi)`` of a trace of ``npts`` samples at ``rate`` Hz starting at ``t0`` that obspy's
    ``Trace.slice(start, end)`` (nearest sample, both ends included) keeps: ``lo = max(0, round_half_away((start - t0)
    * rate))``, ``hi = min(npts, round_half_away((end - t0) * rate) + 1)``; an empty window is ``lo == hi``.  All times
    in seconds on one axis.  obspy is not a dependency of this package: the rule is written from its documented
    behaviour (``nearest_sample=True``) and is NOT checked against it by a test.
    """
    lo = max(0, round_half_away((start - t0) * rate))
    hi = min(int(npts), round_half_away((end - t0) * rate) + 1)
    lo = min(lo, int(npts))
    return lo, max(hi, lo)


def amplitude_windows(p_pick, s_pick, p_tt, s_tt, marginal_window, fraction_tt, signal_window):
    """
    ``_get_amplitude_windows`` (amplitude.py:590-639) in seconds after the origin time.  ``p_pick`` / ``s_pick``: the
    pick's offset from the origin time, or ``"-1"`` (no pick made: the modelled time ``p_tt`` / ``s_tt`` stands in) or
    ``"No P onset"`` / ``"No S onset"`` (no onset function: the modelled times stand in for BOTH phases).  Returns
    ``(status, [[p_start, p_end], [s_start, s_end]])``: status 0, or 1 where the P pick is not before the S pick
    (the reference's ``PickOrderException``; the windows are ``None`` then).
    """
    for pick, phase in ((p_pick, "P"), (s_pick, "S")):
        if isinstance(pick, str):
            if pick == "-1":
                if phase == "P":
                    p_pick = p_tt
                else:
                    s_pick = s_tt
            elif pick == f"No {phase} onset":
                p_pick, s_pick = p_tt, s_tt
                break
    if not p_pick < s_pick:
        return 1, None
    mw = marginal_window
    p_start = p_pick - mw - p_tt * fraction_tt
    p_end = p_pick + mw + p_tt * fraction_tt
    s_start = s_pick - mw - s_tt * fraction_tt
    s_end = s_pick + mw + s_tt * fraction_tt + signal_window
    if s_start < p_end:
        mid_time = p_end + (s_start - p_end) / 2
        return 0, [[p_start, mid_time], [mid_time, s_end]]
    if s_start - p_end < signal_window:
        return 0, [[p_start, s_start], [s_start, s_end]]
    return 0, [[p_start, p_end + signal_window], [s_start, s_end]]


def station_picks(picks, station, otime):
    """``_get_picks`` (amplitude.py:641-690) on a picker's table (``DevicePicker.pick``; ``None``: nothing was
    picked): ``(p_pick, s_pick, picked)`` with the picks in seconds after ``otime``."""
    out, picked = {}, False
    rows = [] if picks is None else [r for r, s in enumerate(picks["Station"]) if s == station]
    if not rows:
        return "-1", "-1", False
    for phase in ("P", "S"):
        mine = [r for r in rows if picks["Phase"][r] == phase]
        if not mine:
            out[phase] = f"No {phase} onset"
            continue
        t = picks["PickTime"][mine[0]]
        if isinstance(t, (int, float, np.integer, np.floating, str)) and str(t) in ("-1", "-1.0"):
            out[phase] = "-1"
        else:
            out[phase] = _seconds_since(t, otime)
            picked = True
    return out["P"], out["S"], picked


def _field(trace, name):
    return trace[name] if isinstance(trace, dict) else getattr(trace, name)


def _line_detrend(x):
    """The window detrend of the device stage (include/qmhip.h: qm_engine_measure_amplitudes, stage B step 3)."""
    n = len(x)
    i = np.arange(n, dtype=np.float64)
    tbar = 0.5 * (n - 1)
    mean = x.mean()
    sxx = np.sum((i - tbar) ** 2)
    slope = np.sum((i - tbar) * (x - mean)) / sxx if sxx > 0 else 0.0
    return x - (mean + slope * (i - tbar))


class DeviceAmplitude:
    """
    Stands in for ``Amplitude`` where the engine is: the same parameter dictionary (``signal_window``,
    ``noise_window``, ``noise_measure`` "RMS" / "STD" / "ENV", ``loc_method``, ``highpass_filter`` + ``highpass_freq``,
    ``bandpass_filter`` + ``bandpass_lowcut`` / ``bandpass_highcut``, ``filter_corners``, ``prominence_multiplier``),
    the same defaults, the same two ``AttributeError``\\ s and ``pad()``.  ``distance_fn(ev_loc, station)`` ->
    ``(epi_dist, z_dist)`` in kilometres fills the two distance columns (NaN without it); ``ev_loc`` is whatever
    ``get_amplitudes`` was given.  The reference's ``_get_distances`` receives the geographic hypocentre (longitude,
    latitude, depth); ``MigrationScan.locate_compute`` hands over the hypocentre as FRACTIONAL GRID INDICES (the
    location named by ``loc_method``: spline, gaussian, or the covariance fit's expectation over the node spacing) --
    a ``distance_fn`` used there transforms them with its lookup table.
    """

    def __init__(self, amplitude_params=None, distance_fn=None):
        p = dict(amplitude_params or {})
        self.signal_window = p.get("signal_window", 0.0)
        self.noise_window = p.get("noise_window", 5.0)
        self.noise_measure = p.get("noise_measure", "RMS")
        if self.noise_measure not in ("RMS", "STD", "ENV"):
            raise NotImplementedError("Only 'RMS', 'STD' and 'ENV' are available currently.")
        self.prominence_multiplier = p.get("prominence_multiplier", 0.0)
        self.loc_method = p.get("loc_method", "spline")
        self.highpass_filter = p.get("highpass_filter", False)
        if self.highpass_filter:
            try:
                self.highpass_freq = p["highpass_freq"]
            except KeyError as e:
                raise AttributeError(f"Highpass filter frequency not specified! {e}")
        self.bandpass_filter = p.get("bandpass_filter", False)
        if self.bandpass_filter:
            try:
                self.bandpass_lowcut = p["bandpass_lowcut"]
                self.bandpass_highcut = p["bandpass_highcut"]
            except KeyError as e:
                raise AttributeError(f"Bandpass filter frequencies not specified! {e}")
        self.filter_corners = p.get("filter_corners", 4)
        if self.highpass_filter and self.bandpass_filter:
            raise AttributeError("Both bandpass filter *and* highpass filter selected! Please choose one or the "
                                 "other.")
        if any(name in p for name in ("water_level", "pre_filt", "remove_full_response")):
            raise AttributeError("The response removal parameters ('water_level', 'pre_filt', "
                                 "'remove_full_response') belong to the Archive object.")
        self.distance_fn = distance_fn

    def pad(self, marginal_window, max_tt, fraction_tt):
        """``Amplitude.pad`` (amplitude.py:1011-1051): ``(pre_pad, post_pad)`` in seconds around the origin time."""
        pre_pad = self.noise_window + marginal_window
        post_pad = self.signal_window + max_tt * (1 + fraction_tt) + marginal_window
        timespan = pre_pad + post_pad
        pre_pad += np.ceil(timespan * 0.06)
        post_pad += np.ceil(timespan * 0.06)
        return pre_pad, post_pad

    def filter_sos(self, rate):
        """``_filter_trace``'s choice for a trace at ``rate`` Hz (amplitude.py:432-439, :470-475): the band-pass, the
        high-pass at ``bandpass_lowcut`` where ``bandpass_highcut`` reaches the Nyquist frequency, the high-pass, or
        ``None`` without a filter."""
        if self.bandpass_filter:
            if self.bandpass_highcut / (0.5 * rate) - 1.0 > -1e-6:
                return preprocess.butter_highpass_sos(self.bandpass_lowcut, rate, self.filter_corners)
            return preprocess.butter_bandpass_sos(self.bandpass_lowcut, self.bandpass_highcut, rate,
                                                  self.filter_corners)
        if self.highpass_filter:
            return preprocess.butter_highpass_sos(self.highpass_freq, rate, self.filter_corners)
        return None

    def plan(self, wa_traces, stations, picks, otime, marginal_window, p_ttimes, s_ttimes, fraction_tt,
             tr_start=None, tr_end=None):
        """
        The host half in front of the launch: per (station, component) row the trace that qualifies
        (amplitude.py:316-332: exactly one, and -- where ``tr_start`` / ``tr_end``, the window that was read, are
        given -- trimmed to it and covering it to within a sample), its filter and taper, its three windows in
        samples.  Returns a dict: ``rows`` (per row ``None`` or the index of its trace record), ``ids``, ``picked``,
        ``row_status``, ``data`` (the traces to pack), ``starts``, ``rates``, ``trace_records``, ``window_records``
        (three per measured row: noise, P, S), ``sos`` (n_filters, n_sections, 6: cascades of fewer sections are
        filled up with identity sections), ``gain_sos`` (per filter, as designed), ``taper_table``,
        ``taper_weights``.
        """
        rows, ids, picked, row_status = [], [], [], []
        data, starts, rates, trecs, wrecs, windows = [], [], [], [], [], []
        filters, gain_sos, tapers, table, weights = {}, [], {}, [], []
        offset = 0
        for i, station in enumerate(stations):
            mine = [tr for tr in wa_traces if _field(tr, "station") == station]
            p_pick, s_pick, was_picked = station_picks(picks, station, otime)
            w_status, w = amplitude_windows(p_pick, s_pick, float(p_ttimes[i]), float(s_ttimes[i]),
                                            float(marginal_window), float(fraction_tt), self.signal_window)
            for comp in COMPONENTS:
                found = [tr for tr in mine if fnmatch.fnmatchcase(str(_field(tr, "component")), comp)]
                tr = found[0] if len(found) == 1 else None
                x = t0 = None
                if tr is not None:
                    rate = float(_field(tr, "sampling_rate"))
                    x = np.asarray(_field(tr, "data"), dtype=np.float64)
                    t0 = _field(tr, "starttime")
                    if tr_start is not None:
                        lo, hi = window_samples(_seconds_since(tr_start, t0), _seconds_since(tr_end, t0), 0.0, rate,
                                                len(x))
                        x, t0 = x[lo:hi], _shift(t0, lo / rate)
                        covered = (len(x) > 0 and _seconds_since(t0, tr_start) < 1.0 / rate
                                   and _seconds_since(tr_end, _shift(t0, (len(x) - 1) / rate)) < 1.0 / rate)
                        if not covered:
                            tr = None
                    elif len(x) == 0:
                        tr = None
                if tr is None or w_status:
                    rows.append(None)
                    ids.append(f".{station}..{comp}" if tr is None else _field(tr, "id"))
                    picked.append(False)
                    row_status.append(NOT_MEASURED if tr is None else PICK_ORDER)
                    windows.append(np.full((3, 2), -1))
                    continue
                ids.append(_field(tr, "id"))
                n = len(x)
                f = t = -1
                sos = self.filter_sos(rate)
                if sos is not None:
                    if rate not in filters:
                        filters[rate] = len(gain_sos)
                        gain_sos.append(sos)
                    f = filters[rate]
                    if n not in tapers:
                        left, right = preprocess.cosine_taper_sides(n, 0.05)
                        tapers[n] = -1
                        if len(left):
                            tapers[n] = len(table)
                            table.append([len(weights), len(left)])
                            weights.extend(left)
                            weights.extend(right)
                    t = tapers[n]
                since = _seconds_since(t0, otime)
                bounds = [window_samples(w[0][0] - self.noise_window, w[0][0], since, rate, n),
                          window_samples(w[0][0], w[0][1], since, rate, n),
                          window_samples(w[1][0], w[1][1], since, rate, n)]
                k = len(trecs)
                rows.append(k)
                picked.append(was_picked)
                row_status.append(0)
                windows.append(np.array(bounds))
                trecs.append([offset, n, f, t])
                wrecs.extend([k, lo, hi, kind] for (lo, hi), kind in zip(bounds, (0, 1, 1)))
                data.append(x)
                starts.append(t0)
                rates.append(rate)
                offset += n
        n_sections = max((len(s) for s in gain_sos), default=1)
        identity = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
        sos = np.array([np.vstack([s] + [identity] * (n_sections - len(s))) for s in gain_sos])
        return dict(rows=rows, ids=ids, picked=picked, row_status=row_status,
                    windows=np.array(windows).reshape(-1, 3, 2), data=data, starts=starts, rates=rates,
                    trace_records=np.array(trecs, dtype=np.int64).reshape(-1, 4),
                    window_records=np.array(wrecs, dtype=np.int64).reshape(-1, 4),
                    sos=sos.reshape(-1, n_sections, 6), gain_sos=gain_sos,
                    taper_table=np.array(table, dtype=np.int32).reshape(-1, 2),
                    taper_weights=np.array(weights, dtype=np.float64))

    def _envelope_average(self, y, kind):
        """``noise_measure = "ENV"`` (amplitude.py:999) over one window of the filtered trace, on the host."""
        from scipy.signal import hilbert

        if len(y) == 0 or not np.all(np.isfinite(y)):
            return np.nan
        if kind == 0 and y.max() == y.min():
            return np.nan
        y = _line_detrend(y)
        if kind == 1 and y.max() == y.min():
            return np.nan
        return float(np.mean(np.abs(hilbert(y))))

    def get_amplitudes(self, engine, wa_traces, stations, picks, otime, marginal_window, p_ttimes, s_ttimes,
                       fraction_tt, ev_loc=None, tr_start=None, tr_end=None):
        """
        The amplitude table of one located event.  ``wa_traces``: the Wood-Anderson displacement traces (metres) of
        the event's window, objects or dicts with ``id, station, component, starttime, sampling_rate, data``;
        ``stations``: the lookup table's station names, in its order; ``picks``: the picker's table
        (``DevicePicker.pick``) or ``None``; ``otime``: the origin time; ``p_ttimes`` / ``s_ttimes`` (n_stations,):
        seconds from the hypocentre; ``tr_start`` / ``tr_end``: the window that was read (``otime -/+ pad()``) -- with
        them the traces are trimmed to it and a trace that does not cover it is left out, as in the reference.

        Returns a dict of arrays, one entry per (station, component) row in the reference's order (station-major,
        components ``[E,2]``, ``[N,1]``, ``Z``): the reference's 15 columns (``COLUMNS``; NaN and ``.STATION..COMP``
        ids where a row is missing, gappy or too short, amplitude.py:316-332) and ``status`` (n_rows, 3) -- the device
        status of the noise, P and S window, ``-1`` for a row without a usable trace, ``-2`` where the P pick is not
        before the S pick -- and ``windows`` (n_rows, 3, 2), the windows' sample bounds.
        """
        plan = self.plan(wa_traces, stations, picks, otime, marginal_window, p_ttimes, s_ttimes, fraction_tt,
                         tr_start, tr_end)
        n_rows = len(plan["rows"])
        table = {name: np.full(n_rows, np.nan, dtype=object if name in ("id", "P_time", "S_time") else np.float64)
                 for name in COLUMNS}
        table["id"][:] = plan["ids"]
        table["is_picked"] = np.array(plan["picked"], dtype=bool)
        status = np.repeat(np.array(plan["row_status"], dtype=np.int32)[:, None], 3, axis=1)
        for r, station in enumerate(np.repeat(np.asarray(stations, dtype=object), 3)):
            if self.distance_fn is not None:
                table["epi_dist"][r], table["z_dist"][r] = self.distance_fn(ev_loc, station)
        table.update(status=status, windows=plan["windows"])
        if not len(plan["trace_records"]):
            return table
        envelope = self.noise_measure == "ENV"
        out = engine.measure_amplitudes(
            plan["data"], plan["trace_records"], plan["window_records"], sos=plan["sos"] if len(plan["sos"]) else None,
            taper_table=plan["taper_table"], taper_weights=plan["taper_weights"], detrend_windows=True,
            average_method="RMS" if envelope else self.noise_measure,
            prominence_multiplier=self.prominence_multiplier, want_filtered=envelope)
        values, index = out[0], out[1]
        for r, k in enumerate(plan["rows"]):
            if k is None:
                continue
            offset, _, f, _ = plan["trace_records"][k]
            rate, start = plan["rates"][k], plan["starts"][k]
            status[r] = index[3 * k:3 * k + 3, 0]
            average = values[3 * k:3 * k + 3, 1].copy()
            if envelope:
                for j, (lo, hi) in enumerate(plan["windows"][r]):
                    average[j] = self._envelope_average(out[2][offset + lo:offset + hi], 0 if j == 0 else 1)
            if status[r, 0] == 0:
                table["Noise_amp"][r] = average[0] * 1000.0
            for j, phase in ((1, "P"), (2, "S")):
                if status[r, j] != 0:
                    continue
                peak, trough = int(index[3 * k + j, 1]), int(index[3 * k + j, 2])
                half_amp = values[3 * k + j, 0] * 1000 / 2
                approx_freq = 1.0 / (abs(peak - trough) / rate * 2.0)
                average_amp = average[j] * 1000.0
                gain = np.nan
                if f >= 0:
                    from scipy.signal import sosfreqz

                    gain = float(np.abs(sosfreqz(plan["gain_sos"][f], worN=[approx_freq], fs=rate)[1][0]))
                    if not gain:
                        continue
                    half_amp /= gain
                    average_amp /= gain
                table[f"{phase}_amp"][r], table[f"{phase}_freq"][r] = half_amp, approx_freq
                table[f"{phase}_time"][r] = _shift(start, (peak + (trough - peak) / 2) / rate)
                table[f"{phase}_avg_amp"][r], table[f"{phase}_filter_gain"][r] = average_amp, gain
        return table
