# -*- coding: utf-8 -*-
"""
Trigger on the GPU engine: coalescence series in, triggered events out -- the reference's ``Trigger``
(quakemigrate/signal/trigger.py) without pandas and obspy, as far as the events go (the summary plot stays with the
reference).

``DeviceTrigger`` carries the reference's parameter names and defaults (trigger.py:213-228).  Per batch it cuts the
series to ``[batchstart - pad, batchend + pad]``, hands the two coalescence series to ``Engine.trigger_series`` --
smoothing, threshold, candidates and merge run there (include/qmhip.h: ``qm_engine_trigger``) -- and applies the host
rules of ``_filter_events`` (trigger.py:641-686): the time window with the midnight rule, the optional region, the
``EventID``.

Time.  The engine compares times as int64 nanoseconds from the first sample of the cut series.  The reference compares
obspy ``UTCDateTime`` values: nanosecond counts to which ``+ seconds`` adds ``round(seconds * 1e9)``, with differences
rounded to 1 us.  The two agree wherever every time is a whole number of microseconds, so the front end refuses, with
``ValueError``, a sampling period, ``marginal_window``, ``min_event_interval`` or ``pad`` that is not one -- and, like
the reference (trigger.py:694-699), ``min_event_interval < 2 * marginal_window``.  Times are naive ``datetime`` in UTC,
as everywhere in this package.
"""

from __future__ import annotations

import csv
import datetime as _dt
import logging
import pathlib

import numpy as np

from quakemigrate_amd import scanmseed

EVENT_COLS = ("EventID", "CoaTime", "TRIG_COA", "COA_X", "COA_Y", "COA_Z", "MinTime", "MaxTime", "COA", "COA_NORM")
OUTPUT_COLS = ("EventID", "CoaTime", "TRIG_COA", "COA_X", "COA_Y", "COA_Z", "COA", "COA_NORM")   # triggered_events.py:22


class NoScanMseedData(ValueError):
    """The series holds no sample inside the batch and its pads."""


def _whole_us(seconds, name):
    us = float(seconds) * 1e6
    if not np.isfinite(us) or abs(us - round(us)) > 1e-6:
        raise ValueError(f"{name} = {seconds} s is not a whole number of microseconds")
    return int(round(us))


def _us(delta):
    return (delta.days * 86400 + delta.seconds) * 1_000_000 + delta.microseconds


def gaussian_weights(sd, truncate):
    """``(r, w)`` of ``scipy.ndimage.gaussian_filter1d(x, sd, truncate=truncate)``: r = int(truncate sd + 0.5),
    w = exp(-0.5 / sd^2 k^2) for k = -r..r over their sum."""
    r = int(truncate * sd + 0.5)
    k = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sd * sd) * k ** 2)
    return r, w / w.sum()


def stamp(t):
    """A time as the reference prints it: ``YYYY-MM-DDTHH:MM:SS.ffffffZ``."""
    return t.strftime("%Y-%m-%dT%H:%M:%S.%f") + "Z"


def event_id(t):
    """trigger.py:624-628: the stamp without ``- : . space Z T``, cut to 17 characters, right-padded with 0."""
    uid = stamp(t)
    for char_ in ["-", ":", ".", " ", "Z", "T"]:
        uid = uid.replace(char_, "")
    return uid[:17].ljust(17, "0")


def triggers(events):
    """The ``(uid, trigger_time)`` list ``MigrationScan.locate_compute`` takes."""
    return [(ev["EventID"], ev["CoaTime"]) for ev in events]


class DeviceTrigger:
    """The reference's ``Trigger`` parameters (names and defaults of trigger.py:213-228); ``threshold_method``
    "dynamic" is taken as "mad", as there."""

    def __init__(self, threshold_method="static", static_threshold=1.5, mad_window_length=3600.0, mad_multiplier=8.0,
                 median_window_length=3600.0, median_multiplier=1.2, marginal_window=2.0, min_event_interval=4.0,
                 normalise_coalescence=False, pad=120.0, smooth_coa=False, smoothing_kernel_sigma=0.2,
                 smoothing_kernel_width=4.0, max_events=65536):
        if threshold_method == "dynamic":
            threshold_method = "mad"
        if threshold_method not in ("static", "mad", "median_ratio"):
            raise ValueError(f"threshold_method must be 'static', 'mad' or 'median_ratio', got {threshold_method!r}")
        self.threshold_method = threshold_method
        self.static_threshold = float(static_threshold)
        self.mad_window_length, self.mad_multiplier = float(mad_window_length), float(mad_multiplier)
        self.median_window_length, self.median_multiplier = float(median_window_length), float(median_multiplier)
        self.marginal_window, self.min_event_interval = float(marginal_window), float(min_event_interval)
        self.normalise_coalescence = bool(normalise_coalescence)
        self.pad = float(pad)
        self.smooth_coa = bool(smooth_coa)
        self.smoothing_kernel_sigma = float(smoothing_kernel_sigma)
        self.smoothing_kernel_width = float(smoothing_kernel_width)
        self.max_events = int(max_events)
        self._mw_us = _whole_us(marginal_window, "marginal_window")
        self._mei_us = _whole_us(min_event_interval, "min_event_interval")
        self._pad_us = _whole_us(pad, "pad")
        if self._mw_us < 0 or self._pad_us < 0:
            raise ValueError("marginal_window and pad must not be negative")
        if self._mei_us < 2 * self._mw_us:
            raise ValueError("Minimum event interval must be >= 2 * marginal window.")
        self.last = None                                    # the engine's answer for the last batch (plots, tests)

    # -- one batch ------------------------------------------------------------------------------------------------
    def _engine_arguments(self, sampling_rate):
        rate = float(sampling_rate)
        if self.threshold_method == "static":
            method, value, chunk = "static", self.static_threshold, 1
        elif self.threshold_method == "mad":
            method, value, chunk = "mad", self.mad_multiplier, int(self.mad_window_length * rate)
        else:
            method, value, chunk = "median_ratio", self.median_multiplier, int(self.median_window_length * rate)
        if method != "static" and chunk < 1:
            raise ValueError(f"the threshold window holds no sample at {rate} Hz")
        weights = None
        if self.smooth_coa:
            _, weights = gaussian_weights(self.smoothing_kernel_sigma * rate, self.smoothing_kernel_width)
        return method, value, chunk, weights

    def trigger_series(self, engine, starttime, sampling_rate, columns, batchstart, batchend, region=None,
                       want_candidates=False):
        """
        One batch (``Trigger._trigger_batch``, trigger.py:318-380).  ``starttime``, ``sampling_rate``, ``columns``: what
        ``scanmseed.read_scanmseed`` returns; ``region``: ``[Xmin, Ymin, Zmin, Xmax, Ymax, Zmax]``.  Returns the events
        as a list of dicts with the reference's ten columns (``EVENT_COLS``); ``CoaTime``, ``MinTime``, ``MaxTime``
        are ``datetime``.  ``self.last`` keeps the engine's answer with ``first_sample`` and ``last_sample``, the cut.
        """
        period_us = _whole_us(1.0 / float(sampling_rate), "the sampling period")
        if period_us < 1:
            raise ValueError(f"sampling_rate {sampling_rate}: the period is below a microsecond")
        n_all = len(columns["COA"])
        pad = _dt.timedelta(microseconds=self._pad_us)
        lo_us, hi_us = _us(batchstart - pad - starttime), _us(batchend + pad - starttime)
        i_lo, i_hi = max(0, -(-lo_us // period_us)), min(n_all - 1, hi_us // period_us)
        if i_hi < i_lo:
            raise NoScanMseedData(f"no sample between {batchstart - pad} and {batchend + pad}")
        # midnight belongs to the next day (trigger.py:343-347); the window read keeps the original batchend + pad
        if batchend.time() == _dt.time(0, 0):
            batchend = batchend - _dt.timedelta(microseconds=period_us)
        if hasattr(columns["COA"], "data_ptr"):          # device-resident series (read_scanmseed, device=True)
            coa, coa_n = columns["COA"][i_lo:i_hi + 1], columns["COA_N"][i_lo:i_hi + 1]
        else:
            coa = np.ascontiguousarray(columns["COA"][i_lo:i_hi + 1], dtype=np.float64)
            coa_n = np.ascontiguousarray(columns["COA_N"][i_lo:i_hi + 1], dtype=np.float64)
        method, value, chunk, weights = self._engine_arguments(sampling_rate)
        out = engine.trigger_series(coa, coa_n, period_us * 1000, self._mw_us * 1000, self._mei_us * 1000,
                                    trigger_on=1 if self.normalise_coalescence else 0, method=method, value=value,
                                    chunk_samples=chunk, weights=weights, max_events=self.max_events,
                                    want_candidates=want_candidates)
        out["first_sample"], out["last_sample"] = i_lo, i_hi
        self.last = out
        t_cut = starttime + _dt.timedelta(microseconds=i_lo * period_us)
        events = []
        for (p, t_min, t_max, _), (trig, c, c_n) in zip(out["events_i"], out["events_f"]):
            at = t_cut + _dt.timedelta(microseconds=int(p) * period_us)
            if not batchstart <= at <= batchend:
                continue
            x, y, z = (float(columns[k][i_lo + int(p)]) for k in ("X", "Y", "Z"))
            if region is not None and not (region[0] <= x <= region[3] and region[1] <= y <= region[4]
                                           and region[2] <= z <= region[5]):
                continue
            events.append({"EventID": event_id(at), "CoaTime": at, "TRIG_COA": float(trig), "COA_X": x, "COA_Y": y,
                           "COA_Z": z, "MinTime": t_cut + _dt.timedelta(microseconds=int(t_min) // 1000),
                           "MaxTime": t_cut + _dt.timedelta(microseconds=int(t_max) // 1000), "COA": float(c),
                           "COA_NORM": float(c_n)})
        return events

    # -- days -----------------------------------------------------------------------------------------------------
    def trigger(self, directory, starttime, endtime, ucf, region=None, engine=None):
        """
        ``Trigger.trigger`` (trigger.py:273-314) over the day files a ``scanmseed.CoalescenceSink`` writes into
        ``directory``: one batch per day between ``starttime`` and ``endtime``, the events of all of them in one
        list.  A batch's window -- the batch and its pads -- is clipped to its own day's file: the pads do not reach
        into the neighbouring days' files (what the reference effectively does for a run of a single day).  A day
        without a file is logged and skipped.  ``engine``: the ``Engine`` to run on; the day files are then decoded on
        it as well and COA / COA_N go from the file to the trigger kernels without a host round trip (default: the
        process's own engine, ``core.lib.default_engine()``, and the Python reader).
        """
        resident = hasattr(engine, "scanmseed_decode")       # (an engine of the caller's that has the device codec)
        if engine is None:
            from quakemigrate_amd.core import lib

            engine = lib.default_engine()
        if starttime > endtime:
            raise ValueError(f"starttime {starttime} is after endtime {endtime}")
        directory = pathlib.Path(directory)
        events = []
        batchstart = starttime
        while batchstart < endtime:
            next_day = _dt.datetime(batchstart.year, batchstart.month, batchstart.day) + _dt.timedelta(days=1)
            batchend = next_day if next_day <= endtime else endtime
            path = directory / f"{batchstart.year}_{batchstart.timetuple().tm_yday:03d}.scanmseed"
            if path.is_file():
                # an engine of the caller's: the file is decoded on it and COA / COA_N stay there for the trigger
                t0, rate, columns = (scanmseed.read_scanmseed(path, ucf, engine=engine, device=True) if resident
                                     else scanmseed.read_scanmseed(path, ucf))
                events += self.trigger_series(engine, t0, rate, columns, batchstart, batchend, region)
            else:
                logging.info(f"\n\t    No .scanmseed file found for day {path.stem}!")
            batchstart = next_day
        return events


# -- TriggeredEvents.csv -----------------------------------------------------------------------------------------------
def _number(v):
    """pandas prints a column of whole values as integers (the reference's COA_Z = 7)."""
    v = float(v)
    return str(int(v)) if v.is_integer() and abs(v) < 1e15 else repr(v)


def write_triggered_events(path, events, write_event_time_windows=False):
    """The reference's ``<run>_<year>_<julday>_TriggeredEvents.csv`` (io/triggered_events.py:106-138): its columns in
    its order, time stamps as ``...ffffffZ``; ``MinTime`` and ``MaxTime`` with ``write_event_time_windows``."""
    cols = list(OUTPUT_COLS) + (["MinTime", "MaxTime"] if write_event_time_windows else [])
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(cols)
        for ev in events:
            w.writerow([ev[c] if c == "EventID" else stamp(ev[c]) if isinstance(ev[c], _dt.datetime)
                        else _number(ev[c]) for c in cols])


def read_triggered_events(path):
    """A ``TriggeredEvents.csv`` back as a list of dicts: ``EventID`` a string, the times ``datetime``, the rest
    floats."""
    events = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            ev = {}
            for k, v in row.items():
                if k == "EventID":
                    ev[k] = v
                elif k in ("CoaTime", "MinTime", "MaxTime"):
                    ev[k] = _dt.datetime.strptime(v, "%Y-%m-%dT%H:%M:%S.%fZ")
                else:
                    ev[k] = float(v)
            events.append(ev)
    return events
