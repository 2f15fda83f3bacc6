# -*- coding: utf-8 -*-
"""
What the device's resampling, pre-processing and onset stages are set up from: the filter coefficients, the taper
ramps, :class:`OnsetStage`, the description of one onset function's stage that ``Engine.preprocess`` /
``Engine.onsets`` and the pipeline (``StreamingDetector(..., onset_stage=...)``, ``qm_stream_set_onset_stage``) take,
and :class:`ResampleStage`, the plan that brings a timestep's raw traces to the scan rate in front of them
(``Engine.resample``, ``StreamingDetector(..., resample_stage=...)``, ``qm_stream_set_resample_stage``).

The reference's ``STALTAOnset.calculate_onsets`` (quakemigrate/signal/onsets/stalta.py:137-211, :353-489) does this
per timestep and component trace on the host: linear detrend, demean, 5 % cosine taper, zero-phase Butterworth
band-pass, STA/LTA.  The device stage covers its default case -- gap-free traces of the full timespan
(``full_timespan=True, allow_gaps=False``) -- and, with ``OnsetStage(fill_gaps=True)`` and :func:`plan_segments`,
gappy traces as ``allow_gaps=True`` / ``full_timespan=False`` treat them (stalta.py:442-461): every segment
conditioned on its own, a second taper, the gaps and the window's ends filled with ``sqrt(finfo(float).tiny)``
(``Engine.preprocess_segments``, ``StreamingDetector.push_segments``).  The ``env`` / ``env_squared`` transforms stay
on the host plugin path.

Before that the reference brings every raw trace to the scan rate (``util.resample``, quakemigrate/util.py:404-604):
integer decimation behind a detrend, a cosine taper and a zero-phase low-pass, and -- for rates that do not divide --
linear-interpolation upsampling by an integer factor first.  :class:`ResampleStage` plans that per trace by the
reference's rules; the device does the arithmetic (include/qmhip.h: ``qm_engine_resample``).
"""

from __future__ import annotations

import dataclasses

import numpy as np


def butter_bandpass_sos(lowcut, highcut, sampling_rate, corners):
    """
    Second-order sections (n_sections, 6) of the Butterworth band-pass the reference filters with, built as
    obspy's ``bandpass`` builds them: ``scipy.signal.iirfilter(corners, [low, high], btype="band",
    ftype="butter", output="zpk")``, then ``zpk2sos``.  ``corners`` corners give ``corners`` sections.  Raises
    ``ImportError`` without SciPy and ``ValueError`` for a ``highcut`` at or above the Nyquist frequency, as the
    reference does (stalta.py:198).
    """
    from scipy.signal import iirfilter, zpk2sos

    nyquist = 0.5 * float(sampling_rate)
    if not 0.0 < float(lowcut) < float(highcut):
        raise ValueError(f"band-pass corners must satisfy 0 < lowcut < highcut (got {lowcut}, {highcut})")
    if float(highcut) >= nyquist:
        raise ValueError(f"highcut {highcut} Hz is at or above the Nyquist frequency {nyquist} Hz of "
                         f"{sampling_rate} Hz data")
    z, p, k = iirfilter(int(corners), [float(lowcut) / nyquist, float(highcut) / nyquist], btype="band",
                        ftype="butter", output="zpk")
    return np.ascontiguousarray(zpk2sos(z, p, k), dtype=np.float64)


def butter_lowpass_sos(freq, sampling_rate, corners=2):
    """
    Second-order sections (n_sections, 6) of the Butterworth low-pass the reference decimates behind, built as obspy's
    ``lowpass`` builds them: ``scipy.signal.iirfilter(corners, freq / nyquist, btype="lowpass", ftype="butter",
    output="zpk")``, then ``zpk2sos``; two corners give one section.  The reference passes
    ``freq = rate_out / 2.000001`` (util.py:509-511).  Raises ``ImportError`` without SciPy and ``ValueError`` for a
    ``freq`` at or above the Nyquist frequency.
    """
    from scipy.signal import iirfilter, zpk2sos

    nyquist = 0.5 * float(sampling_rate)
    if not 0.0 < float(freq) < nyquist:
        raise ValueError(f"low-pass corner {freq} Hz: it must lie between 0 and the Nyquist frequency {nyquist} Hz "
                         f"of {sampling_rate} Hz data")
    z, p, k = iirfilter(int(corners), float(freq) / nyquist, btype="lowpass", ftype="butter", output="zpk")
    return np.ascontiguousarray(zpk2sos(z, p, k), dtype=np.float64)


def butter_highpass_sos(freq, sampling_rate, corners):
    """
    Second-order sections (n_sections, 6) of the Butterworth high-pass the reference's amplitude measurement filters
    with (amplitude.py:500-539), built as obspy's ``highpass`` builds them: ``scipy.signal.iirfilter(corners,
    freq / nyquist, btype="highpass", ftype="butter", output="zpk")``, then ``zpk2sos``; ``corners`` corners give
    ``ceil(corners / 2)`` sections.  Raises ``ImportError`` without SciPy and ``ValueError`` for a ``freq`` at or above
    the Nyquist frequency.
    """
    from scipy.signal import iirfilter, zpk2sos

    nyquist = 0.5 * float(sampling_rate)
    if not 0.0 < float(freq) < nyquist:
        raise ValueError(f"high-pass corner {freq} Hz: it must lie between 0 and the Nyquist frequency {nyquist} Hz "
                         f"of {sampling_rate} Hz data")
    z, p, k = iirfilter(int(corners), float(freq) / nyquist, btype="highpass", ftype="butter", output="zpk")
    return np.ascontiguousarray(zpk2sos(z, p, k), dtype=np.float64)


def cosine_taper_sides(npts, max_percentage=0.05):
    """
    The two ramps ``(left, right)`` of a cosine taper over ``int(max_percentage * npts)`` samples on each end:
    ``left[k] = 0.5 (1 - cos(pi k / m))`` for ``k = 0..m-1`` with ``m`` the ramp length, ``right`` its mirror
    image -- half-cosine ramps from 0 towards 1, as obspy's ``Trace.taper(type="cosine")`` applies them.  obspy
    is not a dependency of this package and equality with its ``cosine_taper`` to the last bit is NOT pinned
    by a test; the device kernel takes the weights as input, so any taper can be passed instead.
    """
    m = int(float(max_percentage) * int(npts))
    if m < 0 or 2 * m > int(npts):
        raise ValueError(f"a taper of {max_percentage} of {npts} samples does not fit twice")
    if m == 0:
        return np.zeros(0), np.zeros(0)
    left = 0.5 * (1.0 - np.cos(np.pi * np.arange(m, dtype=np.float64) / m))
    return left, np.ascontiguousarray(left[::-1])


# the columns of a segment's record (include/qmhip.h: qm_engine_preprocess_segments)
SEGMENT_FIELDS = ("trace", "first", "n", "fill_before", "fill_after", "w_offset", "m", "reserved")
# what the reference pads gaps and the window's ends with (stalta.py:455-461): 2**-511
GAP_FILL_VALUE = float(np.sqrt(np.finfo(float).tiny))


def plan_segments(t_samples, n_traces, segments, taper_percentage=0.05):
    """
    The records and taper weights of a timestep's gappy traces, as ``Engine.preprocess_segments`` and
    ``qm_stream_push_segments`` take them.  ``segments``: a list of ``(trace, first, n)`` -- samples
    ``[first, first + n)`` of row ``trace`` of the (n_traces, t_samples) window hold data --, the segments of one
    trace in ascending order with at least one sample between two of them.  Returns ``(records, taper_weights)``:
    records (n_segments, 8) int64 in the order given (columns: ``SEGMENT_FIELDS``), their ``fill_before`` /
    ``fill_after`` set so that each trace's records tile the window -- a segment fills up to its predecessor, or from
    sample 0, and the trace's last one to the window's end --, ``m = int(taper_percentage * n)`` with the weights of
    :func:`cosine_taper_sides`, one set per distinct length.  ``ValueError`` for a segment outside the window,
    overlapping or touching segments or segments out of order, and a trace without a segment.
    """
    T, n_traces = int(t_samples), int(n_traces)
    segments = [tuple(int(v) for v in seg) for seg in segments]
    records = np.zeros((len(segments), len(SEGMENT_FIELDS)), dtype=np.int64)
    tapers, weights, n_weights = {}, [], 0
    last = {}                                           # trace -> index of its latest record
    for i, (tr, first, n) in enumerate(segments):
        if not 0 <= tr < n_traces:
            raise ValueError(f"segment {i}: trace {tr} out of range ({n_traces} traces)")
        if n < 1 or first < 0 or first + n > T:
            raise ValueError(f"segment {i}: samples [{first}, {first + n}) of trace {tr} leave the window of {T} "
                             "(at least one sample, inside it)")
        start = 0
        if tr in last:
            prev = records[last[tr]]
            start = int(prev[1] + prev[2])
            if first <= start:
                raise ValueError(f"segment {i}: samples [{first}, {first + n}) of trace {tr} overlap, touch or precede "
                                 f"the trace's segment before them, which ends at {start} (segments of a trace go in "
                                 "ascending order, a gap between them)")
        if n not in tapers:
            left, right = cosine_taper_sides(n, taper_percentage)
            tapers[n] = (n_weights, len(left))
            weights += [left, right]
            n_weights += 2 * len(left)
        records[i] = (tr, first, n, first - start, 0, tapers[n][0], tapers[n][1], 0)
        last[tr] = i
    for tr in range(n_traces):
        if tr not in last:
            raise ValueError(f"trace {tr} has no segment (a trace without data is not part of the stage)")
        r = records[last[tr]]
        r[4] = T - (r[1] + r[2])
    return records, (np.concatenate(weights) if weights else np.zeros(0))


_TRANSFORMS = {"energy": 0, "abs": 1}
_POSITIONS = {"classic": 0, "centred": 1, "recursive": 2}


@dataclasses.dataclass(frozen=True)
class OnsetStage:
    """
    One onset function's device stage: how component traces become the rows the stack reads.

    filters : ``{phase: (lowcut, highcut, corners)}`` -- one band-pass per phase (the reference's
        ``bandpass_filters``).
    sta_lta_windows : ``{phase: (sta_seconds, lta_seconds)}``.
    trace_row : (n_traces,) onset row each trace feeds; every row needs at least one trace.
    trace_phase : (n_traces,) phase of each trace (a key of ``filters``): with the order of ``filters`` this is the
        ``trace_filter`` layout.
    row_phase : (n_rows,) phase of each onset row (its STA/LTA windows).
    transform : "energy" or "abs";  position : "classic", "centred" or "recursive".
    taper_pad : samples of the onset's taper windows, < 0 for none;  min_onset_value : the clip.
    detrend, taper_percentage : the pre-processing's linear detrend + demean and its cosine taper.
    fill_gaps : the traces come in segments (the reference's ``allow_gaps=True`` / ``full_timespan=False``): every
        segment is conditioned on its own and tapered a second time behind the filter, gaps and the window's ends
        are filled with ``sqrt(finfo(float).tiny)`` (:func:`plan_segments`, ``StreamingDetector.push_segments``).

    Two stages compare equal when they describe the same kernels' inputs: a pipeline is rebuilt when the stage
    changes (``MigrationScan.continuous_compute``).
    """

    filters: dict
    sta_lta_windows: dict
    trace_row: tuple
    trace_phase: tuple
    row_phase: tuple
    transform: str = "energy"
    position: str = "classic"
    taper_pad: int = -1
    min_onset_value: float = 0.4
    detrend: bool = True
    taper_percentage: float = 0.05
    fill_gaps: bool = False

    def __post_init__(self):
        object.__setattr__(self, "filters", {k: tuple(v) for k, v in dict(self.filters).items()})
        object.__setattr__(self, "sta_lta_windows", {k: tuple(v) for k, v in dict(self.sta_lta_windows).items()})
        object.__setattr__(self, "trace_row", tuple(int(v) for v in self.trace_row))
        object.__setattr__(self, "trace_phase", tuple(self.trace_phase))
        object.__setattr__(self, "row_phase", tuple(self.row_phase))
        if self.transform not in _TRANSFORMS:
            raise ValueError(f"transform {self.transform!r}: the device stage takes 'energy' or 'abs' (the envelope "
                             "transforms stay on the host plugin path)")
        if self.position not in _POSITIONS:
            raise ValueError(f"position {self.position!r}: 'classic', 'centred' or 'recursive'")
        if len(self.trace_row) != len(self.trace_phase):
            raise ValueError("trace_row and trace_phase differ in length")
        for ph in list(self.trace_phase) + list(self.row_phase):
            if ph not in self.filters or ph not in self.sta_lta_windows:
                raise ValueError(f"phase {ph!r} has no filter or no STA/LTA windows")
        if len({tuple(f)[2] for f in self.filters.values()}) != 1:
            raise ValueError("the filters of one stage share their number of corners (sections of one cascade)")

    def __hash__(self):
        return hash((tuple(self.filters.items()), tuple(self.sta_lta_windows.items()), self.trace_row,
                     self.trace_phase, self.row_phase, self.transform, self.position, self.taper_pad,
                     self.min_onset_value, self.detrend, self.taper_percentage, self.fill_gaps))

    @property
    def n_traces(self):
        return len(self.trace_row)

    @property
    def n_rows(self):
        return len(self.row_phase)

    def arrays(self, t_samples, sampling_rate):
        """The stage as the C ABI takes it, for windows of ``t_samples`` samples at ``sampling_rate`` Hz: a dict
        with ``trace_row``, ``trace_filter``, ``sos`` (n_filters, n_sections, 6), ``taper_left``, ``taper_right``,
        ``nsta``, ``nlta`` (samples, as the reference counts them: ``int(round(seconds * rate)) + 1``, stalta.py:394-396),
        ``transform``, ``position`` (their integer codes), ``taper_pad``, ``min_onset_value`` and ``detrend``; with
        ``fill_gaps`` also ``second_taper`` = 1 and ``fill_value`` = ``sqrt(finfo(float).tiny)``."""
        phases = list(self.filters)
        sos = np.stack([butter_bandpass_sos(*self.filters[ph][:2], sampling_rate, self.filters[ph][2])
                        for ph in phases])
        left, right = cosine_taper_sides(t_samples, self.taper_percentage)
        windows = np.array([[int(round(w * int(sampling_rate))) + 1 for w in self.sta_lta_windows[ph]]
                            for ph in self.row_phase], dtype=np.int32).reshape(-1, 2)
        gaps = {"second_taper": 1, "fill_value": GAP_FILL_VALUE} if self.fill_gaps else {}
        return {
            "trace_row": np.array(self.trace_row, dtype=np.int32),
            "trace_filter": np.array([phases.index(ph) for ph in self.trace_phase], dtype=np.int32),
            "sos": np.ascontiguousarray(sos),
            "taper_left": left, "taper_right": right,
            "nsta": np.ascontiguousarray(windows[:, 0]), "nlta": np.ascontiguousarray(windows[:, 1]),
            "transform": _TRANSFORMS[self.transform], "position": _POSITIONS[self.position],
            "taper_pad": int(self.taper_pad), "min_onset_value": float(self.min_onset_value),
            "detrend": 1 if self.detrend else 0,
            **gaps,
        }


# the columns of a trace's record (include/qmhip.h: qm_engine_resample)
RESAMPLE_FIELDS = ("raw_offset", "n_raw", "up", "pad_left", "pad_right", "up_first", "n_up", "dec", "lowpass", "taper",
                   "out_first")
_TRIM_SLACK = 0.00001       # seconds: the reference trims to the window widened by this much (util.py:472-474, :599-601)


def _inner_samples(t_first, n, rate, length):
    """First and last index of the samples of a series (first sample at ``t_first`` seconds after the window's start,
    ``n`` samples at ``rate`` Hz) whose times lie in ``[-slack, length + slack]``: a trim to the inner samples
    (obspy's ``nearest_sample=False``, which rounds the sample count to 7 digits before it cuts)."""
    lo = max(0, int(np.ceil(round((-_TRIM_SLACK - t_first) * rate, 7))))
    hi = min(n - 1, int(np.floor(round((length + _TRIM_SLACK - t_first) * rate, 7))))
    return lo, hi


def resample_pads(gap_start, gap_end, raw_rate, upfactor):
    """``(pad_left, pad_right)`` of an upsampled trace: ``round(gap * raw_rate * upfactor)`` constant samples where
    the trace starts (ends) ``gap`` seconds inside the window with ``0 < gap < 1 / raw_rate`` -- strictly less than
    one raw sample --, none otherwise: traces that float in the middle of the window are left alone (util.py:553-585).
    The gaps are compared in whole nanoseconds, the resolution of the reference's time stamps: a gap of exactly one
    raw sample that arrives here a rounding error short of it is still a whole sample."""
    scale = float(raw_rate) * int(upfactor)
    delta = round(1.0 / float(raw_rate), 9)
    gaps = (round(float(gap_start), 9), round(float(gap_end), 9))
    return tuple(int(round(g * scale)) if 0.0 < g < delta else 0 for g in gaps)


@dataclasses.dataclass(frozen=True)
class ResampleStage:
    """
    A timestep's raw traces and how they reach the scan rate: the plan of the device's resampling stage.

    sampling_rate : the scan rate (Hz, an integer as in the reference).
    raw_rate, n_raw : (n_traces,) rate (Hz) and sample count of each raw trace.
    first_offset : (n_traces,) seconds from the window's start to the trace's first sample (> 0: it starts late).
    last_offset : (n_traces,) seconds from the window's end to the trace's last sample (< 0: it ends early);
        ``None``: ``first_offset + (n_raw - 1) / raw_rate`` minus the window's length.
    upfactor : the integer factor rates that do not divide are upsampled by first (40 Hz to 50 Hz: 5), or ``None``.
    detrend, taper_percentage, corners : the decimation's detrend + demean, cosine taper and low-pass order.

    The raw samples of a timestep are packed trace behind trace, in this order.
    """

    sampling_rate: int
    raw_rate: tuple
    n_raw: tuple
    first_offset: tuple
    last_offset: tuple = None
    upfactor: int = None
    detrend: bool = True
    taper_percentage: float = 0.05
    corners: int = 2

    def __post_init__(self):
        object.__setattr__(self, "raw_rate", tuple(float(v) for v in self.raw_rate))
        object.__setattr__(self, "n_raw", tuple(int(v) for v in self.n_raw))
        object.__setattr__(self, "first_offset", tuple(float(v) for v in self.first_offset))
        if self.last_offset is not None:
            object.__setattr__(self, "last_offset", tuple(float(v) for v in self.last_offset))
        lengths = {len(self.raw_rate), len(self.n_raw), len(self.first_offset)}
        if self.last_offset is not None:
            lengths.add(len(self.last_offset))
        if len(lengths) != 1 or not self.raw_rate:
            raise ValueError("raw_rate, n_raw, first_offset and last_offset: one entry per trace each, at least one trace")
        if self.upfactor is not None and int(self.upfactor) < 1:
            raise ValueError(f"upfactor {self.upfactor}: an integer >= 1, or None")
        if min(self.n_raw) < 1:
            raise ValueError("every trace needs at least one raw sample")

    @property
    def n_traces(self):
        return len(self.raw_rate)

    @property
    def total_raw_samples(self):
        return int(sum(self.n_raw))

    def arrays(self, t_samples):
        """
        The stage as the C ABI takes it, for windows of ``t_samples`` samples at the scan rate: a dict with ``records``
        (n_traces, 11) int64 (columns: ``RESAMPLE_FIELDS``), ``sos_lp`` (n_lowpass, n_sections, 6), ``taper_table``
        (n_tapers, 2) int32, ``taper_weights``, ``detrend``, ``t_samples`` and ``total_raw_samples``.  Planned by the
        reference's rules (util.py:446-474, :553-601): equal rates pass through; a rate the scan rate divides is
        decimated; another one is upsampled by ``upfactor`` first if the scan rate divides ``int(raw_rate * upfactor)``,
        with constant pads of ``round(gap * raw_rate * upfactor)`` samples where the trace starts or ends strictly less
        than one raw sample inside the window, and trimmed to the window; everything is trimmed to the window at the
        end.  ``ValueError``, naming the trace, for a rate that can be neither decimated nor upsampled (the reference
        logs it and leaves the trace at its rate) and for a planned length other than ``t_samples``.
        """
        rate, T = self.sampling_rate, int(t_samples)
        length = (T - 1) / float(rate)
        records = np.zeros((self.n_traces, len(RESAMPLE_FIELDS)), dtype=np.int64)
        lowpasses, tapers, weights = {}, {}, []
        offset = 0
        for i, (rr, n, t0) in enumerate(zip(self.raw_rate, self.n_raw, self.first_offset)):
            gap_end = (length - (t0 + (n - 1) / rr)) if self.last_offset is None else -self.last_offset[i]
            u, pad_l, pad_r = 1, 0, 0
            if rr == rate:
                d = 1
            elif rr % rate == 0:
                d = int(rr / rate)
            elif self.upfactor is not None and int(rr * self.upfactor) % rate == 0:
                u = int(self.upfactor)
                d = int(int(rr * u) / rate)
            else:
                raise ValueError(f"trace {i}: {rr:g} Hz can be neither decimated to {rate} Hz nor upsampled by "
                                 f"upfactor = {self.upfactor} to a multiple of it")
            rate_up, first, n_up, t_kept = rr, 0, n, t0
            if u > 1:
                rate_up = float(int(rr * u))
                pad_l, pad_r = resample_pads(t0, gap_end, rr, u)
                t_up = t0 - pad_l / (rr * u)
                first, last = _inner_samples(t_up, pad_l + (n - 1) * u + 1 + pad_r, rate_up, length)
                n_up, t_kept = last - first + 1, t_up + first / rate_up
                if n_up < 1:
                    raise ValueError(f"trace {i}: no upsampled sample lies in the window")
            lo, hi = _inner_samples(t_kept, -(-n_up // d), float(rate), length)
            if hi - lo + 1 != T:
                raise ValueError(f"trace {i}: {rr:g} Hz, {n} raw samples from {t0:g} s on give {max(hi - lo + 1, 0)} "
                                 f"samples at {rate} Hz, the window holds {T}")
            out_first = lo
            lp = tp = 0
            if d == 1:                                  # nothing between the trims: one slice
                first, n_up, out_first = first + lo, T, 0
            else:
                if rate_up not in lowpasses:
                    lowpasses[rate_up] = (len(lowpasses),
                                          butter_lowpass_sos(float(rate) / 2.000001, rate_up, self.corners))
                lp = lowpasses[rate_up][0]
                if n_up not in tapers:
                    left, right = cosine_taper_sides(n_up, self.taper_percentage)
                    tapers[n_up] = (len(tapers), sum(len(w) for w in weights), len(left))
                    weights += [left, right]
                tp = tapers[n_up][0]
            records[i] = (offset, n, u, pad_l, pad_r, first, n_up, d, lp, tp, out_first)
            offset += n
        n_sections = (int(self.corners) + 1) // 2
        sos = (np.stack([s for _, s in lowpasses.values()]) if lowpasses else np.zeros((0, n_sections, 6)))
        table = np.array([[off, m] for _, off, m in tapers.values()], dtype=np.int32).reshape(-1, 2)
        return {
            "records": records, "sos_lp": np.ascontiguousarray(sos), "taper_table": table,
            "taper_weights": np.concatenate(weights) if weights else np.zeros(0),
            "detrend": 1 if self.detrend else 0, "t_samples": T, "total_raw_samples": offset,
        }
