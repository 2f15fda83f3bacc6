# -*- coding: utf-8 -*-
"""
What the device's pre-processing and onset stages are set up from: the band-pass coefficients, the taper ramps and
:class:`OnsetStage`, the description of one onset function's stage that ``Engine.preprocess`` / ``Engine.onsets``
and the pipeline (``StreamingDetector(..., onset_stage=...)``, ``qm_stream_set_onset_stage``) take.

The reference's ``STALTAOnset.calculate_onsets`` (quakemigrate/signal/onsets/stalta.py:137-211, :353-489) does this
per timestep and component trace on the host: linear detrend, demean, 5 % cosine taper, zero-phase Butterworth
band-pass, STA/LTA.  The device stage covers its default case -- gap-free traces of the full timespan
(``full_timespan=True, allow_gaps=False``).  Gappy traces (their second taper and tiny-float padding,
stalta.py:442-461), resampling and the ``env`` / ``env_squared`` transforms stay on the host plugin path.
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
                     self.min_onset_value, self.detrend, self.taper_percentage))

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
        ``transform``, ``position`` (their integer codes), ``taper_pad``, ``min_onset_value`` and ``detrend``."""
        phases = list(self.filters)
        sos = np.stack([butter_bandpass_sos(*self.filters[ph][:2], sampling_rate, self.filters[ph][2])
                        for ph in phases])
        left, right = cosine_taper_sides(t_samples, self.taper_percentage)
        windows = np.array([[int(round(w * int(sampling_rate))) + 1 for w in self.sta_lta_windows[ph]]
                            for ph in self.row_phase], dtype=np.int32).reshape(-1, 2)
        return {
            "trace_row": np.array(self.trace_row, dtype=np.int32),
            "trace_filter": np.array([phases.index(ph) for ph in self.trace_phase], dtype=np.int32),
            "sos": np.ascontiguousarray(sos),
            "taper_left": left, "taper_right": right,
            "nsta": np.ascontiguousarray(windows[:, 0]), "nlta": np.ascontiguousarray(windows[:, 1]),
            "transform": _TRANSFORMS[self.transform], "position": _POSITIONS[self.position],
            "taper_pad": int(self.taper_pad), "min_onset_value": float(self.min_onset_value),
            "detrend": 1 if self.detrend else 0,
        }
