# -*- coding: utf-8 -*-
"""
NumPy restatement of the pre-processing of gappy traces (include/qmhip.h: qm_engine_preprocess_segments) -- the
specification the GPU tests compare against.  Per segment: the detrend in the device's summation order
(preprocess_ref.detrend_device_order), the taper, the cascade (preprocess_ref.sosfilt, SciPy's bits), the taper again;
then the fills.  Every step is bit-level.  ``reference_order`` is the same sequence as the reference runs it, in plain
NumPy / SciPy order (scipy.signal.detrend twice, sosfilt forward-backward): what tests/test_preprocess_segments_host.py
holds the restatement against, within the stage's bound.
"""

import numpy as np

import preprocess_ref as pr

FILL = 2.0 ** -511                                      # sqrt(np.finfo(float).tiny)


def segment(x, sos, w, m, detrend_on=True, zero_phase=True, second_taper=True):
    """One segment's samples through steps 1-4.  w: the segment's 2 m weights."""
    y = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if detrend_on:
        y = pr.detrend_device_order(y, True)
    y = pr.taper(y, w[:m], w[m:2 * m])
    y = pr.sosfilt_zero_phase(sos, y) if zero_phase else pr.sosfilt(sos, y)
    if second_taper:
        y = pr.taper(y, w[:m], w[m:2 * m])
    return y


def preprocess_segments(signals, trace_filter, sos, records, weights, detrend_on=True, zero_phase=True,
                        second_taper=True, fill_value=FILL):
    """The whole stage: signals (n_traces, T) in window layout, records (n_segments, 8), the taper weights.  Samples no
    record names keep NaN: a layout that does not tile the window shows."""
    x = np.asarray(signals, dtype=np.float64)
    out = np.full(x.shape, np.nan)
    for tr, first, n, before, after, off, m, _ in np.asarray(records, dtype=np.int64).tolist():
        out[tr, first:first + n] = segment(x[tr, first:first + n], sos[trace_filter[tr]], weights[off:off + 2 * m], m,
                                           detrend_on, zero_phase, second_taper)
        out[tr, first - before:first] = fill_value
        out[tr, first + n:first + n + after] = fill_value
    return out


def reference_order(signals, trace_filter, sos, records, weights, fill_value=FILL):
    """The reference's sequence per segment (stalta.py:137-211, :442-461) in NumPy / SciPy order: detrend("linear"),
    detrend("constant"), taper, zero-phase sosfilt, taper, then the fill."""
    from scipy import signal

    x = np.asarray(signals, dtype=np.float64)
    out = np.full(x.shape, np.nan)
    for tr, first, n, before, after, off, m, _ in np.asarray(records, dtype=np.int64).tolist():
        w = np.asarray(weights[off:off + 2 * m], dtype=np.float64)
        y = x[tr, first:first + n]
        y = signal.detrend(signal.detrend(y, type="linear"), type="constant") if n > 1 else y - y
        y = pr.taper(y, w[:m], w[m:])
        c = sos[trace_filter[tr]]
        y = signal.sosfilt(c, signal.sosfilt(c, y)[::-1])[::-1]
        out[tr, first:first + n] = pr.taper(y, w[:m], w[m:])
        out[tr, first - before:first] = fill_value
        out[tr, first + n:first + n + after] = fill_value
    return out


def gappy_traces(seed, n_traces, t_samples, segments):
    """Seeded noisy traces (preprocess_ref.noisy_traces) with NaN wherever no segment holds data: a kernel that read
    outside its segments would carry the NaN into its output."""
    x = pr.noisy_traces(seed, n_traces, t_samples)
    keep = np.zeros(x.shape, dtype=bool)
    for tr, first, n in segments:
        keep[tr, first:first + n] = True
    x[~keep] = np.nan
    return x
