# -*- coding: utf-8 -*-
"""
NumPy restatement of the pre-processing stage (include/qmhip.h: qm_engine_preprocess) -- the specification the
GPU tests compare against: per trace a linear detrend in the centred closed form and a demean, the taper weights
on both ends, then the cascade of second-order sections in direct form II transposed with the operation order of
SciPy's ``_sosfilt``, forward and (zero-phase) again over the reversed result.  tests/test_preprocess_host.py pins
the filter to ``scipy.signal.sosfilt`` bit for bit and the detrend to ``scipy.signal.detrend`` applied twice.
"""

import numpy as np


def detrend(x, also_mean=True):
    """Least-squares line over t = 0..n-1 subtracted, then (``also_mean``) the mean of the rest.  x: (..., n).  The
    tolerance-level restatement: NumPy's sums add in another order than the device."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    t = np.arange(n, dtype=np.float64)
    tbar = 0.5 * (n - 1)
    mean = x.mean(axis=-1, keepdims=True)
    sxx = np.sum((t - tbar) ** 2)
    slope = np.sum((t - tbar) * (x - mean), axis=-1, keepdims=True) / sxx if sxx > 0 else 0.0
    y = x - (mean + slope * (t - tbar))
    return y - y.mean(axis=-1, keepdims=True) if also_mean else y


def wave_sum(values):
    """The sum as a wavefront of the device adds it (csrc/qm_condition.hpp: wave_sum): lane l adds elements l, l + 64,
    ... one after the other from 0.0, then a butterfly over the 64 partials; lane 0's value."""
    values = np.asarray(values, dtype=np.float64)
    padded = np.zeros(-(-max(len(values), 1) // 64) * 64)
    padded[:len(values)] = values
    acc = np.zeros(64)
    for row in padded.reshape(-1, 64):                  # (row by row: np.sum is pairwise and gives other bits)
        acc = acc + row
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[np.arange(64) ^ m]
    return float(acc[0])


def detrend_device_order(x, also_mean):
    """``detrend`` of one trace with the device's expressions in the device's order (csrc/qm_condition.hpp:
    detrend_line): the bit-level restatement.  Elementwise NumPy rounds each product and sum separately."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    centred = np.arange(n, dtype=np.float64) - 0.5 * float(n - 1)
    mean = wave_sum(x) / float(n)
    sxx = wave_sum(centred * centred)
    sxy = wave_sum(centred * (x - mean))
    slope = sxy / sxx if sxx > 0.0 else 0.0
    y = x - (mean + slope * centred)
    return y - wave_sum(y) / float(n) if also_mean else y


def taper(x, left, right):
    y = np.array(x, dtype=np.float64, copy=True)
    left, right = np.asarray(left, dtype=np.float64), np.asarray(right, dtype=np.float64)
    n = y.shape[-1]
    if len(left):
        y[..., :len(left)] *= left
    if len(right):
        y[..., n - len(right):] *= right
    return y


def sosfilt(sos, x):
    """One forward pass over the last axis from a zero state.  sos: (n_sections, 6) with a0 == 1; x: (n,) or
    (m, n) -- the traces are independent, so they run side by side (NumPy's elementwise operations round each
    product and sum separately: no contraction)."""
    sos = np.asarray(sos, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    flat = np.atleast_2d(x)
    out = np.empty_like(flat)
    z = np.zeros((sos.shape[0], 2, flat.shape[0]))
    for n in range(flat.shape[1]):
        xc = flat[:, n]
        for s in range(sos.shape[0]):
            b0, b1, b2, _, a1, a2 = sos[s]
            xn = b0 * xc + z[s, 0]
            z[s, 0] = b1 * xc - a1 * xn + z[s, 1]
            z[s, 1] = b2 * xc - a2 * xn
            xc = xn
        out[:, n] = xc
    return out.reshape(x.shape)


def sosfilt_zero_phase(sos, x):
    """Forward, then the same filter over the reversed result, reversed back."""
    return sosfilt(sos, sosfilt(sos, x)[..., ::-1])[..., ::-1]


def preprocess(signals, trace_filter, sos, left=(), right=(), detrend_on=True, zero_phase=True, device_order=False):
    """The whole stage: signals (n_traces, T), sos (n_filters, n_sections, 6).  ``device_order``: the detrend's sums as
    the device adds them -- then every step is bit-level."""
    x = np.asarray(signals, dtype=np.float64)
    if detrend_on and device_order:
        y = np.stack([detrend_device_order(row, True) for row in x])
    else:
        y = detrend(x) if detrend_on else x.copy()
    y = taper(y, left, right)
    out = np.empty_like(y)
    trace_filter = np.asarray(trace_filter)
    for f in np.unique(trace_filter):
        rows = np.flatnonzero(trace_filter == f)
        out[rows] = sosfilt_zero_phase(sos[f], y[rows]) if zero_phase else sosfilt(sos[f], y[rows])
    return out


def impulse_l1(sos, n):
    """l1 norm of the forward filter's response to a unit impulse over n samples."""
    d = np.zeros(n)
    d[0] = 1.0
    return float(np.sum(np.abs(sosfilt(sos, d))))


def noisy_traces(seed, n_traces, n, amplitude=1e3):
    """Seeded Gaussian noise of amplitude ~1e3 on a ramp and an offset: no dead traces."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    ramp = rng.uniform(-3.0, 3.0, size=(n_traces, 1)) * t
    offset = rng.uniform(-5e3, 5e3, size=(n_traces, 1))
    return np.ascontiguousarray(amplitude * rng.standard_normal((n_traces, n)) + ramp + offset)
