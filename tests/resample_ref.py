# -*- coding: utf-8 -*-
"""
NumPy restatement of the resampling stage (include/qmhip.h: qm_engine_resample) -- the specification the GPU tests
compare against.  Per trace: linear-interpolation upsampling by an integer factor, constant pads, the kept slice;
then, where the trace is decimated, the detrend, taper and zero-phase cascade of tests/preprocess_ref.py (the same
arithmetic the pre-processing stage is held to) and every d-th sample; then the output slice.
tests/test_resample_host.py pins the filter to ``scipy.signal.sosfilt``, the detrend to ``scipy.signal.detrend`` and
the upsampling to a direct evaluation of the interpolation expression.
"""

import numpy as np

import preprocess_ref as pr

FIELDS = ("raw_offset", "n_raw", "up", "pad_left", "pad_right", "up_first", "n_up", "dec", "lowpass", "taper",
          "out_first")


def record(raw_offset, n_raw, up=1, pad_left=0, pad_right=0, up_first=0, n_up=None, dec=1, lowpass=0, taper=0,
           out_first=0):
    """One trace's record; ``n_up`` None: everything from ``up_first`` to the end of the padded series."""
    if n_up is None:
        n_up = pad_left + (n_raw - 1) * up + 1 + pad_right - up_first
    return [raw_offset, n_raw, up, pad_left, pad_right, up_first, n_up, dec, lowpass, taper, out_first]


def upsample(x, u):
    """(len(x) - 1) u + 1 samples: x[j] at j u, between them the two-term interpolation, built sample by sample --
    weight of the right neighbour i / u, of the left one (u - i) / u, each a float64 quotient, each product and the
    sum rounded on its own."""
    x = np.asarray(x)
    xf = x.astype(np.float64)
    out = np.empty((len(x) - 1) * u + 1)
    for q in range(len(out)):
        j, i = divmod(q, u)
        if i == 0:
            out[q] = xf[j]
        else:
            w_right, w_left = np.float64(i) / np.float64(u), np.float64(u - i) / np.float64(u)
            out[q] = np.float64(w_right * xf[j + 1]) + np.float64(w_left * xf[j])
    return out


def kept_series(x, up, pad_left, pad_right, up_first, n_up):
    """The padded, upsampled series cut to [up_first, up_first + n_up)."""
    x = np.asarray(x)
    series = upsample(x, up) if up > 1 else x.astype(np.float64)
    padded = np.concatenate([np.full(pad_left, float(x[0])), series, np.full(pad_right, float(x[-1]))])
    assert 0 <= up_first and up_first + n_up <= len(padded)
    return padded[up_first:up_first + n_up]


def lowpassed(kept, sos, left=(), right=(), detrend_on=True, device_order=False):
    """The decimation's filter chain over one kept series (or several of one length): detrend, taper, zero-phase
    cascade.  ``device_order`` (one series): the detrend's sums as the device adds them."""
    if detrend_on and device_order:
        y = pr.detrend_device_order(kept, True)
    else:
        y = pr.detrend(kept) if detrend_on else np.array(kept, dtype=np.float64)
    return pr.sosfilt_zero_phase(sos, pr.taper(y, left, right))


def taper_of(table, weights, index):
    off, m = (int(v) for v in np.asarray(table).reshape(-1, 2)[index])
    return weights[off:off + m], weights[off + m:off + 2 * m]


def resample(raw, records, sos_lp, taper_table, taper_weights, t_samples, detrend_on=True):
    """The whole stage.  raw: the packed samples (int32 or float64); records: (n_traces, 11)."""
    raw = np.asarray(raw)
    out = np.empty((len(records), t_samples))
    for i, rec in enumerate(np.asarray(records, dtype=np.int64)):
        r = dict(zip(FIELDS, (int(v) for v in rec)))
        x = raw[r["raw_offset"]:r["raw_offset"] + r["n_raw"]]
        k = kept_series(x, r["up"], r["pad_left"], r["pad_right"], r["up_first"], r["n_up"])
        if r["dec"] > 1:
            left, right = taper_of(taper_table, taper_weights, r["taper"])
            k = lowpassed(k, sos_lp[r["lowpass"]], left, right, detrend_on)[::r["dec"]]
        assert r["out_first"] + t_samples <= len(k)
        out[i] = k[r["out_first"]:r["out_first"] + t_samples]
    return out


def pack(traces, dtype):
    """Traces packed one behind the other, and their offsets."""
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in traces])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(traces).astype(dtype)), offsets


def raw_traces(seed, lengths, dtype=np.float64):
    """Seeded noise of amplitude ~1e3 on a ramp and an offset, one trace per length; int32: rounded."""
    out = []
    for k, n in enumerate(lengths):
        x = pr.noisy_traces(seed + 17 * k, 1, n)[0]
        out.append(np.rint(x).astype(np.int32) if np.dtype(dtype) == np.int32 else x)
    return out


def stable_sos(seed, n_filters, n_sections):
    """Random stable sections, a0 == 1: complex pole pairs of radius 0.5-0.95, arbitrary zeros, gains near 1 (the
    recipe of tests/test_preprocess_gpu.py)."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.5, 0.95, size=(n_filters, n_sections))
    th = rng.uniform(0.2, 2.9, size=(n_filters, n_sections))
    sos = np.empty((n_filters, n_sections, 6))
    sos[..., :3] = rng.uniform(-1.0, 1.0, size=(n_filters, n_sections, 3))
    sos[..., 3] = 1.0
    sos[..., 4] = -2.0 * r * np.cos(th)
    sos[..., 5] = r * r
    return sos
