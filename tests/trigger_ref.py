# -*- coding: utf-8 -*-
"""
NumPy restatement of the trigger stage (include/qmhip.h: qm_engine_trigger) -- the specification the kernels are
tested against.  The rules are the reference's (quakemigrate/signal/trigger.py:318-686), stated on arrays:

* ``gaussian_weights`` / ``smooth``: ``scipy.ndimage.gaussian_filter1d`` (``_smooth_coa``, :420-433) in the summation
  order of SciPy's symmetric path, boundary ``reflect`` (``d c b a | a b c d | d c b a``, period 2n, also for n <= r);
* ``chunk_thresholds``: ``_get_threshold`` (:436-484), one value per chunk of W samples counted from sample 0;
* ``find_candidates``: ``_identify_candidates`` (:487-567): maximal runs of ``trig >= threshold``, the FIRST maximum of
  COA over the run, the MinTime / MaxTime rule;
* ``merge``: ``_refine_candidates`` (:592-621): pairwise separation, a prefix sum, a segmented reduction.

Time.  All time arithmetic is in int64 nanoseconds from the first sample of the series, t(i) = i * period_ns.  The
reference works on obspy's ``UTCDateTime``: an integer count of nanoseconds to which ``+ seconds`` adds
``round(seconds * 1e9)``, and whose differences come back rounded to 1 us.  Where the sampling period,
``marginal_window``, ``min_event_interval`` and ``pad`` are whole numbers of microseconds -- the front end
(quakemigrate_amd/trigger.py) refuses anything else -- every time stamp is a whole number of microseconds, the rounding
changes nothing and the integer comparisons here equal the reference's.

``trigger_series`` is the C call restated: same arguments, same outputs.  tests/test_trigger_host.py pins the parts to
SciPy, NumPy, pandas and the reference's recorded ``TriggeredEvents.csv`` files.
"""

import numpy as np

STATIC, MAD, MEDIAN_RATIO = 0, 1, 2
MAD_SCALE = 1.4826


class Refused(Exception):
    """What the C call refuses (a message, outputs untouched)."""


# -- a. smoothing ----------------------------------------------------------------------------------------------------
def gaussian_weights(sd, truncate):
    """(r, w[2r+1]) of ``gaussian_filter1d(x, sd, truncate=truncate)`` (scipy/ndimage/_filters.py)."""
    r = int(truncate * sd + 0.5)
    k = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sd * sd) * k ** 2)
    return r, w / w.sum()


def reflect_index(g, n):
    """Index into x[0..n) of position g of the periodic extension d c b a | a b c d | d c b a."""
    m = np.mod(g, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def smooth(x, r, w):
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    i = np.arange(n)
    out = x * w[r]
    for j in range(r, 0, -1):
        out = out + (x[reflect_index(i - j, n)] + x[reflect_index(i + j, n)]) * w[r - j]
    return out


# -- b. threshold ----------------------------------------------------------------------------------------------------
def middle(v):
    """np.median written on the sorted array: what the kernel selects."""
    v = np.sort(v)
    n = len(v)
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2


def chunk_thresholds(trig, method, value, chunk):
    """One threshold per chunk of ``chunk`` samples (the last one shorter; one chunk when n < chunk)."""
    if method == STATIC:
        return np.array([value], dtype=np.float64)
    n = len(trig)
    out = []
    for c0 in range(0, n, chunk):
        part = trig[c0:c0 + chunk]
        med = np.median(part)
        if method == MAD:
            out.append(med + (MAD_SCALE * np.median(np.abs(part - med))) * value)
        else:
            out.append(med * value)
    return np.array(out, dtype=np.float64)


def threshold_trace(thr, method, chunk, n):
    return np.full(n, thr[0]) if method == STATIC else thr[np.arange(n) // chunk]


# -- c. candidates ---------------------------------------------------------------------------------------------------
def find_candidates(coa, trig, thr_trace, period_ns, mw_ns, mei_ns):
    """int64 [n_candidates][5]: f, l, p, MinTime ns, MaxTime ns."""
    flag = np.concatenate([[False], trig >= thr_trace, [False]])
    first = np.flatnonzero(flag[1:-1] & ~flag[:-2])
    last = np.flatnonzero(flag[1:-1] & ~flag[2:])
    gap = mei_ns - mw_ns
    out = np.zeros((len(first), 5), dtype=np.int64)
    for k, (f, l) in enumerate(zip(first, last)):
        p = f + int(np.argmax(coa[f:l + 1]))
        tp, tf, tl = p * period_ns, f * period_ns, l * period_ns
        out[k] = (f, l, p, tp - mei_ns if tp - tf < mw_ns else tf - gap, tp + mei_ns if tl - tp < mw_ns else tl + gap)
    return out


# -- d. merge --------------------------------------------------------------------------------------------------------
def merge(cand, trig, coa, coa_n, period_ns, mw_ns):
    """(int64 [n_events][4]: peak index, MinTime ns, MaxTime ns, members; float64 [n_events][3]: TRIG_COA, COA,
    COA_NORM)."""
    nc = len(cand)
    if nc == 0:
        return np.zeros((0, 4), dtype=np.int64), np.zeros((0, 3))
    tp = cand[:, 2] * period_ns
    separate = (cand[:-1, 4] < tp[1:] - mw_ns) & (cand[1:, 3] > tp[:-1] + mw_ns)
    number = np.concatenate([[0], np.cumsum(separate)])
    ne = int(number[-1]) + 1
    ev_i, ev_f = np.zeros((ne, 4), dtype=np.int64), np.zeros((ne, 3))
    for e in range(ne):
        members = np.flatnonzero(number == e)
        best = members[int(np.argmax(trig[cand[members, 2]]))]          # (np.argmax: the first largest)
        p = cand[best, 2]
        ev_i[e] = (p, cand[members, 3].min(), cand[members, 4].max(), len(members))
        ev_f[e] = (trig[p], coa[p], coa_n[p])
    return ev_i, ev_f


# -- the C call ------------------------------------------------------------------------------------------------------
def trigger_series(coa, coa_n, trigger_on=0, weights=None, method=STATIC, value=1.5, chunk=1, period_ns=20_000_000,
                   mw_ns=2_000_000_000, mei_ns=4_000_000_000, max_events=1 << 30, max_radius=4096):
    """qm_engine_trigger restated.  Returns a dict: n_candidates, n_events, events_i, events_f, thresholds, smoothed
    (None when off), candidates."""
    coa, coa_n = np.asarray(coa, dtype=np.float64), np.asarray(coa_n, dtype=np.float64)
    n = len(coa)
    if n < 1 or len(coa_n) != n:
        raise Refused("empty input")
    if method not in (STATIC, MAD, MEDIAN_RATIO) or trigger_on not in (0, 1):
        raise Refused("selector")
    if method != STATIC and chunk < 1:
        raise Refused("chunk length")
    if period_ns < 1 or mw_ns < 0 or mei_ns < 2 * mw_ns:
        raise Refused("times")
    r = 0
    if weights is not None:
        r = (len(weights) - 1) // 2
        if r > max_radius:
            raise Refused("radius")
    bad = int(np.count_nonzero(~np.isfinite(coa)) + np.count_nonzero(~np.isfinite(coa_n)))
    if bad:
        raise Refused(f"{bad} non-finite samples")
    smoothed = None
    if weights is not None:
        coa, coa_n = smooth(coa, r, weights), smooth(coa_n, r, weights)
        smoothed = np.stack([coa, coa_n])
    trig = coa_n if trigger_on else coa
    thr = chunk_thresholds(trig, method, value, chunk)
    cand = find_candidates(coa, trig, threshold_trace(thr, method, chunk, n), period_ns, mw_ns, mei_ns)
    ev_i, ev_f = merge(cand, trig, coa, coa_n, period_ns, mw_ns)
    if len(ev_i) > max_events:
        raise Refused(f"{len(ev_i)} events, room for {max_events}")
    return {"n_candidates": len(cand), "n_events": len(ev_i), "events_i": ev_i, "events_f": ev_f,
            "thresholds": thr, "smoothed": smoothed, "candidates": cand}
