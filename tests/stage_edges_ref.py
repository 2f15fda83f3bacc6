# -*- coding: utf-8 -*-
"""
Restatements of three older stages -- the specification their kernels are tested against at the edges
(tests/test_stage_edges_gpu.py), pinned on the CPU by tests/test_stage_edges_host.py:

* the on-device STA/LTA onset stage (include/qmhip.h: qm_engine_onsets; kernels stalta_sums_kernel and
  onset_rows_kernel, csrc/qm_kernels.hpp): ``stalta_strict`` and ``onset_stage_strict``;
* on-device table serving (qm_engine_serve; serve_table_kernel<256 | 64>): ``serve_expected``;
* the scan of a materialised volume (qm_engine_find_max_coa; scan_volume_kernel and combine_kernel in mode 2):
  ``scan_expected``.

``stalta_strict`` is a plain Python float64 loop with ONE operation per statement, in the order of the reference's
``onsetlib.c`` (classic :35-59, centred :79-108, recursive :126-148).  The running sums of the sliding windows are a
serial chain, and where a window has run out of signal (a dead stretch behind a burst) what they hold is rounding
residue: the centred ``lta > 0`` guard and the classic ratio there depend on the last bits of the sums, so the ORDER
of the additions is part of the result.  The C oracle (oracle/qm_oracle.c) is built with the reference's ``-Ofast``
and is therefore no order reference for such data; a Python float is an IEEE double and Python re-associates nothing.

The ``*_plan`` helpers restate the launch arithmetic of the host code, so that a test can show which path a shape
takes (which serving instantiation, whether a trace is staged in LDS, how a volume is split).
"""

import math

import numpy as np

from oracle import qm_oracle

INT32_MIN = -(1 << 31)
INT32_MAX = (1 << 31) - 1
POSITIONS = ("classic", "centred", "recursive")


# -- onset stage -------------------------------------------------------------------------------------------------------
def stalta_strict(f, nsta, nlta, position):
    """
    (S, L, onset) of one transformed trace ``f`` (``x * x`` or ``|x|``), each a float64 array of len(f).

    S and L are the running short- and long-window sums as the recurrence leaves them at every sample it visits (NaN
    where it visits none); onset is the reference's output: pre-filled with ones (classic, centred) or zeros
    (recursive), ``sta / lta * (nlta / nsta)`` where the C loop writes.  The engine's rules where the reference has
    none (it would read or write out of bounds): a trace with ``nlta > n``, ``nsta > nlta`` or ``nsta < 1`` is all
    ones, a centred trace with ``nsta + nlta > n`` is all ones, a recursive trace nulls the first ``nlta`` samples
    only when ``nlta < n`` (that one is the reference's own) and stays all zeros for a window shorter than 1.
    """
    f = [float(v) for v in np.asarray(f, dtype=np.float64)]
    n = len(f)
    nsta, nlta = int(nsta), int(nlta)
    S, L = [math.nan] * n, [math.nan] * n
    if position == "recursive":
        onset = [0.0] * n
        if nsta < 1 or nlta < 1:
            return np.array(S), np.array(L), np.array(onset)
        csta = 1.0 / float(nsta)
        clta = 1.0 / float(nlta)
        ksta = 1 - csta
        klta = 1 - clta
        sta, lta = 0.0, 0.0
        if n > 0:
            S[0], L[0] = 0.0, 0.0
        for i in range(1, n):
            buf = f[i]
            a = csta * buf
            b = ksta * sta
            sta = a + b
            a = clta * buf
            b = klta * lta
            lta = a + b
            S[i], L[i] = sta, lta
            onset[i] = _div(sta, lta)
        if nlta < n:
            for i in range(nlta):
                onset[i] = 1.0
        return np.array(S), np.array(L), np.array(onset)
    onset = [1.0] * n
    if nlta > n or nsta > nlta or nsta < 1:
        return np.array(S), np.array(L), np.array(onset)
    frac = float(nlta) / float(nsta)
    if position == "classic":
        sta = 0.0
        for i in range(nsta):
            sta = sta + f[i]
        lta = sta
        for i in range(nsta, nlta):
            buf = f[i]
            lta = lta + buf
            d = buf - f[i - nsta]
            sta = sta + d
        S[nlta - 1], L[nlta - 1] = sta, lta
        onset[nlta - 1] = _ratio(sta, lta, frac)
        for i in range(nlta, n):
            buf = f[i]
            d = buf - f[i - nsta]
            sta = sta + d
            d = buf - f[i - nlta]
            lta = lta + d
            S[i], L[i] = sta, lta
            onset[i] = _ratio(sta, lta, frac)
    elif position == "centred":
        if nsta + nlta > n:
            return np.array(S), np.array(L), np.array(onset)
        sta, lta = 0.0, 0.0
        for i in range(nlta):
            lta = lta + f[i]
        for i in range(nlta, nlta + nsta):
            sta = sta + f[i]
        S[nlta - 1], L[nlta - 1] = sta, lta
        onset[nlta - 1] = _ratio(sta, lta, frac)
        for i in range(nlta, n - nsta):
            d = f[i + nsta] - f[i]
            sta = sta + d
            d = f[i] - f[i - nlta]
            lta = lta + d
            S[i], L[i] = sta, lta
            onset[i] = _ratio(sta, lta, frac) if lta > 0.0 else 1.0
    else:
        raise ValueError(position)
    return np.array(S), np.array(L), np.array(onset)


def _div(a, b):
    """``a / b`` in IEEE arithmetic (Python raises where C divides by zero)."""
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _ratio(sta, lta, frac):
    q = _div(sta, lta)
    return q * frac


def onset_stage_strict(signals, trace_row, nsta, nlta, transform="energy", position="classic", taper_pad=-1,
                       min_onset_value=0.4):
    """
    The loop of ``oracle.np_onset_stage`` (STALTAOnset._onset, stalta.py:515-546, with the taper windows of
    _trim_taper_pad, :579-581, then lib.migrate's clip + log, lib.py:93-94) built on ``stalta_strict``, with the
    recursive position added: it pre-fills with zeros; taper, clip and log are those of the other two.  The squares of
    a row's components are added in trace order, one operation per statement.  Returns (raw, logged), (n_rows, T).
    """
    signals = np.asarray(signals, dtype=np.float64)
    trace_row = np.asarray(trace_row)
    n = signals.shape[1]
    raw = np.empty((len(nsta), n))
    for row in range(len(nsta)):
        ns, nl = int(nsta[row]), int(nlta[row])
        sumsq, count = np.zeros(n), 0
        for tr in np.flatnonzero(trace_row == row):
            x = signals[tr] * signals[tr] if transform == "energy" else np.abs(signals[tr])
            o = stalta_strict(x, ns, nl, position)[2]
            if taper_pad >= 0:
                o[:min(max(taper_pad + nl - 1, 0), n)] = 1.0
                o[max(n - (ns + taper_pad), 0):] = 1.0
            sq = o * o
            sumsq = sumsq + sq
            count += 1
        mean = sumsq / float(count)
        onset = np.sqrt(mean)
        raw[row] = np.where(onset < min_onset_value, min_onset_value, onset)      # (a NaN stays a NaN)
    with np.errstate(invalid="ignore", divide="ignore"):
        logged = np.log(np.where(raw < 0.01, 0.01, raw))
    return raw, logged


def window_sums_exact(f, n):
    """Correctly rounded sum of ``f[i - n + 1 : i + 1]`` at every i >= n - 1 (``math.fsum``); NaN before that."""
    f = [float(v) for v in np.asarray(f, dtype=np.float64)]
    out = np.full(len(f), np.nan)
    for i in range(n - 1, len(f)):
        out[i] = math.fsum(f[i - n + 1:i + 1])
    return out


def stress_traces(n=2001, count=3, seed=1):
    """[count][n]: unit normal noise, a 40-sample burst at x 1000, then a 200-sample gap of exact zeros.  Behind the
    burst the sliding sums hold rounding residue of the burst's size where the exact window sum is 0; with this seed
    the residue of the long sum comes out positive on some traces and negative on others, for x * x and for |x|."""
    x = np.random.default_rng(seed).standard_normal((count, n))
    x[:, 700:740] *= 1000.0
    x[:, 1200:1400] = 0.0
    return x


def onset_in_lds(t_samples):
    """OnsetStage::launch: the transformed trace is staged in LDS while it fits 160 KB (20 480 samples)."""
    return t_samples * 8 <= 160 * 1024


# -- table serving -----------------------------------------------------------------------------------------------------
def serve_expected(grids, rows, rate, decimate=(1, 1, 1)):
    """
    int32 [nx][ny][nz][len(rows)]: ``Grid3D.decimate`` (oracle.np_decimate) of the selected grids, stacked on the last
    axis, ``np.rint(tt * rate)``, and the int32 conversion written out: the value where r is finite and in
    [-2^31, 2^31 - 1], otherwise INT32_MIN (what x86-64's conversion gives ``.astype(np.int32)`` in the reference,
    lut.py:538; ``astype`` itself is platform-defined there and warns).
    """
    tt = np.stack([qm_oracle.np_decimate(np.asarray(grids[r], dtype=np.float64), decimate) for r in rows], axis=-1)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(tt * float(rate))
    ok = np.isfinite(r) & (r >= float(INT32_MIN)) & (r <= float(INT32_MAX))
    out = np.full(r.shape, INT32_MIN, dtype=np.int32)
    out[ok] = r[ok].astype(np.int32)
    return out


def serve_plan(n_rows):
    """(nodes per workgroup, pitch in words, LDS bytes) of qm_engine_serve; nodes = 0: refused ("too many rows")."""
    pitch = (n_rows + 1) | 1
    npb = 256 if 256 * pitch * 4 <= 64 * 1024 else 64
    lds = npb * pitch * 4
    return (npb if lds <= 64 * 1024 else 0), pitch, lds


# -- volume scan -------------------------------------------------------------------------------------------------------
def scan_expected(vol):
    """
    (max_coa, max_norm_coa, index) of a volume [n_nodes][n_samples] (migratelib.c:85-111): per sample the FIRST index of
    the largest value under a strict ``>`` that starts from -inf at index 0 -- so a NaN never wins, and a sample where
    nothing compares greater keeps (-inf, 0) --, the node sum by ``math.fsum``, and ``max_coa * N / sum``.
    """
    vol = np.asarray(vol, dtype=np.float64)
    n_nodes, n_samples = vol.shape
    best = np.full(n_samples, -np.inf)
    idx = np.zeros(n_samples, dtype=np.int64)
    for node in range(n_nodes):
        wins = vol[node] > best
        best = np.where(wins, vol[node], best)
        idx = np.where(wins, node, idx)
    total = np.array([math.fsum(vol[:, t]) for t in range(n_samples)])
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = best * float(n_nodes) / total
    return best, norm, idx


def scan_plan(n_samples, n_nodes, n_cu, scan_waves=32):
    """scan_fold's split (csrc/qm_engine.hip): dict of tiles, time workgroups, wavefronts per workgroup, sets, nodes
    per set and nodes of the last set."""
    tiles = (n_samples + 63) // 64
    groups = (tiles + 15) // 16
    waves = (tiles + groups - 1) // groups
    xgroups = (tiles + waves - 1) // waves
    sets = max(1, (scan_waves * n_cu + tiles - 1) // tiles)
    sets = min(sets, max(1, n_nodes // 256), 65535)
    per = (n_nodes + sets - 1) // sets
    sets = (n_nodes + per - 1) // per
    return dict(tiles=tiles, xgroups=xgroups, waves=waves, sets=sets, per=per, last=n_nodes - (sets - 1) * per)
