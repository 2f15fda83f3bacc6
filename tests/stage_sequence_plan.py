# -*- coding: utf-8 -*-
"""
Seeded call sequences over EVERY family of stage call of one long-lived engine (tests/test_stage_sequences.py walks
them on the GPU; tests/test_stage_sequence_plan.py checks on the CPU that they cover what they are meant to cover).
The companion of tests/sequence_plan.py, which walks the stacking launches alone.

Pure Python, no GPU (the limits and some input helpers are imported from the families' GPU-marked test modules, which
import without a device): a roster of seventeen *kinds* of call, a short fixed list of *requests* per kind (one call with all of
its arguments, hashable; :func:`build` makes a request's inputs with the families' own helpers), and a generator that
turns ``(flavour, seed, steps)`` into a list of operations.  The generator scores every request it could issue next by
what that request would add to the coverage conditions -- an ordered pair of kinds that was not adjacent yet, a long
call in front of a short one on a shared buffer, the good call behind a refusal -- and takes one of the best; the
conditions themselves are computed from the finished plan alone (:func:`coverage`, :func:`unmet`).

Why these conditions: the engine's scratch is not separate per family (csrc/qm_engine.hpp).  ``SHARING`` lists the
buffers the code shows to be shared on purpose; the condition on ALL ordered pairs of kinds is there so that the walk
does not depend on that list being complete.
"""

import collections
import copy
import functools
import itertools
import pathlib
import random

import numpy as np

import sequence_plan as sp

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "quakemigrate_amd" / "csrc"

# ---------------------------------------------------------------------------------------------- the roster
STACKING = ("detect", "migrate_host", "marginal_map")
KINDS = ("resample", "preprocess", "onsets", "pick_phases", "measure_amplitudes", "trigger_series",
         "scanmseed_encode", "scanmseed_decode", "tt_homogeneous", "tt_sections", "tt_sweep", "locate_fits",
         "rbf_peak", "exp_probe") + STACKING
TABLES = ("c3_30", "c2_11")         # two of sequence_plan.TABLES: shift-reuse, and the exact-row-count kernels
STREAM_TABLE = "c2_11"              # the with_stream flavour's one table
SCAN_LENGTHS = (1, 257, 401)
CAPACITIES = sp.CAPACITIES

# Buffers the code shows to be shared between families (csrc/qm_engine.hpp): the kinds of each set are walked in every
# order, several times, and with a long call in front of a short one and the other way round.
SHARING = collections.OrderedDict([
    ("staging.sig", ("preprocess", "onsets", "pick_phases")),
    ("staging.pre_out", ("preprocess", "resample")),
    ("d_onsets", ("onsets",) + STACKING),
    ("fit.a / fit.b / fit.part", ("locate_fits", "rbf_peak", "exp_probe")),
    ("fit.part / sweep.work", ("exp_probe", "detect")),
])
LDS_KINDS = ("resample", "measure_amplitudes", "pick_phases", "tt_sections")

# kind, name (unique within the kind), table ("" where the call needs none), element count of what the call stages,
# "short" / "long" / None, host input? host output? (None: the call offers no choice), "under" / "over" the family's
# LDS limit or None, is it refused?, the kind's own arguments (a sequence_plan.Request for the stacking kinds)
Request = collections.namedtuple("Request", "kind name table size length host_in host_out lds refusal args")
# op: "load" (table) | "select" (table, capacity, expect) | "launch" (table resident or None, request) |
#     "set_stream" ("torch" / "own") | "release" | "push" (index of the raw step)
Op = sp.Op

FLAVOURS = collections.OrderedDict([
    # name -> (configuration, has table operations, steps of the walk)
    ("engine", ({}, True, 680)),
    ("screen", ({"screen": 1}, True, 680)),
    ("shift_wide", ({"shift_wide": 1}, True, 680)),
    ("with_stream", ({}, False, 540)),
])
SEEDS = {name: 20261021 for name in FLAVOURS}
POISON_STEPS = 150                  # the shorter plan of the poisoned-pool children
POISON_FLAVOURS = ("engine", "with_stream")
PUSH_STEPS = 12                     # the stream's fixed list of raw steps; push k pushes step k % PUSH_STEPS
PUSH_EVERY = 24                     # operations between two pushes

LIMIT_KEYS = collections.OrderedDict([
    # read-out key of Engine.get -> (header, constant); "resample_lds_samples" is tests/test_resample_gpu.py's
    ("amp_lds_samples", ("qm_amplitudes.hpp", "kAmpLdsSamples")),
    ("pick_lds_samples", ("qm_picks.hpp", "kPicksLdsSamples")),
    ("tt_lds_nodes", ("qm_traveltimes.hpp", "kTtLdsNodes")),
])
TT_LIMIT_NZ = 125                   # tests/test_traveltimes_gpu.py: sections of 125 rows on both sides of the limit


@functools.lru_cache(maxsize=None)
def header_limits():
    """The families' LDS limits as the headers state them (the GPU test reads them where each family's own test does,
    ``Engine.get`` or tests/test_resample_gpu.py's constant, and asserts that they are these)."""
    from locate_edges_ref import header_constant
    from test_resample_gpu import LDS_SAMPLES

    out = {key: header_constant(name, (CSRC / header).read_text()) for key, (header, name) in LIMIT_KEYS.items()}
    out["resample_lds_samples"] = LDS_SAMPLES
    return out


def _r(kind, name, size, length=None, host_in=None, host_out=None, lds=None, refusal=False, table="", args=()):
    return Request(kind, name, table, int(size), length, host_in, host_out, lds, refusal, args)


@functools.lru_cache(maxsize=None)
def rosters():
    """kind -> the fixed list of its requests.  The stacking kinds hold their requests on both TABLES (a flavour
    draws those of the table that is resident).  Sizes: the smallest shape at which each kernel still takes each of
    its paths, none larger than its family's own small cases; a kind's long requests stage at least twice what its
    short ones do, so a staging buffer both moves and keeps a stale tail."""
    lim = header_limits()
    rs, amp, pick, tt = (lim[k] for k in ("resample_lds_samples", "amp_lds_samples", "pick_lds_samples",
                                           "tt_lds_nodes"))
    out = collections.OrderedDict()
    # size: the kept series.  Upsampling alone (NumPy's bits); decimation through the detrend, taper and low-pass
    out["resample"] = [
        _r("resample", "up_short", 131, "short", True, True),
        _r("resample", "dec_long_dev", 601, "long", False, False),
        _r("resample", "dec_long_host", 601, "long", True, True),
        _r("resample", "dec_under", rs, "long", True, True, lds="under"),
        _r("resample", "dec_over", rs + 1, "long", True, True, lds="over"),
    ]
    # five traces: zero phase with tapers of T // 2, forward only without a taper, zero phase with unequal tapers
    out["preprocess"] = [
        _r("preprocess", "zero_phase_taper_short", 5 * 65, "short", True, True, args=(65, True, 1)),
        _r("preprocess", "forward_plain_dev", 5 * 301, "long", False, False, args=(301, False, 0)),
        _r("preprocess", "zero_phase_taper_long", 5 * 301, "long", True, True, args=(301, True, 2)),
        _r("preprocess", "forward_taper_dev_short", 5 * 64, "short", False, True, args=(64, False, 2)),
    ]
    out["onsets"] = [
        _r("onsets", "classic_short", 3 * 84, "short", True, True, args=("classic", "energy", 84)),
        _r("onsets", "centred_long_dev", 7 * 150, "long", False, False, args=("centred", "abs", 150)),
        _r("onsets", "recursive_long", 3 * 200, "long", True, True, args=("recursive", "energy", 200)),
        _r("onsets", "classic_long_dev_in", 7 * 150, "long", False, True, args=("classic", "energy", 150)),
    ]
    out["pick_phases"] = [
        _r("pick_phases", "family_given_thresholds_short", 16 * 451, "short", True, None, lds="under", args=(1,)),
        _r("pick_phases", "designed_long_dev", 25 * 700, "long", False, None, lds="under", args=(0,)),
        _r("pick_phases", "noise_sets_long", 40 * 331, None, True, None, lds="under", args=(0,)),
        _r("pick_phases", "at_the_limit", 2 * pick, "long", True, None, lds="under", args=(0,)),
        # (this family has no scratch form: a row past the limit is refused by name)
        _r("pick_phases", "over_the_limit", 2 * (pick + 1), None, True, None, lds="over", refusal=True, args=(0,)),
        _r("pick_phases", "window_outside_its_row", 4 * 451, None, True, None, refusal=True, args=(0,)),
    ]
    out["measure_amplitudes"] = [
        _r("measure_amplitudes", "designed_short", 64, "short", True, None, lds="under", args=("plain",)),
        _r("measure_amplitudes", "family_long_dev", 12824, "long", False, None, lds="under", args=("plain",)),
        _r("measure_amplitudes", "filtered_host", 2 * (65 + 301), None, True, None, lds="under", args=("filter",)),
        _r("measure_amplitudes", "windows_under", 64 + amp, "long", True, None, lds="under", args=("plain",)),
        _r("measure_amplitudes", "windows_over", 64 + amp + 1, "long", True, None, lds="over", args=("plain",)),
        _r("measure_amplitudes", "window_outside_its_trace", 64, None, True, None, refusal=True, args=("plain",)),
    ]
    out["trigger_series"] = [
        _r("trigger_series", "static_short", 1000, "short", True, None, args=("static",)),
        _r("trigger_series", "mad_smoothed_long", 5000, "long", True, None, args=("mad",)),
        _r("trigger_series", "median_ratio_long_dev", 2500, "long", False, None, args=("median_ratio",)),
        # (refused after the series were staged and the stage clock begun: the event tables have no room)
        _r("trigger_series", "too_many_events", 1000, None, True, None, refusal=True, args=("static",)),
    ]
    out["scanmseed_encode"] = [
        _r("scanmseed_encode", "int_short", 5 * 40, "short", True, None, args=("int",)),
        _r("scanmseed_encode", "int_long_dev", 5 * 3000, "long", False, None, args=("int",)),
        _r("scanmseed_encode", "float_long", 5 * 2000, "long", True, None, args=("float",)),
        _r("scanmseed_encode", "float_short_dev", 5 * 300, "short", False, None, args=("float",)),
        _r("scanmseed_encode", "difference_of_2_29", 5 * 3000, None, True, None, refusal=True, args=("int",)),
    ]
    out["scanmseed_decode"] = [
        _r("scanmseed_decode", "ints_short", 5 * 600, "short", None, True, args=(False,)),
        _r("scanmseed_decode", "factors_long_dev", 5 * 9000, "long", None, False, args=(True,)),
        _r("scanmseed_decode", "factors_short", 5 * 600, "short", None, True, args=(True,)),
        _r("scanmseed_decode", "ints_long_dev", 5 * 9000, "long", None, False, args=(False,)),
        _r("scanmseed_decode", "flipped_constant", 5 * 9000, None, None, True, refusal=True, args=(False,)),
    ]
    nodes = 23 * 19 * 17
    out["tt_homogeneous"] = [
        _r("tt_homogeneous", "two_rows", 2 * nodes, "short", None, True, args=(2,)),
        _r("tt_homogeneous", "ten_rows_dev", 10 * nodes, "long", None, False, args=(10,)),
    ]
    under, over = tt // TT_LIMIT_NZ, tt // TT_LIMIT_NZ + 1
    out["tt_sections"] = [
        _r("tt_sections", "small", 2 * 67 * 45, "short", None, True, lds="under", args=(67, 45, False)),
        _r("tt_sections", "small_forced_dev", 2 * 67 * 45, "short", None, False, lds="over", args=(67, 45, True)),
        # (one section each, the low-velocity model: the restatement of these two costs a second apiece)
        _r("tt_sections", "under", under * TT_LIMIT_NZ, "long", None, True, lds="under",
           args=(under, TT_LIMIT_NZ, False)),
        _r("tt_sections", "over", over * TT_LIMIT_NZ, "long", None, True, lds="over",
           args=(over, TT_LIMIT_NZ, False)),
        _r("tt_sections", "one_round", 67 * 45, None, None, True, refusal=True, args=(67, 45, False)),
    ]
    out["tt_sweep"] = [
        _r("tt_sweep", "host_sections", 5 * nodes, "short", True, True, args=(5,)),
        _r("tt_sweep", "device_sections_long", 10 * nodes, "long", False, False, args=(10,)),
        _r("tt_sweep", "node_outside_its_section", 5 * nodes, None, True, True, refusal=True, args=(5,)),
    ]
    out["locate_fits"] = [
        _r("locate_fits", "small", 13 * 12 * 11, "short", True, True, args=("small", 0.8)),
        _r("locate_fits", "short_dev", 64 * 63 * 40, "long", False, False, args=("short", 3.3)),
        _r("locate_fits", "short_host", 64 * 63 * 40, "long", True, True, args=("short", 3.3)),
    ]
    # args: index into locate_edges_ref.RBF_CASES (n = 2 at a small refinement; n = 5, upscale 16: 65^3 points)
    out["rbf_peak"] = [
        _r("rbf_peak", "n2", 8, "short", None, None, args=(3,)),
        _r("rbf_peak", "n5_past_one_pass", 125, "long", None, None, args=(0,)),
    ]
    # one request each: exp_correctly_rounded stages its arguments through fit.a and fit.b, exp2f_max_error folds
    # through fit.part alone (that is what "long" and "short" mean for this kind)
    out["exp_probe"] = [
        _r("exp_probe", "exp_correctly_rounded", 4099, "long", None, None),
        _r("exp_probe", "exp2f_max_error", 1, "short", None, None),
    ]
    for kind in STACKING:
        out[kind] = []
    for t in TABLES:
        for ns in SCAN_LENGTHS:
            length = "short" if ns == 1 else "long"
            out["detect"].append(_r("detect", f"{t}_{ns}", ns, length, True, True, table=t,
                                    args=sp.Request("detect", t, 0, ns, ())))
            first, end = {1: (0, 1), 257: (0, 257), 401: (10, 200)}[ns]
            out["marginal_map"].append(_r("marginal_map", f"{t}_{ns}", ns, length, True, True, table=t,
                                          args=sp.Request("marginal_map", t, 0, ns, (first, end))))
            scan, chunked = {1: (True, False), 257: (False, True), 401: (True, True)}[ns]
            out["migrate_host"].append(_r("migrate_host", f"{t}_{ns}", ns, length, True, True, table=t,
                                          args=sp.Request("migrate_host", t, 0, ns, (scan, chunked, False))))
        out["migrate_host"].append(_r("migrate_host", f"{t}_257_accumulate", 257, "long", True, True, table=t,
                                      args=sp.Request("migrate_host", t, 0, 257, (False, True, True))))
    assert tuple(out) == KINDS
    return out


def has_tables(flavour):
    return FLAVOURS[flavour][1]


def requests_of(flavour):
    """kind -> the requests a flavour's walk draws from (with_stream: its one table's stacking requests)."""
    out = collections.OrderedDict()
    for kind, reqs in rosters().items():
        out[kind] = [r for r in reqs if has_tables(flavour) or r.table in ("", STREAM_TABLE)]
    return out


def refusals_of(flavour):
    return [r for reqs in requests_of(flavour).values() for r in reqs if r.refusal]


def sharing_pairs():
    """Ordered pairs of distinct kinds that share a buffer."""
    out = []
    for kinds in SHARING.values():
        out += [p for p in itertools.permutations(kinds, 2) if p not in out]
    return out


# ---------------------------------------------------------------------------------------------- the inputs
TT_LL, TT_SPACING, TT_COUNT, TT_H, TT_H_OFF = (-3.0, 1.5, -1.0), (0.5, 0.4, 0.25), (23, 19, 17), 0.125, 0.07


@functools.lru_cache(maxsize=None)
def build(req, limits=None):
    """The inputs of a request as a dict of NumPy arrays and plain values, made with the families' own helpers and
    seeds of their own; ``"elements"`` is what ``req.size`` promises.  Device inputs are made from these by the GPU
    test.  ``limits``: the items of the LDS limits as the engine states them (default: the headers')."""
    lim = dict(limits) if limits is not None else header_limits()
    make = globals()[f"_build_{req.kind}"] if req.kind not in STACKING else _build_stacking
    d = make(req, lim)
    assert d["elements"] == req.size, (req, d["elements"])
    return d


def _build_resample(req, lim):
    import resample_ref as rr
    from test_resample_gpu import NO_TAPER, _arrays

    if req.name == "up_short":
        u, n_raw, pad = 2, 65, 1
        x = rr.raw_traces(100 * u + n_raw, [n_raw], np.float64)[0]
        T = (n_raw - 1) * u + 1 + 2 * pad
        a = _arrays([rr.record(0, n_raw, up=u, pad_left=pad, pad_right=pad)], T)
        return dict(raw=x, arrays=a, sos=None, elements=T, bits="upsample")
    n_up = {"dec_long_dev": 601, "dec_long_host": 601, "dec_under": lim["resample_lds_samples"],
            "dec_over": lim["resample_lds_samples"] + 1}[req.name]
    sos = rr.stable_sos(n_up, 2, 2)
    x = rr.raw_traces(500 + n_up, [n_up])[0]
    m = n_up // 20
    rng = np.random.default_rng(n_up)
    weights = np.concatenate([np.sort(rng.uniform(0, 1, m)), np.sort(rng.uniform(0, 1, m))[::-1]])
    a = _arrays([rr.record(0, n_up, dec=2, lowpass=1)], -(-n_up // 2), sos, [[0, m]] if m else NO_TAPER, weights,
                detrend=1)
    return dict(raw=x, arrays=a, sos=sos, weights=weights, m=m, elements=n_up, bits="decimate")


def _build_preprocess(req, lim):
    import preprocess_ref as pr
    from test_preprocess_gpu import TRACE_FILTER, _tapers, stable_sos

    T, zero_phase, taper = req.args
    left, right = _tapers(T, T)[taper]
    return dict(x=pr.noisy_traces(300 + T, 5, T), trace_filter=TRACE_FILTER, sos=stable_sos(T, 2, 2), left=left,
                right=right, zero_phase=zero_phase, elements=5 * T)


def _build_onsets(req, lim):
    position, transform, T = req.args
    if req.name in ("classic_short", "recursive_long"):
        x = np.random.default_rng(103 + T).standard_normal((3, T))
        rows, nsta, nlta = [0, 1, 0], [7, 7], [40, 40]
        kw = dict(taper_pad=5 if position == "recursive" else -1, min_onset_value=0.4)
    else:                               # four rows of 1, 2, 3 and 1 components, the traces interleaved
        x = np.random.default_rng(104).standard_normal((7, T))
        rows, nsta, nlta = [2, 0, 1, 2, 3, 1, 2], [3, 5, 7, 4], [20, 31, 50, 64]
        kw = dict(taper_pad=3, min_onset_value=0.4)
    return dict(x=x, trace_row=rows, nsta=nsta, nlta=nlta, kw=dict(kw, transform=transform, position=position),
                elements=x.size)


def _build_pick_phases(req, lim):
    import picks_ref as pk

    limit = lim["pick_lds_samples"]
    if req.name in ("at_the_limit", "over_the_limit"):              # (tests/test_picks_gpu.py's longest row)
        rng = np.random.default_rng(3)
        t = np.arange(limit, dtype=np.float64)
        onsets = 1.3 + 0.1 * rng.random((2, limit))
        centres = (limit - 40, limit // 2)
        for r, c in enumerate(centres):
            onsets[r] += 6.0 * np.exp(-((t - c) ** 2) / (2.0 * 5.0 ** 2))
        windows = np.array([[limit - 100, c, limit] if r == 0 else [c - 60, c, c + 60]
                            for r, c in enumerate(centres)], dtype=np.int32)
        if req.name == "over_the_limit":
            onsets = np.concatenate([onsets, np.full((2, 1), 1.3)], axis=1)
        d = dict(onsets=np.ascontiguousarray(onsets), windows=windows, row_group=np.array([0, 1], dtype=np.int32),
                 sampling_rate=50.0, halfwidth=np.array([5.0, 5.0]))
    elif req.name == "designed_long_dev":
        d = pk.designed_rows()
    elif req.name == "noise_sets_long":
        d = pk.noise_set_rows()
    else:
        d = pk.family(n_stations=8)
        if req.name == "window_outside_its_row":
            d = {k: (v[:4].copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
            d["windows"][0] = (-1, 10, 50)
    d = dict(d, mode=req.args[0], elements=d["onsets"].size)
    if d["mode"] == 1:                  # the thresholds the MAD mode gives, handed in
        d["thresholds"] = pk.pick_rows(d["onsets"], d["windows"], d["row_group"], d["sampling_rate"],
                                       d["halfwidth"])[0][:, 0].copy()
    return d


def _build_measure_amplitudes(req, lim):
    import amplitudes_ref as ar
    import preprocess_ref as pp

    limit = lim["amp_lds_samples"]
    d = dict(sos=None, table=None, weights=None, detrend=False, want_filtered=False)
    if req.name in ("designed_short", "window_outside_its_trace"):
        rows = ar.designed_rows()
        names = [k for k, v in rows.items() if v[1] == 0.0]
        traces = [rows[k][0] if len(rows[k][0]) else np.zeros(3) for k in names]
        # (as many of the designed rows as make up the short request's 64 samples)
        keep, total = [], 0
        for k, x in enumerate(traces):
            if total + len(x) <= 64:
                keep.append(k)
                total += len(x)
        traces = [traces[k] for k in keep] + [np.arange(64 - total, dtype=np.float64) % 3]
        recs = [[k, 0, len(rows[names[j]][0]), 1] for k, j in enumerate(keep)] + [[len(keep), 0, 64 - total, 1]]
        if req.name == "window_outside_its_trace":
            recs[0] = [0, 0, len(traces[0]) + 1, 1]
    elif req.name == "family_long_dev":
        fam = ar.family()
        return dict(d, traces=fam["traces"], packed=fam["packed"], trecs=fam["trace_records"],
                    recs=fam["window_records"], elements=fam["packed"].size, check="family")
    elif req.name == "filtered_host":
        import resample_ref as rr

        lengths, sos, rng = [65, 301], rr.stable_sos(13, 2, 2), np.random.default_rng(13)
        traces, trecs, table, weights = [], [], [], []
        for k, n in enumerate(lengths):
            m = n // 3
            table.append([len(weights), m])
            weights += list(np.sort(rng.uniform(0, 1, m))) + list(np.sort(rng.uniform(0, 1, m))[::-1])
            for taper in (k, -1):
                traces.append(pp.noisy_traces(100 * n + taper + 1, 1, n)[0])
                trecs.append([0, n, len(traces) % 2, taper])
        packed, offsets = ar.pack(traces)
        trecs = np.array(trecs, dtype=np.int64)
        trecs[:, 0] = offsets
        return dict(d, traces=traces, packed=packed, trecs=trecs, recs=[[k, 0, len(x), 0] for k, x in enumerate(traces)],
                    sos=sos, table=table, weights=np.array(weights), detrend=False, want_filtered=True,
                    elements=packed.size, check="filter")
    else:                               # noise windows through the window detrend, the long one in LDS or in scratch
        n = limit + (1 if req.name == "windows_over" else 0)
        x = pp.noisy_traces(43, 1, 64 + n)[0]
        return dict(d, traces=[x], packed=x, trecs=np.array([[0, len(x), -1, -1]], dtype=np.int64),
                    recs=[[0, 0, 64, 0], [0, 64, 64 + n, 0]], detrend=True, elements=x.size, check="window_detrend")
    packed, offsets = ar.pack(traces)
    trecs = np.stack([offsets, [len(x) for x in traces], [-1] * len(traces), [-1] * len(traces)], axis=1)
    return dict(d, traces=traces, packed=packed, trecs=trecs, recs=recs, elements=packed.size, check="bits")


def _build_trigger_series(req, lim):
    import trigger_ref as tr

    n = req.size
    rng = np.random.default_rng(n + len(req.name))
    method = req.args[0]
    x = np.round(rng.gamma(2.0, 1.0, (2, n)), 5)
    d = dict(coa=np.ascontiguousarray(x[0]), coa_n=np.ascontiguousarray(x[1]), method=method, weights=None,
             trigger_on=0, chunk_samples=1, value=4.0, max_events=n, elements=n)
    if method == "static":              # quiet series with a few bursts further apart than the events merge over
        x *= 0.1
        for at in (150, 450, 451, 452, 800):
            x[:, at] = 5.0 + 0.001 * at
        d.update(coa=np.ascontiguousarray(x[0]), coa_n=np.ascontiguousarray(x[1]))
    if method == "mad":
        d.update(weights=tr.gaussian_weights(2.5, 4.0)[1], value=2.0, chunk_samples=1000, trigger_on=1)
    elif method == "median_ratio":
        d.update(value=4.0, chunk_samples=700)
    if req.refusal:
        d.update(max_events=1)
    return d


def _build_scanmseed_encode(req, lim):
    import scanmseed_ref as ref
    from quakemigrate_amd import scanmseed as sm

    n = req.size // 5
    if req.args[0] == "int":
        if req.refusal:
            series = np.zeros((5, n), dtype=np.int32)
            series[3, 2500:] = 1 << 29                              # a difference of 2^29 at Y[2500]
        elif req.name == "int_short":
            x = np.asarray(ref.designed_series()["tail5"], dtype=np.int32)
            assert len(x) == n
            series = np.stack([np.concatenate([np.full(j, x[0], dtype=np.int32), x])[:n] for j in range(5)])
        else:
            rng = np.random.default_rng(11)
            classes = [(0, 1, 2), (0, 1, 2, 3, 4), (2, 3, 4, 5), (0, 1, 2, 3, 4, 5, 6), (0, 6)]
            series = np.stack([ref.switching_walk(rng, n, classes=cl, max_run=17) for cl in classes])
        return dict(series=np.ascontiguousarray(series, dtype=np.int32), factors=None, clips=None, elements=series.size)
    rng = np.random.default_rng(n)
    k = np.arange(n)
    coa = (2 * (k % 400) + 1) / 64.0                                # exact ties of both parities
    coa[n // 2:n // 2 + 4] = [21474.0, 21474.00001, 3e4, 21473.999995]
    coa_n = 1.0 + rng.uniform(0, 0.5, n)
    coord = np.stack([((2 * (k % 300) + 1) / 128.0) * np.where(k % 2, -1, 1),
                      -64.5 + np.cumsum(rng.uniform(-1e-5, 1e-5, n)), (2 * (k % 50) + 1) / 128.0 - 0.25], axis=1)
    ucf = 1000.0
    # (across the 21474 clip and back in steps a 30-bit difference holds)
    coa[n // 2 - 60:n // 2] = np.linspace(coa[n // 2 - 61], 21473.9, 60)
    coa[n // 2 + 4:n // 2 + 64] = np.linspace(21473.9, coa[n // 2 + 64], 60)
    stacked = np.ascontiguousarray(np.stack([coa, coa_n, coord[:, 0], coord[:, 1], coord[:, 2]]))
    return dict(series=stacked, factors=[sm.scale_factors(ucf)[ch] for ch in sm.CHANNELS],
                clips=[sm.COA_CLIP, sm.COA_CLIP, None, None, None], quantised=sm.quantise(coa, coa_n, coord, ucf),
                elements=stacked.size)


def _build_scanmseed_decode(req, lim):
    import datetime as dt

    import scanmseed_ref as ref
    from quakemigrate_amd import scanmseed as sm

    n = req.size // 5
    x = ref.switching_walk(np.random.default_rng(7 + n), n, classes=(0, 1, 2, 3))
    series = {ch: np.concatenate([np.full(j, x[0], dtype=np.int32), x])[:n].astype(np.int32)
              for j, ch in enumerate(sm.CHANNELS)}
    blob = sm.encode_scanmseed(dt.datetime(2014, 6, 29, 23, 59, 0), 50.0, series)
    records = np.frombuffer(blob, dtype=np.uint8).reshape(-1, sm.RECLEN).copy()
    samples = np.array([sm.parse_header(r.tobytes())[4] for r in records])
    offsets = np.concatenate([[0], np.cumsum(samples)[:-1]])
    stations = [sm.parse_header(r.tobytes())[0] for r in records]
    factors = np.array([sm.scale_factors(1000.0)[s] for s in stations]) if req.args[0] else None
    if req.refusal:
        assert len(records) >= 8
        records[3, sm.DATA_OFFSET + 8 + 3] ^= 1                     # record 3's reverse integration constant
    return dict(records=records, samples=samples, offsets=offsets, total=int(samples.sum()), factors=factors,
                ints=np.concatenate([series[ch] for ch in sm.CHANNELS]), elements=int(samples.sum()))


def _tt_stations():
    from test_traveltimes_gpu import STATIONS

    return STATIONS


def _build_tt_homogeneous(req, lim):
    from test_traveltimes_gpu import VELOCITIES

    st = _tt_stations()
    xyz, vel = np.repeat(st, len(VELOCITIES), axis=0), np.tile(VELOCITIES, len(st))
    n = req.args[0]
    sel = slice(2, 2 + n) if n == 2 else slice(None)
    return dict(xyz=xyz[sel], vel=vel[sel], elements=n * int(np.prod(TT_COUNT)))


def _build_tt_sections(req, lim):
    from test_traveltimes_gpu import H, section_inputs

    nr, nz, force = req.args
    names = ("low_velocity",) if req.refusal or req.length == "long" else ("gradient", "low_velocity")
    slowness, zs, s0 = section_inputs(nz, names=names, depths=[7.4 * H])
    return dict(slowness=slowness, zs=zs, s0=s0, nr=nr, nz=nz, h=H, force_scratch=force,
                max_iters=1 if req.refusal else 64, elements=len(zs) * nr * nz)


def _build_tt_sweep(req, lim):
    from quakemigrate_amd import traveltimes as tt

    st = _tt_stations()
    h = TT_H if req.args[0] == 5 else TT_H_OFF
    plan = tt.plan_sections(TT_LL, TT_SPACING, TT_COUNT, st, h)
    rng = np.random.default_rng(20261020 + req.args[0])
    sections = rng.uniform(0.0, 9.0, size=(3, plan["nr"], plan["nz"] + 1))
    origins = np.column_stack([np.zeros(len(st)), plan["z0"] - (0.0 if h == TT_H else 0.4 * h)])
    row_section, xy = np.array([2, 0, 1, 1, 2], dtype=np.int32), st[:, :2]
    if req.args[0] == 10:
        origins, xy = np.concatenate([origins, origins]), np.concatenate([xy, xy])
        row_section = np.concatenate([row_section, (row_section + 1) % 3]).astype(np.int32)
    if req.refusal:
        sections = np.ones((1, plan["nr"], plan["nz"]))
        origins[3, 1] = TT_LL[2] + 3 * h            # row 3's section now starts below the grid's first depths
        row_section = np.zeros(5, dtype=np.int32)
    return dict(sections=sections, origins=origins, row_section=row_section, xy=xy, h=h, nr=plan["nr"],
                nz=plan["nz"], elements=len(xy) * int(np.prod(TT_COUNT)))


def _build_locate_fits(req, lim):
    import locate_edges_ref as ref

    m = ref.named_map(req.args[0])
    return dict(map=m, name=req.args[0], sgm=req.args[1], elements=m.size)


def _build_rbf_peak(req, lim):
    import locate_edges_ref as ref
    from quakemigrate_amd import locate

    n, upscale, centre, scale, seed = ref.RBF_CASES[req.args[0]]
    return dict(case=ref.RBF_CASES[req.args[0]], upscale=upscale,
                weights=locate._cubic_rbf_weights(ref.rbf_window(n, centre, scale, seed)), elements=n ** 3)


def _build_exp_probe(req, lim):
    if req.name == "exp2f_max_error":
        return dict(lo=1.0, hi=1.0625, elements=1)                  # 2^19 float32 arguments
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(-12, 12, 3000), rng.uniform(0, 3, 1000), rng.uniform(-700, 700, 91),
                         [0.0, -0.0, 1.0, 709.0, -740.0, 800.0, -800.0, np.nan]])
    return dict(x=xs, elements=xs.size)


def _build_stacking(req, lim):
    return dict(request=req.args, elements=req.args.ns)


# -- the with_stream flavour's stream: the set-up of tests/test_ownership_gpu.py on STREAM_TABLE's eleven rows
STREAM_RATE = 50
STREAM_NS = 64
STREAM_TRACE_ROW = np.array([0, 1, 2, 3, 4, 5, 5, 6, 7, 7, 8, 9, 9, 10], dtype=np.int32)    # 11 rows (5 P, 6 S)
STREAM_TRACE_PHASE = tuple("PPPPPSSSSSSSSS")
STREAM_RAW_RATE = (50, 100, 40, 100, 50, 40, 100, 40, 50, 100, 50, 40, 100, 50)


@functools.lru_cache(maxsize=None)
def stream_setup():
    """What the stream of the with_stream flavour is built from: (fsmp, lsmp, T, onset stage, resample stage, the
    PUSH_STEPS raw steps)."""
    import resample_ref as rr
    from quakemigrate_amd.preprocess import OnsetStage, ResampleStage

    tt, _, fsmp, _ = sp.table_case(STREAM_TABLE)
    lsmp = int(tt.max())
    T = fsmp + STREAM_NS + lsmp
    onset = OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 12.0, 2)},
                       sta_lta_windows={"P": (0.2, 1.0), "S": (0.3, 1.5)}, trace_row=STREAM_TRACE_ROW,
                       trace_phase=STREAM_TRACE_PHASE, row_phase=tuple("PPPPPSSSSSS"), taper_pad=20)
    n_raw = [(T - 1) * r // STREAM_RATE + 1 for r in STREAM_RAW_RATE]
    resample = ResampleStage(STREAM_RATE, STREAM_RAW_RATE, n_raw, [0.0] * len(STREAM_RAW_RATE), upfactor=5)
    raws = [rr.raw_traces(500 + 31 * k, n_raw, np.int32) for k in range(PUSH_STEPS)]
    return dict(fsmp=fsmp, lsmp=lsmp, T=T, rows=tt.shape[-1], onset=onset, resample=resample, raws=raws)


# ---------------------------------------------------------------------------------------------- what a plan covers
class Tracker:
    """The coverage of a plan, operation by operation (``add``), and what a launch would add to it (``gain``).  Two
    launches are adjacent when no table operation lies between them; a set_stream, a release or a push may."""

    def __init__(self, flavour):
        self.flavour = flavour
        self.reqs = requests_of(flavour)
        self.model = sp.ParkingModel()
        self.table = STREAM_TABLE if not has_tables(flavour) else None
        self.prev = None                # the previous launch's request, None behind a table operation
        self.prev_op = None
        self.stream = "own"
        self.c = {"steps": 0, "launches": 0, "requests": collections.Counter(), "kinds": collections.Counter(),
                  "pairs": collections.Counter(), "long_short": set(), "short_long": set(),
                  "lds": set(),         # (kind, "under" | "over" first)
                  "refusals": collections.Counter(), "refusal_then_own": set(), "refusal_then_other": set(),
                  "refusal_then_release": set(), "set_stream": 0, "release": 0,
                  "on_stream": set(),   # (kind, stream)
                  "capacities": collections.Counter(), "load_between_stages": 0, "select_expectations_hold": True,
                  "pushes": 0, "between_pushes": set(), "after_last_push": set()}
        self.pending_refusal = None     # a refusal with nothing but a release behind it so far
        self._load_after = None         # the launch directly in front of the last load, if there was one

    # what is still open, as a list of strings (empty: every condition holds)
    def unmet(self, floor="full"):
        c, out = self.c, []
        kinds = list(self.reqs)
        if floor == "poison":           # the shorter plan's own floor
            out += [f"kind {k} never" for k in kinds if c["kinds"][k] < 1]
            out += [f"sharing pair {p} never" for p in sharing_pairs() if c["pairs"][p] < 1]
            if sum(c["refusals"].values()) < 2:
                out.append("fewer than two refusals")
            return out
        for k in kinds:
            out += [f"request {r.kind}/{r.name} never" for r in self.reqs[k] if c["requests"][r] < 1]
            if c["kinds"][k] < 3:
                out.append(f"kind {k} fewer than three times")
        out += [f"pair {p} never adjacent" for p in itertools.product(kinds, kinds) if c["pairs"][p] < 1]
        for p in sharing_pairs():
            if c["pairs"][p] < 3:
                out.append(f"sharing pair {p} fewer than three times")
            if p not in c["long_short"]:
                out.append(f"sharing pair {p}: no long call in front of a short one")
            if p not in c["short_long"]:
                out.append(f"sharing pair {p}: no short call in front of a long one")
        for k in LDS_KINDS:
            out += [f"{k}: never {side} the limit and then on its other side" for side in ("under", "over")
                    if (k, side) not in c["lds"]]
        for r in refusals_of(self.flavour):
            if r not in c["refusal_then_own"]:
                out.append(f"refusal {r.kind}/{r.name}: no good call of its kind behind it")
            if r not in c["refusal_then_other"]:
                out.append(f"refusal {r.kind}/{r.name}: no good call of another kind behind it")
        if not c["refusal_then_release"]:
            out.append("no refusal with a release behind it")
        if c["set_stream"] < 6 or c["release"] < 6:
            out.append(f"set_stream {c['set_stream']}, release {c['release']}: six each")
        out += [f"kind {k} never on the {s} stream" for k in kinds for s in ("own", "torch")
                if (k, s) not in c["on_stream"]]
        if has_tables(self.flavour):
            m = self.model
            for t in TABLES:
                if m.loads[t] < 3:
                    out.append(f"table {t} loaded fewer than three times")
            if not sum(m.returned.values()):
                out.append("no table came back from parking")
            if not sum(m.rebuilt.values()):
                out.append("no table rebuilt after a cache of 0 or 1 threw it away")
            if c["load_between_stages"] < 3:
                out.append("a load between two non-stacking calls fewer than three times")
            if not c["select_expectations_hold"]:
                out.append("a select's expectation does not hold")
        else:
            if c["pushes"] < 8:
                out.append("fewer than eight pushes")
            out += [f"kind {k} never between two pushes" for k in kinds if k not in c["between_pushes"]]
        return out

    def _events(self, req):
        """What issuing ``req`` now would record: (name of the set or counter, item) pairs."""
        p, ev = self.prev, [("requests", req), ("kinds", req.kind), ("on_stream", (req.kind, self.stream))]
        if req.refusal:
            ev.append(("refusals", req))
        if self.c["pushes"]:
            ev.append(("after_last_push", req.kind))
        if p is None:
            return ev
        pair = (p.kind, req.kind)
        ev.append(("pairs", pair))
        if p.kind != req.kind and p.host_in is not False and req.host_in is not False:
            if (p.length, req.length) == ("long", "short"):
                ev.append(("long_short", pair))
            if (p.length, req.length) == ("short", "long"):
                ev.append(("short_long", pair))
        if p.kind == req.kind and p.lds and req.lds and p.lds != req.lds:
            ev.append(("lds", (p.kind, p.lds)))
        if p.refusal and not req.refusal:
            ev.append(("refusal_then_own" if p.kind == req.kind else "refusal_then_other", p))
        return ev

    def gain(self, req):
        """How much of what is still open ``req`` would close if it were issued now."""
        c, score = self.c, 0.0
        share = set(sharing_pairs())
        kinds = list(self.reqs)
        for name, item in self._events(req):
            if name == "requests":
                score += 3.0 if c[name][item] == 0 else 0.0
            elif name == "kinds":
                score += 2.0 if c[name][item] < 3 else 0.0
            elif name == "pairs":
                score += 10.0 if c[name][item] == 0 else 0.0
                if item in share and c[name][item] < 3:
                    score += 6.0
            elif name in ("long_short", "short_long"):
                score += 8.0 if item in share and item not in c[name] else 0.0
            elif name == "lds":
                score += 9.0 if item not in c[name] else 0.0
            elif name == "refusals":
                open_ = (item not in c["refusal_then_own"]) + (item not in c["refusal_then_other"])
                # (a refusal behind a refusal closes nothing of the first one's)
                score += 5.0 * open_ - (20.0 if self.prev is not None and self.prev.refusal else 0.0)
                score -= 4.0 if open_ == 0 else 0.0
            elif name in ("refusal_then_own", "refusal_then_other"):
                score += 12.0 if item not in c[name] else 0.0
            elif name == "on_stream":
                score += 4.0 if item not in c[name] else 0.0
            elif name == "after_last_push":
                score += 2.0 if item not in c["between_pushes"] and item not in c[name] else 0.0
        # ... and a little for what it sets up: its side of an LDS limit with the other side still to follow, a long or
        # a short call in front of a kind it shares a buffer with,
        if req.lds and req.kind in LDS_KINDS and (req.kind, req.lds) not in c["lds"]:
            score += 3.0
        if req.length and req.host_in is not False:
            name = "long_short" if req.length == "long" else "short_long"
            score += 1.5 * any(p[0] == req.kind and p not in c[name] for p in share)
        # for where it leads: pairs that start at its kind and have not occurred
        score += 0.6 * sum(c["pairs"][(req.kind, b)] == 0 for b in kinds)
        score += 0.6 * sum(c["pairs"][(req.kind, b)] < 3 for b in kinds if (req.kind, b) in share)
        return score

    def add(self, op):
        c = self.c
        c["steps"] += 1
        if op.op == "launch":
            req = op.arg
            assert req.table in ("", self.table), (op, self.table)
            c["launches"] += 1
            for name, item in self._events(req):
                if isinstance(c[name], set):
                    c[name].add(item)
                else:
                    c[name][item] += 1
            if self.pending_refusal is not None and self.prev_op == "release":
                c["refusal_then_release"].add(self.pending_refusal)
            self.pending_refusal = req if req.refusal else None
            self.prev = req
        elif op.op == "load":
            before = self.prev
            self.model.load(op.table)
            self.table, self.prev, self.pending_refusal = op.table, None, None
            self._load_after = before if self.prev_op == "launch" else None
        elif op.op == "select":
            c["capacities"][op.arg] += 1
            if self.model.select(op.table, op.arg) != op.expect:
                c["select_expectations_hold"] = False
            self.table = op.table if op.expect else None
            self.prev, self.pending_refusal = None, None
        elif op.op == "set_stream":
            c["set_stream"] += 1
            self.stream = op.arg
        elif op.op == "release":
            c["release"] += 1
        elif op.op == "push":
            c["pushes"] += 1
            c["between_pushes"] |= c["after_last_push"]
            c["after_last_push"] = set()
        else:
            raise AssertionError(op)
        # a load directly between two non-stacking calls
        if op.op == "launch" and self.prev_op == "load" and self._load_after is not None:
            if self._load_after.kind not in STACKING and op.arg.kind not in STACKING:
                c["load_between_stages"] += 1
        self.prev_op = op.op


def coverage(plan, flavour=None):
    """The :class:`Tracker` of a finished plan (from the plan alone: the parking model is run again over its table
    operations).  ``flavour``: which roster the plan is held to (default: read off the plan: one without table
    operations is with_stream's)."""
    if flavour is None:
        flavour = "engine" if any(op.op in ("load", "select") for op in plan) else "with_stream"
    tracker = Tracker(flavour)
    for op in plan:
        tracker.add(op)
    return tracker


def unmet(plan, flavour=None, floor="full"):
    return coverage(plan, flavour).unmet(floor)


# ---------------------------------------------------------------------------------------------- the generator
def make_plan(flavour, seed=None, steps=None):
    """The list of :class:`Op` of one walk, a pure function of its arguments; a shorter plan is a prefix of a longer
    one.  A "select" whose table is not resident is followed by its "load"."""
    seed = SEEDS[flavour] if seed is None else seed
    steps = FLAVOURS[flavour][2] if steps is None else steps
    rng = random.Random(f"stages/{flavour}/{seed}")
    tables = has_tables(flavour)
    tr = Tracker(flavour)
    plan = []

    def emit(op):
        plan.append(op)
        tr.add(op)

    def switch_table(plain_load):
        model = tr.model
        others = [t for t in TABLES if t != model.table]
        if model.table is None or not plain_load:
            # towards a table that has yet to come back from parking or to be rebuilt, else any
            wanted = [t for t in others if t in model.parked() and not model.returned[t]] or \
                     [t for t in others if t in model.lost_small] or others
            target = rng.choice(wanted)
            need_small = not sum(model.rebuilt.values()) and not model.lost_small
            cap = rng.choice((0, 1)) if need_small and rng.random() < 0.5 else rng.choice(CAPACITIES)
            if target in model.parked():
                cap = 4                 # (bring it back: a smaller cache could evict it on the way)
            resident = copy.deepcopy(model).select(target, cap)       # (what the engine will answer)
            emit(Op("select", target, cap, resident))
            if not resident:
                emit(Op("load", target))
        else:
            emit(Op("load", rng.choice(others)))

    def launch(stage_only=False):
        cands = [r for k, reqs in tr.reqs.items() for r in reqs
                 if r.table in ("", tr.table) and not (stage_only and k in STACKING)]
        scored = [(tr.gain(r), r) for r in cands]
        best = max(s for s, _ in scored)
        if best < 1.0:                  # nothing left to steer towards
            req = rng.choice(cands)
        else:
            req = rng.choice([r for s, r in scored if s >= best - 1e-9])
        emit(Op("launch", tr.table if req.table else None, req))

    burst, since_stream, since_release, since_push, stage_next, pushes = 0, 0, 0, PUSH_EVERY - 6, False, 0
    while len(plan) < steps:
        c = tr.c
        if tables and (tr.table is None or burst <= 0):
            # a plain load between two non-stacking calls (on shift_wide: the wide build borrowing sweep.work)
            plain = (tr.table is not None and tr.prev is not None and tr.prev.kind not in STACKING
                     and (c["load_between_stages"] < 3 or rng.random() < 0.3))
            switch_table(plain)
            stage_next = plain
            burst = rng.randint(8, 16)
            continue
        if not tables and since_push >= PUSH_EVERY:
            emit(Op("push", None, pushes))
            pushes, since_push = pushes + 1, 0
            continue
        refused = tr.prev is not None and tr.prev.refusal and tr.prev_op == "launch"
        if refused and (not c["refusal_then_release"] or rng.random() < 0.15):
            emit(Op("release", tr.table))
            since_release = 0
            continue
        if since_stream >= 9 and rng.random() < 0.35:
            emit(Op("set_stream", tr.table, "torch" if tr.stream == "own" else "own"))
            since_stream = 0
            continue
        if since_release >= 12 and rng.random() < 0.2:
            emit(Op("release", tr.table))
            since_release = 0
            continue
        launch(stage_only=stage_next)
        stage_next = False
        burst, since_stream, since_release, since_push = burst - 1, since_stream + 1, since_release + 1, since_push + 1
    return plan[:steps]


# ---------------------------------------------------------------------------------------------- printing
def describe(flavour, plan=None):
    """A short table of what a flavour's plan holds (printed by tests/test_stage_sequence_plan.py -s and by
    ``python tests/stage_sequence_plan.py``)."""
    plan = make_plan(flavour) if plan is None else plan
    tr = coverage(plan, flavour)
    c, kinds = tr.c, list(tr.reqs)
    short = [k[:6] for k in kinds]
    lines = [f"{flavour}: {c['steps']} steps, {c['launches']} launches, {len(c['requests'])} distinct requests of "
             f"{sum(len(r) for r in tr.reqs.values())}, {sum(c['refusals'].values())} refusals, {c['set_stream']} "
             f"set_stream, {c['release']} release, {c['pushes']} push, select capacities {dict(c['capacities'])}",
             "  adjacent pairs (row: first, column: second)",
             "  " + " " * 19 + " ".join(f"{k:>6}" for k in short)]
    for a in kinds:
        lines.append(f"  {a:>19}" + " ".join(f"{c['pairs'][(a, b)]:>6}" for b in kinds))
    lines.append("  sharing pairs, fewest occurrences: "
                 + str(min(c["pairs"][p] for p in sharing_pairs()))
                 + f"; long->short on {len(c['long_short'] & set(sharing_pairs()))}, short->long on "
                 f"{len(c['short_long'] & set(sharing_pairs()))} of {len(sharing_pairs())}")
    lines.append(f"  LDS limit crossed within a kind: {sorted(c['lds'])}")
    lines.append(f"  refusals with a good call of their kind / of another kind / a release behind them: "
                 f"{len(c['refusal_then_own'])} / {len(c['refusal_then_other'])} / {len(c['refusal_then_release'])} "
                 f"of {len(refusals_of(flavour))}")
    if has_tables(flavour):
        m = tr.model
        lines.append("  table: loads / brought back from parking / rebuilt after a cache of 0 or 1 threw it away")
        lines += [f"  {t:>19}: {m.loads[t]} / {m.returned[t]} / {m.rebuilt[t]}" for t in TABLES]
        lines.append(f"  a load directly between two non-stacking calls: {c['load_between_stages']}")
    else:
        lines.append(f"  kinds between two pushes: {len(c['between_pushes'])} of {len(kinds)}")
    lines.append(f"  unmet: {tr.unmet() or 'nothing'}")
    return "\n".join(lines)


def format_ops(ops):
    """One line per operation, for a failure message: the prefix that replays it."""
    out = []
    for i, op in enumerate(ops):
        if op.op == "launch":
            r = op.arg
            out.append(f"{i}: {r.kind}/{r.name}(table={op.table}, size={r.size}, args={tuple(r.args)})")
        elif op.op == "select":
            out.append(f"{i}: select_table({op.table}, capacity={op.arg}) -> resident={op.expect}")
        else:
            out.append(f"{i}: {op.op}({op.table if op.op == 'load' else op.arg})")
    return "\n".join(out)


if __name__ == "__main__":
    for name in FLAVOURS:
        print(describe(name))
