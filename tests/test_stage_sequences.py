# -*- coding: utf-8 -*-
"""
One engine for the life of a process, serving EVERY family of stage call: call sequences against fresh engines.

tests/test_call_sequences.py walks the stacking launches of one long-lived engine.  Each later family of calls --
resampling, pre-processing, onsets, picks, amplitudes, the trigger, the .scanmseed codec, the locate fits, the
travel-time calls -- has a careful test of its own against its NumPy restatement, on an engine that only ever sees that
family.  A production engine serves all of them, in any order, between stacking launches and table changes, out of
scratch that is NOT separate per family (csrc/qm_engine.hpp: the staging bounce buffers, ``d_onsets``, ``fit.*``,
``sweep.work`` are shared on purpose; every buffer grows and never shrinks; refusals return early).  This file holds
those buffers to their contract: a stage call's result depends on the call, never on what ran before it.

* ``test_stage_walk``: a seeded plan (tests/stage_sequence_plan.py; its coverage is checked on the CPU by
  tests/test_stage_sequence_plan.py) drives one long-lived engine of each flavour through seventeen kinds of call, table
  loads and selects, stream changes and pool releases.  Every distinct request is also evaluated ONCE on a fresh engine
  of the flavour, and that result is held to the family's restatement exactly as the family's own GPU test holds it --
  by that test's own check function where it has one (the fresh result is replayed into it), by its bounds imported
  from it otherwise.  Two bounds are written out here because their tests state them inline, with no name to import,
  and they are those tests' own: ``exp2f_max_error`` at most one unit in the last place of a float32 (2^-23,
  tests/test_gpu_parity.py) and at most 2 % of a pick family's rows left out of the fit comparison
  (tests/test_picks_gpu.py).  Only then does it serve as the expectation: at every
  step everything the long-lived engine wrote, into outputs pre-filled with NaN / -1 where the call takes them, must
  have the fresh result's BITS, a refusal its text, and the stage clocks must read without error.
* ``with_stream``: a StreamingDetector with an onset and a resampling stage lives on the engine; raw steps are pushed
  between the calls, and the triples it hands back must be those of the same pushes with nothing in between.
* ``test_stage_walk_with_a_poisoned_pool``: the ``engine`` and ``with_stream`` walks once more, shorter, in a child
  process each with ``QM_HIP_POOL_POISON=1`` (every block the device pool hands out starts as 0xFF bytes).

The walks have found nothing so far; profiles/stage_sequences.txt holds their wall times and where hand mutations of
the shared scratch were caught.
"""

import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT                           # (first: it puts the repository root on sys.path)
import sequence_plan as sp                          # noqa: E402
import stage_sequence_plan as ssp                   # noqa: E402
import test_call_sequences as tcs                   # noqa: E402

pytestmark = pytest.mark.gpu

CLOCK_KEYS = ([f"trigger_ns_{s}" for s in ("smooth", "stats", "runs", "compact", "peaks", "merge")]
              + [f"scanmseed_ns_{s}" for s in ("quantise", "scan", "compose", "pack", "frame", "decode")]
              + [f"tt_ns_{s}" for s in ("homogeneous", "sections", "sweep")])
# what each refusal must say (the families' own refusal tests); "{first}": the first node outside, restated
REFUSALS = {
    ("scanmseed_encode", "difference_of_2_29"): r"channel Y, sample 2500: difference does not fit 30 bits",
    ("scanmseed_decode", "flipped_constant"): r"record 3: STEIM2 reverse integration constant mismatch",
    ("tt_sections", "one_round"): r"section 0: not settled after 1 rounds",
    ("tt_sweep", "node_outside_its_section"): r"row 3: node {first} .* lies outside section 0",
    ("trigger_series", "too_many_events"): r"3 events, the event tables have room for 1 \(max_events\)",
    ("pick_phases", "window_outside_its_row"): r"row 0: window",
    ("pick_phases", "over_the_limit"): r"LDS",
    ("measure_amplitudes", "window_outside_its_trace"): r"window 0: samples",
}


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    assert _lib.qmlib.qm_device_count() >= 1, "no HIP device visible"
    return _lib


def _make(lib, flavour):
    # ("trigger_timing": the trigger's stage clock runs, so that its refusal leaves a clock begun and not collected)
    return lib.Engine(0, trigger_timing=1, **ssp.FLAVOURS[flavour][0])


@functools.lru_cache(maxsize=None)
def _limits(lib):
    """The LDS limits, each read where its family's own test reads it; they are what the roster was sized with."""
    from test_resample_gpu import LDS_SAMPLES

    eng = lib.Engine(0)
    try:
        got = {key: eng.get(key) for key in ssp.LIMIT_KEYS}
    finally:
        eng.close()
    got["resample_lds_samples"] = LDS_SAMPLES
    assert got == ssp.header_limits(), (got, ssp.header_limits())
    return tuple(sorted(got.items()))


# ------------------------------------------------------------------------------------------------ one request
def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _filled(shape, host, dtype=np.float64):
    """An output array nobody has written: NaN (floats) or -1, on the host or on the device."""
    import torch

    fill = np.nan if dtype == np.float64 else -1
    if host:
        return np.full(shape, fill, dtype=dtype)
    return torch.full(tuple(np.atleast_1d(shape)), fill, dtype=torch.float64 if dtype == np.float64 else torch.int32,
                      device="cuda:0")


def _run_stage(lib, eng, req, d):
    """One non-stacking request on ``eng``: a dict name -> array of everything the call wrote (and ``"readouts"``: its
    counts).  Device tensors are the test's own, made on torch's stream and complete before the call; device outputs
    are read after ``eng.synchronize()``."""
    import torch

    out, kind = {}, req.kind
    if kind == "resample":
        a = d["arrays"]
        res = _filled((1, a["t_samples"]), req.host_out)
        raw = d["raw"] if req.host_in else _dev(d["raw"])
        torch.cuda.synchronize()
        eng.resample(raw, a, out=res)
        eng.synchronize()
        out["traces"] = _host(res)
    elif kind == "preprocess":
        x = d["x"] if req.host_in else _dev(d["x"])
        res = _filled(d["x"].shape, req.host_out)
        torch.cuda.synchronize()
        eng.preprocess(x, d["trace_filter"], d["sos"], taper=(d["left"], d["right"]), zero_phase=d["zero_phase"],
                       out=res)
        eng.synchronize()
        out["filtered"] = _host(res)
    elif kind == "onsets":
        x = d["x"] if req.host_in else _dev(d["x"])
        shape = (len(d["nsta"]), d["x"].shape[1])
        raw, logged = _filled(shape, req.host_out), _filled(shape, req.host_out)
        torch.cuda.synchronize()
        eng.onsets(x, d["trace_row"], d["nsta"], d["nlta"], raw_out=raw, log_out=logged, **d["kw"])
        eng.synchronize()
        out["raw"], out["logged"] = _host(raw), _host(logged)
    elif kind == "pick_phases":
        onsets = d["onsets"] if req.host_in else _dev(d["onsets"])
        torch.cuda.synchronize()
        out["picks"], out["status"] = eng.pick_phases(onsets, d["windows"], d["row_group"], d["sampling_rate"],
                                                      d["halfwidth"], threshold_mode=d["mode"],
                                                      thresholds=d.get("thresholds"))
    elif kind == "measure_amplitudes":
        traces = d["packed"] if req.host_in else _dev(d["packed"])
        torch.cuda.synchronize()
        got = eng.measure_amplitudes(traces, d["trecs"], d["recs"], sos=d["sos"], taper_table=d["table"],
                                     taper_weights=d["weights"], detrend_windows=d["detrend"],
                                     want_filtered=d["want_filtered"])
        out["values"], out["index"] = got[:2]
        if d["want_filtered"]:
            out["filtered"] = got[2]
    elif kind == "trigger_series":
        from test_trigger_gpu import PERIOD

        coa, coa_n = (d["coa"], d["coa_n"]) if req.host_in else (_dev(d["coa"]), _dev(d["coa_n"]))
        torch.cuda.synchronize()
        got = eng.trigger_series(coa, coa_n, PERIOD, 1_000_000_000, 2_000_000_000, trigger_on=d["trigger_on"],
                                 method=d["method"], value=d["value"], chunk_samples=d["chunk_samples"],
                                 weights=d["weights"], max_events=d["max_events"], want_candidates=True)
        out["readouts"] = {"n_candidates": got["n_candidates"], "n_events": got["n_events"]}
        out.update({k: got[k] for k in ("events_i", "events_f", "thresholds", "candidates")})
        if got["smoothed"] is not None:
            out["smoothed"] = got["smoothed"]
    elif kind == "scanmseed_encode":
        series = d["series"] if req.host_in else _dev(d["series"])
        out.update(eng.scanmseed_encode(series, d["factors"], d["clips"]))
    elif kind == "scanmseed_decode":
        ints, vals = eng.scanmseed_decode(d["records"], d["samples"], d["offsets"], d["total"], rec_factor=d["factors"],
                                          device=not req.host_out)
        eng.synchronize()
        out["ints"] = _host(ints)
        if vals is not None:
            out["values"] = _host(vals)
    elif kind == "tt_homogeneous":
        got = eng.traveltimes_homogeneous(ssp.TT_LL, ssp.TT_SPACING, ssp.TT_COUNT, d["xyz"], d["vel"],
                                          device=not req.host_out)
        eng.synchronize()
        out["grids"] = _host(got)
    elif kind == "tt_sections":
        got = eng.traveltime_sections(d["slowness"], d["zs"], d["nr"], d["h"], source_slowness=d["s0"],
                                      max_iters=d["max_iters"], force_scratch=d["force_scratch"],
                                      device=not req.host_out)
        eng.synchronize()
        out["T"], out["rounds"], out["status"] = (_host(x) for x in got)
    elif kind == "tt_sweep":
        sections = d["sections"] if req.host_in else _dev(d["sections"])
        torch.cuda.synchronize()
        got = eng.sweep_sections(sections, ssp.TT_LL, ssp.TT_SPACING, ssp.TT_COUNT, d["xy"], d["row_section"],
                                 d["origins"], d["h"], device=not req.host_out)
        eng.synchronize()
        out["grids"] = _host(got)
    elif kind == "locate_fits":
        from test_locate_edges_gpu import FIELDS, ONES

        m = np.array(d["map"])                                          # (a writable copy, for torch)
        norm, smoothed = _filled(m.shape, req.host_out), _filled(m.shape, req.host_out)
        src = m if req.host_in else _dev(m)
        torch.cuda.synchronize()
        got = eng.locate_fits(src, ONES, sgm=d["sgm"], cov_thresh=0.90, norm_out=norm, smoothed_out=smoothed)
        eng.synchronize()
        out.update({k: np.asarray(got[k]) for k in FIELDS})
        out["norm"], out["smoothed"] = _host(norm), _host(smoothed)
        assert np.array_equal(_host(src), m)                            # the input is left alone
    elif kind == "rbf_peak":
        value, index = eng.rbf_peak(d["weights"], d["upscale"])
        out["value"], out["index"] = np.array(value), np.array(index)
    elif kind == "exp_probe":
        if req.name == "exp2f_max_error":
            out["worst"] = np.array(eng.exp2f_max_error(d["lo"], d["hi"]))
        else:
            out["exp"] = eng.exp_correctly_rounded(d["x"])
    else:
        raise AssertionError(f"unknown kind {kind}")
    return out


def _run(lib, eng, req, flavour):
    """One request on ``eng`` (a stacking request's table is resident).  A refusal's result is its text."""
    if req.kind in ssp.STACKING:
        counts = ("screened_steps", "fallback_steps")
        before = [eng.get(k) for k in counts]
        out = tcs._run(lib, eng, req.args)
        # (the increments, not the totals: the long-lived engine has screened before)
        out["readouts"].update({f"{k}_increment": eng.get(k) - b for k, b in zip(counts, before)})
        return out
    d = ssp.build(req, _limits(lib))
    try:
        out = _run_stage(lib, eng, req, d)
    except lib.QMHipError as e:
        assert req.refusal, f"{req.kind}/{req.name} was refused: {e}"
        return {"error": str(e)}
    assert not req.refusal, f"{req.kind}/{req.name} was not refused"
    return out


def _clocks(eng):
    """The stage clocks read without error and are not negative -- after every call, a refused one included."""
    for key in CLOCK_KEYS:
        assert eng.get(key) >= 0, key


# ------------------------------------------------------------------------------------------------ restatements
class _Replay:
    """Stands in for the engine in a family's own check function (``check_onsets``, ``check``,
    ``check_against_reference``, ``test_rbf_peak_past_one_pass``): the call the function makes hands back what the
    fresh engine returned for the same arguments, so the function's own assertions, at its own bounds, are what the
    fresh result is held to."""

    def __init__(self, lib, out):
        self.lib, self.out, self.calls = lib, out, 0

    def onsets(self, signals, trace_row, nsta, nlta, **kw):
        self.calls += 1
        return self.out["raw"], self.out["logged"]

    def trigger_series(self, coa, coa_n, period_ns, mw_ns, mei_ns, **kw):
        self.calls += 1
        assert kw["max_events"] == len(coa) and kw["want_candidates"]       # (what the walk's call passed as well)
        return dict(self.out["readouts"], smoothed=self.out.get("smoothed"),
                    **{k: self.out[k] for k in ("events_i", "events_f", "thresholds", "candidates")})

    def locate_fits(self, m, spacing, sgm=0.8, cov_thresh=0.90, norm_out=None, smoothed_out=None):
        from test_locate_edges_gpu import FIELDS

        self.calls += 1
        norm_out[...] = self.out["norm"]
        smoothed_out[...] = self.out["smoothed"]
        return {k: (self.out[k] if self.out[k].ndim else self.out[k][()]) for k in FIELDS}

    def rbf_peak(self, weights, upscale=10):
        if "value" in self.out:                     # the request itself
            self.calls += 1
            return float(self.out["value"]), tuple(int(v) for v in self.out["index"])
        eng = self.lib.Engine(0)                    # (the spline refinement of the locate check: a call of its own)
        try:
            return eng.rbf_peak(weights, upscale)
        finally:
            eng.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_RESTATED = {}


def _restated(key, compute):
    """A restatement that costs seconds on a CPU, computed once per process and shared by the flavours' walks."""
    if key not in _RESTATED:
        _RESTATED[key] = compute()
    return _RESTATED[key]


def _check_picks(req, d, got):
    import picks_ref as pk
    import test_picks_gpu as tpg

    picks, status = got
    want = pk.pick_rows(d["onsets"], d["windows"], d["row_group"], d["sampling_rate"], d["halfwidth"],
                        **(dict(threshold_mode=1, thresholds_in=d["thresholds"]) if d["mode"] == 1 else {}))
    tpg.assert_discrete(got, want[0], want[1], d.get("names"))
    if req.name == "noise_sets_long":
        empty = np.array([name.startswith("0 ") for name in d["names"]])
        assert np.all(np.isnan(picks[empty, 0])) and np.all(np.isfinite(picks[~empty, 0])) and np.all(status == 1)
        return
    if req.name == "at_the_limit":
        assert np.all(status == 0)
        assert np.max(np.abs(picks[:, 2] - want[0][:, 2])) * d["sampling_rate"] <= tpg.RTOL
        return
    if req.name == "designed_long_dev":
        assert np.array_equal(want[1], d["expected"]), "the restatement itself"
    # the fitted values against the least-squares minimum (tests/test_picks_gpu.py: test_designed_rows)
    import warnings

    tight, default = {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r in np.flatnonzero(status == 0):
            x, y, p0 = pk.fit_inputs(d["onsets"][r], int(picks[r, 5]), int(picks[r, 6]), d["sampling_rate"],
                                     d["halfwidth"][r])
            tight[r], default[r] = pk.scipy_tight(x, y, p0), pk.scipy_default(x, y, p0)
    dist, left_out, _ = tpg.fitted_distances(d, picks, status, tight, default)
    assert dist and max(dist.values()) <= tpg.RTOL, dist
    if req.name == "designed_long_dev":
        assert not left_out
    else:                               # (tests/test_picks_gpu.py's own rule for the family's rows)
        assert len(left_out) <= 0.02 * len(status)


def _check_amplitudes(req, d, out):
    import amplitudes_ref as ar
    import preprocess_ref as pp
    import test_amplitudes_gpu as tag

    values, index = out["values"], out["index"]
    recs = np.array(d["recs"])
    if d["check"] == "window_detrend":
        assert np.all(index[:, 0] == 0)
        x = d["packed"]
        for k, (_, lo, hi, _) in enumerate(recs):
            y = pp.detrend_device_order(x[lo:hi], False)
            want = [0.0, np.sqrt(pp.wave_sum(y * y) / float(hi - lo)), np.max(np.abs(y)), 0.0]
            assert np.array_equal(_bits(values[k]), _bits(want)), (hi - lo, values[k], want)
        return
    traces, trecs = d["traces"], d["trecs"]
    if d["check"] == "filter":
        want = []
        for x, (_, n, f, taper) in zip(traces, trecs):
            y = pp.detrend_device_order(x, False)
            if taper >= 0:
                o, m = d["table"][taper]
                y = pp.taper(y, d["weights"][o:o + m], d["weights"][o + m:o + 2 * m])
            want.append(pp.sosfilt(d["sos"][f], y))
        assert np.array_equal(_bits(out["filtered"]), _bits(np.concatenate(want)))
        # the windows, cut from the traces as the device filtered them (test_filter_stage)
        traces = [out["filtered"][off:off + n] for off, n, _, _ in trecs]
        trecs = np.array(trecs)
        trecs[:, 2:] = -1
    want_v, want_i, _ = ar.measure(traces, trecs, d["recs"], detrend=False)
    assert np.array_equal(index, want_i), (index, want_i)
    if d["check"] == "bits":
        assert np.array_equal(_bits(values), _bits(want_v))
        return
    assert np.array_equal(_bits(values[:, 0]), _bits(want_v[:, 0]))
    assert np.array_equal(_bits(values[:, 2]), _bits(want_v[:, 2])) and np.all(values[:, 3] == 0.0)
    tag.check_averages(values[:, 1], want_v[:, 1], tag.window_lengths(recs), "RMS", want_v[:, 2],
                       f"{req.kind}/{req.name}")


def _check_against_restatement(lib, oracle, flavour, req, out):
    """The fresh engine's result of a request against the family's restatement, as the family's own GPU test holds
    it: equal bits where that test demands bits, its own bound (its check function, or a constant imported from it)
    otherwise.  A refusal: the family's documented text."""
    what = f"fresh {flavour} engine, {req.kind}/{req.name}"
    if req.kind in ssp.STACKING:
        tcs._check_against_oracle(oracle, "screen" if flavour == "screen" else "engine", req.args, out)
        return
    d = ssp.build(req, _limits(lib))
    if req.refusal:
        import re

        pattern = REFUSALS[req.kind, req.name]
        if "{first}" in pattern:
            import traveltimes_ref as tr

            dist, depth = tr.distances_depths(ssp.TT_LL, ssp.TT_SPACING, ssp.TT_COUNT, d["xy"][3])
            first = tr.outside(dist, depth, d["origins"][3, 0], d["origins"][3, 1], d["h"], d["nr"], d["nz"])[0]
            pattern = pattern.format(first=first)
        assert set(out) == {"error"} and re.search(pattern, out["error"]), f"{what}: {out} does not say {pattern!r}"
        return
    for name, x in out.items():                     # nothing the call should have written is still as pre-filled
        if name != "readouts" and req.kind in ("resample", "preprocess", "onsets"):
            assert not np.isnan(x).any(), f"{what}: {name} holds elements nobody wrote"
    kind = req.kind
    if kind == "resample":
        import resample_ref as rr
        from test_resample_gpu import _want

        if d["bits"] == "upsample":
            want = _want(d["raw"], d["arrays"])
        else:
            m, w = d["m"], d["weights"]
            want = _restated(req, lambda: rr.lowpassed(d["raw"], d["sos"][1], w[:m], w[m:],
                                                       device_order=True)[None, ::2])
        assert out["traces"].shape == want.shape and np.array_equal(out["traces"], want), what
    elif kind == "preprocess":
        import preprocess_ref as pr

        want = pr.preprocess(d["x"], d["trace_filter"], d["sos"], d["left"], d["right"], zero_phase=d["zero_phase"],
                             device_order=True)
        assert np.array_equal(out["filtered"], want), (what, float(np.max(np.abs(out["filtered"] - want))))
    elif kind == "onsets":
        from test_stage_edges_gpu import check_onsets

        replay = _Replay(lib, out)
        check_onsets(replay, d["x"], d["trace_row"], d["nsta"], d["nlta"], **d["kw"])
        assert replay.calls == 1
    elif kind == "pick_phases":
        _check_picks(req, d, (out["picks"], out["status"]))
    elif kind == "measure_amplitudes":
        _check_amplitudes(req, d, out)
    elif kind == "trigger_series":
        from test_trigger_gpu import check

        replay = _Replay(lib, out)
        check(replay, d["coa"], d["coa_n"], trigger_on=d["trigger_on"], method=d["method"], value=d["value"],
              chunk_samples=d["chunk_samples"], weights=d["weights"])
        assert replay.calls == 1 and out["readouts"]["n_events"] >= 3
    elif kind == "scanmseed_encode":
        from quakemigrate_amd import scanmseed as sm
        from test_scanmseed_codec_gpu import T0

        series = d["quantised"] if d["factors"] is not None else {ch: d["series"][j] for j, ch in enumerate(sm.CHANNELS)}
        # (a copy: fill_headers writes into the records it is given, and the fresh result stays as the engine left it)
        assert not out["records"][:, :sm.DATA_OFFSET].any(), f"{what}: the 64 header bytes are not zero"
        got = sm.fill_headers(out["records"].copy(), out["n_records"], out["rec_first"], out["rec_count"], T0, 50.0)
        assert got == sm.encode_scanmseed(T0, 50.0, series), what
    elif kind == "scanmseed_decode":
        assert out["ints"].dtype == np.int32 and np.array_equal(out["ints"], d["ints"]), what
        assert ("values" in out) == (d["factors"] is not None)
        if "values" in out:                         # the Python codec's descaling: sample / factor
            want = d["ints"] / np.repeat(d["factors"], d["samples"])
            assert np.array_equal(_bits(out["values"]), _bits(want)), what
    elif kind == "tt_homogeneous":
        import traveltimes_ref as tr

        for r in range(len(d["vel"])):
            want = tr.homogeneous(ssp.TT_LL, ssp.TT_SPACING, ssp.TT_COUNT, d["xyz"][r], d["vel"][r])
            assert np.array_equal(_bits(out["grids"][r]), _bits(want)), (what, r)
    elif kind == "tt_sections":
        import traveltimes_ref as tr

        T, rounds, status = _restated(("tt_sections", d["nr"], d["nz"], len(d["zs"])),
                                      lambda: tr.solve_sections(d["slowness"], d["zs"], d["s0"], d["nr"], d["h"]))
        assert np.array_equal(out["status"], status) and not status.any(), what
        assert np.array_equal(out["rounds"], rounds), what
        assert np.array_equal(_bits(out["T"]), _bits(T)), what
    elif kind == "tt_sweep":
        import traveltimes_ref as tr

        for r in range(len(d["xy"])):
            want = tr.sweep(ssp.TT_LL, ssp.TT_SPACING, ssp.TT_COUNT, d["xy"][r], d["sections"][d["row_section"][r]],
                            d["origins"][r][0], d["origins"][r][1], d["h"])
            assert np.array_equal(_bits(out["grids"][r]), _bits(want)), (what, r)
    elif kind == "locate_fits":
        from test_locate_edges_gpu import check_against_reference

        replay = _Replay(lib, out)
        check_against_reference(replay, d["name"], d["sgm"])
        assert replay.calls == 1
    elif kind == "rbf_peak":
        from test_locate_edges_gpu import test_rbf_peak_past_one_pass

        replay = _Replay(lib, out)
        test_rbf_peak_past_one_pass(replay, d["case"])
        assert replay.calls == 1
    elif kind == "exp_probe":
        if req.name == "exp2f_max_error":
            # (tests/test_gpu_parity.py's bound for v_exp_f32: one unit in the last place of a float32)
            assert 0.0 <= float(out["worst"]) <= float(np.finfo(np.float32).eps), out["worst"]
        else:
            want = np.array([lib.qmlib.qm_exp_correctly_rounded(float(v)) for v in d["x"]])
            assert np.array_equal(out["exp"], want, equal_nan=True), what
    else:
        raise AssertionError(kind)


def _same(req, got, fresh, what):
    """Bit equality of everything a call wrote, of its counts, or of its refusal's text."""
    if req.kind in ssp.STACKING:
        tcs._same(got, fresh, what)
        return
    assert set(got) == set(fresh), f"{what}: wrote {sorted(got)}, the fresh engine {sorted(fresh)}"
    for name in got:
        if name in ("readouts", "error"):
            assert got[name] == fresh[name], f"{what}: {name} {got[name]!r} on the long-lived engine, " \
                                             f"{fresh[name]!r} on a fresh one"
            continue
        x, y = np.asarray(got[name]), np.asarray(fresh[name])
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {name} {x.shape} {x.dtype}, fresh {y.shape} {y.dtype}"
        if x.tobytes() != y.tobytes():  # (bytes: a NaN equals a NaN of the same payload, +0.0 is not -0.0)
            as_bytes = lambda a: np.frombuffer(a.tobytes(), np.uint8).reshape(a.size, a.dtype.itemsize)  # noqa: E731
            bad = np.flatnonzero((as_bytes(x) != as_bytes(y)).any(axis=1))
            raise AssertionError(f"{what}: {name} differs from the fresh engine's in {bad.size} of {x.size} elements "
                                 f"(first at {bad[:6]}: {x.reshape(-1)[bad[:3]]} for {y.reshape(-1)[bad[:3]]})")


# ------------------------------------------------------------------------------------------------ the stream
def _stream(lib, eng):
    from quakemigrate_amd.stream import StreamingDetector

    s = ssp.stream_setup()
    return StreamingDetector(eng, s["rows"], s["T"], s["fsmp"], s["lsmp"], s["rows"], depth=2, steps_per_launch=2,
                             onset_stage=s["onset"], sampling_rate=ssp.STREAM_RATE, resample_stage=s["resample"])


def _push(det, raw, triples):
    """One raw step into the stream; what it hands back meanwhile goes to ``triples``, in push order."""
    while not det.push_raw(raw):
        _take(det, min(det.k, det.pending()[0]), triples)


def _take(det, n, triples):
    a, b, c = det.pop(n)
    triples += [(a[j], b[j], c[j]) for j in range(n)]


def _drain(det, triples):
    det.flush()
    left = det.pending()[0]
    while left > 0:
        n = min(det.k, left)
        _take(det, n, triples)
        left -= n


_UNDISTURBED = {}


def _undisturbed(lib, n_pushes):
    """The triples of ``n_pushes`` pushes on a fresh engine and stream with no other call in between, computed once."""
    if n_pushes not in _UNDISTURBED:
        raws = ssp.stream_setup()["raws"]
        eng = _make(lib, "with_stream")
        try:
            eng.load_lut(sp.table_case(ssp.STREAM_TABLE)[0])
            det = _stream(lib, eng)
            triples = []
            for k in range(n_pushes):
                _push(det, raws[k % ssp.PUSH_STEPS], triples)
            _drain(det, triples)
            det.close()
        finally:
            eng.close()
        assert len(triples) == n_pushes and np.ptp(triples[0][0]) > 0
        _UNDISTURBED[n_pushes] = triples
    return _UNDISTURBED[n_pushes]


# ------------------------------------------------------------------------------------------------ the walk
_FRESH = {}                             # (flavour's configuration, request) -> the fresh result, held to its restatement
_SPENT = {"fresh": 0.0, "restatements": 0.0}    # seconds on fresh engines / in the CPU restatements, this process


def run_stage_walk(lib, oracle, flavour, seed=None, steps=None, plan=None):
    seed = ssp.SEEDS[flavour] if seed is None else seed
    plan = ssp.make_plan(flavour, seed, steps) if plan is None else plan
    import torch

    side = torch.cuda.Stream()
    config = tuple(sorted(ssp.FLAVOURS[flavour][0].items()))
    used = set()

    def fresh(req):
        key = (config, req)
        if key not in _FRESH:
            t0 = time.time()
            e2 = _make(lib, flavour)
            try:
                if req.table:
                    e2.load_lut(sp.table_case(req.table)[0])
                out = _run(lib, e2, req, flavour)
                _clocks(e2)
            finally:
                e2.close()
            t1 = time.time()
            # only a result that was held to its restatement may serve as an expectation
            _check_against_restatement(lib, oracle, flavour, req, out)
            _FRESH[key] = out
            _SPENT["fresh"] += t1 - t0
            _SPENT["restatements"] += time.time() - t1
        used.add(req)
        return _FRESH[key]

    eng = _make(lib, flavour)
    det, triples, pushes, came_back = None, [], 0, 0
    try:
        if not ssp.has_tables(flavour):
            eng.load_lut(sp.table_case(ssp.STREAM_TABLE)[0])
            det = _stream(lib, eng)
        for i, op in enumerate(plan):
            try:
                if op.op == "load":
                    eng.load_lut(sp.table_case(op.table)[0])
                elif op.op == "select":
                    resident = eng.select_table(op.table, capacity=op.arg)
                    assert resident == op.expect, f"select_table says resident={resident}, the model {op.expect}"
                    came_back += bool(resident)
                elif op.op == "set_stream":
                    eng.synchronize()
                    eng.set_stream(side.cuda_stream if op.arg == "torch" else None)
                elif op.op == "release":
                    lib.release_cached_memory()
                elif op.op == "push":
                    _push(det, ssp.stream_setup()["raws"][op.arg % ssp.PUSH_STEPS], triples)
                    pushes += 1
                else:
                    want = fresh(op.arg)
                    got = _run(lib, eng, op.arg, flavour)
                    _clocks(eng)
                    _same(op.arg, got, want, f"{op.arg.kind}/{op.arg.name}")
            except Exception as e:
                raise AssertionError(f"flavour {flavour}, seed {seed}, step {i} of {len(plan)}: {e}\n"
                                     f"operations up to it:\n{ssp.format_ops(plan[:i + 1])}") from e
        if det is not None:
            _drain(det, triples)
            want = _undisturbed(lib, pushes)
            assert len(triples) == pushes == len(want)
            for k, (g, w) in enumerate(zip(triples, want)):
                for name, gs, ws in zip(("max_coa", "max_norm_coa", "max_coa_idx"), g, w):
                    assert gs.tobytes() == ws.tobytes(), \
                        f"flavour {flavour}, seed {seed}: push {k}'s {name} differs from the undisturbed stream's"
    finally:
        if det is not None:
            det.close()
        eng.close()
    hits = sum(1 for op in plan if op.op == "select" and op.expect)
    assert came_back == hits
    return len(plan), len(used)


@pytest.mark.parametrize("flavour", list(ssp.FLAVOURS))
def test_stage_walk(lib, oracle, flavour):
    """A long-lived engine's stage calls equal a fresh engine's, bit for bit, at every step of the flavour's plan."""
    t0, before = time.time(), dict(_SPENT)
    steps, requests = run_stage_walk(lib, oracle, flavour)
    print(f"\nstage walk {flavour}: {steps} steps, {requests} distinct requests, {time.time() - t0:.1f} s "
          f"({_SPENT['fresh'] - before['fresh']:.1f} s of it on fresh engines, "
          f"{_SPENT['restatements'] - before['restatements']:.1f} s in the CPU restatements)")


def test_stage_walk_with_a_poisoned_pool(lib):
    """The engine and with_stream walks once more, shorter, with QM_HIP_POOL_POISON=1 (read once per process: a child
    each, one at a time, under a time limit; the second only if the first passed)."""
    env = dict(os.environ, QM_HIP_POOL_POISON="1")
    for flavour in ssp.POISON_FLAVOURS:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), flavour, str(ssp.POISON_STEPS)], env=env,
                              cwd=str(ROOT), timeout=600, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert done.returncode == 0, f"poisoned-pool stage walk {flavour}: exit {done.returncode}\n{done.stdout[-6000:]}"
        assert f"stage walk {flavour} ok" in done.stdout, done.stdout[-2000:]


if __name__ == "__main__":              # the poisoned-pool child: one walk, exit status 0 only if it held
    from quakemigrate_amd.core import lib as _lib
    from oracle import qm_oracle as _oracle

    _flavour, _steps = sys.argv[1], int(sys.argv[2])
    assert os.environ.get("QM_HIP_POOL_POISON") == "1"
    _n, _m = run_stage_walk(_lib, _oracle, _flavour, steps=_steps)
    print(f"stage walk {_flavour} ok: {_n} steps, {_m} distinct requests")
