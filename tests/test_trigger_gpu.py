# -*- coding: utf-8 -*-
"""
The trigger stage on the GPU (include/qmhip.h: qm_engine_trigger; kernels: csrc/qm_trigger.hpp) against its NumPy
restatement (tests/trigger_ref.py, pinned to SciPy, NumPy, pandas and the reference's recorded events by
tests/test_trigger_host.py).  Every integer is equal and every float has the same bits: the values this stage puts out
are copied samples, sums in SciPy's order and medians in NumPy's -- there is no tolerance anywhere.  (One exception to
"bits": where a threshold is zero its sign is left open -- np.median's pick among equal zeros of either sign depends on
its partition, and no comparison `trig >= threshold` can tell them apart.)
"""

import ctypes
import datetime as dt
import importlib.util

import numpy as np
import pytest

import trigger_ref as tr
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

PERIOD = 20_000_000             # 50 Hz
METHODS = {"static": tr.STATIC, "mad": tr.MAD, "median_ratio": tr.MEDIAN_RATIO}


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    if _lib.qmlib.qm_device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


@pytest.fixture(scope="module")
def engine(lib):
    eng = lib.Engine(0)
    yield eng
    eng.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def restate(coa, coa_n=None, period_ns=PERIOD, mw_ns=1_000_000_000, mei_ns=2_000_000_000, trigger_on=0,
            method="static", value=1.0, chunk_samples=1, weights=None):
    """trigger_ref's answer to check()'s arguments."""
    return tr.trigger_series(coa, coa if coa_n is None else coa_n, trigger_on, weights, METHODS[method], value,
                             chunk_samples, period_ns, mw_ns, mei_ns)


def check(eng, coa, coa_n=None, period_ns=PERIOD, mw_ns=1_000_000_000, mei_ns=2_000_000_000, trigger_on=0,
          method="static", value=1.0, chunk_samples=1, weights=None, want=None):
    """One call on the engine and on the restatement (`want`: its answer to these arguments, where the caller has it
    already); everything equal.  Returns the engine's answer."""
    coa = np.ascontiguousarray(coa, dtype=np.float64)
    coa_n = coa.copy() if coa_n is None else np.ascontiguousarray(coa_n, dtype=np.float64)
    got = eng.trigger_series(coa, coa_n, period_ns, mw_ns, mei_ns, trigger_on=trigger_on, method=method, value=value,
                             chunk_samples=chunk_samples, weights=weights, max_events=len(coa), want_candidates=True)
    if want is None:
        want = restate(coa, coa_n, period_ns, mw_ns, mei_ns, trigger_on, method, value, chunk_samples, weights)
    assert (got["n_candidates"], got["n_events"]) == (want["n_candidates"], want["n_events"])
    assert np.array_equal(got["candidates"], want["candidates"])
    assert np.array_equal(got["events_i"], want["events_i"])
    assert np.array_equal(bits(got["events_f"]), bits(want["events_f"]))
    assert np.array_equal(got["thresholds"], want["thresholds"])
    nonzero = want["thresholds"] != 0
    assert np.array_equal(bits(got["thresholds"])[nonzero], bits(want["thresholds"])[nonzero])
    if weights is not None:
        assert np.array_equal(bits(got["smoothed"]), bits(want["smoothed"]))
    return got


# -- the reference's recorded events ----------------------------------------------------------------------------------
BENCHMARKS = {
    "icequake": dict(scan="icequake_iceland_2014_180.scanmseed", csv="icequake_iceland_2014_180_TriggeredEvents.csv",
                     mw=0.06, mei=0.12, threshold=2.15, start=dt.datetime(2014, 6, 29, 18, 42, 5),
                     end=dt.datetime(2014, 6, 29, 18, 42, 15), region=None, counts=(9, 3, 3)),
    "volcanotectonic": dict(scan="volcanotectonic_iceland_2014_236.scanmseed",
                            csv="volcanotectonic_iceland_2014_236_TriggeredEvents.csv", mw=0.75, mei=1.5,
                            threshold=1.85, start=dt.datetime(2014, 8, 24, 0, 1, 0),
                            end=dt.datetime(2014, 8, 24, 0, 11, 0),
                            region=[-17.15, 64.72, 0.0, -16.65, 64.93, 14.0], counts=(54, 29, 28)),
}


@pytest.mark.parametrize("name", sorted(BENCHMARKS))
def test_benchmark_fixture_gives_the_references_events(engine, name):
    from quakemigrate_amd import scanmseed, trigger

    b = BENCHMARKS[name]
    t0, rate, cols = scanmseed.read_scanmseed(GOLDEN / b["scan"], 1000)
    t = trigger.DeviceTrigger(marginal_window=b["mw"], min_event_interval=b["mei"], normalise_coalescence=True,
                              static_threshold=b["threshold"])
    events = t.trigger_series(engine, t0, rate, cols, b["start"], b["end"], region=b["region"], want_candidates=True)
    assert (t.last["n_candidates"], t.last["n_events"], len(events)) == b["counts"]
    recorded = trigger.read_triggered_events(GOLDEN / b["csv"])
    assert [e["EventID"] for e in events] == [e["EventID"] for e in recorded]
    for got, want in zip(events, recorded):
        for col in trigger.OUTPUT_COLS[1:]:
            assert got[col] == want[col], (got["EventID"], col)
    i0, i1 = t.last["first_sample"], t.last["last_sample"] + 1
    period_ns = int(round(1e9 / rate))
    want = tr.trigger_series(cols["COA"][i0:i1], cols["COA_N"][i0:i1], 1, None, tr.STATIC, b["threshold"], 1, period_ns,
                             int(round(b["mw"] * 1e9)), int(round(b["mei"] * 1e9)))
    assert np.array_equal(t.last["candidates"], want["candidates"])
    assert np.array_equal(t.last["events_i"], want["events_i"])


# -- smoothing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 20, "cap"])
def test_smoothing_has_scipys_bits(engine, radius):
    from scipy.ndimage import gaussian_filter1d

    tile = engine.get("trigger_smooth_tile")
    r = engine.get("trigger_max_radius") if radius == "cap" else radius
    sd = r / 4.0                                            # int(4 sd + 0.5) = r
    r_w, w = tr.gaussian_weights(sd, 4.0)
    assert r_w == r and len(w) == 2 * r + 1
    rng = np.random.default_rng(r)
    for n in sorted({1, 2, r, r + 1, 2 * r + 1, tile - 1, tile, tile + 1, 3 * tile + 5}):
        x = np.round(rng.gamma(2.0, 1.0, (2, n)), 5)
        got = engine.trigger_series(x[0].copy(), x[1].copy(), PERIOD, 10 ** 9, 2 * 10 ** 9, value=1e9, weights=w)
        for k in range(2):
            assert np.array_equal(bits(got["smoothed"][k]), bits(gaussian_filter1d(x[k], sd, truncate=4.0))), (n, k)
        assert got["n_candidates"] == 0


def test_smoothed_series_feed_threshold_peak_and_values(engine):
    rng = np.random.default_rng(5)
    x = np.round(rng.gamma(2.0, 1.0, (2, 5000)), 5)
    _, w = tr.gaussian_weights(2.5, 4.0)
    for on in (0, 1):
        got = check(engine, x[0], x[1], trigger_on=on, method="mad", value=2.0, chunk_samples=1000, weights=w)
        assert got["n_events"] > 3


# -- thresholds ---------------------------------------------------------------------------------------------------------
def chunk_data(kind, n, rng):
    if kind == "equal":
        return np.full(n, 1.23457)
    if kind == "duplicated":                                # half of the values are one value
        x = np.round(rng.normal(2.0, 1.0, n), 5)
        x[rng.permutation(n)[:n // 2]] = 2.0
        return x
    if kind == "signed":                                    # negative values, +0.0 and -0.0
        x = np.round(rng.normal(0.0, 1.0, n), 1)
        x[rng.permutation(n)[:n // 3]] = 0.0
        x[rng.permutation(n)[:n // 3]] = -0.0
        return x
    if kind == "last_bit":                                  # neighbours in the last mantissa bit
        return (bits(np.full(n, 1.5)) + rng.integers(0, 4, n).astype(np.uint64)).view(np.float64)
    if kind == "between":                                   # the median of an even chunk falls between two values
        return np.where(np.arange(n) % 2 == 0, 1.0, 3.0) + 0.0
    return np.round(rng.gamma(2.0, 1.0, n), 5)             # "quantised": what .scanmseed holds


KINDS = ("quantised", "equal", "duplicated", "signed", "last_bit", "between")


@pytest.mark.parametrize("chunk", [1, 2, 3, 64, 65, 8192, 8193, 180_000])
def test_thresholds_have_numpys_bits(engine, chunk):
    """Lengths with a last chunk of 1 and of W - 1 samples, and n < W; 8192 / 8193: the statistics kernel changes its
    workgroup size there; 180 000: an hour at 50 Hz, re-read from L2 on every radix pass."""
    rng = np.random.default_rng(chunk)
    repeats = 3 if chunk < 1000 else 1
    lengths = sorted({repeats * chunk + 1, (repeats + 1) * chunk - 1, max(chunk - 1, 1), chunk})
    for n in lengths:
        for kind in KINDS:
            x = chunk_data(kind, n, rng)
            for method, value in (("mad", 8.0), ("median_ratio", 1.2), ("static", 1.5)):
                got = check(engine, x, method=method, value=value, chunk_samples=chunk)
                assert len(got["thresholds"]) == (1 if method == "static" else -(-n // chunk))


# -- runs ---------------------------------------------------------------------------------------------------------------
def test_designed_runs(engine):
    block = engine.get("trigger_run_block")
    n = 3 * block + 17
    quiet = np.zeros(n)
    assert check(engine, quiet)["n_candidates"] == 0                          # none above
    whole = check(engine, np.full(300_000, 2.0))                                # all above: one run of n
    assert whole["n_candidates"] == 1 and tuple(whole["candidates"][0, :3]) == (0, 299_999, 0)
    x = quiet.copy()                                                            # runs touching both ends, single samples
    x[:3], x[n - 2:], x[100], x[102] = 2.0, 2.0, 3.0, 3.0
    got = check(engine, x)
    assert [tuple(c[:2]) for c in got["candidates"]] == [(0, 2), (100, 100), (102, 102), (n - 2, n - 1)]
    x = np.zeros(20_001)                                                        # alternating: 10 001 candidates
    x[::2] = 2.0
    assert check(engine, x, mw_ns=PERIOD // 2, mei_ns=PERIOD)["n_candidates"] == 10_001
    # runs that start, end and peak at workgroup boundaries +- 1
    for edge in (block, 2 * block):
        for d in (-1, 0, 1):
            x = quiet.copy()
            x[edge + d - 40:edge + d] = 2.0                                     # ends at edge + d - 1
            x[edge + d + 5:edge + d + 45] = 2.0                                 # starts at edge + d + 5
            x[edge + d - 1], x[edge + d + 5] = 5.0, 4.0
            got = check(engine, x)
            assert [tuple(c[:3]) for c in got["candidates"]] == [
                (edge + d - 40, edge + d - 1, edge + d - 1), (edge + d + 5, edge + d + 44, edge + d + 5)]
            x = quiet.copy()
            x[edge - 70:edge + 70] = 2.0                                        # a run across the boundary, peak beside it
            x[edge + d] = 3.0
            assert tuple(check(engine, x)["candidates"][0, :3]) == (edge - 70, edge + 69, edge + d)


def test_equal_maxima_keep_the_lowest_index(engine):
    x = np.zeros(1000)
    x[100:400] = 2.0
    for first, second in ((110, 111), (110, 174), (163, 164), (100 + 63, 100 + 64), (130, 399)):
        y = x.copy()
        y[first] = y[second] = 7.0
        assert check(engine, y)["candidates"][0, 2] == first
    assert check(engine, x)["candidates"][0, 2] == 100                          # all equal: the run's first sample


def test_peak_is_taken_on_coa_values_on_the_trigger_series(engine):
    coa, coa_n = np.zeros(500), np.zeros(500)
    coa_n[100:200], coa[100:200] = 2.0, 0.5
    coa_n[120], coa[170] = 9.0, 0.9                                             # COA_N peaks at 120, COA at 170
    got = check(engine, coa, coa_n, trigger_on=1)
    assert got["candidates"][0, 2] == 170
    assert tuple(got["events_f"][0]) == (2.0, 0.9, 2.0)                         # TRIG_COA = COA_N[p], COA, COA_NORM


# -- MinTime / MaxTime ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mw_ns", [1_000_000_000, 990_000_000])                # 50 samples; 49.5 samples
def test_min_and_max_time_rule(engine, mw_ns):
    mei_ns, gap = 3_000_000_000, 3_000_000_000 - mw_ns
    mw = -(-mw_ns // PERIOD)                                                    # samples from which t >= mw
    x, at, expect = np.zeros(40_000), 500, []
    for before in (mw - 1, mw, mw + 1):
        for after in (mw - 1, mw, mw + 1):
            x[at - before:at + after + 1] = 2.0
            x[at] = 3.0
            t_min = at * PERIOD - mei_ns if before * PERIOD < mw_ns else (at - before) * PERIOD - gap
            t_max = at * PERIOD + mei_ns if after * PERIOD < mw_ns else (at + after) * PERIOD + gap
            expect.append((at - before, at + after, at, t_min, t_max))
            at += 2000
    got = check(engine, x, mw_ns=mw_ns, mei_ns=mei_ns)
    assert [tuple(c) for c in got["candidates"]] == expect
    assert got["n_events"] == 9


# -- merge --------------------------------------------------------------------------------------------------------------
def spikes(n, at, values=None):
    x = np.zeros(n)
    x[np.asarray(at)] = 2.0 if values is None else values
    return x


def test_merge_chains(engine):
    stride = engine.get("trigger_merge_stride")
    # single samples: MinTime / MaxTime = t -+ 2 s, separate iff more than 3 s = 150 samples apart (both conditions)
    got = check(engine, spikes(1000, [500]))
    assert got["n_events"] == 1 and got["events_i"][0, 3] == 1
    got = check(engine, spikes(1000, [500, 650]))                               # at equality: merged (strict <, >)
    assert got["n_events"] == 1 and got["events_i"][0, 3] == 2
    assert check(engine, spikes(1000, [500, 651]))["n_events"] == 2
    chain = 100 + 50 * np.arange(300)                                           # 300 candidates 1 s apart: one event
    got = check(engine, spikes(20_000, chain))
    assert got["n_events"] == 1 and tuple(got["events_i"][0]) == (100, 100 * PERIOD - 2 * 10 ** 9,
                                                                 chain[-1] * PERIOD + 2 * 10 ** 9, 300)
    # separate events up to the merge loop's stride, a chain of 20 across it, separate events behind it
    at = list(200 * np.arange(stride - 10))
    at += [at[-1] + 200 + 50 * k for k in range(20)]
    at += [at[-1] + 200 * (k + 1) for k in range(stride)]
    values = 2.0 + (np.arange(len(at)) % 7) * 0.25
    got = check(engine, spikes(at[-1] + 10, at, values))
    assert got["n_candidates"] == len(at) and got["n_events"] == len(at) - 19
    assert got["events_i"][stride - 10, 3] == 20


def test_merge_conditions_one_at_a_time(engine):
    # A: a 5-s run peaking at its first sample (MaxTime = t(l) + 1 s), B: a single sample 1.5 s behind A's end --
    # MaxTime[A] < t(B) - mw fails alone
    x = np.zeros(2000)
    x[500:751], x[500], x[750 + 75] = 2.0, 3.0, 2.5
    got = check(engine, x)
    a, b = got["candidates"]
    assert not a[4] < b[2] * PERIOD - 10 ** 9 and b[3] > a[2] * PERIOD + 10 ** 9 and got["n_events"] == 1
    # A: a single sample, B: a 5-s run peaking at its last sample (MinTime = t(f) - 1 s) starting 1.5 s behind A --
    # MinTime[B] > t(A) + mw fails alone
    x = np.zeros(2000)
    x[500], x[575:826], x[825] = 2.5, 2.0, 3.0
    got = check(engine, x)
    a, b = got["candidates"]
    assert a[4] < b[2] * PERIOD - 10 ** 9 and not b[3] > a[2] * PERIOD + 10 ** 9 and got["n_events"] == 1
    # each condition at equality and one sample beyond it
    for lag, events in ((100, 1), (101, 2)):                                    # t(l) + 1 s < t(B) - 1 s
        x = np.zeros(2000)
        x[500:751], x[500], x[750 + lag] = 2.0, 3.0, 2.5
        assert check(engine, x)["n_events"] == events
    for lag, events in ((100, 1), (101, 2)):                                    # t(f) - 1 s > t(A) + 1 s
        x = np.zeros(2000)
        x[500], x[500 + lag:500 + lag + 251], x[500 + lag + 250] = 2.5, 2.0, 3.0
        assert check(engine, x)["n_events"] == events


def test_equal_trigger_values_keep_the_first_member(engine):
    coa, coa_n = spikes(3000, [500, 550, 600, 650], [1.0, 2.0, 3.0, 4.0]), spikes(3000, [500, 550, 600, 650])
    got = check(engine, coa, coa_n, trigger_on=1, value=2.0)
    assert got["n_events"] == 1 and got["events_i"][0, 0] == 500 and tuple(got["events_f"][0]) == (2.0, 1.0, 2.0)
    coa_n[600] = 2.5
    assert check(engine, coa, coa_n, trigger_on=1, value=2.0)["events_i"][0, 0] == 600


# -- seeded differential ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_seeded_parameter_sets_equal_the_restatement(engine, seed):
    rng = np.random.default_rng(1000 + seed)
    events = 0
    for _ in range(50):
        n = int(rng.integers(2000, 50_001))
        noise = rng.gamma(2.0, 0.5, (2, n))
        for at in rng.integers(0, n, int(rng.integers(0, 40))):               # bursts of random width and height
            width = int(rng.integers(1, 200))
            shape = rng.uniform(2.0, 8.0) * np.hanning(width + 2)[1:-1]
            stop = min(n, at + width)
            noise[:, at:stop] += shape[:stop - at] * rng.uniform(0.5, 1.5, (2, 1))
        x = np.round(noise, 5)
        period_ns = int(rng.choice([4_000_000, 10_000_000, 20_000_000]))
        mw_ns = int(rng.integers(1, 3000)) * 1_000_000
        mei_ns = 2 * mw_ns + int(rng.integers(0, 3000)) * 1_000_000
        method = str(rng.choice(["static", "mad", "median_ratio"]))
        value = {"static": rng.uniform(1.5, 4.0), "mad": rng.uniform(1.0, 8.0), "median_ratio": rng.uniform(1.1, 3.0)}
        weights = tr.gaussian_weights(rng.uniform(0.5, 12.0), 4.0)[1] if rng.random() < 0.4 else None
        got = check(engine, x[0], x[1], period_ns=period_ns, mw_ns=mw_ns, mei_ns=mei_ns,
                    trigger_on=int(rng.integers(0, 2)), method=method, value=float(value[method]),
                    chunk_samples=int(rng.integers(50, n + 2000)), weights=weights)
        events += got["n_events"]
    assert events > 200


# -- refusals -----------------------------------------------------------------------------------------------------------
def raw_call(lib, eng, coa, coa_n, n=None, max_events=8, max_candidates=64, nulls=(), **par):
    """The C call itself, every output pre-filled with 7: (rc, message, untouched).  The tables hold `max_events`
    events and `max_candidates` candidates, the series may be of any length."""
    vp = ctypes.c_void_p
    fields = dict(trigger_on=0, threshold_method=0, threshold_value=1.0, chunk_samples=1, smooth_radius=0, reserved=0,
                  smooth_weights=vp(None), period_ns=PERIOD, mw_ns=10 ** 9, mei_ns=2 * 10 ** 9)
    weights = par.pop("weights", None)
    fields.update(par)
    if weights is not None:
        fields["smooth_weights"] = weights.ctypes.data_as(vp)
    p = lib.TriggerParams(**fields)
    out = {"events_i": np.full((max_events, 4), 7, dtype=np.int64), "events_f": np.full((max_events, 3), 7.0),
           "thresholds": np.full(64, 7.0), "smoothed": np.full((2, len(coa)), 7.0),
           "candidates": np.full((max_candidates, 5), 7, dtype=np.int64)}
    nc, ne = ctypes.c_int64(7), ctypes.c_int64(7)
    args = {"e": eng._h, "coa": coa.ctypes.data_as(vp), "coa_n": coa_n.ctypes.data_as(vp), "p": ctypes.byref(p),
            "nc": ctypes.byref(nc), "ne": ctypes.byref(ne), "events_i": out["events_i"].ctypes.data_as(vp),
            "events_f": out["events_f"].ctypes.data_as(vp)}
    for name in nulls:
        args[name] = None
    rc = lib.qmlib.qm_engine_trigger(args["e"], args["coa"], args["coa_n"], len(coa) if n is None else n, args["p"],
                                     max_events, args["nc"], args["ne"], args["events_i"], args["events_f"],
                                     out["thresholds"].ctypes.data_as(vp), out["smoothed"].ctypes.data_as(vp),
                                     out["candidates"].ctypes.data_as(vp), max_candidates)
    untouched = nc.value == 7 and ne.value == 7 and all(np.all(a == 7) for a in out.values())
    return rc, lib.qmlib.qm_last_error().decode(), untouched


def test_refusals_leave_the_outputs_untouched(lib, engine):
    x = spikes(4000, 200 * np.arange(1, 15))                                    # 14 separate events
    cap = engine.get("trigger_max_radius")
    wide = np.full(2 * (cap + 1) + 1, 1.0 / (2 * cap + 3))
    bad = x.copy()
    bad[[5, 6, 3000]] = np.nan, np.inf, -np.inf
    cases = [
        (dict(nulls=("e",)), "NULL argument"), (dict(nulls=("coa",)), "NULL argument"),
        (dict(nulls=("coa_n",)), "NULL argument"), (dict(nulls=("p",)), "NULL argument"),
        (dict(nulls=("nc",)), "NULL argument"), (dict(nulls=("ne",)), "NULL argument"),
        (dict(nulls=("events_i",)), "NULL argument"), (dict(nulls=("events_f",)), "NULL argument"),
        (dict(n=0), "empty input"),
        (dict(threshold_method=1, chunk_samples=0), "chunk_samples"),
        (dict(threshold_method=2, chunk_samples=-3), "chunk_samples"),
        (dict(threshold_method=3), "threshold_method"), (dict(trigger_on=2), "trigger_on"),
        (dict(weights=wide, smooth_radius=cap + 1), "smoothing radius"),
        (dict(mei_ns=2 * 10 ** 9 - 1), "mei_ns"), (dict(period_ns=0), "period_ns"),
    ]
    for kw, text in cases:
        rc, message, untouched = raw_call(lib, engine, x, x, **kw)
        assert rc != 0 and text in message and untouched, (kw, message)
    rc, message, untouched = raw_call(lib, engine, bad, x)
    assert rc != 0 and "3 non-finite samples" in message and untouched, message
    rc, message, untouched = raw_call(lib, engine, x, bad)
    assert rc != 0 and "3 non-finite samples" in message and untouched, message
    rc, message, untouched = raw_call(lib, engine, x, x)                       # room for 8 events, 14 needed
    assert rc != 0 and "14 events" in message and "room for 8" in message and untouched, message
    with pytest.raises(lib.QMHipError, match="14 events"):
        engine.trigger_series(x, x, PERIOD, 10 ** 9, 2 * 10 ** 9, value=1.0, max_events=13)
    assert engine.trigger_series(x, x, PERIOD, 10 ** 9, 2 * 10 ** 9, value=1.0, max_events=14)["n_events"] == 14
    with pytest.raises(TypeError):
        engine.trigger_series(x.astype(np.float32), x, PERIOD, 10 ** 9, 2 * 10 ** 9)
    with pytest.raises(ValueError, match="contiguous"):
        engine.trigger_series(np.zeros(8000)[::2], x, PERIOD, 10 ** 9, 2 * 10 ** 9)
    with pytest.raises(ValueError, match="coa_n of shape"):
        engine.trigger_series(x, x[:-1].copy(), PERIOD, 10 ** 9, 2 * 10 ** 9)


# -- past one trip of the scan and merge loops --------------------------------------------------------------------------
# trig_scan_kernel carries the run starts, the run ends and the non-finite count from one tile of run blocks to the next;
# trig_merge_kernel carries a segment from one pass of "trigger_merge_stride" candidates to the next.  The tile has no
# read-out: 600 run blocks are more than two of any tile up to 299 blocks (it is 256).  Every test asserts on the
# restatement alone, before the device is asked, what makes it able to fail.
LONG_BLOCKS = 600
SHORT = dict(mw_ns=PERIOD, mei_ns=2 * PERIOD)                                  # most candidates are events of their own


@pytest.fixture(scope="module")
def boundary_series(engine):
    """T1's series, built and restated once: (x, [(f, l, p)] in order, trigger_ref's answer under SHORT)."""
    block = engine.get("trigger_run_block")
    n = LONG_BLOCKS * block + 17
    x, runs = np.zeros(n), []

    def run(f, l, p, peak):
        x[f:l + 1] = 2.0
        x[p] = peak
        runs.append((f, l, p))

    for b in range(LONG_BLOCKS):
        e = b * block
        if b and b % 3 == 0:
            run(e - 40, e - 1, e - 1, 5.0)                                      # ends at e - 1, the next starts at e + 5
            run(e + 5, e + 44, e + 5, 4.0)
        elif b % 3 == 1:
            run(e - 41, e - 2, e - 2, 5.0)                                      # ends at e - 2, the next starts at e
            run(e, e + 39, e + 20, 4.0)
        elif b % 3 == 2:
            run(e - 70, e + 69, e + (b // 3) % 3 - 1, 3.0)                      # across e, peak at e - 1, e, e + 1
        for j in range(1 + b % 5):                                              # single samples inside the block
            run(e + 500 + 100 * j, e + 500 + 100 * j, e + 500 + 100 * j, 2.0 + 0.25 * j)
    run(n - 3, n - 1, n - 2, 6.0)                                               # ... and a run up to the last sample
    return x, sorted(runs), restate(x, **SHORT)


def test_long_series_runs_at_every_block_boundary(engine, boundary_series):
    block, stride = engine.get("trigger_run_block"), engine.get("trigger_merge_stride")
    x, runs, want = boundary_series
    assert len(x) == LONG_BLOCKS * block + 17
    cand = want["candidates"]
    starts, ends = np.bincount(cand[:, 0] // block), np.bincount(cand[:, 1] // block)
    print("blocks with starts / ends:", np.count_nonzero(starts), np.count_nonzero(ends), "start counts per block:",
          sorted(set(starts.tolist())), "end counts:", sorted(set(ends.tolist())), "candidates:", len(cand), "events:", want["n_events"])
    assert np.count_nonzero(starts) > 512 and np.count_nonzero(ends) > 512    # prefixes carried over two tiles
    assert len(set(starts)) > 3 and np.count_nonzero(starts != ends) > 100     # ... and no two alike to cancel out
    assert len(cand) > 4 * stride and want["n_events"] > len(cand) // 2
    assert [tuple(c) for c in cand[:, :3]] == runs                              # (the restatement against the list)
    got = check(engine, x, want=want, **SHORT)
    assert [tuple(c) for c in got["candidates"][:, :3]] == runs


def test_long_series_non_finite_samples_are_counted_across_tiles(lib, engine, boundary_series):
    block = engine.get("trigger_run_block")
    x, _, want = boundary_series
    coa, coa_n = x.copy(), x.copy()
    coa[[7, 300 * block + 1000, 599 * block + 2047]] = np.nan, np.inf, -np.inf
    coa_n[[257 * block, 511 * block + 2047]] = np.nan, -np.inf
    assert sorted(np.flatnonzero(~np.isfinite(coa)) // block) == [0, 300, 599]
    assert sorted(np.flatnonzero(~np.isfinite(coa_n)) // block) == [257, 511]
    room = dict(max_events=want["n_events"], max_candidates=want["n_candidates"], **SHORT)
    for a, b, count in ((coa, coa_n, 5), (x, coa_n, 2), (coa, x, 3)):
        with pytest.raises(tr.Refused, match=f"^{count} non-finite samples"):
            restate(a, b, **SHORT)
        rc, message, untouched = raw_call(lib, engine, a, b, **room)
        assert rc != 0 and f" {count} non-finite samples" in message and untouched, message
    check(engine, x, want=want, **SHORT)                                        # the same engine, the clean series


def long_event_layout(stride, chain, tail):
    """Sample positions: stride - 56 separate single samples, a chain of `chain` 1 s apart, `tail` separate ones."""
    at = list(200 * np.arange(1, stride - 55))
    first = len(at)
    at += [at[-1] + 200 + 50 * k for k in range(chain)]
    at += [at[-1] + 200 * (k + 1) for k in range(tail)]
    return np.array(at), first


def test_event_longer_than_a_pass_of_the_merge_loop(engine):
    stride = engine.get("trigger_merge_stride")
    members = 2 * stride + 188
    at, first = long_event_layout(stride, members, stride)
    last = first + members - 1
    passes = list(range(first // stride, last // stride + 1))
    filled = [q for q in passes if first <= q * stride and (q + 1) * stride - 1 <= last]
    print("chain of", members, "from candidate", first, "to", last, ": passes", passes, "filled", filled)
    assert len(passes) >= 3 and filled and first % stride and (last + 1) % stride
    two_s = 2 * 10 ** 9
    peaks = {"first pass": [first + 30], "filled pass": [filled[0] * stride + stride // 2],
             "last pass": [last - 40], "equal, two passes": [filled[0] * stride + 44, last - 3]}
    for name, where in peaks.items():
        values = 2.0 + (np.arange(len(at)) % 7) * 0.25
        values[where] = 9.0
        x = spikes(at[-1] + 10, at, values)
        want = restate(x)
        cand_of = {int(p): k for k, p in enumerate(want["candidates"][:, 2])}
        event = want["events_i"][first]
        peak_pass = cand_of[int(event[0])] // stride
        print(name, ": peak at candidate", cand_of[int(event[0])], "pass", peak_pass, "members", event[3])
        assert want["n_candidates"] == len(at) and want["n_events"] == len(at) - members + 1
        assert event[3] == members and cand_of[int(event[0])] == where[0]
        assert peak_pass == {"first pass": passes[0], "filled pass": filled[0], "last pass": passes[-1],
                             "equal, two passes": filled[0]}[name]
        if len(where) == 2:
            assert where[1] // stride != where[0] // stride
        got = check(engine, x, want=want)
        assert tuple(got["events_i"][first]) == (at[where[0]], at[first] * PERIOD - two_s, at[last] * PERIOD + two_s,
                                                 members)
        assert tuple(got["events_f"][first]) == (9.0, 9.0, 9.0)
        for row, k in ((first - 1, first - 1), (first + 1, last + 1)):         # its neighbours: untouched single events
            assert tuple(got["events_i"][row]) == (at[k], at[k] * PERIOD - two_s, at[k] * PERIOD + two_s, 1)
            assert got["events_f"][row, 0] == values[k]
    # a chain that ends in the last slot of a pass, a separate event in slot 0 of the next
    at, first = long_event_layout(stride, 2 * stride - (stride - 56), stride)
    last = 2 * stride - 1
    values = 2.0 + (np.arange(len(at)) % 7) * 0.25
    x = spikes(at[-1] + 10, at, values)
    want = restate(x)
    sizes = want["events_i"][:, 3]
    assert list(sizes[first - 1:first + 3]) == [1, last - first + 1, 1, 1] and first + sizes[first] - 1 == last
    assert want["events_i"][first + 1, 0] == at[2 * stride]                      # slot 0 of pass 2 opens an event
    got = check(engine, x, want=want)
    assert tuple(got["events_i"][first + 1]) == (at[last + 1], at[last + 1] * PERIOD - two_s,
                                                 at[last + 1] * PERIOD + two_s, 1)
    assert got["events_i"][first, 2] == at[last] * PERIOD + two_s


def test_long_seeded_series_equals_the_restatement_from_host_and_device(engine):
    import torch

    block = engine.get("trigger_run_block")
    n = LONG_BLOCKS * block + 17
    rng = np.random.default_rng(2014)
    noise = rng.gamma(2.0, 0.5, (2, n))
    for at in rng.integers(0, n, 400):                                          # bursts of random width and height
        width = int(rng.integers(1, 200))
        shape = rng.uniform(4.0, 12.0) * np.hanning(width + 2)[1:-1]
        stop = min(n, at + width)
        noise[:, at:stop] += shape[:stop - at] * rng.uniform(0.5, 1.5, (2, 1))
    x = np.round(noise, 5)
    par = dict(trigger_on=1, method="mad", value=3.0, chunk_samples=180_000,
               weights=tr.gaussian_weights(2.5, 4.0)[1])
    want = restate(x[0], x[1], **par)
    blocks = np.count_nonzero(np.bincount(want["candidates"][:, 0] // block, minlength=LONG_BLOCKS + 1))
    print("candidates:", want["n_candidates"], "events:", want["n_events"], "blocks with starts:", blocks,
          "chunks:", len(want["thresholds"]))
    assert want["n_events"] > 100 and len(want["thresholds"]) == -(-n // 180_000)
    assert want["candidates"][:, 0].min() < 256 * block and want["candidates"][:, 0].max() > 512 * block
    got = check(engine, x[0], x[1], want=want, **par)
    where = f"cuda:{engine.device}"
    coa, coa_n = torch.from_numpy(x[0]).to(where), torch.from_numpy(x[1]).to(where)
    torch.cuda.synchronize(where)
    resident = engine.trigger_series(coa, coa_n, PERIOD, 10 ** 9, 2 * 10 ** 9, max_events=n, want_candidates=True,
                                     **par)
    assert sorted(resident) == sorted(got)
    for key, value in got.items():
        if isinstance(value, np.ndarray) and value.dtype == np.float64:
            assert np.array_equal(bits(resident[key]), bits(value)), key
        else:
            assert np.array_equal(resident[key], value), key


def test_long_lived_engine_equals_fresh_engines(lib, engine):
    import picks_ref as pr
    from quakemigrate_amd import synth

    case = synth.make_case("C2", step=0, grid=(26, 25, 14), n_samples=700)
    logged = np.ascontiguousarray(np.log(np.clip(case.onsets, 0.01, np.inf)))
    fam = pr.family_results(n_stations=10)
    rng = np.random.default_rng(77)
    series = [np.round(rng.gamma(2.0, 0.8, (2, n)), 5) for n in (30_000, 2_500, 12_345)]
    _, w = tr.gaussian_weights(3.0, 4.0)
    calls = [dict(method="mad", value=3.0, chunk_samples=5000, weights=w), dict(value=3.0, trigger_on=1),
             dict(method="median_ratio", value=2.0, chunk_samples=700)]

    def trig(eng, k):
        got = eng.trigger_series(series[k][0].copy(), series[k][1].copy(), PERIOD, 10 ** 9, 2 * 10 ** 9,
                                 want_candidates=True, **calls[k])
        return [got["n_events"], got["candidates"], got["events_i"], bits(got["events_f"]), bits(got["thresholds"])]

    def picks(eng):
        return eng.pick_phases(fam["onsets"], fam["windows"], fam["row_group"], fam["sampling_rate"],
                               fam["halfwidth"])

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    engine.load_lut(case.traveltimes)
    detect0 = engine.detect(logged, case.fsmp, case.lsmp, case.available)
    picks0 = picks(engine)
    first = [trig(engine, k) for k in range(3)]
    assert first[0][0] > 3
    for _ in range(2):
        for k in (2, 0, 1):
            assert same(engine.detect(logged, case.fsmp, case.lsmp, case.available), detect0)
            assert same(trig(engine, k), first[k])
            assert same(picks(engine), picks0)
    for k in range(3):
        fresh = lib.Engine(0)
        try:
            assert same(trig(fresh, k), first[k])
        finally:
            fresh.close()


# -- the example --------------------------------------------------------------------------------------------------------
def test_example_triggers_and_locates_the_synthetic_events(tmp_path):
    spec = importlib.util.spec_from_file_location("trigger_events", ROOT / "examples" / "trigger_events.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    events, located, truth = mod.run(tmp_path)
    assert len(sorted(tmp_path.glob("*.scanmseed"))) == 2                       # the run crosses midnight
    assert len(events) == len(truth) and len(located) == len(events)
    by_uid = {r["uid"]: r for r in located}
    for ev, (node, origin) in zip(events, truth):
        assert abs((ev["CoaTime"] - origin).total_seconds()) <= 0.04
        # (depth is the poorly resolved axis of a surface network)
        assert np.abs(np.asarray(by_uid[ev["EventID"]]["fits"].spline) - np.asarray(node)).max() <= 2.0
    from quakemigrate_amd import trigger

    assert [e["EventID"] for e in trigger.read_triggered_events(tmp_path / "TriggeredEvents.csv")] == \
        [e["EventID"] for e in events]
