# -*- coding: utf-8 -*-
"""
CPU-side checks of the trigger stage (no GPU): the NumPy restatement the GPU tests compare against
(tests/trigger_ref.py) reproduces the reference's recorded ``TriggeredEvents.csv`` files from their ``.scanmseed`` and
is pinned to SciPy, NumPy and an independent pandas statement of the reference's rules; the front end
(quakemigrate_amd/trigger.py) refuses what it documents and applies the host rules; the C ABI carries the new symbol
and refuses what it can refuse without a device.
"""

import ctypes
import datetime as dt

import numpy as np
import pytest

import trigger_ref as tr
from conftest import GOLDEN, ROOT

PERIOD = 20_000_000
METHODS = {"static": tr.STATIC, "mad": tr.MAD, "median_ratio": tr.MEDIAN_RATIO}


class RefEngine:
    """``Engine.trigger_series`` answered by the restatement."""

    def __init__(self):
        self.calls = []

    def trigger_series(self, coa, coa_n, period_ns, mw_ns, mei_ns, trigger_on=0, method="static", value=1.5,
                       chunk_samples=1, weights=None, max_events=65536, want_candidates=False):
        self.calls.append(dict(n=len(coa), period_ns=period_ns, mw_ns=mw_ns, mei_ns=mei_ns, trigger_on=trigger_on,
                               method=method, value=value, chunk_samples=chunk_samples, weights=weights))
        return tr.trigger_series(coa, coa_n, trigger_on, weights, METHODS[method], value, chunk_samples, period_ns,
                                 mw_ns, mei_ns, max_events)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_engine()
    from quakemigrate_amd.core import lib as _lib

    return _lib


# -- 1. the reference's recorded results -------------------------------------------------------------------------------
BENCHMARKS = {
    "icequake": dict(scan="icequake_iceland_2014_180.scanmseed", csv="icequake_iceland_2014_180_TriggeredEvents.csv",
                     mw=0.06, mei=0.12, threshold=2.15, start=dt.datetime(2014, 6, 29, 18, 42, 5),
                     end=dt.datetime(2014, 6, 29, 18, 42, 15), region=None, n=2500, rate=250.0, counts=(9, 3, 3)),
    "volcanotectonic": dict(scan="volcanotectonic_iceland_2014_236.scanmseed",
                            csv="volcanotectonic_iceland_2014_236_TriggeredEvents.csv", mw=0.75, mei=1.5,
                            threshold=1.85, start=dt.datetime(2014, 8, 24, 0, 1, 0),
                            end=dt.datetime(2014, 8, 24, 0, 11, 0),
                            region=[-17.15, 64.72, 0.0, -16.65, 64.93, 14.0], n=30000, rate=50.0,
                            counts=(54, 29, 28)),
}


@pytest.mark.parametrize("name", sorted(BENCHMARKS))
def test_restatement_reproduces_the_references_recorded_events(name, tmp_path):
    import csv

    from quakemigrate_amd import scanmseed, trigger

    b = BENCHMARKS[name]
    t0, rate, cols = scanmseed.read_scanmseed(GOLDEN / b["scan"], 1000)
    assert (len(cols["COA"]), rate) == (b["n"], b["rate"])
    t = trigger.DeviceTrigger(marginal_window=b["mw"], min_event_interval=b["mei"], normalise_coalescence=True,
                              static_threshold=b["threshold"])
    events = t.trigger_series(RefEngine(), t0, rate, cols, b["start"], b["end"], region=b["region"])
    assert (t.last["n_candidates"], t.last["n_events"], len(events)) == b["counts"]
    with open(GOLDEN / b["csv"], newline="") as f:
        recorded = list(csv.DictReader(f))
    assert len(recorded) == len(events)
    for got, want in zip(events, recorded):
        assert got["EventID"] == want["EventID"] and trigger.stamp(got["CoaTime"]) == want["CoaTime"]
        for col in ("TRIG_COA", "COA_X", "COA_Y", "COA_Z", "COA", "COA_NORM"):
            assert got[col] == float(want[col]), (got["EventID"], col)
    # ... and written out, the file parses to the recorded one
    trigger.write_triggered_events(tmp_path / "events.csv", events)
    assert trigger.read_triggered_events(tmp_path / "events.csv") == trigger.read_triggered_events(GOLDEN / b["csv"])


# -- 2. smoothing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 37, 300, 1000, 5000, 200_001])
def test_smoothing_is_scipys_gaussian_filter(n):
    from scipy.ndimage import gaussian_filter1d

    x = np.round(np.random.default_rng(n).gamma(2.0, 1.0, n), 5)
    for sd in (0.4, 2.5, 10.0):
        for truncate in (2.0, 4.0):
            r, w = tr.gaussian_weights(sd, truncate)
            assert len(w) == 2 * r + 1
            assert np.array_equal(tr.smooth(x, r, w), gaussian_filter1d(x, sd, truncate=truncate)), (sd, truncate)


def test_front_end_weights_are_the_restatements():
    from quakemigrate_amd import trigger

    for sd, truncate in ((0.4, 2.0), (10.0, 4.0), (2.5, 4.0)):
        (r0, w0), (r1, w1) = trigger.gaussian_weights(sd, truncate), tr.gaussian_weights(sd, truncate)
        assert r0 == r1 and np.array_equal(w0, w1)


# -- 3. thresholds -------------------------------------------------------------------------------------------------------
def get_threshold(x, method, chunk, value):
    """``Trigger._get_threshold`` (trigger.py:454-479) in its own terms: np.split at the multiples of the chunk
    length, np.median per piece, every value repeated over its chunk and the trace cut to the series."""
    idx = np.arange(len(x))
    pieces = np.split(x, idx[idx % chunk == 0][1:])
    shape = (len(pieces), len(pieces[0]))
    med = np.asarray([np.median(p) for p in pieces])
    med_trace = np.reshape(np.broadcast_to(med[:, None], shape), shape[0] * shape[1])[:len(x)]
    if method == tr.MEDIAN_RATIO:
        return med_trace * value
    mad = np.asarray([1.4826 * np.median(np.abs(p - np.median(p))) for p in pieces])
    mad_trace = np.reshape(np.broadcast_to(mad[:, None], shape), shape[0] * shape[1])[:len(x)]
    return med_trace + (mad_trace * value)


@pytest.mark.parametrize("chunk", [7, 64])                 # odd and even
def test_thresholds_are_the_references_expression(chunk):
    rng = np.random.default_rng(chunk)
    for n in (chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1):
        x = np.round(rng.gamma(2.0, 1.0, n), 5)
        for method, value in ((tr.MAD, 8.0), (tr.MEDIAN_RATIO, 1.2)):
            thr = tr.chunk_thresholds(x, method, value, chunk)
            assert len(thr) == -(-n // chunk)
            assert np.array_equal(tr.threshold_trace(thr, method, chunk, n), get_threshold(x, method, chunk, value))
            # what the kernel selects: the middle of the sorted chunk
            for c, t in enumerate(thr):
                part = x[c * chunk:(c + 1) * chunk]
                med = tr.middle(part)
                assert t == (med + (1.4826 * tr.middle(np.abs(part - med))) * value if method == tr.MAD
                             else med * value)
    assert np.array_equal(tr.chunk_thresholds(x, tr.STATIC, 1.5, chunk), [1.5])


# -- 4. candidates and merge ---------------------------------------------------------------------------------------------
def pandas_events(coa, coa_n, thr_trace, trigger_on, period_ns, mw_ns, mei_ns):
    """``_identify_candidates`` and ``_refine_candidates`` (trigger.py:517-621) on a DataFrame, times as int64
    nanoseconds: groupby(index - arange), idxmax, the sequential event count."""
    pd = pytest.importorskip("pandas")
    data = pd.DataFrame({"DT": np.arange(len(coa), dtype=np.int64) * period_ns, "COA": coa, "COA_N": coa_n})
    on = "COA_N" if trigger_on else "COA"
    gap = mei_ns - mw_ns
    above = data[data[on] >= thr_trace]
    rows = []
    for _, d in above.groupby(above.index - np.arange(len(above))):
        peak = d.loc[d["COA"].idxmax()]
        t_min = peak["DT"] - mei_ns if peak["DT"] - d["DT"].iloc[0] < mw_ns else d["DT"].iloc[0] - gap
        t_max = peak["DT"] + mei_ns if d["DT"].iloc[-1] - peak["DT"] < mw_ns else d["DT"].iloc[-1] + gap
        rows.append(dict(first=d.index[0], last=d.index[-1], peak=int(d["COA"].idxmax()), CoaTime=int(peak["DT"]),
                         TRIG_COA=peak[on], MinTime=int(t_min), MaxTime=int(t_max), COA=peak["COA"],
                         COA_NORM=peak["COA_N"], EventNum=0))
    cand = pd.DataFrame(rows)
    if cand.empty:
        return cand, cand
    count = 1
    for i, ev1 in cand.iterrows():
        cand.loc[i, "EventNum"] = count
        if i + 1 == len(cand):
            continue
        ev2 = cand.iloc[i + 1]
        if all([ev1["MaxTime"] < ev2["CoaTime"] - mw_ns, ev2["MinTime"] > ev1["CoaTime"] + mw_ns]):
            count += 1
    events = []
    for _, members in cand.groupby(cand["EventNum"]):
        ev = members.loc[members["TRIG_COA"].idxmax()].copy()
        ev["MinTime"], ev["MaxTime"], ev["members"] = members["MinTime"].min(), members["MaxTime"].max(), len(members)
        events.append(ev)
    return cand, pd.DataFrame(events)


def compare_with_pandas(coa, coa_n, trigger_on, thr, period_ns, mw_ns, mei_ns):
    out = tr.trigger_series(coa, coa_n, trigger_on, None, tr.STATIC, thr, 1, period_ns, mw_ns, mei_ns)
    cand, events = pandas_events(coa, coa_n, np.full(len(coa), thr), trigger_on, period_ns, mw_ns, mei_ns)
    assert len(cand) == out["n_candidates"] and len(events) == out["n_events"]
    if len(cand):
        assert np.array_equal(cand[["first", "last", "peak", "MinTime", "MaxTime"]].to_numpy(dtype=np.int64),
                              out["candidates"])
        assert np.array_equal(events["peak"].to_numpy(dtype=np.int64), out["events_i"][:, 0])
        assert np.array_equal(events[["MinTime", "MaxTime", "members"]].to_numpy(dtype=np.int64),
                              out["events_i"][:, 1:])
        assert np.array_equal(events[["TRIG_COA", "COA", "COA_NORM"]].to_numpy(dtype=np.float64), out["events_f"])
    return out


@pytest.mark.parametrize("seed", range(6))
def test_candidates_and_merge_equal_the_pandas_statement_on_seeded_series(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(500, 4000))
    x = np.round(rng.gamma(2.0, 0.6, (2, n)), 5)
    for at in rng.integers(0, n - 60, 12):
        x[:, at:at + 60] += np.round(rng.uniform(1.0, 4.0) * np.hanning(60), 5)
    mw_ns = int(rng.integers(1, 30)) * 10_000_000
    out = compare_with_pandas(x[0], x[1], seed % 2, 2.5, PERIOD, mw_ns, 2 * mw_ns + int(rng.integers(0, 50)) * 10 ** 7)
    assert out["n_candidates"] > out["n_events"] > 1


def test_candidates_and_merge_equal_the_pandas_statement_on_designed_series():
    x = np.zeros(3000)
    x[0:3] = 2.0                                            # a run at the first sample
    x[200:260], x[230], x[240] = 2.0, 3.0, 3.0              # equal maxima: the first one
    x[400], x[550], x[701] = 2.0, 2.0, 2.0                  # 3 s apart: merged (strict), one sample more: separate
    x[1000:1300], x[1000] = 2.0, 2.5                        # a long run peaking at its first sample ...
    x[1375] = 2.2                                           # ... and a sample 1.5 s behind it: one condition fails
    x[2990:] = 2.0                                          # a run at the last sample
    y = x.copy()
    y[235] = 9.0                                            # the trigger series peaks elsewhere
    for on in (0, 1):
        out = compare_with_pandas(x, y, on, 2.0, PERIOD, 10 ** 9, 2 * 10 ** 9)
        assert out["n_candidates"] == 8 and out["n_events"] == 6
        assert out["candidates"][1, 2] == 230
    quiet = compare_with_pandas(np.zeros(100), np.zeros(100), 0, 2.0, PERIOD, 10 ** 9, 2 * 10 ** 9)
    assert quiet["n_candidates"] == 0 and quiet["events_i"].shape == (0, 4)


def test_restatement_refuses_what_the_call_refuses():
    x = np.ones(10)
    for kw in (dict(method=tr.MAD, chunk=0), dict(mei_ns=1, mw_ns=1), dict(period_ns=0),
               dict(weights=np.ones(2 * 4097 + 1)), dict(max_events=0, value=0.5)):
        with pytest.raises(tr.Refused):
            tr.trigger_series(x, x, **kw)
    with pytest.raises(tr.Refused, match="2 non-finite"):
        tr.trigger_series(np.array([1.0, np.nan]), np.array([np.inf, 1.0]))
    with pytest.raises(tr.Refused):
        tr.trigger_series(np.zeros(0), np.zeros(0))


# -- 5. the C ABI and the front end --------------------------------------------------------------------------------------
def test_symbol_is_exported_and_refuses_without_a_device(lib):
    assert hasattr(lib.qmlib, "qm_engine_trigger")
    assert "int qm_engine_trigger(" in (ROOT / "include" / "qmhip.h").read_text()
    vp = ctypes.c_void_p
    x = np.ones(50)
    ev_i, ev_f = np.full((4, 4), 7, dtype=np.int64), np.full((4, 3), 7.0)
    nc, ne = ctypes.c_int64(7), ctypes.c_int64(7)
    par = lib.TriggerParams(0, 0, 1.5, 1, 0, 0, vp(None), PERIOD, 10 ** 9, 2 * 10 ** 9)
    rc = lib.qmlib.qm_engine_trigger(vp(None), x.ctypes.data_as(vp), x.ctypes.data_as(vp), 50, ctypes.byref(par), 4,
                                     ctypes.byref(nc), ctypes.byref(ne), ev_i.ctypes.data_as(vp),
                                     ev_f.ctypes.data_as(vp), vp(None), vp(None), vp(None), 0)
    assert rc != 0 and b"NULL argument" in lib.qmlib.qm_last_error()
    assert (nc.value, ne.value) == (7, 7) and np.all(ev_i == 7) and np.all(ev_f == 7.0)
    # the struct the binding passes is the header's: 64 bytes, the weights pointer at 32
    assert ctypes.sizeof(lib.TriggerParams) == 64 and lib.TriggerParams.smooth_weights.offset == 32


def test_binding_checks_arrays_before_the_call(lib):
    eng = lib.Engine.__new__(lib.Engine)                    # no device here: the checks come before the C call
    eng._h, eng.device = None, 0
    x = np.ones(50)
    with pytest.raises(TypeError, match="float64"):
        eng.trigger_series(x.astype(np.float32), x, PERIOD, 10 ** 9, 2 * 10 ** 9)
    with pytest.raises(TypeError, match="NumPy array"):
        eng.trigger_series(list(x), x, PERIOD, 10 ** 9, 2 * 10 ** 9)
    with pytest.raises(ValueError, match="contiguous"):
        eng.trigger_series(x, np.ones(100)[::2], PERIOD, 10 ** 9, 2 * 10 ** 9)
    with pytest.raises(ValueError, match="coa_n of shape"):
        eng.trigger_series(x, np.ones(49), PERIOD, 10 ** 9, 2 * 10 ** 9)
    with pytest.raises(ValueError, match="method must be"):
        eng.trigger_series(x, x, PERIOD, 10 ** 9, 2 * 10 ** 9, method="mean")
    with pytest.raises(ValueError, match="odd number"):
        eng.trigger_series(x, x, PERIOD, 10 ** 9, 2 * 10 ** 9, weights=np.ones(4))
    with pytest.raises(lib.QMHipError, match="NULL argument"):      # the engine handle is NULL
        eng.trigger_series(x, x, PERIOD, 10 ** 9, 2 * 10 ** 9)


def test_front_end_value_errors():
    from quakemigrate_amd.trigger import DeviceTrigger

    assert DeviceTrigger(threshold_method="dynamic").threshold_method == "mad"
    d = DeviceTrigger()                                     # the reference's defaults (trigger.py:213-228)
    assert (d.threshold_method, d.static_threshold, d.mad_window_length, d.mad_multiplier, d.median_window_length,
            d.median_multiplier, d.marginal_window, d.min_event_interval, d.normalise_coalescence, d.pad, d.smooth_coa,
            d.smoothing_kernel_sigma, d.smoothing_kernel_width) == ("static", 1.5, 3600.0, 8.0, 3600.0, 1.2, 2.0, 4.0,
                                                                    False, 120.0, False, 0.2, 4.0)
    with pytest.raises(ValueError, match="threshold_method"):
        DeviceTrigger(threshold_method="mean")
    with pytest.raises(ValueError, match="marginal_window .* microseconds"):
        DeviceTrigger(marginal_window=0.0000015, min_event_interval=1.0)
    with pytest.raises(ValueError, match="min_event_interval .* microseconds"):
        DeviceTrigger(marginal_window=0.5, min_event_interval=1.0000001)
    with pytest.raises(ValueError, match="pad .* microseconds"):
        DeviceTrigger(pad=1.00000049)
    with pytest.raises(ValueError, match="Minimum event interval must be >= 2"):
        DeviceTrigger(marginal_window=2.0, min_event_interval=3.999999)
    cols = {k: np.zeros(30) for k in ("COA", "COA_N", "X", "Y", "Z")}
    t0 = dt.datetime(2024, 1, 1)
    with pytest.raises(ValueError, match="sampling period .* microseconds"):
        DeviceTrigger().trigger_series(RefEngine(), t0, 3.0, cols, t0, t0 + dt.timedelta(seconds=5))
    assert DeviceTrigger().trigger_series(RefEngine(), t0, 3.2, cols, t0, t0 + dt.timedelta(seconds=5)) == []
    with pytest.raises(ValueError, match="no sample between"):
        DeviceTrigger(pad=1.0).trigger_series(RefEngine(), t0, 50.0, cols, t0 + dt.timedelta(hours=1),
                                              t0 + dt.timedelta(hours=2))


def test_event_id_formatting():
    from quakemigrate_amd.trigger import event_id, stamp

    assert event_id(dt.datetime(2014, 6, 29, 18, 42, 8, 376000)) == "20140629184208376"
    assert event_id(dt.datetime(2014, 8, 24, 0, 1, 54)) == "20140824000154000"         # zero microseconds
    assert event_id(dt.datetime(2014, 8, 24, 0, 1, 54, 123456)) == "20140824000154123"
    assert stamp(dt.datetime(2014, 8, 24, 0, 1, 54)) == "2014-08-24T00:01:54.000000Z"


def series_with_spikes(n, at, value=3.0):
    cols = {k: np.zeros(n) for k in ("COA", "COA_N")}
    cols.update(X=np.arange(n) * 1.0, Y=np.arange(n) * 2.0, Z=np.arange(n) * 3.0)
    cols["COA"][list(at)] = value
    cols["COA_N"][list(at)] = value / 2
    return cols


def test_fake_engine_drives_the_front_end_end_to_end():
    from quakemigrate_amd.trigger import DeviceTrigger, EVENT_COLS, triggers

    t0 = dt.datetime(2024, 3, 1, 12, 0, 0)
    cols = series_with_spikes(50 * 600, [50 * 10, 50 * 100, 50 * 101, 50 * 300, 50 * 590])
    eng = RefEngine()
    t = DeviceTrigger(static_threshold=2.0, marginal_window=1.0, min_event_interval=2.0, pad=30.0)
    start, end = t0 + dt.timedelta(seconds=60), t0 + dt.timedelta(seconds=400)
    events = t.trigger_series(eng, t0, 50.0, cols, start, end)
    # the cut: [start - 30 s, end + 30 s] inclusive; the spike at 10 s lies before it, the one at 590 s behind it
    assert eng.calls[0]["n"] == 50 * 400 + 1 and t.last["first_sample"] == 50 * 30
    assert (eng.calls[0]["period_ns"], eng.calls[0]["mw_ns"], eng.calls[0]["mei_ns"]) == (PERIOD, 10 ** 9, 2 * 10 ** 9)
    assert t.last["n_candidates"] == 3 and [e["CoaTime"] for e in events] == [
        t0 + dt.timedelta(seconds=100), t0 + dt.timedelta(seconds=300)]
    first = events[0]
    assert tuple(first) == EVENT_COLS
    assert (first["MinTime"], first["MaxTime"]) == (t0 + dt.timedelta(seconds=98), t0 + dt.timedelta(seconds=103))
    assert (first["TRIG_COA"], first["COA"], first["COA_NORM"]) == (3.0, 3.0, 1.5)
    assert (first["COA_X"], first["COA_Y"], first["COA_Z"]) == (5000.0, 10000.0, 15000.0)
    assert triggers(events) == [("20240301120140000", t0 + dt.timedelta(seconds=100)),
                                ("20240301120500000", t0 + dt.timedelta(seconds=300))]
    # an event in the pad is triggered and dropped; the region keeps what lies inside it
    assert len(t.trigger_series(eng, t0, 50.0, cols, t0 + dt.timedelta(seconds=120), end)) == 1
    inside = t.trigger_series(eng, t0, 50.0, cols, start, end, region=[0, 0, 0, 6000.0, 1e9, 1e9])
    assert [e["COA_X"] for e in inside] == [5000.0]
    # the parameters reach the engine: normalised series, MAD chunks in samples, the smoothing kernel
    t = DeviceTrigger(threshold_method="mad", mad_window_length=60.0, mad_multiplier=5.0, normalise_coalescence=True,
                      smooth_coa=True, smoothing_kernel_sigma=0.2, smoothing_kernel_width=4.0, pad=30.0,
                      marginal_window=1.0, min_event_interval=2.0)
    t.trigger_series(eng, t0, 50.0, cols, start, end)
    call = eng.calls[-1]
    assert (call["trigger_on"], call["method"], call["value"], call["chunk_samples"]) == (1, "mad", 5.0, 3000)
    assert len(call["weights"]) == 2 * 40 + 1 and t.last["smoothed"].shape == (2, 50 * 400 + 1)


def test_midnight_belongs_to_the_next_day():
    from quakemigrate_amd.trigger import DeviceTrigger

    t0 = dt.datetime(2024, 3, 1, 23, 50, 0)
    midnight = dt.datetime(2024, 3, 2)
    cols = series_with_spikes(50 * 1200, [50 * 600 - 2, 50 * 600, 50 * 900])     # 23:59:59.96, 00:00:00, 00:05:00
    t = DeviceTrigger(static_threshold=2.0, marginal_window=0.005, min_event_interval=0.01, pad=60.0)
    eng = RefEngine()
    day1 = t.trigger_series(eng, t0, 50.0, cols, t0, midnight)
    assert [e["CoaTime"] for e in day1] == [midnight - dt.timedelta(milliseconds=40)]
    assert eng.calls[0]["n"] == 50 * 660 + 1                # (the read keeps the original batchend + pad)
    day2 = t.trigger_series(eng, t0, 50.0, cols, midnight, midnight + dt.timedelta(minutes=8))
    assert [e["CoaTime"] for e in day2] == [midnight, midnight + dt.timedelta(minutes=5)]
    # an end that is not midnight is inclusive
    assert len(t.trigger_series(eng, t0, 50.0, cols, t0, midnight - dt.timedelta(milliseconds=40))) == 1


def test_trigger_batches_by_day_over_the_sinks_files(tmp_path):
    from quakemigrate_amd import scanmseed
    from quakemigrate_amd.trigger import DeviceTrigger

    rate, t0 = 50, dt.datetime(2024, 3, 1, 23, 58, 0)
    n = rate * 240                                          # two minutes either side of midnight
    coa = np.ones(n)
    coa[[rate * 30, rate * 120 - 2, rate * 120, rate * 200]] = 3.0
    sink = scanmseed.CoalescenceSink(tmp_path, rate)
    for k in range(4):                                      # appended a minute at a time: the sink splits at midnight
        part = slice(k * rate * 60, (k + 1) * rate * 60)
        coord = np.stack([np.arange(n)[part] * 1e-3, np.zeros(rate * 60), np.zeros(rate * 60)], axis=-1)
        sink.append(t0 + dt.timedelta(seconds=60 * k), coa[part], coa[part] / 2, coord, 1000.0)
    sink.write()
    assert [p.name for p in sorted(tmp_path.glob("*.scanmseed"))] == ["2024_061.scanmseed", "2024_062.scanmseed"]
    t = DeviceTrigger(static_threshold=2.0, marginal_window=0.005, min_event_interval=0.01, pad=60.0)
    eng = RefEngine()
    events = t.trigger(tmp_path, t0, t0 + dt.timedelta(seconds=240), 1000.0, engine=eng)
    midnight = dt.datetime(2024, 3, 2)
    assert [e["CoaTime"] for e in events] == [t0 + dt.timedelta(seconds=30), midnight - dt.timedelta(milliseconds=40),
                                              midnight, t0 + dt.timedelta(seconds=200)]
    assert [c["n"] for c in eng.calls] == [rate * 120, rate * 120]       # each batch clipped to its own day's file
    assert events[0]["COA_X"] == pytest.approx(rate * 30 * 1e-3, abs=1e-6)
    # a day without a file is skipped; the window may start inside a day
    assert t.trigger(tmp_path, t0 - dt.timedelta(days=1), t0 + dt.timedelta(seconds=60), 1000.0, engine=eng)[0][
        "CoaTime"] == t0 + dt.timedelta(seconds=30)
    with pytest.raises(ValueError, match="after endtime"):
        t.trigger(tmp_path, t0, t0 - dt.timedelta(seconds=1), 1000.0, engine=eng)


def test_csv_round_trip(tmp_path):
    from quakemigrate_amd import trigger

    t0 = dt.datetime(2014, 8, 24, 0, 1, 9, 140000)
    events = [{"EventID": trigger.event_id(t0), "CoaTime": t0, "TRIG_COA": 2.35673, "COA_X": -16.948544,
               "COA_Y": 64.754113, "COA_Z": 7.0, "MinTime": t0 - dt.timedelta(seconds=1.5),
               "MaxTime": t0 + dt.timedelta(seconds=1.5), "COA": 2.40836, "COA_NORM": 2.35673}]
    trigger.write_triggered_events(tmp_path / "a.csv", events)
    lines = (tmp_path / "a.csv").read_text().splitlines()
    assert lines[0] == "EventID,CoaTime,TRIG_COA,COA_X,COA_Y,COA_Z,COA,COA_NORM"
    assert lines[1] == "20140824000109140,2014-08-24T00:01:09.140000Z,2.35673,-16.948544,64.754113,7,2.40836,2.35673"
    back = trigger.read_triggered_events(tmp_path / "a.csv")
    assert back == [{k: v for k, v in events[0].items() if k in trigger.OUTPUT_COLS}]
    trigger.write_triggered_events(tmp_path / "b.csv", events, write_event_time_windows=True)
    assert (tmp_path / "b.csv").read_text().splitlines()[0].endswith("COA_NORM,MinTime,MaxTime")
    assert trigger.read_triggered_events(tmp_path / "b.csv") == events
    trigger.write_triggered_events(tmp_path / "c.csv", [])
    assert trigger.read_triggered_events(tmp_path / "c.csv") == []
