# -*- coding: utf-8 -*-
"""
The pre-processing of gappy traces on the GPU (qm_engine_preprocess_segments, qm_stream_set_segment_feed /
qm_stream_push_segments, MigrationScan.continuous_compute's 4-tuple device stage) against its per-segment NumPy
restatement, tests/preprocess_segments_ref.py, bit for bit.

Inputs are seeded Gaussian noise of amplitude ~1e3 on a ramp and an offset with NaN wherever no segment holds data: a
kernel that read a sample outside its segments would carry the NaN into its output.
"""

import dataclasses

import numpy as np
import pytest

import preprocess_ref as pr
import preprocess_segments_ref as sr

pytestmark = pytest.mark.gpu

LDS_SAMPLES = 20480
T = 301
TRACE_FILTER = np.array([0, 1, 0, 1], dtype=np.int32)          # 4 traces, two filters of 2 sections

# every trace has at least one segment; (trace, first, n)
LAYOUTS = {
    "one segment": [(0, 0, T), (1, 0, T), (2, 0, T), (3, 0, T)],
    "n = 1 and n = 2 at the ends": [(0, 0, 1), (0, T - 2, 2), (1, 0, 1), (2, T - 2, 2), (3, 0, T)],
    "63 / 64 / 65 / 129": [(0, 0, 63), (0, 70, 64), (0, 140, 65), (1, 100, 129), (2, 3, 129), (2, 140, 63),
                           (3, 2, 64), (3, 67, 65), (3, 172, 129)],
    "one sample apart": [(0, 0, 150), (0, 151, 150), (1, 10, 100), (1, 111, 100), (2, 0, T), (3, 0, 299), (3, 300, 1)],
    "late start, early end": [(0, 17, 200), (1, 1, 299), (2, 120, 60), (3, 0, T)],
}


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


def stable_sos(seed, n_filters, n_sections):
    """Random stable sections, a0 == 1: complex pole pairs of radius 0.5-0.95, arbitrary zeros, gains near 1."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.5, 0.95, size=(n_filters, n_sections))
    th = rng.uniform(0.2, 2.9, size=(n_filters, n_sections))
    sos = np.empty((n_filters, n_sections, 6))
    sos[..., :3] = rng.uniform(-1.0, 1.0, size=(n_filters, n_sections, 3))
    sos[..., 3] = 1.0
    sos[..., 4] = -2.0 * r * np.cos(th)
    sos[..., 5] = r * r
    return sos


SOS = stable_sos(17, 2, 2)


def _plan(t_samples, n_traces, segments):
    from quakemigrate_amd.preprocess import plan_segments

    return plan_segments(t_samples, n_traces, segments)


def _same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


# -- 1. bit-for-bit equality with the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts_are_the_restatement_bit_for_bit(engine, name):
    segments = LAYOUTS[name]
    records, weights = _plan(T, 4, segments)
    x = sr.gappy_traces(11 + len(segments), 4, T, segments)
    try:
        for second_taper in (True, False):
            for zero_phase in (True, False):
                want = sr.preprocess_segments(x, TRACE_FILTER, SOS, records, weights, zero_phase=zero_phase,
                                              second_taper=second_taper)
                assert not np.any(np.isnan(want))
                for skew in (1, 0):
                    engine.config("preproc_skew", skew)
                    got = engine.preprocess_segments(x, TRACE_FILTER, SOS, records, weights, zero_phase=zero_phase,
                                                     second_taper=second_taper, out=np.full(x.shape, np.nan))
                    assert _same_bits(got, want), (second_taper, zero_phase, skew,
                                                   float(np.nanmax(np.abs(got - want))))
    finally:
        engine.config("preproc_skew", 1)
    data = np.zeros(x.shape, dtype=bool)
    for tr, first, n in segments:
        data[tr, first:first + n] = True
    assert np.all(want[~data] == 2.0 ** -511) and np.ptp(want[data]) > 0


def test_records_in_any_order_and_the_detrend_switch(engine):
    segments = LAYOUTS["63 / 64 / 65 / 129"]
    records, weights = _plan(T, 4, segments)
    x = sr.gappy_traces(5, 4, T, segments)
    want = sr.preprocess_segments(x, TRACE_FILTER, SOS, records, weights, detrend_on=False, fill_value=-3.5)
    shuffled = records[np.random.default_rng(1).permutation(len(records))]
    got = engine.preprocess_segments(x, TRACE_FILTER, SOS, shuffled, weights, detrend=False, fill_value=-3.5)
    assert _same_bits(got, want)


# -- 2. above the LDS limit ---------------------------------------------------------------------------------------------
def test_a_segment_above_the_lds_limit_bit_for_bit(engine):
    """A segment of 20 481 samples is worked on in place in its output row, beside a 300-sample segment of the same
    trace that lives in LDS.  (The row holds 20 800 samples: 20 481 + 300 with a gap between them do not fit 20 600.)"""
    n_long, t_samples = LDS_SAMPLES + 1, 20800
    segments = [(0, 7, n_long), (0, n_long + 12, 300)]
    records, weights = _plan(t_samples, 1, segments)
    x = sr.gappy_traces(79, 1, t_samples, segments)
    tf = np.array([1], dtype=np.int32)
    want = sr.preprocess_segments(x, tf, SOS, records, weights)
    got = {}
    try:
        for skew in (1, 0):
            engine.config("preproc_skew", skew)
            got[skew] = engine.preprocess_segments(x, tf, SOS, records, weights, out=np.full(x.shape, np.nan))
            assert _same_bits(got[skew], want), (skew, float(np.nanmax(np.abs(got[skew] - want))))
    finally:
        engine.config("preproc_skew", 1)
    assert _same_bits(got[0], got[1])


# -- 3. the gap-free one-segment layout is Engine.preprocess ------------------------------------------------------------
@pytest.mark.parametrize("t_samples", [64, 301, 2049])
def test_gap_free_layout_without_second_taper_is_engine_preprocess(engine, t_samples):
    from quakemigrate_amd.preprocess import cosine_taper_sides

    x = pr.noisy_traces(23, 4, t_samples)
    records, weights = _plan(t_samples, 4, [(i, 0, t_samples) for i in range(4)])
    left, right = cosine_taper_sides(t_samples)
    assert np.array_equal(weights, np.concatenate([left, right]))
    for zero_phase in (True, False):
        want = engine.preprocess(x, TRACE_FILTER, SOS, taper=(left, right), zero_phase=zero_phase)
        got = engine.preprocess_segments(x, TRACE_FILTER, SOS, records, weights, zero_phase=zero_phase,
                                         second_taper=False)
        assert _same_bits(got, want), zero_phase
    assert np.ptp(want) > 0


# -- 4. host / device, in place -----------------------------------------------------------------------------------------
def test_host_and_device_arrays_agree_and_in_place_works(engine):
    import torch

    segments = LAYOUTS["one sample apart"]
    records, weights = _plan(T, 4, segments)
    x = sr.gappy_traces(31, 4, T, segments)
    host = engine.preprocess_segments(x, TRACE_FILTER, SOS, records, weights)
    assert _same_bits(host, sr.preprocess_segments(x, TRACE_FILTER, SOS, records, weights))
    dev = f"cuda:{engine.device}"
    d_in = torch.from_numpy(x).to(dev)
    d_out = torch.full_like(d_in, float("nan"))
    engine.preprocess_segments(d_in, TRACE_FILTER, SOS, records, weights, out=d_out)        # device -> device
    engine.synchronize()
    assert _same_bits(d_out.cpu().numpy(), host)
    assert _same_bits(d_in.cpu().numpy(), x)                                                # (the input is left alone)
    assert _same_bits(engine.preprocess_segments(d_in, TRACE_FILTER, SOS, records, weights), host)   # device -> host
    d_out.fill_(float("nan"))
    engine.preprocess_segments(x, TRACE_FILTER, SOS, records, weights, out=d_out)           # host -> device
    engine.synchronize()
    assert _same_bits(d_out.cpu().numpy(), host)
    engine.preprocess_segments(d_in, TRACE_FILTER, SOS, records, weights, out=d_in)         # in place
    engine.synchronize()
    assert _same_bits(d_in.cpu().numpy(), host)
    ms = engine.last_kernel_ms()
    assert ms is not None and ms > 0.0


# -- 5. the buffer contract on a long-lived engine ----------------------------------------------------------------------
def _sequence_calls():
    from quakemigrate_amd.preprocess import ResampleStage

    big, small = 2049, 64
    rows = np.array([0, 0, 1, 2], dtype=np.int32)
    nsta, nlta = np.array([4, 6, 5], dtype=np.int32), np.array([17, 23, 20], dtype=np.int32)
    left, right = np.linspace(0, 1, 15, endpoint=False), np.linspace(1, 0, 15, endpoint=False)

    def segments_call(t_samples, segments, seed):
        records, weights = _plan(t_samples, 4, segments)
        x = sr.gappy_traces(seed, 4, t_samples, segments)
        return lambda e: e.preprocess_segments(x, TRACE_FILTER, SOS, records, weights)

    def preprocess_call(t_samples, seed):
        x = pr.noisy_traces(seed, 4, t_samples)
        return lambda e: e.preprocess(x, TRACE_FILTER, SOS, taper=(left, right))

    def onsets_call(t_samples, seed):
        x = pr.noisy_traces(seed, 4, t_samples)
        return lambda e: e.onsets(x, rows, nsta, nlta, transform="abs", taper_pad=3, min_onset_value=0.3)[1]

    def resample_call(t_samples, seed):
        stage = ResampleStage(sampling_rate=50, raw_rate=(100.0,) * 4, n_raw=(2 * t_samples - 1,) * 4,
                              first_offset=(0.0,) * 4)
        raw = np.random.default_rng(seed).integers(-2000, 2000, size=4 * (2 * t_samples - 1)).astype(np.int32)
        return lambda e: e.resample(raw, stage, t_samples=t_samples)

    gappy_big = [(0, 5, 1000), (0, 1010, 1039), (1, 0, big), (2, 100, 1900), (3, 0, 63), (3, 64, 1985)]
    gappy_small = [(0, 0, 20), (0, 30, 34), (1, 0, small), (2, 1, 62), (3, 0, 1), (3, 2, 62)]
    # larger before smaller and the reverse, the segment call between each of the other three
    return [preprocess_call(big, 1), segments_call(small, gappy_small, 2), resample_call(big, 3),
            segments_call(big, gappy_big, 4), onsets_call(small, 5), segments_call(small, gappy_small, 6),
            preprocess_call(small, 7), segments_call(big, gappy_big, 8), resample_call(small, 9),
            onsets_call(big, 10), segments_call(T, LAYOUTS["63 / 64 / 65 / 129"], 11), preprocess_call(big, 12)]


def test_a_long_lived_engine_equals_fresh_engines(lib, engine):
    for k, call in enumerate(_sequence_calls()):
        got = np.array(call(engine))
        fresh = lib.Engine(engine.device)
        try:
            want = np.array(call(fresh))
        finally:
            fresh.close()
        assert _same_bits(got, want), k
        assert np.ptp(want) > 0, k


# -- 6. the pipeline equals the staged calls ---------------------------------------------------------------------------
N_STEPS = 7
N_ROWS = 20                                                     # the c2_mini golden's table: C2, 20 rows
TRACE_ROW = np.array(list(range(10)) + [r for r in range(10, 20) for _ in (0, 1)], dtype=np.int32)  # 30 traces
TRACE_PHASE = tuple("P" * 10 + "S" * 20)
MAX_SEGMENTS = 2 * len(TRACE_ROW)


def _stage():
    from quakemigrate_amd.preprocess import OnsetStage

    return OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 12.0, 2)},
                      sta_lta_windows={"P": (0.2, 1.0), "S": (0.3, 1.5)}, trace_row=TRACE_ROW,
                      trace_phase=TRACE_PHASE, row_phase=tuple("P" * 10 + "S" * 10), taper_pad=20, fill_gaps=True)


def _step_layout(step, t_samples):
    """Another layout every timestep: step 0 uses one segment per trace, step 1 all MAX_SEGMENTS records."""
    n = len(TRACE_ROW)
    if step == 0:
        return [(i, 0, t_samples) for i in range(n)]
    if step == 1:
        half = t_samples // 2
        return [seg for i in range(n) for seg in ((i, i % 3, half - 5 - i), (i, half + i % 7, t_samples - half - 9))]
    rng = np.random.default_rng(300 + step)
    out = []
    for i in range(n):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            out.append((i, 0, t_samples))
        elif kind == 1:
            first = int(rng.integers(1, 40))
            out.append((i, first, t_samples - first - int(rng.integers(0, 40))))
        else:
            cut = int(rng.integers(100, t_samples - 100))
            out += [(i, 0, cut), (i, cut + int(rng.integers(1, 30)), t_samples - cut - 30)]
    return out


def _signals(case, steps):
    """Gappy component traces whose bursts follow the case's arrivals."""
    t_samples = case.onsets.shape[1]
    out = []
    for k in range(steps):
        segments = _step_layout(k, t_samples)
        x = sr.gappy_traces(900 + k, len(TRACE_ROW), t_samples, segments)
        rng = np.random.default_rng(70 + k)
        for i, row in enumerate(TRACE_ROW):
            peak = int(np.argmax(case.onsets[row]))
            n = min(40, t_samples - peak)
            x[i, peak:peak + n] += 2e4 * rng.standard_normal(n) * np.exp(-np.arange(n) / 12.0)
        out.append((x, segments))
    return out


def _staged(engine, a, case, x, segments):
    records, weights = _plan(x.shape[1], x.shape[0], segments)
    f = engine.preprocess_segments(x, a["trace_filter"], a["sos"], records, weights,
                                   second_taper=a["second_taper"], fill_value=a["fill_value"])
    _, logged = engine.onsets(f, a["trace_row"], a["nsta"], a["nlta"], transform="energy", position="classic",
                              taper_pad=a["taper_pad"], min_onset_value=a["min_onset_value"])
    return engine.detect(logged, case.fsmp, case.lsmp, case.available)


@pytest.fixture(scope="module")
def pipeline_case(lib):
    from conftest import load_golden
    from quakemigrate_amd import synth

    case = synth.make_case("C2", step=0, grid=tuple(load_golden("c2_mini")["grid"]), n_samples=120)
    assert case.onsets.shape[0] == N_ROWS
    stage = _stage()
    a = stage.arrays(case.onsets.shape[1], 50)
    signals = _signals(case, N_STEPS)
    assert len(signals[0][1]) == len(TRACE_ROW) and len(signals[1][1]) == MAX_SEGMENTS
    eng = lib.Engine(0)
    eng.load_lut(case.traveltimes)
    want = [tuple(np.array(s) for s in _staged(eng, a, case, x, segments)) for x, segments in signals]
    eng.close()
    return case, stage, signals, want


@pytest.mark.parametrize("replicas", [False, True], ids=["engine", "replicas"])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_pipeline_equals_the_staged_calls(lib, pipeline_case, K, replicas):
    from quakemigrate_amd.stream import StreamingDetector

    case, stage, signals, want = pipeline_case
    t_samples = case.onsets.shape[1]
    eng = lib.EngineReplicas([0, 0]) if replicas else lib.Engine(0)
    try:
        eng.load_lut(case.traveltimes)
        if K == 2:
            eng.config("stream_pull", 0)                        # (slots this small are pulled: the copy stream as well)
        det = StreamingDetector(eng, N_ROWS, t_samples, case.fsmp, case.lsmp, case.available, depth=2,
                                steps_per_launch=K, onset_stage=stage, sampling_rate=50, max_segments=MAX_SEGMENTS)
        got = det.run(signals)                                  # (7 steps: the last slot goes out partly filled)
        det.close()
    finally:
        eng.close()
    assert len(got) == N_STEPS
    for step, (g, w) in enumerate(zip(got, want)):
        for name, gs, ws in zip(("max_coa", "max_norm_coa", "max_coa_idx"), g, w):
            assert np.array_equal(gs, ws), (step, name)
        assert np.ptp(w[0]) > 0 and np.ptp(w[1]) > 0 and np.ptp(w[2]) > 0, step     # (not flat series)


# -- 7. refusals --------------------------------------------------------------------------------------------------------
def _good_layout(n_traces, t):
    return [(0, 0, 40), (0, 50, t - 50)] + [(i, 0, t) for i in range(1, n_traces)]


def _bad_records(n_traces, t):
    """(records, weights, fill_value, text) -- every refusal of the records, each one change to a good layout of
    n_traces x t: trace 0 in two segments (records 0 and 1), every other trace in one (record 2 is trace 1's)."""
    good, w = _plan(t, n_traces, _good_layout(n_traces, t))
    assert good[:2].tolist() == [[0, 0, 40, 0, 0, 0, 2, 0], [0, 50, t - 50, 10, 0, 4, int(0.05 * (t - 50)), 0]]
    off2, m2, n_w = int(good[2, 5]), int(good[2, 6]), len(w)
    tiles = "its segments and fills do not tile the window [0, %d) exactly once" % t

    def changed(row, col, value):
        r = good.copy()
        r[row, col] = value
        return r

    fill = sr.FILL
    return [
        (good[:0], w, fill, "at least one segment is needed (got 0)"),
        (changed(1, 0, n_traces), w, fill, f"segment 1: trace {n_traces} out of range ({n_traces} traces)"),
        (changed(1, 0, -1), w, fill, f"segment 1: trace -1 out of range ({n_traces} traces)"),
        (changed(0, 2, 0), w, fill, "segment 0: n = 0, at least one sample is needed"),
        (changed(1, 3, -1), w, fill, "segment 1: a fill of -1 + 0 samples (fills are >= 0)"),
        (changed(1, 4, -2), w, fill, "segment 1: a fill of 10 + -2 samples (fills are >= 0)"),
        (changed(1, 4, 1), w, fill, f"segment 1: samples [40, {t + 1}) with their fill leave the window of {t}"),
        (changed(0, 3, 1), w, fill, f"segment 0: samples [-1, 40) with their fill leave the window of {t}"),
        (changed(0, 6, 21), np.ones(n_w + 60), fill,
         "segment 0: its taper's ramps cover 2 x 21 samples, the segment holds 40"),
        (changed(2, 5, n_w - 2 * m2 + 1), w, fill,
         f"segment 2: 2 x {m2} weights from {n_w - 2 * m2 + 1} on, {n_w} weights given"),
        (changed(2, 5, -1), w, fill, f"segment 2: 2 x {m2} weights from -1 on, {n_w} weights given"),
        (changed(2, 6, -1), w, fill, f"segment 2: 2 x -1 weights from {off2} on, {n_w} weights given"),
        (changed(0, 7, 3), w, fill, "segment 0: field 7 is 3, it must be 0"),
        (good, w, float("inf"), "fill_value inf is not finite"),
        (good, w, float("nan"), "is not finite"),
        (changed(1, 3, 9), w, fill, f"trace 0: {tiles} (a hole at sample 40)"),
        (changed(0, 4, 11), w, fill, f"trace 0: {tiles} (an overlap at sample 40)"),
        (changed(2, 2, t - 1), w, fill, f"trace 1: {tiles} (a hole at sample {t - 1})"),
        (np.delete(good, 2, axis=0), w, fill, f"trace 1: {tiles} (no segment at sample 0)"),
        (np.concatenate([good, good[2:3]]), w, fill, f"trace 1: {tiles} (an overlap at sample 0)"),
    ]


def test_engine_refusals_leave_the_output_untouched(lib, engine):
    import re

    x = pr.noisy_traces(3, 2, 100)
    tf = np.array([0, 1], dtype=np.int32)
    good, w = _plan(100, 2, _good_layout(2, 100))

    def refused(text, records=good, weights=w, fill=sr.FILL, tf=tf, sos=SOS):
        out = np.full(x.shape, 123.0)
        with pytest.raises(lib.QMHipError, match=re.escape(text)):
            engine.preprocess_segments(x, tf, sos, records, weights, fill_value=fill, out=out)
        assert np.all(out == 123.0), text

    for records, weights, fill, text in _bad_records(2, 100):
        refused("qm_engine_preprocess_segments: " + text if np.isfinite(fill) else text, records, weights, fill)
    # what qm_engine_preprocess refuses
    refused("n_sections must be in 1..8 (got 9)", sos=stable_sos(9, 2, 9))
    refused("trace 1: filter 2 out of range (2 filters)", tf=np.array([0, 2], dtype=np.int32))
    bad = SOS.copy()
    bad[1, 0, 3] = 2.0
    refused("sections must be normalised to a0 == 1", sos=bad)
    # ... and the engine still works
    got = engine.preprocess_segments(x, tf, SOS, good, w)
    assert _same_bits(got, sr.preprocess_segments(x, tf, SOS, good, w))


def test_stream_refusals_leave_the_stream_unchanged(lib, pipeline_case):
    import re

    from quakemigrate_amd.stream import StreamingDetector

    case, stage, signals, want = pipeline_case
    t_samples, n = case.onsets.shape[1], len(TRACE_ROW)
    plain = dataclasses.replace(stage, fill_gaps=False)
    logged = np.log(np.clip(case.onsets, 0.01, np.inf))
    x0, seg0 = signals[0]
    eng = lib.Engine(0)
    try:
        eng.load_lut(case.traveltimes)

        def detector(**kw):
            return StreamingDetector(eng, N_ROWS, t_samples, case.fsmp, case.lsmp, case.available, depth=2,
                                     steps_per_launch=1, sampling_rate=50, **kw)

        det = detector()                                        # no onset stage
        with pytest.raises(lib.QMHipError, match="no onset stage"):
            det.set_segment_feed(4)
        with pytest.raises(lib.QMHipError, match=re.escape("no segment feed (qm_stream_set_segment_feed)")):
            det.push_segments(x0, seg0)
        det.close()

        det = detector(onset_stage=plain)                       # an onset stage that does not fill gaps: no feed yet
        with pytest.raises(lib.QMHipError, match=re.escape("no segment feed (qm_stream_set_segment_feed)")):
            det.push_segments(x0, seg0)
        for args, text in (((0,), "max_segments must be at least 1 (got 0)"),
                           ((4, -1), "max_taper_weights must be at least 0 (got -1)"),
                           ((4, 10, 1, float("inf")), "fill_value inf is not finite")):
            with pytest.raises(lib.QMHipError, match=re.escape(text)):
                det.set_segment_feed(*args)
        det.set_segment_feed(MAX_SEGMENTS)                      # (a refused feed leaves the stream usable)
        with pytest.raises(lib.QMHipError, match="already"):
            det.set_segment_feed(MAX_SEGMENTS)
        with pytest.raises(lib.QMHipError, match=re.escape("this stream takes gappy traces")):
            det.push_signals(np.nan_to_num(x0))
        with pytest.raises(lib.QMHipError, match=re.escape("this stream takes gappy traces")):
            det.set_resample_stage({"records": np.zeros((n, 11), dtype=np.int64), "sos_lp": np.zeros((0, 1, 6)),
                                    "taper_table": np.zeros((0, 2)), "taper_weights": np.zeros(0),
                                    "t_samples": t_samples})
        # the push's own checks: nothing goes into the stream
        records, weights = _plan(t_samples, n, seg0)
        over = _plan(t_samples, n, [(i, a, b) for i in range(n) for a, b in ((0, 10), (20, 10), (40, t_samples - 40))])
        with pytest.raises(lib.QMHipError, match=re.escape(f"{3 * n} segments, the feed was set for up to "
                                                           f"{MAX_SEGMENTS} (max_segments)")):
            det.push_segments(x0, *over)
        many = np.zeros(det.max_taper_weights + 1)
        with pytest.raises(lib.QMHipError, match=re.escape(f"{len(many)} taper weights, the feed was set for up to "
                                                           f"{det.max_taper_weights} (max_taper_weights)")):
            det.push_segments(x0, records, many)
        hole = records.copy()
        hole[3, 4] = 0                                          # (trace 3's only record no longer reaches the end)
        hole[3, 2] -= 1
        with pytest.raises(lib.QMHipError, match=re.escape("qm_stream_push_segments: trace 3: its segments and fills "
                                                           "do not tile the window")):
            det.push_segments(x0, hole, weights)
        field = records.copy()
        field[0, 7] = 1
        with pytest.raises(lib.QMHipError, match=re.escape("segment 0: field 7 is 1, it must be 0")):
            det.push_segments(x0, field, weights)
        for bad, bad_w, fill, text in _bad_records(n, t_samples):  # what the engine call refuses, by the same text
            if np.isfinite(fill):                               # (the fill value is the feed's, refused above)
                with pytest.raises(lib.QMHipError, match=re.escape("qm_stream_push_segments: " + text)):
                    det.push_segments(x0, bad, bad_w)
        assert det.pending() == (0, 0)
        # ... and the stream is what it was: its steps are the staged calls'
        for x, segments in signals[:2]:
            assert det.push_segments(x, segments)
        with pytest.raises(lib.QMHipError, match=re.escape("this stream takes gappy traces (qm_stream_push_segments): "
                                                           "one stream, one kind of input")):
            det.push(logged)
        for step in range(2):
            got = det.pop(1)
            for name, gs, ws in zip(("max_coa", "max_norm_coa", "max_coa_idx"), got, want[step]):
                assert np.array_equal(gs[0], ws), (step, name)
        det.close()

        det = detector(onset_stage=stage)                       # log-onsets first: the feed's push is refused by name
        assert det.push(logged)
        with pytest.raises(lib.QMHipError, match=re.escape("this stream takes log-onsets (qm_stream_push): one stream, "
                                                           "one kind of input")):
            det.push_segments(x0, seg0)
        det.pop(1)
        det.close()

        det = detector(onset_stage=plain)                       # the feed after a push
        assert det.push_signals(np.nan_to_num(x0))
        with pytest.raises(lib.QMHipError, match="before the first push"):
            det.set_segment_feed(4)
        det.pop(1)
        det.close()
        with pytest.raises(ValueError, match="does not fill gaps"):
            detector(onset_stage=plain, max_segments=4)
    finally:
        eng.close()


# -- 8. continuous_compute ----------------------------------------------------------------------------------------------
RATE = 50
PRE_PAD, TIMESTEP = 2.0, 3.0
CC_STEPS = 5
CC_ROW = np.array([0, 1, 2, 3, 3, 4, 4, 5, 5], dtype=np.int32)          # 6 rows (3 P, 3 S), 9 traces
OVER_STEP = 2                                                           # the timestep with more than 4 x 9 segments


class _Data:
    def __init__(self, starttime, signals, segments):
        self.starttime, self.signals, self.segments = starttime, signals, segments


class _OnsetData:
    def __init__(self, availability):
        self.sampling_rate, self.availability = RATE, availability


def _cc_layout(step, t_samples):
    n = len(CC_ROW)
    if step == OVER_STEP:                                       # 5 segments per trace: 45 > 36
        w = t_samples // 5
        return [(i, j * w + 1, w - 2) for i in range(n) for j in range(5)]
    out = []
    for i in range(n):
        if (i + step) % 3 == 0:
            out += [(i, 0, 60 + i), (i, 70 + i + step, t_samples - 70 - i - step)]
        elif (i + step) % 3 == 1:
            out.append((i, 3 + step, t_samples - 10 - step))
        else:
            out.append((i, 0, t_samples))
    return out


class _Archive:
    """Gappy component traces per window, one event per timestep whose bursts follow the table's arrivals."""

    def __init__(self, case):
        self.tt = case.traveltimes.reshape(-1, case.traveltimes.shape[-1])

    def read_waveform_data(self, w_beg, w_end):
        t_samples = int(round((w_end - w_beg) * RATE)) + 1
        step = int(round((w_beg + PRE_PAD) / TIMESTEP))
        segments = _cc_layout(step, t_samples)
        x = sr.gappy_traces(4000 + step, len(CC_ROW), t_samples, segments)
        rng = np.random.default_rng(5000 + step)
        node = int(rng.integers(0, self.tt.shape[0]))
        t0 = int(PRE_PAD * RATE) + int(rng.integers(20, int(TIMESTEP * RATE) - 20))
        for i, row in enumerate(CC_ROW):
            at = t0 + int(self.tt[node, row])
            n = min(50, t_samples - at)
            x[i, at:at + n] += 3e4 * rng.standard_normal(n) * np.exp(-np.arange(n) / 15.0)
        return _Data(w_beg, x, segments)


class _HostPlugin:
    """calculate_onsets on the host: the per-segment restatement in the device's order, then the STA/LTA of the staged
    call on an engine of its own -- the bits the pipeline's onset kernels see."""

    def __init__(self, lib, stage, t_samples):
        self.stage, self.a = stage, stage.arrays(t_samples, RATE)
        self.availability = {f"ST{r % 3}_{'PS'[r // 3]}": 1 for r in range(6)}
        self.helper = lib.Engine(0)
        self.raw, self.steps = [], []

    def calculate_onsets(self, data):
        a = self.a
        records, weights = _plan(data.signals.shape[1], data.signals.shape[0], data.segments)
        f = sr.preprocess_segments(data.signals, a["trace_filter"], a["sos"], records, weights)
        raw, _ = self.helper.onsets(f, a["trace_row"], a["nsta"], a["nlta"], transform="energy", position="classic",
                                    taper_pad=a["taper_pad"], min_onset_value=a["min_onset_value"])
        self.raw.append(np.array(raw))
        self.steps.append(int(round((data.starttime + PRE_PAD) / TIMESTEP)))
        return raw, _OnsetData(self.availability)


class _DevicePlugin(_HostPlugin):
    def device_stage(self, data):
        return data.signals, self.stage, _OnsetData(self.availability), data.segments


class _Lut:
    def __init__(self, case):
        self.case = case

    def serve_traveltimes(self, sampling_rate, availability):
        return self.case.traveltimes

    def index2coord(self, idx, unravel=True):
        return np.column_stack(np.unravel_index(np.asarray(idx), self.case.grid))


class _Sink:
    written = False

    def __init__(self):
        self.steps = []

    def append(self, time, max_coa, max_coa_n, coord, ucf):
        self.steps.append((time, np.array(max_coa), np.array(max_coa_n), np.array(coord)))

    def empty(self, *args):
        raise AssertionError("no timestep of this archive is empty")

    def write(self):
        self.written = True


def test_continuous_compute_segments_equal_the_host_plugin_path(lib, oracle):
    """
    The host path conditions every segment with the restatement (the device's bits) and takes its STA/LTA from the
    staged onset call, so both runs stack the same onset functions up to the last bit of their logarithm (the host path
    logs with NumPy).  Values within the project's 1e-6 relative contract; node indices equal on every sample where the
    host path's two largest node values differ by more than 1e-9 relative -- at most 1 % of the samples may lie under
    that gap (asserted on the host path alone, computed with the oracle from the host plugin's onsets).  The timestep
    with 45 segments (more than 4 x 9) goes through calculate_onsets in the device run as well; its neighbours do not.
    """
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd import synth
    from quakemigrate_amd.preprocess import OnsetStage
    from quakemigrate_amd.scan import MigrationScan

    case = synth.make_case("C3", step=2, grid=(16, 16, 16), rows=6, n_samples=int(TIMESTEP * RATE))
    fsmp, lsmp = int(PRE_PAD * RATE), case.lsmp
    post_pad = lsmp / RATE
    t_samples = fsmp + int(TIMESTEP * RATE) + lsmp
    stage = OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 12.0, 2)},
                       sta_lta_windows={"P": (0.2, 1.0), "S": (0.3, 1.5)}, trace_row=CC_ROW,
                       trace_phase=tuple("PPPSSSSSS"), row_phase=tuple("PPPSSS"), taper_pad=10, fill_gaps=True)
    runs = {}
    for name, kind in (("host", _HostPlugin), ("device", _DevicePlugin)):
        plugin = kind(lib, stage, t_samples)
        eng = lib.Engine(0)
        try:
            sink = _Sink()
            scan = MigrationScan(_Lut(case), plugin, PRE_PAD, post_pad, engine=eng)
            rows = scan.continuous_compute(_Archive(case), 0.0, CC_STEPS, TIMESTEP, RATE, sink,
                                           steps_per_launch=2, depth=2)
        finally:
            eng.close()
            plugin.helper.close()
        assert len(rows) == CC_STEPS and len(sink.steps) == CC_STEPS and sink.written
        runs[name] = (sink.steps, plugin)
    assert runs["host"][1].steps == list(range(CC_STEPS))
    assert runs["device"][1].steps == [OVER_STEP]               # (only the over-full timestep made host onsets)
    under = total = 0
    for step, (h, d) in enumerate(zip(runs["host"][0], runs["device"][0])):
        assert h[0] == d[0]
        assert np.ptp(h[1]) > 0
        np.testing.assert_allclose(d[1], h[1], rtol=1e-6)
        np.testing.assert_allclose(d[2], h[2], rtol=1e-6)
        vol = oracle.c_migrate(runs["host"][1].raw[step], case.traveltimes, fsmp, lsmp, 6, threads=4)
        top = np.partition(vol.reshape(-1, vol.shape[-1]), -2, axis=0)[-2:]
        clear = (top[1] - top[0]) > 1e-9 * top[1]
        under += int(np.sum(~clear))
        total += clear.size
        assert np.array_equal(d[3][clear], h[3][clear]), step
    print(f"samples under the 1e-9 gap on the host path: {under} of {total}")
    assert under <= 0.01 * total
