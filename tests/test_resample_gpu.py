# -*- coding: utf-8 -*-
"""
The resampling stage on the GPU (qm_engine_resample, qm_stream_set_resample_stage / qm_stream_push_raw) against its
NumPy restatement, tests/resample_ref.py.

Inputs are seeded Gaussian noise of amplitude ~1e3 on a ramp and an offset, rounded where they are int32.  The
upsampling alone and the decimation without its detrend are held to the restatement's bits -- which are NumPy's and
scipy.signal.sosfilt's (tests/test_resample_host.py); the whole stage to a bound derived from the detrend sums'
rounding and the low-pass's l1 gain.
"""

import ctypes

import numpy as np
import pytest

import preprocess_ref as pr
import resample_ref as rr

pytestmark = pytest.mark.gpu

LDS_SAMPLES = 20480


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


def _arrays(records, T, sos=None, table=None, weights=None, detrend=0, total=None):
    records = np.array(records, dtype=np.int64).reshape(-1, 11)
    return {"total_raw_samples": int(np.max(records[:, 0] + records[:, 1])) if total is None else total,
            "records": records,
            "sos_lp": np.zeros((0, 1, 6)) if sos is None else np.asarray(sos, dtype=np.float64),
            "taper_table": np.zeros((0, 2), dtype=np.int32) if table is None else np.array(table, dtype=np.int32),
            "taper_weights": np.zeros(0) if weights is None else np.asarray(weights, dtype=np.float64),
            "detrend": detrend, "t_samples": T}


def _want(raw, a):
    return rr.resample(raw, a["records"], a["sos_lp"], a["taper_table"], a["taper_weights"], a["t_samples"],
                       detrend_on=bool(a["detrend"]))


def _bound(raw, a, i):
    """||h||_1^2 * 4 n_up 2^-53 max|x| for trace i: h the restated low-pass's response to a unit impulse over n_up
    samples, x the kept series (the derivation of tests/test_preprocess_gpu.py: the detrend's sums carry at most
    n_up eps relative error in any order, and a linear filter run twice amplifies a perturbation of its input by at
    most its l1 gain squared).  Returns (tolerance, gain squared, the record as a dict)."""
    r = dict(zip(rr.FIELDS, (int(v) for v in a["records"][i])))
    x = np.asarray(raw)[r["raw_offset"]:r["raw_offset"] + r["n_raw"]]
    kept = rr.kept_series(x, r["up"], r["pad_left"], r["pad_right"], r["up_first"], r["n_up"])
    gain = pr.impulse_l1(a["sos_lp"][r["lowpass"]], r["n_up"]) ** 2
    return gain * 4 * r["n_up"] * 2.0 ** -53 * float(np.max(np.abs(kept))), gain, r


NO_TAPER = [[0, 0]]


# -- 1. upsampling alone: NumPy's bits -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.float64], ids=["int32", "float64"])
@pytest.mark.parametrize("u", [2, 5])
def test_upsample_alone_is_numpys_bit_for_bit(engine, u, dtype):
    for n_raw in (1, 2, 3, 64, 65, 601):
        x = rr.raw_traces(100 * u + n_raw, [n_raw], dtype)[0]
        whole = (n_raw - 1) * u + 1
        for pad in (0, 1, u - 1):
            for up_first in (0, min(2, whole + 2 * pad - 1)):
                T = whole + 2 * pad - up_first
                a = _arrays([rr.record(0, n_raw, up=u, pad_left=pad, pad_right=pad, up_first=up_first)], T)
                got = engine.resample(x, a)
                assert got.shape == (1, T) and np.array_equal(got, _want(x, a)), (n_raw, pad, up_first)
    # the restatement's interior is the expression as NumPy evaluates it on whole arrays
    x = rr.raw_traces(7, [601], dtype)[0]
    want = np.zeros(600 * u + 1)
    want[::u] = x
    for i in range(1, u):
        want[i::u] = (i / u) * x[1:] + ((u - i) / u) * x[:-1]
    got = engine.resample([x], _arrays([rr.record(0, 601, up=u)], len(want)))
    assert np.array_equal(got[0], want)


# -- 2. decimation without the detrend: the restatement's bits -----------------------------------------------------
@pytest.mark.parametrize("n_sections", [1, 2, 8])
def test_decimation_without_detrend_is_the_restatement_bit_for_bit(engine, n_sections):
    sos = rr.stable_sos(n_sections, 2, n_sections)
    lowpass = (0, 1, 0)                                         # 3 traces, 2 low-passes
    try:
        for n_up in (2, 63, 64, 65, 129, 601, 4099):
            raw, offsets = rr.pack(rr.raw_traces(1000 * n_sections + n_up, [n_up] * 3), np.float64)
            x = raw.reshape(3, n_up)
            m = n_up // 20
            rng = np.random.default_rng(n_up)
            weights = np.concatenate([np.sort(rng.uniform(0, 1, m)), np.sort(rng.uniform(0, 1, m))[::-1]])
            # the filtered series once per length (the traces of one low-pass side by side), decimated below
            full = np.empty_like(x)
            for f in (0, 1):
                rows = [i for i in range(3) if lowpass[i] == f]
                full[rows] = rr.lowpassed(x[rows], sos[f], weights[:m], weights[m:], detrend_on=False)
            for d in (2, 4, 5):
                n_dec = -(-n_up // d)                           # (n_up < d: one sample)
                for out_first in sorted({0, min(3, n_dec - 1)}):
                    T = n_dec - out_first
                    recs = [rr.record(int(offsets[i]), n_up, dec=d, lowpass=lowpass[i], out_first=out_first)
                            for i in range(3)]
                    a = _arrays(recs, T, sos, [[0, m]], weights)
                    want = full[:, ::d][:, out_first:out_first + T]
                    got = {}
                    for skew in (1, 0):
                        engine.config("preproc_skew", skew)
                        got[skew] = engine.resample(raw, a)
                        assert np.array_equal(got[skew], want), (n_up, d, out_first, skew,
                                                                 float(np.max(np.abs(got[skew] - want))))
                    assert got[0].tobytes() == got[1].tobytes(), (n_up, d, out_first)
            if n_up == 601:                                     # ... and the pieces above are the whole restatement
                assert np.array_equal(_want(raw, a), want)
    finally:
        engine.config("preproc_skew", 1)


# -- 3. above the LDS limit ----------------------------------------------------------------------------------------
def test_kept_series_above_and_at_the_lds_limit(engine):
    """One launch, two traces: 20 481 kept samples (global scratch) and 20 480 (LDS)."""
    lengths = [LDS_SAMPLES + 1, LDS_SAMPLES]
    sos = rr.stable_sos(78, 2, 1)
    traces = rr.raw_traces(78, lengths, np.int32)
    raw, offsets = rr.pack(traces, np.int32)
    T = LDS_SAMPLES // 2
    recs = [rr.record(int(offsets[0]), lengths[0], dec=2, lowpass=1, out_first=1),
            rr.record(int(offsets[1]), lengths[1], dec=2, lowpass=0)]
    a = _arrays(recs, T, sos, NO_TAPER)
    want = _want(raw, a)
    try:
        for skew in (1, 0):
            engine.config("preproc_skew", skew)
            got = engine.resample(raw, a)
            assert np.array_equal(got, want), (skew, float(np.max(np.abs(got - want))))
    finally:
        engine.config("preproc_skew", 1)


@pytest.mark.parametrize("n_up", [1, 2, 64, 65, 301, LDS_SAMPLES + 1])
def test_decimation_with_detrend_is_the_device_order_restatement_bit_for_bit(engine, n_up):
    """One decimating record with the detrend on: its sums restated in the device's order
    (preprocess_ref.detrend_device_order), then the bit-level taper and low-pass.  n_up = 1: the line's slope is
    guarded (sxx == 0); 20 481: the kept series lives in global scratch."""
    sos = rr.stable_sos(n_up, 2, 2)
    x = rr.raw_traces(500 + n_up, [n_up])[0]
    m = n_up // 20
    rng = np.random.default_rng(n_up)
    weights = np.concatenate([np.sort(rng.uniform(0, 1, m)), np.sort(rng.uniform(0, 1, m))[::-1]])
    d = 2
    a = _arrays([rr.record(0, n_up, dec=d, lowpass=1)], -(-n_up // d), sos, [[0, m]], weights, detrend=1)
    want = rr.lowpassed(x, sos[1], weights[:m], weights[m:], device_order=True)[None, ::d]
    try:
        for skew in (1, 0):
            engine.config("preproc_skew", skew)
            got = engine.resample(x, a)
            assert np.array_equal(got, want), (skew, float(np.max(np.abs(got - want))))
    finally:
        engine.config("preproc_skew", 1)


# -- 4. the whole stage --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [301, 1033])
def test_whole_stage_against_the_restatement(engine, T):
    """
    u = 5 then d = 4 (40 Hz to 50 Hz) and d = 2 alone (100 Hz), with the detrend and 5 % cosine tapers, as
    ``ResampleStage`` plans them (T = 1033: the 40 Hz traces end 0.6 raw samples inside the window and are padded).
    Tolerance: ``_bound``.  The figures are printed before they are asserted (run with ``-s``).
    Traces 2 and 3 are pure ramps plus an offset: their output, what the detrend leaves of them, must lie under the
    same bound.  That holds for a ramp; a ramp with constant pads behind it is a ramp with a kink, which a detrend
    does not remove, so the padded 40 Hz ramp of T = 1033 is held to the restatement only and its residue printed.
    The 100 Hz ramp (both T) and the unpadded 40 Hz ramp (T = 301) are asserted.
    """
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import ResampleStage

    n40, n100 = (T - 1) * 4 // 5 + 1, 2 * (T - 1) + 1
    stage = ResampleStage(50, [40, 100, 40, 100], [n40, n100, n40, n100], [0.0] * 4, upfactor=5)
    a = stage.arrays(T)
    traces = rr.raw_traces(T, stage.n_raw)
    traces[2] = 0.75 * np.arange(n40, dtype=np.float64) - 4321.0       # pure ramps plus offset: nothing is left
    traces[3] = -0.5 * np.arange(n100, dtype=np.float64) + 1234.0
    raw, _ = rr.pack(traces, np.float64)
    want = _want(raw, a)
    got = engine.resample(traces, stage, t_samples=T)
    assert got.shape == (4, T)
    for i in range(4):
        tol, gain, r = _bound(raw, a, i)
        assert r["dec"] == (4, 2)[i % 2] and r["up"] == (5, 1)[i % 2]
        err = float(np.max(np.abs(got[i] - want[i])))
        print(f"T = {T}, trace {i} (u = {r['up']}, d = {r['dec']}, n_up = {r['n_up']}, pads {r['pad_left']} + "
              f"{r['pad_right']}): max |device - restatement| = {err:.3e}, tolerance {tol:.3e} (l1 gain squared "
              f"{gain:.3f})")
        assert err <= tol
        if i >= 2:
            ramp = float(np.max(np.abs(got[i])))
            print(f"    ramp residue {ramp:.3e}")
            # (the constant pad behind a ramp that ends early is a kink, not a ramp: only the unpadded one vanishes)
            if r["pad_left"] == 0 and r["pad_right"] == 0:
                assert ramp <= tol


# -- 5. ragged traces in one call; device-resident in and out; scratch reuse ---------------------------------------
def _ragged(T, seed, dtype):
    """Five traces, five (length, u, d) combinations: a pass-through slice, d = 2, u = 5 with pads then d = 4,
    u = 2 alone with a pad, d = 5 from the second decimated sample on."""
    n2 = 2 * T + 1                                              # d = 2: ceil(n2 / 2) = T + 1, out_first = 1
    n54 = (4 * T - 3 - 3) // 5 + 2                              # u = 5, pads 2 + 1, d = 4
    n_u2 = (T + 1) // 2 + 1                                     # u = 2, pad 1: 2 (n - 1) + 2 >= T + 1
    n5 = 5 * T + 2                                              # d = 5: ceil(n5 / 5) = T + 1
    lengths = [T + 3, n2, n54, n_u2, n5]
    traces = rr.raw_traces(seed, lengths, dtype)
    raw, off = rr.pack(traces, dtype)
    sos = rr.stable_sos(seed, 2, 1)
    recs = [rr.record(int(off[0]), lengths[0], up_first=2, n_up=T),
            rr.record(int(off[1]), n2, dec=2, lowpass=0, taper=0, out_first=1),
            rr.record(int(off[2]), n54, up=5, pad_left=2, pad_right=1, up_first=1, dec=4, lowpass=1, taper=1),
            rr.record(int(off[3]), n_u2, up=2, pad_left=1, up_first=1, n_up=T),
            rr.record(int(off[4]), n5, dec=5, lowpass=1, taper=2, out_first=1)]
    tapers, weights = [], []
    for rec in (recs[1], recs[2], recs[4]):
        m = rec[6] // 20
        tapers.append([sum(len(w) for w in weights), m])
        weights += [np.linspace(0, 1, m, endpoint=False), np.linspace(1, 0, m, endpoint=False)]
    assert -(-recs[2][6] // 4) >= T
    return traces, raw, _arrays(recs, T, sos, tapers, np.concatenate(weights), detrend=1, total=len(raw))


@pytest.mark.parametrize("dtype", [np.int32, np.float64], ids=["int32", "float64"])
def test_ragged_traces_device_resident_and_a_reused_engine(lib, engine, dtype):
    import torch

    for k, T in enumerate((64, 301, 33)):                       # growing, then shrinking: the scratch is reused
        traces, raw, a = _ragged(T, 40 + k, dtype)
        host = engine.resample(raw, a)
        assert np.array_equal(engine.resample(traces, a), host)         # a list of traces is the packed array
        want = _want(raw, a)
        assert np.array_equal(host[[0, 3]], want[[0, 3]])               # (no filter: equal bits)
        for i in (1, 2, 4):
            tol, _, r = _bound(raw, a, i)
            err = float(np.max(np.abs(host[i] - want[i])))
            print(f"T = {T}, trace {i} (u = {r['up']}, d = {r['dec']}): max |device - restatement| = {err:.3e}, "
                  f"tolerance {tol:.3e}")
            assert err <= tol
        d_in = torch.from_numpy(raw).to(f"cuda:{engine.device}")
        d_out = torch.full((5, T), -7.0, dtype=torch.float64, device=d_in.device)
        engine.resample(d_in, a, out=d_out)
        engine.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), host), T
        assert engine.last_kernel_ms() > 0.0
        fresh = lib.Engine(engine.device)
        try:
            assert np.array_equal(fresh.resample(raw, a), host), T
        finally:
            fresh.close()


# -- 6. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(lib, engine):
    T = 50
    traces, raw, good = _ragged(T, 3, np.float64)
    out = np.full((5, T), -7.0)

    def refused(match, a=None, raw_=raw, exc=None, **changes):
        a = dict(good if a is None else a, **changes)
        with pytest.raises(exc or lib.QMHipError, match=match):
            engine.resample(raw_, a, out=out)
        assert np.all(out == -7.0), match

    def with_field(trace, field, value):
        recs = good["records"].copy()
        recs[trace, rr.FIELDS.index(field)] = value
        return recs

    refused("n_raw", records=with_field(1, "n_raw", 0))
    refused("leave the raw buffer", records=with_field(4, "n_raw", good["records"][4, 1] + 1))
    refused("factors of at least 1", records=with_field(2, "up", 0))
    refused("factors of at least 1", records=with_field(1, "dec", 0))
    refused("pads go with an upsampling", records=with_field(1, "pad_left", 1))
    refused("pads go with an upsampling", records=with_field(0, "pad_right", 2))
    refused("kept slice", records=with_field(0, "up_first", 4))
    refused("kept slice", records=with_field(3, "n_up", good["records"][3, 6] + 2))
    refused("kept slice", records=with_field(3, "up_first", -1))
    refused("decimated ones", records=with_field(1, "out_first", 2))
    refused("decimated ones", records=with_field(0, "out_first", 1))
    refused("n_sections_lp", sos_lp=rr.stable_sos(9, 2, 9))
    refused("n_sections_lp", sos_lp=np.zeros((2, 0, 6)))
    bad = good["sos_lp"].copy()
    bad[1, 0, 3] = 2.0
    refused("a0", sos_lp=bad)
    refused("low-pass 2 out of range", records=with_field(2, "lowpass", 2))
    refused("low-pass -1 out of range", records=with_field(1, "lowpass", -1))
    refused("taper 3 out of range", records=with_field(4, "taper", 3))
    table = good["taper_table"].copy()
    table[0, 1] = good["records"][1, 6] // 2 + 1
    refused("ramps cover", taper_table=table, taper_weights=np.ones(4 * T))
    refused("weights given", taper_table=table)                 # (a taper that leaves its weights)
    refused("empty input", records=np.zeros((0, 11), dtype=np.int64))
    refused("empty input", t_samples=0)
    refused("int32 or float64", raw_=raw.astype(np.float32), exc=TypeError)
    # straight through the C ABI: NULL arguments and a raw dtype that is neither
    r, s, t, w, detrend, _, total = lib.resample_arrays(good)
    args = lambda raw_p, code, out_p: (engine._h, raw_p, code, 0, total, 5, r.reshape(-1), s.reshape(-1), 2, 1,  # noqa: E731
                                       detrend, t.reshape(-1), len(t), w, len(w), T, out_p, 0)
    p_raw, p_out = raw.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    assert lib.qmlib.qm_engine_resample(*args(p_raw, 2, p_out)) != 0
    assert b"raw_dtype 2" in lib.qmlib.qm_last_error()
    assert lib.qmlib.qm_engine_resample(*args(None, 1, p_out)) != 0
    assert b"NULL" in lib.qmlib.qm_last_error()
    assert lib.qmlib.qm_engine_resample(*args(p_raw, 1, None)) != 0
    assert b"NULL" in lib.qmlib.qm_last_error()
    assert lib.qmlib.qm_engine_resample(None, *args(p_raw, 1, p_out)[1:]) != 0
    assert np.all(out == -7.0)
    assert lib.qmlib.qm_engine_resample(*args(p_raw, 1, p_out)) == 0       # (and the good call goes through)
    assert np.array_equal(out, engine.resample(raw, good))


# -- 7. the pipeline equals the staged calls -------------------------------------------------------------------------
N_STEPS = 7
TRACE_ROW = np.array([0, 1, 2, 3, 3, 4, 4, 5, 5], dtype=np.int32)       # 6 rows (3 P, 3 S), 9 traces
TRACE_PHASE = tuple("PPPSSSSSS")
RAW_RATE = (50, 100, 40, 100, 50, 40, 100, 40, 50)                      # pass-through, d = 2, u = 5 then d = 4
SCAN_RATE = 50


def _stages(T):
    from quakemigrate_amd.preprocess import OnsetStage, ResampleStage

    onset = OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 12.0, 2)},
                       sta_lta_windows={"P": (0.2, 1.0), "S": (0.3, 1.5)}, trace_row=TRACE_ROW,
                       trace_phase=TRACE_PHASE, row_phase=tuple("PPPSSS"), taper_pad=20)
    n_raw = [(T - 1) * r // SCAN_RATE + 1 for r in RAW_RATE]
    return onset, ResampleStage(SCAN_RATE, RAW_RATE, n_raw, [0.0] * len(RAW_RATE), upfactor=5)


def _raw_steps(case, resample, steps):
    """int32 raw traces whose bursts follow the case's arrivals: noise ~1e3 on a ramp and an offset."""
    out = []
    for k in range(steps):
        traces = rr.raw_traces(900 + 31 * k, resample.n_raw)
        rng = np.random.default_rng(70 + k)
        for i, (row, rate) in enumerate(zip(TRACE_ROW, RAW_RATE)):
            peak = int(np.argmax(case.onsets[row])) * rate // SCAN_RATE
            n = min(40 * rate // SCAN_RATE, len(traces[i]) - peak)
            traces[i][peak:peak + n] += 2e4 * rng.standard_normal(n) * np.exp(-np.arange(n) * SCAN_RATE / (12.0 * rate))
        out.append([np.rint(t).astype(np.int32) for t in traces])
    return out


@pytest.fixture(scope="module")
def pipeline_case(lib):
    from quakemigrate_amd import synth

    case = synth.make_case("C3", step=1, grid=(16, 16, 16), rows=6, n_samples=120)
    T = case.onsets.shape[1]
    onset, resample = _stages(T)
    raws = _raw_steps(case, resample, N_STEPS)
    eng = lib.Engine(0)
    signals = [eng.resample(raw, resample, t_samples=T) for raw in raws]
    eng.close()
    assert np.ptp(signals[0][2]) > 0
    return case, onset, resample, raws, signals


@pytest.mark.parametrize("replicas", [False, True], ids=["engine", "replicas"])
@pytest.mark.parametrize("K", [1, 3])
def test_push_raw_equals_resample_then_push_signals(lib, pipeline_case, K, replicas):
    from quakemigrate_amd.stream import StreamingDetector

    case, onset, resample, raws, signals = pipeline_case
    T = case.onsets.shape[1]
    eng = lib.EngineReplicas([0, 0]) if replicas else lib.Engine(0)
    try:
        eng.load_lut(case.traveltimes)
        if K == 3:
            eng.config("stream_pull", 0)                        # (slots this small are pulled: the copy stream as well)
        kw = dict(depth=2, steps_per_launch=K, onset_stage=onset, sampling_rate=SCAN_RATE)
        det = StreamingDetector(eng, 6, T, case.fsmp, case.lsmp, case.available, resample_stage=resample, **kw)
        got = det.run(raws)                                     # (7 steps: the last slot goes out partly filled)
        det.close()
        det = StreamingDetector(eng, 6, T, case.fsmp, case.lsmp, case.available, **kw)
        want = det.run(signals)
        det.close()
    finally:
        eng.close()
    assert len(got) == N_STEPS and len(want) == N_STEPS
    for step, (g, w) in enumerate(zip(got, want)):
        for name, gs, ws in zip(("max_coa", "max_norm_coa", "max_coa_idx"), g, w):
            assert np.array_equal(gs, ws), (step, name)
    assert np.ptp(want[0][0]) > 0                               # (not a flat series)


@pytest.fixture(scope="module")
def other_resamples(lib):
    """The ragged float64 record sets of test_ragged_traces_device_resident_and_a_reused_engine, each with its result
    on an engine of its own."""
    out = []
    for k, T in enumerate((64, 301, 33)):
        _, raw, a = _ragged(T, 40 + k, np.float64)
        fresh = lib.Engine(0)
        try:
            out.append((raw, a, fresh.resample(raw, a)))
        finally:
            fresh.close()
    return out


@pytest.mark.parametrize("replicas", [False, True], ids=["engine", "replicas"])
def test_a_stream_and_its_engines_resample_calls_keep_their_own_stage(lib, pipeline_case, other_resamples, replicas):
    """The stream's resampling stage (int32 raw traces) and the stage of the engine's own resample calls (other
    records, float64) are two sets of device arrays: calls between the pushes change nothing in the stream, nor the
    stream in them.  On replicas the calls run on the lead, which is lane 0's engine."""
    from quakemigrate_amd.stream import StreamingDetector

    case, onset, resample, raws, signals = pipeline_case
    T = case.onsets.shape[1]
    between = []
    eng = lib.EngineReplicas([0, 0]) if replicas else lib.Engine(0)
    try:
        eng.load_lut(case.traveltimes)

        def feed():
            for k, step in enumerate(raws):
                yield step
                raw, a, _ = other_resamples[k % 3]              # (after step k's push, before the next)
                between.append((k % 3, eng.resample(raw, a)))

        kw = dict(depth=2, steps_per_launch=2, onset_stage=onset, sampling_rate=SCAN_RATE)
        det = StreamingDetector(eng, 6, T, case.fsmp, case.lsmp, case.available, resample_stage=resample, **kw)
        got = det.run(feed())
        det.close()
        det = StreamingDetector(eng, 6, T, case.fsmp, case.lsmp, case.available, **kw)
        want = det.run(signals)
        det.close()
    finally:
        eng.close()
    assert len(got) == N_STEPS and len(want) == N_STEPS and len(between) == N_STEPS
    for step, (g, w) in enumerate(zip(got, want)):
        for name, gs, ws in zip(("max_coa", "max_norm_coa", "max_coa_idx"), g, w):
            assert np.array_equal(gs, ws), (step, name)
    for step, (which, out) in enumerate(between):
        assert np.array_equal(out, other_resamples[which][2]), (step, which)
    assert np.ptp(want[0][0]) > 0                               # (not a flat series)


def test_pipeline_order_errors(lib, pipeline_case):
    from quakemigrate_amd.stream import StreamingDetector

    case, onset, resample, raws, signals = pipeline_case
    T = case.onsets.shape[1]
    packed = np.concatenate(raws[0])
    logged = np.log(np.clip(case.onsets, 0.01, np.inf))
    for replicas in (False, True):
        eng = lib.EngineReplicas([0, 0]) if replicas else lib.Engine(0)
        try:
            eng.load_lut(case.traveltimes)

            def detector(**kw):
                return StreamingDetector(eng, 6, T, case.fsmp, case.lsmp, case.available, depth=2, steps_per_launch=1,
                                         **kw)

            det = detector()                                    # no onset stage
            with pytest.raises(lib.QMHipError, match="no onset stage"):
                det.set_resample_stage(resample)
            with pytest.raises(lib.QMHipError, match="no resampling stage"):
                det.push_raw(raws[0])                           # (a list of ragged traces: refused before it is packed)
            assert lib.qmlib.qm_stream_push_raw(det._h, packed.ctypes.data_as(ctypes.c_void_p)) != 0
            assert b"no resampling stage" in lib.qmlib.qm_last_error()      # (the library's refusal itself)
            det.close()

            det = detector(onset_stage=onset, sampling_rate=SCAN_RATE)      # the stage after a push
            assert det.push_signals(signals[0])
            with pytest.raises(lib.QMHipError, match="before the first push"):
                det.set_resample_stage(resample)
            with pytest.raises(lib.QMHipError, match="no resampling stage"):
                det.push_raw(packed)
            det.pop(1)
            det.close()

            det = detector(onset_stage=onset, sampling_rate=SCAN_RATE, resample_stage=resample)
            with pytest.raises(lib.QMHipError, match="already"):            # the stage twice
                det.set_resample_stage(resample)
            assert det.push_raw(raws[0])                        # raw first, then signals or log-onsets
            with pytest.raises(lib.QMHipError, match="one kind of input"):
                det.push_signals(signals[0])
            with pytest.raises(lib.QMHipError, match="one kind of input"):
                det.push(logged)
            det.pop(1)
            det.close()

            det = detector(onset_stage=onset, sampling_rate=SCAN_RATE, resample_stage=resample)
            assert det.push(logged)                             # log-onsets first, then raw
            with pytest.raises(lib.QMHipError, match="one kind of input"):
                det.push_raw(packed)
            det.pop(1)
            det.close()

            det = detector(onset_stage=onset, sampling_rate=SCAN_RATE)
            a = resample.arrays(T)                              # another shape than the onset stage's
            with pytest.raises(lib.QMHipError, match="the onset stage takes"):
                det.set_resample_stage(dict(a, records=a["records"][:8]))
            bad = a["records"].copy()
            bad[1, rr.FIELDS.index("dec")] = 0
            with pytest.raises(lib.QMHipError, match="factors of at least 1"):
                det.set_resample_stage(dict(a, records=bad))
            det.set_resample_stage(a, np.float64)               # (a refused stage leaves the stream usable)
            assert det.push_raw(packed.astype(np.float64))
            det.flush()
            det.pop(1)
            det.close()
        finally:
            eng.close()
