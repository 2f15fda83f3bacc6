# -*- coding: utf-8 -*-
"""
The amplitude stage on the GPU (qm_engine_measure_amplitudes, Engine.measure_amplitudes, amplitudes.DeviceAmplitude,
MigrationScan.locate_compute(amplitudes=...)) against the NumPy restatement tests/amplitudes_ref.py, which
tests/test_amplitudes_host.py pins to SciPy.

Discrete results -- statuses, peak and trough samples, peak counts -- must be EQUAL.  A peak-to-trough value is one
subtraction and max|y| one maximum: with ``detrend_windows = 0`` both are bit-equal.  The averages are sums of n terms
in another order than NumPy's: RMS within 2 n 2^-53 relative (any order of n non-negative terms is within (n - 1) u of
the exact sum, both sides pay it, plus the square root), STD within 4 n 2^-53 max|y| absolute.  Through the window
detrend everything is within the detrend's bound 4 n 2^-53 max|x| (tests/test_preprocess_host.py's), twice that for the
peak-to-trough, a difference of two samples.
"""

import ctypes

import numpy as np
import pytest

import amplitudes_ref as ar
import preprocess_ref as pp

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def engine(lib):
    eng = lib.Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    if _lib.qmlib.qm_device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


@pytest.fixture(scope="module")
def fam():
    return ar.family()


def window_lengths(records):
    return (records[:, 2] - records[:, 1]).astype(np.float64)


def check_averages(got, want, n, method, scale, what):
    if method == "RMS":
        err = np.abs(got - want) / np.where(want > 0, want, 1.0)
        worst = float(np.max(err / (n * U)))
        print(f"{what}: worst RMS error {worst:.3f} n 2^-53 relative (bound 2)")
        assert np.all(err <= 2 * n * U)
    else:
        err = np.abs(got - want)
        worst = float(np.max(err / (n * U * scale)))
        print(f"{what}: worst STD error {worst:.3f} n 2^-53 max|y| (bound 4)")
        assert np.all(err <= 4 * n * U * scale)


# -- the family, no filter -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["RMS", "STD"])
def test_family_without_detrend(engine, fam, method):
    want_v, want_i, _ = ar.measure(fam["traces"], fam["trace_records"], fam["window_records"], detrend=False,
                                   method=method)
    values, index = engine.measure_amplitudes(fam["packed"], fam["trace_records"], fam["window_records"],
                                              detrend_windows=False, average_method=method)
    assert np.array_equal(index, want_i)
    assert np.all(index[:, 0] == 0) and np.all(index[fam["window_records"][:, 3] == 1, 3] >= 1)
    assert np.array_equal(bits(values[:, 0]), bits(want_v[:, 0]))
    assert np.array_equal(bits(values[:, 2]), bits(want_v[:, 2]))
    assert np.all(values[:, 3] == 0.0)
    check_averages(values[:, 1], want_v[:, 1], window_lengths(fam["window_records"]), method, want_v[:, 2],
                   f"family, no detrend, {method}")


def test_family_through_the_window_detrend(engine, fam):
    recs = fam["window_records"]
    want_v, want_i, _ = ar.measure(fam["traces"], fam["trace_records"], recs, detrend=True)
    n = window_lengths(recs)
    scale = np.array([np.max(np.abs(fam["traces"][tr][lo:hi])) for tr, lo, hi, _ in recs])
    bound = 4 * n * U * scale
    # the margin first: neighbouring samples, and the two largest peak-to-trough swings, lie far further apart than the
    # detrend's bound, so the extrema and the winning pair cannot depend on its rounding
    for k, (tr, lo, hi, kind) in enumerate(recs):
        y = ar.line_detrend(fam["traces"][tr][lo:hi])
        assert np.min(np.abs(np.diff(y))) > 100 * bound[k]
        if kind == 1:
            peaks, troughs = ar.extrema(y)
            order = np.sort(np.concatenate([peaks, troughs]))
            swings = np.sort(np.abs(np.diff(y[order])))
            assert swings[-1] - swings[-2] > 100 * bound[k]
    values, index = engine.measure_amplitudes(fam["packed"], fam["trace_records"], recs, detrend_windows=True)
    assert np.array_equal(index, want_i)
    err = np.abs(values - want_v)
    print("family through the detrend: worst errors / (4 n 2^-53 max|x|):",
          [float(np.max(err[:, c] / bound)) for c in range(3)])
    assert np.all(err[:, 0] <= 2 * bound) and np.all(err[:, 1] <= bound) and np.all(err[:, 2] <= bound)


def test_plateaus_through_the_detrend(engine):
    """Integer samples, mirror-symmetric about the window's centre, their sum a multiple of n's odd part: the mean is
    exact, every product (i - tbar)(x - mean) and every partial sum of them is exact in any order, the slope is exactly
    0 and the detrended window is exactly x - mean(x) -- on the device as in the restatement.  The plateaus survive and
    their midpoints must be SciPy's."""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(23)
    traces, recs = [], []
    for k, n in enumerate((64, 65, 96, 200, 257, 1000)):
        half = np.repeat(rng.integers(-6, 7, size=n), rng.integers(1, 5, size=n))[:n // 2].astype(np.float64)
        x = np.concatenate([half, [0.0] * (n % 2), half[::-1]])
        odd = n
        while odd % 2 == 0:
            odd //= 2
        step = 1 if n % 2 else 2                        # the middle sample alone, or the middle pair
        while x.sum() % odd:
            x[n // 2] += 1
            if step == 2:
                x[n // 2 - 1] += 1
        assert np.array_equal(x, x[::-1]) and (x.sum() / n) * n == x.sum()
        assert np.array_equal(ar.line_detrend(x), x - x.mean())
        traces.append(x)
        recs.append([k, 0, n, 1])
    packed, offsets = ar.pack(traces)
    trecs = np.stack([offsets, [len(x) for x in traces], [-1] * len(traces), [-1] * len(traces)], axis=1)
    for multiplier in (0.0, 0.3):
        want_v, want_i, _ = ar.measure(traces, trecs, recs, detrend=True, multiplier=multiplier)
        values, index = engine.measure_amplitudes(packed, trecs, recs, detrend_windows=True,
                                                  prominence_multiplier=multiplier)
        assert np.array_equal(index, want_i)
        assert np.array_equal(bits(values[:, 0]), bits(want_v[:, 0]))
        assert np.array_equal(bits(values[:, 2]), bits(want_v[:, 2]))
    for x, row in zip(traces, index):                   # (multiplier 0.3)
        y = x - x.mean()
        need = 0.3 * np.max(np.abs(y))
        peaks, troughs = signal.find_peaks(y, prominence=need)[0], signal.find_peaks(-y, prominence=need)[0]
        assert row[3] == len(peaks)
        if row[0] == 0:
            assert row[1] in peaks and row[2] in troughs
    plateaus = sum(int(np.any(x[p] == x[p + 1])) for x in traces for p in signal.find_peaks(x)[0])
    assert plateaus >= 20                               # the windows are full of them


def test_designed_rows_on_the_device(engine):
    rows = ar.designed_rows()
    seen = set()
    for multiplier in (0.0, 0.3):
        names = [k for k, v in rows.items() if v[1] == multiplier]
        traces = [rows[k][0] if len(rows[k][0]) else np.zeros(3) for k in names]
        packed, offsets = ar.pack(traces)
        trecs = np.stack([offsets, [len(x) for x in traces], [-1] * len(names), [-1] * len(names)], axis=1)
        recs = [[k, 0, len(rows[name][0]), 1] for k, name in enumerate(names)]
        want_v, want_i, _ = ar.measure(traces, trecs, recs, detrend=False, multiplier=multiplier)
        assert [int(s) for s in want_i[:, 0]] == [rows[k][2] for k in names]
        values, index = engine.measure_amplitudes(packed, trecs, recs, detrend_windows=False,
                                                  prominence_multiplier=multiplier)
        assert np.array_equal(index, want_i), (names, index, want_i)
        assert np.array_equal(bits(values), bits(want_v))
        seen |= set(int(s) for s in index[:, 0])
    # (status 4 cannot be reached through find_peaks' lists: tests/test_amplitudes_host.py)
    assert seen == {0, 1, 2, 3, 5}
    # a noise record over the same samples: flat before the detrend, no extrema asked for
    x, recs = np.array([2.0, 2.0, 2.0, 1.0, 2.0, 4.0]), [[0, 0, 3, 0], [0, 3, 6, 0], [0, 3, 6, 1], [0, 0, 3, 1]]
    values, index = engine.measure_amplitudes(x, [[0, 6, -1, -1]], recs)
    want_v, want_i, _ = ar.measure([x], [[0, 6, -1, -1]], recs)
    assert np.array_equal(index, want_i) and [int(s) for s in index[:, 0]] == [1, 0, 2, 1]
    assert values[1, 1] > 0.0 and np.all(index[:, 3] == 0) and np.allclose(values, want_v, rtol=1e-12, atol=0.0)


# -- the filter stage ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filtered_family(lib):
    """Six traces through two band-passes and a high-pass, one trace without a filter, one above the trace stage's LDS
    limit beside one just below it."""
    from quakemigrate_amd.preprocess import butter_bandpass_sos, butter_highpass_sos, cosine_taper_sides

    lengths = [700, 1501, 20480, 20481, 333, 1024]
    filters = [0, 1, 0, 0, -1, 2]
    identity = np.array([[1.0, 0, 0, 1.0, 0, 0]])
    high = butter_highpass_sos(1.0, 40.0, 4)
    sos = np.stack([butter_bandpass_sos(2.0, 16.0, 100, 4), butter_bandpass_sos(1.0, 12.0, 50, 4),
                    np.vstack([high, identity, identity])])
    traces = [pp.noisy_traces(n, 1, n, amplitude=1e-3)[0] * 1e-3 for n in lengths]
    table, weights, tapers = [], [], []
    for n, f in zip(lengths, filters):
        left, right = cosine_taper_sides(n)
        tapers.append(len(table) if f >= 0 else -1)
        if f >= 0:
            table.append([len(weights), len(left)])
            weights += list(left) + list(right)
    packed, offsets = ar.pack(traces)
    trecs = np.stack([offsets, lengths, filters, tapers], axis=1).astype(np.int64)
    recs = []
    for k, n in enumerate(lengths):
        recs += [[k, 0, n // 4, 0], [k, n // 4, n // 2, 1], [k, n // 2, n - 7, 1]]
    return dict(traces=traces, packed=packed, trecs=trecs, recs=np.array(recs), sos=sos,
                table=np.array(table, dtype=np.int32), weights=np.array(weights))


def test_filter_stage(lib, filtered_family):
    signal = pytest.importorskip("scipy.signal")
    f = filtered_family
    out = {}
    for skew in (1, 0):
        eng = lib.Engine(0, preproc_skew=skew)
        out[skew] = eng.measure_amplitudes(f["packed"], f["trecs"], f["recs"], sos=f["sos"], taper_table=f["table"],
                                           taper_weights=f["weights"], detrend_windows=False, want_filtered=True)
        eng.close()
    for a, b in zip(out[0], out[1]):                    # the same bits from both filter forms
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
    values, index, filtered = out[1]
    for (off, n, flt, tap), x in zip(f["trecs"], f["traces"]):
        got = filtered[off:off + n]
        if flt < 0:
            assert np.array_equal(bits(got), bits(x))   # measured as given
            continue
        o, m = f["table"][tap]
        shaped = pp.taper(ar.line_detrend(x), f["weights"][o:o + m], f["weights"][o + m:o + 2 * m])
        want = signal.sosfilt(f["sos"][flt], shaped)
        bound = pp.impulse_l1(f["sos"][flt], min(n, 4000)) * 4 * n * U * np.max(np.abs(x))
        err = float(np.max(np.abs(got - want)))
        print(f"filter stage, {n} samples: |device - sosfilt| = {err / bound:.3g} of the bound")
        assert err <= bound
    # the windows, cut from the traces as the device filtered them: the restatement on the same samples
    seen = [filtered[off:off + n] for off, n, _, _ in f["trecs"]]
    plain = np.array(f["trecs"])
    plain[:, 2:] = -1
    want_v, want_i, _ = ar.measure(seen, plain, f["recs"], detrend=False)
    assert np.array_equal(index, want_i)
    assert np.array_equal(bits(values[:, 0]), bits(want_v[:, 0])) and np.array_equal(bits(values[:, 2]), bits(want_v[:, 2]))


def test_windows_at_the_lds_limit(engine):
    limit = engine.get("amp_lds_samples")
    rng = np.random.default_rng(41)
    x = rng.standard_normal(limit + 40)
    recs = [[0, 0, limit, 1], [0, 0, limit + 1, 1], [0, 20, limit + 40, 1], [0, 7, limit + 7, 0]]
    trecs = [[0, len(x), -1, -1]]
    n = window_lengths(np.array(recs))
    for detrend, multiplier in ((False, 0.0), (False, 0.4)):
        want_v, want_i, _ = ar.measure([x], trecs, recs, detrend=detrend, multiplier=multiplier)
        values, index = engine.measure_amplitudes(x, trecs, recs, detrend_windows=detrend,
                                                  prominence_multiplier=multiplier)
        assert np.array_equal(index, want_i)
        assert np.array_equal(bits(values[:, 0]), bits(want_v[:, 0]))
        assert np.array_equal(bits(values[:, 2]), bits(want_v[:, 2]))
        check_averages(values[:, 1], want_v[:, 1], n, "RMS", want_v[:, 2], "LDS limit")
    # through the window detrend, in LDS and in scratch: the margins first, as for the family
    bound = 4 * n * U * np.array([np.max(np.abs(x[lo:hi])) for _, lo, hi, _ in recs])
    for k, (_, lo, hi, kind) in enumerate(recs):
        y = ar.line_detrend(x[lo:hi])
        assert np.min(np.abs(np.diff(y))) > 100 * bound[k]
        if kind == 1:
            order = np.sort(np.concatenate(ar.extrema(y)))
            swings = np.sort(np.abs(np.diff(y[order])))
            assert swings[-1] - swings[-2] > 100 * bound[k]
    want_v, want_i, _ = ar.measure([x], trecs, recs, detrend=True)
    values, index = engine.measure_amplitudes(x, trecs, recs, detrend_windows=True)
    assert np.array_equal(index, want_i)
    err = np.abs(values - want_v)
    print("LDS limit through the detrend: worst errors / (4 n 2^-53 max|x|):",
          [float(np.max(err[:, c] / bound)) for c in range(3)])
    assert np.all(err[:, 0] <= 2 * bound) and np.all(err[:, 2] <= bound)
    assert np.all(err[:, 1] <= bound + 2 * n * U * want_v[:, 1])


# -- the detrends, bit for bit: their sums restated in the device's order (preprocess_ref.detrend_device_order) -------
TRACE_LDS_SAMPLES = 20480


def test_filter_stage_is_the_device_order_restatement_bit_for_bit(lib):
    """Traces of 1 (the line's slope is guarded: sxx == 0), 2, 65, 301 and 20 481 (filtered in place) samples, each with
    a taper and without: line detrend in the device's order, then the bit-level taper and one forward pass."""
    import resample_ref as rr

    lengths = [1, 2, 65, 301, TRACE_LDS_SAMPLES + 1]
    sos = rr.stable_sos(13, 2, 2)
    rng = np.random.default_rng(13)
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
    weights = np.array(weights)
    want = []
    for x, (_, n, f, taper) in zip(traces, trecs):
        y = pp.detrend_device_order(x, False)
        if taper >= 0:
            o, m = table[taper]
            y = pp.taper(y, weights[o:o + m], weights[o + m:o + 2 * m])
        want.append(pp.sosfilt(sos[f], y))
    recs = [[k, 0, len(x), 0] for k, x in enumerate(traces)]
    for skew in (1, 0):
        eng = lib.Engine(0, preproc_skew=skew)
        try:
            _, _, filtered = eng.measure_amplitudes(packed, trecs, recs, sos=sos, taper_table=table,
                                                    taper_weights=weights, want_filtered=True)
        finally:
            eng.close()
        assert np.array_equal(bits(filtered), bits(np.concatenate(want))), skew


def test_window_detrend_is_the_device_order_restatement_bit_for_bit(engine):
    """Noise windows of 3, 64, 65 and ``amp_lds_samples`` + 1 (in scratch) samples through the window detrend: RMS and
    max|y| are the same quantities of the restated detrended window, the RMS's sum in the device's order as well.  A
    signal window of one sample goes through the guarded slope (sxx == 0) and comes out flat."""
    limit = engine.get("amp_lds_samples")
    lengths = [3, 64, 65, limit + 1]
    x = pp.noisy_traces(43, 1, sum(lengths) + 1)[0]
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    recs = [[0, int(lo), int(hi), 0] for lo, hi in zip(bounds[:-1], bounds[1:])] + [[0, len(x) - 1, len(x), 1]]
    values, index = engine.measure_amplitudes(x, [[0, len(x), -1, -1]], recs, detrend_windows=True)
    assert [int(s) for s in index[:, 0]] == [0, 0, 0, 0, ar.EMPTY_OR_FLAT]
    assert np.all(values[4] == 0.0)
    for k, (_, lo, hi, _) in enumerate(recs[:4]):
        y = pp.detrend_device_order(x[lo:hi], False)
        want = [0.0, np.sqrt(pp.wave_sum(y * y) / float(hi - lo)), np.max(np.abs(y)), 0.0]
        assert np.array_equal(bits(values[k]), bits(want)), (hi - lo, values[k], want)


# -- calls -----------------------------------------------------------------------------------------------------------
def test_device_traces_repeats_and_engines(lib, engine, fam, filtered_family):
    torch = pytest.importorskip("torch")
    f = filtered_family
    few = f["trecs"][[0, 1, 4, 5]].copy()               # (the long traces are the filter test's)
    few_recs = np.array([r for r in f["recs"] if r[0] in (0, 1, 4, 5)])
    few_recs[:, 0] = [{0: 0, 1: 1, 4: 2, 5: 3}[k] for k in few_recs[:, 0]]

    def both(eng, packed_a, packed_b):
        return (eng.measure_amplitudes(packed_a, fam["trace_records"], fam["window_records"]) +
                eng.measure_amplitudes(packed_b, few, few_recs, sos=f["sos"], taper_table=f["table"],
                                       taper_weights=f["weights"], prominence_multiplier=0.1, want_filtered=True))

    def same(a, b):
        return all(np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y)
                   for x, y in zip(a, b))

    first = both(engine, fam["packed"], f["packed"])
    assert same(first, both(engine, fam["packed"], f["packed"]))                        # two calls
    d_a, d_b = torch.from_numpy(fam["packed"]).cuda(), torch.from_numpy(f["packed"]).cuda()
    assert same(first, both(engine, d_a, d_b))                                          # device-resident traces
    assert np.array_equal(d_b.cpu().numpy(), f["packed"])                               # ... which stay as they were
    fresh = lib.Engine(0)
    assert same(first, both(fresh, fam["packed"], f["packed"]))                         # a fresh engine
    fresh.close()
    assert engine.last_kernel_ms() > 0.0


def test_two_events_in_one_call(engine, fam):
    other = ar.family(seed=9, n_traces=5)
    a = engine.measure_amplitudes(fam["packed"], fam["trace_records"], fam["window_records"],
                                  prominence_multiplier=0.05)
    b = engine.measure_amplitudes(other["packed"], other["trace_records"], other["window_records"],
                                  prominence_multiplier=0.05)
    shift = other["trace_records"].copy()
    shift[:, 0] += len(fam["packed"])
    recs = other["window_records"].copy()
    recs[:, 0] += len(fam["trace_records"])
    values, index = engine.measure_amplitudes(np.concatenate([fam["packed"], other["packed"]]),
                                              np.concatenate([fam["trace_records"], shift]),
                                              np.concatenate([fam["window_records"], recs]),
                                              prominence_multiplier=0.05)
    assert np.array_equal(bits(values), bits(np.concatenate([a[0], b[0]])))
    assert np.array_equal(index, np.concatenate([a[1], b[1]]))


def test_refusals_leave_the_outputs_untouched(lib, engine):
    from quakemigrate_amd.preprocess import butter_bandpass_sos

    vp = ctypes.c_void_p
    base = dict(traces=np.ones(400), total=400, trecs=np.array([[0, 200, 0, 0], [200, 200, -1, -1]], dtype=np.int64),
                sos=butter_bandpass_sos(2.0, 16.0, 100, 2), n_filters=1, n_sections=2,
                table=np.array([[0, 10]], dtype=np.int32), n_tapers=1, weights=np.ones(20), n_weights=20,
                recs=np.array([[0, 0, 50, 0], [1, 50, 200, 1]], dtype=np.int64), detrend=1, method=0, multiplier=0.0,
                n_traces=2, n_windows=2)

    def call(**change):
        a = {**base, **change}
        values, index = np.full((2, 4), 7.0), np.full((2, 4), 7, dtype=np.int32)
        filtered = np.full(400, 7.0)
        pt = vp(None) if a["traces"] is None else a["traces"].ctypes.data_as(vp)
        rc = lib.qmlib.qm_engine_measure_amplitudes(
            engine._h, pt, 0, a["total"], a["n_traces"], np.ascontiguousarray(a["trecs"]).reshape(-1),
            np.ascontiguousarray(a["sos"]).reshape(-1), a["n_filters"], a["n_sections"],
            np.ascontiguousarray(a["table"]).reshape(-1), a["n_tapers"], a["weights"], a["n_weights"], a["n_windows"],
            np.ascontiguousarray(a["recs"]).reshape(-1), a["detrend"], a["method"], a["multiplier"],
            values.ctypes.data_as(vp) if a.get("values", True) else vp(None), index.ctypes.data_as(vp),
            filtered.ctypes.data_as(vp))
        untouched = np.all(values == 7.0) and np.all(index == 7) and np.all(filtered == 7.0)
        return rc, lib.qmlib.qm_last_error().decode(), untouched

    rc, _, untouched = call()
    assert rc == 0 and not untouched

    def trecs(row, col, v):
        t = base["trecs"].copy()
        t[row, col] = v
        return t

    def recs(row, col, v):
        r = base["recs"].copy()
        r[row, col] = v
        return r

    sos_a0 = base["sos"].copy()
    sos_a0[1, 3] = 2.0
    refused = [
        (dict(traces=None), "NULL"), (dict(values=False), "NULL"),
        (dict(n_traces=0), "empty"), (dict(n_windows=0), "empty"),
        (dict(trecs=trecs(1, 1, 201)), "leave the buffer"), (dict(trecs=trecs(0, 0, -1)), "leave the buffer"),
        (dict(recs=recs(1, 2, 201)), "do not lie"), (dict(recs=recs(1, 1, 201)), "do not lie"),
        (dict(recs=recs(0, 1, -1)), "do not lie"), (dict(recs=recs(0, 0, 2)), "trace 2 of 2"),
        (dict(recs=recs(0, 3, 2)), "kind"), (dict(method=2), "average_method"), (dict(detrend=2), "detrend_windows"),
        (dict(multiplier=-0.1), "prominence_multiplier"), (dict(multiplier=float("nan")), "prominence_multiplier"),
        (dict(multiplier=float("inf")), "prominence_multiplier"),
        (dict(n_sections=0), "n_sections"), (dict(n_sections=9), "n_sections"), (dict(sos=sos_a0), "a0"),
        (dict(trecs=trecs(0, 2, 1)), "filter 1 out of range"), (dict(trecs=trecs(0, 2, -2)), "filter -2 out of range"),
        (dict(trecs=trecs(0, 3, 1)), "taper 1 out of range"),
        (dict(table=np.array([[0, 101]], dtype=np.int32), weights=np.ones(202), n_weights=202), "ramps cover"),
        (dict(table=np.array([[5, 10]], dtype=np.int32)), "weights given"),
        (dict(trecs=trecs(1, 0, 199)), "overlap"), (dict(trecs=trecs(0, 1, 201)), "overlap"),
    ]
    for change, text in refused:
        rc, message, untouched = call(**change)
        assert rc != 0 and text in message, (change, message)
        assert untouched, change


# -- DeviceAmplitude and the locate loop -------------------------------------------------------------------------------
# The table's amplitudes are compared entry by entry with the table the same host code builds over the restatement
# (tests/test_amplitudes_host.py pins that one to the restatement's own trace-by-trace table, exactly), each within
# its own bound: amplitudes_ref.row_bounds -- the filter stage's |h|_1 4 n 2^-53 max|x| carried through the window
# detrend, the detrend's 4 n_w 2^-53 max|y_w|, doubled for the peak-to-trough, over the filter gain.
@pytest.mark.parametrize("case", ["plain", "bandpass", "nyquist"])
def test_device_amplitude_table(engine, case):
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd.amplitudes import DeviceAmplitude

    ev = ar.synthetic_event()
    params = {"plain": {}, "bandpass": dict(bandpass_filter=True, bandpass_lowcut=1.0, bandpass_highcut=15.0),
              "nyquist": dict(bandpass_filter=True, bandpass_lowcut=1.0, bandpass_highcut=20.0, signal_window=1.0)}[case]
    amp = DeviceAmplitude(params)
    args = (ev["traces"], ev["stations"], ev["picks"], ev["otime"], ev["mw"], ev["p_tt"], ev["s_tt"], ev["fraction_tt"])
    table = amp.get_amplitudes(engine, *args)
    rows = ar.expected_rows(ev, amp.filter_sos, signal_window=amp.signal_window)
    assert ar.compare_table(table, rows, ev["otime"], rel=None) >= 8       # ids, statuses, NaNs, frequencies, times
    assert [row["status"][0] for row in rows] == [0, 0, 0, 0, -1, 0, -2, -2, -2]
    want = amp.get_amplitudes(ar.RestatedEngine(), *args)
    checked, worst = ar.table_within_bounds(amp, amp.plan(*args), table, want)
    print(f"DeviceAmplitude table, {case}: {checked} amplitudes, worst error {worst:.3g} of its bound")
    assert checked >= 20


def test_locate_compute_measures_amplitudes():
    import importlib.util

    from conftest import ROOT
    from quakemigrate_amd import amplitudes as amp_mod

    seen = []
    original = amp_mod.DeviceAmplitude.get_amplitudes

    def recording(self, engine, wa_traces, stations, picks, otime, *args, **kw):
        table = original(self, engine, wa_traces, stations, picks, otime, *args, **kw)
        seen.append(dict(traces=wa_traces, stations=stations, picks=picks, otime=otime, args=args, kw=kw,
                         again=original(self, ar.RestatedEngine(), wa_traces, stations, picks, otime, *args, **kw)))
        return table

    spec = importlib.util.spec_from_file_location("locate_events_amplitudes", ROOT / "examples" / "locate_events.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    located = mod.run(n_events=2, with_picker=True)[0]
    assert len(located) == 2 and all("amplitudes" not in r for r in located)
    amp = amp_mod.DeviceAmplitude({"signal_window": 1.0, "bandpass_filter": True, "bandpass_lowcut": 1.0,
                                   "bandpass_highcut": 20.0})
    amp_mod.DeviceAmplitude.get_amplitudes = recording
    try:
        handed = []
        located = mod.run(n_events=2, with_picker=True, amplitudes=amp,
                          on_event=lambda r: handed.append("amplitudes" in r))[0]
    finally:
        amp_mod.DeviceAmplitude.get_amplitudes = original
    assert len(located) == len(seen) == 2 and handed == [True, True]
    measured = 0
    for result, s in zip(located, seen):
        table, want = result["amplitudes"], s["again"]
        assert s["picks"] is result["picks"] and s["stations"] == [f"ST{k}" for k in range(6)]
        assert len(table["id"]) == 18 and list(table["id"]) == list(want["id"])
        assert np.array_equal(table["status"], want["status"]) and np.array_equal(table["windows"], want["windows"])
        assert np.array_equal(table["is_picked"], want["is_picked"]) and np.any(table["is_picked"])
        for name in ("P_time", "S_time", "P_freq", "S_freq", "P_filter_gain", "S_filter_gain", "epi_dist", "z_dist"):
            for got, exp in zip(table[name], want[name]):
                assert got == exp or (got != got and exp != exp), name
        plan = amp.plan(s["traces"], s["stations"], s["picks"], s["otime"], *s["args"],
                        tr_start=s["kw"]["tr_start"], tr_end=s["kw"]["tr_end"])
        checked, worst = ar.table_within_bounds(amp, plan, table, want)
        print(f"locate_compute's table: {checked} amplitudes, worst error {worst:.3g} of its bound")
        assert checked >= 40
        measured += int(np.sum(table["status"][:, 1:] == 0))
        with pytest.raises(ValueError, match="read_wa_waveforms"):
            from quakemigrate_amd import scan

            scan.MigrationScan.locate_compute(type("S", (), {"stage": "locate"})(), object(), [], 1.0, amplitudes=amp)
    assert measured >= 2 * 18                           # the injected wavelets are measured on most rows
