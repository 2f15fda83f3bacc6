# -*- coding: utf-8 -*-
"""
CPU-side checks of the amplitude stage (no GPU): the NumPy restatement the GPU tests compare against
(tests/amplitudes_ref.py) is pinned to SciPy and to a literal transcription of the reference's pairing rules, the
Python helpers behave as documented, and the C ABI carries the new symbol and refuses what it can refuse without a
device.
"""

import datetime as dt

import numpy as np
import pytest

import amplitudes_ref as ar
import preprocess_ref as pp

LENGTHS = (0, 1, 2, 3, 64, 65, 257, 300)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_engine()
    from quakemigrate_amd.core import lib as _lib

    return _lib


def windows_of(n, seed):
    """A random window and an integer-valued one full of plateaus."""
    rng = np.random.default_rng(1000 * n + seed)
    return rng.standard_normal(n), np.repeat(rng.integers(-3, 4, size=n), rng.integers(1, 4, size=n))[:n].astype(float)


class PeakToTroughError(Exception):
    pass


def reference_pairing(data, prominence_multiplier):
    """amplitude.py:858-901, literally, on an array; (full_amp, peak, trough)."""
    from scipy.signal import find_peaks

    prominence = prominence_multiplier * np.max(np.abs(data))
    peaks, _ = find_peaks(data, prominence=prominence)
    troughs, _ = find_peaks(-data, prominence=prominence)
    full_amp = None
    if len(peaks) == 0 or len(troughs) == 0:
        raise PeakToTroughError("No peaks or troughs found!")
    elif len(peaks) == 1 and len(troughs) == 1:
        full_amp = np.abs(data[peaks] - data[troughs])[0]
        pos = 0
    elif len(peaks) == len(troughs):
        if peaks[0] < troughs[0]:
            a, b, c, d = peaks, troughs, peaks[1:], troughs[:-1]
        else:
            a, b, c, d = peaks, troughs, peaks[:-1], troughs[1:]
    elif not np.abs(len(peaks) - len(troughs)) == 1:
        raise PeakToTroughError("Consecutive peaks/troughs!")
    elif len(peaks) > len(troughs):
        try:
            assert peaks[0] < troughs[0]
        except AssertionError:
            raise PeakToTroughError("Consecutive peaks/troughs!")
        a, b, c, d = peaks[:-1], troughs, peaks[1:], troughs
    elif len(peaks) < len(troughs):
        try:
            assert peaks[0] > troughs[0]
        except AssertionError:
            raise PeakToTroughError("Consecutive peaks/troughs!")
        a, b, c, d = peaks, troughs[1:], peaks, troughs[:-1]
    if not full_amp:
        fp1 = np.abs(data[a] - data[b])
        fp2 = np.abs(data[c] - data[d])
        if np.max(fp1) >= np.max(fp2):
            pos = np.argmax(fp1)
            full_amp = np.max(fp1)
            peaks, troughs = a, b
        else:
            pos = np.argmax(fp2)
            full_amp = np.max(fp2)
            peaks, troughs = c, d
    return full_amp, int(peaks[pos]), int(troughs[pos])


# -- extrema ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_extrema_are_find_peaks(n):
    signal = pytest.importorskip("scipy.signal")
    for seed in range(6):
        for y in windows_of(n, seed):
            for multiplier in (0.0, 0.1, 0.3, 0.7):
                need = multiplier * np.max(np.abs(y)) if n else 0.0
                peaks, troughs = ar.extrema(y, need)
                assert np.array_equal(peaks, signal.find_peaks(y, prominence=need)[0])
                assert np.array_equal(troughs, signal.find_peaks(-y, prominence=need)[0])
                if multiplier == 0.0:                   # (with no prominence asked for at all, too)
                    assert np.array_equal(peaks, signal.find_peaks(y)[0])


def test_plateau_midpoints_and_edges():
    y = np.array([0, 2, 2, 2, 0, 3, 3, 0, 1, 1], dtype=np.float64)     # the last plateau touches the window's end
    assert list(ar.local_maxima(y)) == [2, 5]
    assert list(ar.local_maxima(-y)) == [4, 7]
    assert list(ar.local_maxima(np.array([3.0, 1.0, 2.0]))) == []      # first and last sample are never peaks


# -- pairing ---------------------------------------------------------------------------------------------------------
def restated_pairing(y, multiplier):
    need = multiplier * np.max(np.abs(y)) if multiplier > 0.0 else 0.0
    return ar.pair(y, *ar.extrema(y, need))


@pytest.mark.parametrize("name", [k for k, v in ar.designed_rows().items() if len(v[0]) and np.all(np.isfinite(v[0]))
                                  and k != "flat"])
def test_designed_rows_against_the_reference_text(name):
    pytest.importorskip("scipy.signal")
    y, multiplier, expect = ar.designed_rows()[name]
    status, full, p, t = restated_pairing(y, multiplier)
    assert status == expect, (name, status)
    if expect == ar.MEASURED:
        assert (full, p, t) == reference_pairing(y, multiplier)
    else:
        text = "No peaks" if expect == ar.NO_EXTREMUM else "Consecutive"
        with pytest.raises(PeakToTroughError, match=text):
            reference_pairing(y, multiplier)


def test_designed_rows_take_the_branches_they_are_named_for():
    pytest.importorskip("scipy.signal")
    rows = ar.designed_rows()
    counts = {k: tuple(len(e) for e in ar.extrema(v[0], v[1] * np.max(np.abs(v[0])))) for k, v in rows.items()
              if len(v[0]) and np.all(np.isfinite(v[0]))}
    assert counts["one_pair"] == (1, 1)
    assert counts["equal_peak_first"][0] == counts["equal_peak_first"][1] >= 2
    assert counts["equal_trough_first"][0] == counts["equal_trough_first"][1] >= 2
    assert counts["more_peaks"][0] == counts["more_peaks"][1] + 1
    assert counts["more_troughs"][1] == counts["more_troughs"][0] + 1
    assert counts["three_over_one"] == (3, 1)                                   # |P - T| != 1
    assert counts["trough_first_two_peaks"] == (2, 1)                           # P > T, the trough first
    y = rows["trough_first_two_peaks"][0]
    peaks, troughs = ar.extrema(y, 0.3 * np.max(np.abs(y)))
    assert troughs[0] < peaks[0]
    # the winner from fp2; the exact tie goes to fp1 and its FIRST argmax
    y = rows["winner_fp2"][0]
    peaks, troughs = ar.extrema(y)
    assert peaks[0] < troughs[0] and len(peaks) == len(troughs)
    fp1, fp2 = np.abs(y[peaks] - y[troughs]), np.abs(y[peaks[1:]] - y[troughs[:-1]])
    assert fp2.max() > fp1.max()
    assert ar.pair(y, peaks, troughs)[2:] == (int(peaks[1:][np.argmax(fp2)]), int(troughs[:-1][np.argmax(fp2)]))
    y = rows["tie"][0]
    peaks, troughs = ar.extrema(y)
    fp1, fp2 = np.abs(y[peaks] - y[troughs]), np.abs(y[peaks[1:]] - y[troughs[:-1]])
    assert fp1.max() == fp2.max() and np.sum(fp1 == fp1.max()) > 1
    assert ar.pair(y, peaks, troughs)[2:] == (int(peaks[0]), int(troughs[0]))


def test_random_windows_pair_like_the_reference_text():
    pytest.importorskip("scipy.signal")
    seen = set()
    for n in (5, 9, 33, 120):
        for seed in range(40):
            for y in windows_of(n, seed):
                for multiplier in (0.0, 0.3, 0.9):
                    if np.max(np.abs(y)) == 0.0:
                        continue
                    status, full, p, t = restated_pairing(y, multiplier)
                    seen.add(status)
                    if status == ar.MEASURED:
                        assert (full, p, t) == reference_pairing(y, multiplier)
                    else:
                        with pytest.raises(PeakToTroughError):
                            reference_pairing(y, multiplier)
    assert {ar.MEASURED, ar.NO_EXTREMUM, ar.CONSECUTIVE} <= seen


def test_equal_pair_is_a_status_of_its_own():
    """One peak and one trough of equal value: the reference's ``if not full_amp`` falls through to names that were
    never bound (UnboundLocalError); the stage reports status 4.  It cannot occur through ``find_peaks``: between such
    a peak and trough (the peak first, say) the samples fall below their common value v and rise above it again, so
    the highest of them, M > v, is a peak; both of its prominence walks pass samples <= v, so its prominence is at
    least M - v; the trough's left walk ends at the dip below v and meets nothing above M, so its prominence is at
    most M - v.  The peak at M is kept whenever the trough is: two peaks (without a prominence filter all are kept
    anyway).  So the rule is pinned on the lists themselves, and a search confirms the argument."""
    rng = np.random.default_rng(4)
    for _ in range(3000):
        y = rng.integers(-3, 4, size=int(rng.integers(3, 12))).astype(float)
        for multiplier in (0.0, 0.2, 0.5, 1.0):
            peaks, troughs = ar.extrema(y, multiplier * np.max(np.abs(y)))
            assert not (len(peaks) == len(troughs) == 1 and y[peaks[0]] == y[troughs[0]])
    y = np.array([0.0, 1.0, 0.0, 2.0, 1.0, 2.0, 0.0])
    assert ar.pair(y, np.array([1]), np.array([4])) == (ar.EQUAL_PAIR, 0.0, -1, -1)


def test_window_statuses_and_columns():
    rows = ar.designed_rows()
    for name, (y, multiplier, expect) in rows.items():
        values, index = ar.measure_window(y, 1, detrend=False, multiplier=multiplier, lo=100)
        assert index[0] == expect, name
        if expect in (ar.EMPTY_OR_FLAT, ar.NON_FINITE):
            assert np.all(values == 0.0) and list(index[1:]) == [-1, -1, 0]
        else:
            assert values[1] == np.sqrt(np.mean(y * y)) and values[2] == np.max(np.abs(y)) and values[3] == 0.0
        if expect == ar.MEASURED:
            assert values[0] == abs(y[index[1] - 100] - y[index[2] - 100]) and index[3] >= 1
        else:
            assert values[0] == 0.0 and index[1] == index[2] == -1
    # noise: flat is tested before the detrend, signal after it -- a pure ramp is flat only once detrended
    ramp = np.arange(50, dtype=np.float64) * 0.5
    assert ar.measure_window(ramp, 0)[1][0] == ar.MEASURED
    assert ar.measure_window(np.arange(8.0), 1)[1][0] in (ar.EMPTY_OR_FLAT, ar.NO_EXTREMUM)
    assert ar.measure_window(np.full(9, 4.0), 0)[1][0] == ar.EMPTY_OR_FLAT
    y = np.random.default_rng(3).standard_normal(200)
    assert ar.measure_window(y, 1, method="STD")[0][1] == np.std(ar.line_detrend(y))


# -- the filter and the detrends ---------------------------------------------------------------------------------------
def test_forward_filter_is_sosfilt():
    signal = pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import butter_bandpass_sos, butter_highpass_sos, cosine_taper_sides

    for sos in (butter_bandpass_sos(2.0, 16.0, 100, 4), butter_highpass_sos(2.0, 40, 4), butter_highpass_sos(1.0, 50, 3)):
        for n in (64, 301, 2048):
            x = pp.noisy_traces(n, 1, n)[0]
            left, right = cosine_taper_sides(n)
            got = ar.filter_trace(x, sos, np.concatenate([left, right]))
            want = signal.sosfilt(sos, pp.taper(ar.line_detrend(x), left, right))
            assert np.array_equal(got, want)


def test_window_detrend_against_scipy():
    """The restated closed form against ``scipy.signal.detrend(type="linear")`` (a least-squares solve: another
    path, so not the same bits).  A trial over n = 3 .. 13 000 saw at most 3.96 n 2^-53 max|x|; the bound asserted is
    twice that.  The figure is about SciPy and the restatement, not about the kernel."""
    signal = pytest.importorskip("scipy.signal")
    worst = 0.0
    for n in (3, 4, 7, 64, 65, 301, 1000, 2048, 5000, 13000):
        for seed in range(3):
            x = pp.noisy_traces(7 * n + seed, 1, n)[0]
            err = np.max(np.abs(ar.line_detrend(x) - signal.detrend(x, type="linear")))
            scaled = err / (n * 2.0 ** -53 * np.max(np.abs(x)))
            worst = max(worst, scaled)
            assert scaled <= 2 * 3.96, (n, seed, scaled)
    print(f"window detrend: worst |restated - scipy| = {worst:.3f} n 2^-53 max|x|")


def test_both_detrends_give_the_same_extrema():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(17)
    for k in range(300):
        n = int(rng.integers(20, 600))
        x = 1e-3 * rng.standard_normal(n) + 1e-6 * rng.uniform(-5, 5) * np.arange(n) + rng.uniform(-1e-2, 1e-2)
        ours, theirs = ar.line_detrend(x), signal.detrend(x, type="linear")
        for a, b in zip(ar.extrema(ours), (signal.find_peaks(theirs)[0], signal.find_peaks(-theirs)[0])):
            assert np.array_equal(a, b), k


def test_highpass_sections_are_obspys():
    signal = pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import butter_highpass_sos

    for freq, rate, corners in ((2.0, 100, 4), (0.5, 40, 4), (1.0, 50, 3), (5.0, 200, 2)):
        z, p, k = signal.iirfilter(corners, freq / (0.5 * rate), btype="highpass", ftype="butter", output="zpk")
        sos = butter_highpass_sos(freq, rate, corners)
        assert np.array_equal(sos, signal.zpk2sos(z, p, k))
        assert sos.shape == ((corners + 1) // 2, 6) and np.all(sos[:, 3] == 1.0)
        # the sections the reference evaluates the gain on (amplitude.py:535-537): the same filter
        direct = signal.iirfilter(corners, freq / (0.5 * rate), btype="highpass", ftype="butter", output="sos")
        f = np.linspace(0.1, 0.49 * rate, 50)
        np.testing.assert_allclose(np.abs(signal.sosfreqz(sos, worN=f, fs=rate)[1]),
                                   np.abs(signal.sosfreqz(direct, worN=f, fs=rate)[1]), rtol=1e-9, atol=1e-300)
    for freq in (50.0, 60.0, 0.0):
        with pytest.raises(ValueError, match="Nyquist"):
            butter_highpass_sos(freq, 100, 4)


# -- the host rules of quakemigrate_amd.amplitudes ---------------------------------------------------------------------
def test_amplitude_windows_branch_by_branch():
    from quakemigrate_amd.amplitudes import amplitude_windows

    mw, frac = 1.0, 0.1
    # overlap: the windows meet halfway between p_end and s_start
    status, w = amplitude_windows(5.0, 6.0, 5.0, 6.0, mw, frac, 0.0)
    p_end, s_start = 5.0 + mw + 0.5, 6.0 - mw - 0.6
    mid = p_end + (s_start - p_end) / 2
    assert status == 0 and w == [[5.0 - mw - 0.5, mid], [mid, 6.0 + mw + 0.6 + 0.0]]
    # a gap shorter than the signal window: the P window runs up to the S window
    status, w = amplitude_windows(5.0, 10.0, 5.0, 10.0, mw, frac, 3.0)
    assert status == 0 and w == [[3.5, 10.0 - mw - 1.0], [10.0 - mw - 1.0, 10.0 + mw + 1.0 + 3.0]]
    # a wide gap: the P window is extended by the signal window
    status, w = amplitude_windows(5.0, 20.0, 5.0, 20.0, mw, frac, 3.0)
    assert status == 0 and w == [[3.5, 6.5 + 3.0], [20.0 - mw - 2.0, 20.0 + mw + 2.0 + 3.0]]
    # "-1": that phase's modelled time; "No <phase> onset": both modelled times
    assert amplitude_windows("-1", 10.5, 5.0, 10.0, mw, frac, 0.0)[1][0] == [3.5, 6.5]
    assert amplitude_windows("-1", 10.5, 5.0, 10.0, mw, frac, 0.0)[1][1] == [10.5 - 2.0, 10.5 + 2.0]
    assert amplitude_windows(5.2, "-1", 5.0, 10.0, mw, frac, 0.0)[1] == [[5.2 - 1.5, 5.2 + 1.5], [8.0, 12.0]]
    assert amplitude_windows(5.2, "No S onset", 5.0, 10.0, mw, frac, 0.0)[1] == [[3.5, 6.5], [8.0, 12.0]]
    assert amplitude_windows("No P onset", 10.4, 5.0, 10.0, mw, frac, 0.0)[1] == [[3.5, 6.5], [8.0, 12.0]]
    # the P pick is not before the S pick: a status, not an exception
    assert amplitude_windows(10.0, 9.0, 5.0, 10.0, mw, frac, 0.0) == (1, None)
    assert amplitude_windows(9.0, 9.0, 5.0, 10.0, mw, frac, 0.0) == (1, None)
    for args in ((5.0, 6.0, 5.0, 6.0), ("-1", 10.5, 5.0, 10.0), (5.2, "No S onset", 5.0, 10.0), ("No P onset", "-1", 5.0, 9.0),
                 ("-1", "No S onset", 5.0, 9.0), (10.0, 9.0, 5.0, 10.0)):
        for sw in (0.0, 3.0):
            assert amplitude_windows(*args, mw, frac, sw) == ar.amplitude_windows(*args, mw, frac, sw)


def test_window_samples_rule():
    from quakemigrate_amd.amplitudes import round_half_away, window_samples

    assert [round_half_away(v) for v in (0.5, 1.5, 2.4999, -0.5, -1.5, 0.0)] == [1, 2, 2, -1, -2, 0]
    assert window_samples(1.0, 2.0, 0.0, 100.0, 1000) == (100, 201)          # both ends included
    assert window_samples(-3.0, 2.004, 0.0, 100.0, 1000) == (0, 201)         # clipped at the start, nearest sample
    assert window_samples(9.0, 12.0, 0.0, 100.0, 1000) == (900, 1000)        # clipped at the end
    assert window_samples(12.0, 13.0, 0.0, 100.0, 1000) == (1000, 1000)      # empty
    assert window_samples(-5.0, -4.0, 0.0, 100.0, 1000) == (0, 0)
    assert window_samples(1.0, 2.0, 0.25, 50.0, 1000) == ar.window_samples(1.0, 2.0, 0.25, 50.0, 1000)


def test_device_amplitude_parameters():
    from quakemigrate_amd.amplitudes import DeviceAmplitude

    a = DeviceAmplitude()
    assert (a.signal_window, a.noise_window, a.noise_measure, a.prominence_multiplier, a.loc_method,
            a.highpass_filter, a.bandpass_filter, a.filter_corners) == (0.0, 5.0, "RMS", 0.0, "spline", False, False, 4)
    with pytest.raises(AttributeError, match="Both bandpass"):
        DeviceAmplitude({"highpass_filter": True, "highpass_freq": 1.0, "bandpass_filter": True,
                         "bandpass_lowcut": 1.0, "bandpass_highcut": 5.0})
    with pytest.raises(AttributeError, match="Archive"):
        DeviceAmplitude({"water_level": 60.0})
    with pytest.raises(AttributeError, match="Highpass"):
        DeviceAmplitude({"highpass_filter": True})
    # pad(): amplitude.py:1041-1048
    a = DeviceAmplitude({"signal_window": 2.0, "noise_window": 4.0})
    pre, post = 4.0 + 1.0, 2.0 + 30.0 * 1.1 + 1.0
    extra = np.ceil((pre + post) * 0.06)
    assert a.pad(1.0, 30.0, 0.1) == (pre + extra, post + extra)
    # the Nyquist fall-back of _filter_trace
    from quakemigrate_amd.preprocess import butter_bandpass_sos, butter_highpass_sos

    a = DeviceAmplitude({"bandpass_filter": True, "bandpass_lowcut": 2.0, "bandpass_highcut": 20.0})
    assert np.array_equal(a.filter_sos(100.0), butter_bandpass_sos(2.0, 20.0, 100.0, 4))
    assert np.array_equal(a.filter_sos(40.0), butter_highpass_sos(2.0, 40.0, 4))
    assert DeviceAmplitude().filter_sos(100.0) is None


def test_station_picks():
    from quakemigrate_amd.amplitudes import station_picks

    t0 = dt.datetime(2024, 5, 17, 10, 0, 0)
    picks = {"Station": np.array(["A", "A", "B", "B", "C"], dtype=object),
             "Phase": np.array(["P", "S", "P", "S", "P"], dtype=object),
             "PickTime": np.array([t0 + dt.timedelta(seconds=2.5), -1, -1, -1, t0 + dt.timedelta(seconds=1)],
                                  dtype=object)}
    assert station_picks(picks, "A", t0) == (2.5, "-1", True)
    assert station_picks(picks, "B", t0) == ("-1", "-1", False)
    assert station_picks(picks, "C", t0) == (1.0, "No S onset", True)
    assert station_picks(picks, "D", t0) == ("-1", "-1", False)
    assert station_picks(None, "A", t0) == ("-1", "-1", False)


# -- the C ABI and the binding ---------------------------------------------------------------------------------------
def test_symbol_is_exported_and_refuses_without_a_device(lib):
    import ctypes

    from conftest import ROOT

    assert hasattr(lib.qmlib, "qm_engine_measure_amplitudes")
    header = (ROOT / "include" / "qmhip.h").read_text()
    assert "int qm_engine_measure_amplitudes(" in header
    for words in ("amp_lds_samples", "a DEVIATION", "Refused, with the outputs untouched", "_local_maxima_1d",
                  "_peak_prominences", "FIRST argmax"):
        assert words in header
    values, index = np.full((3, 4), 7.0), np.full((3, 4), 7, dtype=np.int32)
    traces = np.ones(100)
    trec = np.array([[0, 100, -1, -1]], dtype=np.int64)
    wrec = np.array([[0, 0, 10, 0], [0, 10, 50, 1], [0, 50, 100, 1]], dtype=np.int64)
    none = np.zeros(0)
    rc = lib.qmlib.qm_engine_measure_amplitudes(
        ctypes.c_void_p(None), traces.ctypes.data_as(ctypes.c_void_p), 0, 100, 1, trec.reshape(-1), none, 0, 1,
        np.zeros(0, dtype=np.int32), 0, none, 0, 3, wrec.reshape(-1), 1, 0, 0.0,
        values.ctypes.data_as(ctypes.c_void_p), index.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(None))
    assert rc != 0 and b"NULL argument" in lib.qmlib.qm_last_error()
    assert np.all(values == 7.0) and np.all(index == 7)


def test_binding_checks_shapes_before_the_call(lib):
    eng = lib.Engine.__new__(lib.Engine)                # no device here: the checks come before the C call
    eng._h, eng.device = None, 0
    traces = np.ones(100)
    trec, wrec = np.array([[0, 100, -1, -1]]), np.array([[0, 0, 10, 0]])
    with pytest.raises(ValueError, match="trace_records of shape"):
        eng.measure_amplitudes(traces, trec[:, :3], wrec)
    with pytest.raises(ValueError, match="window_records of shape"):
        eng.measure_amplitudes(traces, trec, wrec[:, :3])
    with pytest.raises(ValueError, match="average_method"):
        eng.measure_amplitudes(traces, trec, wrec, average_method="ENV")
    with pytest.raises(ValueError, match="sos of shape"):
        eng.measure_amplitudes(traces, trec, wrec, sos=np.ones((2, 6)))
    with pytest.raises(TypeError):
        eng.measure_amplitudes(traces.astype(np.float32), trec, wrec)
    with pytest.raises(lib.QMHipError, match="NULL argument"):      # the engine handle is NULL
        eng.measure_amplitudes(traces, trec, wrec)


@pytest.mark.parametrize("case", ["plain", "bandpass", "nyquist", "std_trim", "env"])
def test_device_amplitude_table_by_the_restatement(case):
    """The host half of ``DeviceAmplitude.get_amplitudes`` -- rows, windows, units, gains -- with the engine's call
    answered by the restatement: it must give the table the restatement builds trace by trace."""
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd.amplitudes import DeviceAmplitude

    ev = ar.synthetic_event()
    params = {"plain": {}, "bandpass": dict(bandpass_filter=True, bandpass_lowcut=1.0, bandpass_highcut=15.0),
              "nyquist": dict(bandpass_filter=True, bandpass_lowcut=1.0, bandpass_highcut=20.0, signal_window=1.0),
              "std_trim": dict(noise_measure="STD", highpass_filter=True, highpass_freq=0.5, prominence_multiplier=0.05),
              "env": dict(noise_measure="ENV")}[case]
    amp = DeviceAmplitude(params)
    trim = (-8.0, 20.0) if case == "std_trim" else None
    kw = {} if trim is None else dict(tr_start=ev["otime"] + dt.timedelta(seconds=trim[0]),
                                      tr_end=ev["otime"] + dt.timedelta(seconds=trim[1]))
    table = amp.get_amplitudes(ar.RestatedEngine(), ev["traces"], ev["stations"], ev["picks"], ev["otime"], ev["mw"],
                               ev["p_tt"], ev["s_tt"], ev["fraction_tt"], **kw)
    if case == "env":                                   # the envelope averages are the host's: checked on their own
        from scipy.signal import hilbert

        rows = ar.expected_rows(ev, amp.filter_sos)
        r = 0                                           # station A, component E: measured
        lo, hi = table["windows"][r][1]
        y = ar.line_detrend(ev["traces"][0]["data"][lo:hi])
        assert table["P_avg_amp"][r] == np.mean(np.abs(hilbert(y))) * 1000.0
        assert table["P_amp"][r] == rows[r]["P_amp"] and table["Noise_amp"][r] != rows[r]["Noise_amp"]
        return
    rows = ar.expected_rows(ev, amp.filter_sos, signal_window=amp.signal_window,
                            method=amp.noise_measure, multiplier=amp.prominence_multiplier, trim=trim)
    assert ar.compare_table(table, rows, ev["otime"]) >= 8
    assert [row["status"][0] for row in rows] == [0, 0, 0, 0, -1, 0, -2, -2, -2]
    assert table["id"][4] == ".B..[N,1]"
    if case == "nyquist":                               # the 40 Hz trace went through the high-pass
        from quakemigrate_amd.preprocess import butter_highpass_sos

        assert np.array_equal(amp.filter_sos(40.0), butter_highpass_sos(1.0, 40.0, 4))
        assert len(amp.filter_sos(100.0)) == 4 and np.isfinite(table["S_filter_gain"][5])


@pytest.mark.parametrize("loc_method", ["spline", "gaussian", "covariance"])
def test_locate_takes_the_location_named_by_loc_method(loc_method):
    """``MigrationScan._measure_amplitudes`` hands the lookup table the hypocentre as fractional grid indices: the
    spline or Gaussian fit as it is, the covariance fit's expectation (xyz from the lower-left corner) over the node
    spacing -- never the 3 x 3 covariance matrix."""
    from quakemigrate_amd import scan
    from quakemigrate_amd.amplitudes import DeviceAmplitude
    from quakemigrate_amd.locate import LocationFits

    asked = []

    class Lut:
        node_spacing = np.array([0.5, 0.25, 2.0])
        fraction_tt, max_traveltime = 0.1, 6.0

        def traveltime_to(self, phase, ijk, station):
            asked.append(np.array(ijk))
            return np.array([2.0 if phase == "P" else 3.5])

    class Archive:
        def read_wa_waveforms(self, start, end):
            self.window = (start, end)
            return []

    fields = {f.name: 0.0 for f in __import__("dataclasses").fields(LocationFits)}
    fields.update(spline=np.array([1.0, 2.0, 3.0]), gaussian=np.array([1.5, 2.5, 3.5]),
                  expectation=np.array([1.0, 1.0, 1.0]), covariance=np.eye(3))
    otime = dt.datetime(2024, 5, 17, 10, 0, 0)
    result = dict(fits=LocationFits(**fields), otime=otime)
    me = type("Scan", (), {"lut": Lut(), "_hypocentre_ijk": scan.MigrationScan._hypocentre_ijk})()
    onset_data = type("OnsetData", (), {"availability": {"A_P": 1, "A_S": 1, "B_P": 1, "B_S": 1}})()
    amp, archive = DeviceAmplitude({"loc_method": loc_method}), Archive()
    table = scan.MigrationScan._measure_amplitudes(me, amp, None, archive, onset_data, result, 1.0)
    want = {"spline": [1.0, 2.0, 3.0], "gaussian": [1.5, 2.5, 3.5], "covariance": [2.0, 4.0, 0.5]}[loc_method]
    assert len(asked) == 4 and all(a.shape == (3,) and np.array_equal(a, want) for a in asked)
    assert list(table["id"]) == [f".{s}..{c}" for s in "AB" for c in ("[E,2]", "[N,1]", "Z")]
    pre, post = amp.pad(1.0, 6.0, 0.1)
    assert archive.window == (otime - dt.timedelta(seconds=float(pre)), otime + dt.timedelta(seconds=float(post)))


def test_locate_refuses_other_loc_methods():
    from quakemigrate_amd import scan
    from quakemigrate_amd.amplitudes import DeviceAmplitude

    me = type("Scan", (), {"stage": "locate"})()
    archive = type("Archive", (), {"read_wa_waveforms": lambda self, a, b: []})()
    with pytest.raises(ValueError, match="loc_method"):
        scan.MigrationScan.locate_compute(me, archive, [], 1.0, amplitudes=DeviceAmplitude({"loc_method": "peak"}))
    with pytest.raises(ValueError, match="loc_method"):
        scan.MigrationScan._hypocentre_ijk(me, None, "peak")
    with pytest.raises(ValueError, match="read_wa_waveforms"):
        scan.MigrationScan.locate_compute(me, object(), [], 1.0, amplitudes=DeviceAmplitude())
