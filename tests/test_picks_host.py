# -*- coding: utf-8 -*-
"""
CPU-side checks of the phase-pick stage (no GPU): the NumPy restatement the GPU tests compare against
(tests/picks_ref.py) is pinned to SciPy and to independent statements of the reference's rules, the Python helpers
behave as documented, and the C ABI carries the new symbol and refuses what it can refuse without a device.
"""

import datetime as dt
import warnings

import numpy as np
import pytest

import picks_ref as pr

RTOL = 1e-6


@pytest.fixture(scope="module")
def fam():
    return pr.family_results(n_stations=80)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_engine()
    from quakemigrate_amd.core import lib as _lib

    return _lib


# -- the restatement's rules ---------------------------------------------------------------------------------------
def test_threshold_is_the_sorted_middle_formula(fam):
    """median + 8 x 1.4826 x median(|x - median|) of the samples outside the station's windows that exceed 1, written
    out on sorted arrays -- what the kernel selects -- has the bits of the reference's NumPy expressions."""
    def middle(v):
        v = np.sort(v)
        n = len(v)
        return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2

    for r in range(len(fam["status"])):
        keep = np.ones(fam["onsets"].shape[1], dtype=bool)
        for k in np.flatnonzero(fam["row_group"] == fam["row_group"][r]):
            keep[fam["windows"][k, 0]:fam["windows"][k, 2]] = False
        noise = fam["onsets"][r][keep & (fam["onsets"][r] > 1)]
        med = middle(noise)
        want = med + (1.4826 * middle(np.abs(noise - med))) * 8.0
        assert want == fam["picks"][r, 0], r
        assert 20 < np.count_nonzero(~keep) and noise.size < keep.sum()        # (windows and pads both bite)


def test_noise_set_rows_have_the_thresholds_written_out_on_sorted_values():
    """tests/picks_ref.py: noise_set_rows -- every size and kind of noise set is what its name says, and the
    restatement's threshold has the bits of the sorted-middle formula on the values the row was built from."""
    d = pr.noise_set_rows()
    picks, status = pr.pick_rows(d["onsets"], d["windows"], d["row_group"], d["sampling_rate"], d["halfwidth"])
    assert len(d["names"]) == len(pr.NOISE_SIZES) * len(pr.NOISE_KINDS) and np.all(status == pr.NOTHING_ABOVE)

    def middle(v):                                      # (sorted)
        n = len(v)
        return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2

    for r, (name, v) in enumerate(zip(d["names"], d["noise"])):
        n, kind = len(v), name.partition(" ")[2]
        lo, hi = d["windows"][r, 0], d["windows"][r, 2]
        assert np.all(d["onsets"][r, lo:hi] == 0.5)
        assert np.array_equal(np.sort(d["onsets"][r][d["onsets"][r] > 1]), v) and name.startswith(f"{n} "), name
        assert np.all((d["onsets"][r] == 0.5) | (d["onsets"][r] > 1))
        if n == 0:
            assert np.isnan(picks[r, 0]), name
            continue
        med = middle(v)
        want = med + (1.4826 * middle(np.sort(np.abs(v - med)))) * 8.0
        assert want == picks[r, 0] and want > 1, name
        if kind == "distinct" or kind == "last bit apart":
            assert len(np.unique(v)) == n
        if kind == "all equal":
            assert len(np.unique(v)) == 1 and want == v[0]
        if kind == "two middle values equal" and n > 1:
            assert v[n // 2 - 1] == v[n // 2] and (n < 4 or len(np.unique(v)) == n - 1)
        if kind == "middle value across the even split" and n > 1:
            assert np.count_nonzero(v == v[n // 2]) == n - 2 * (n // 4) and med == v[n // 2]
        if kind == "last bit apart":
            assert np.all(np.diff(v.view(np.uint64)) == 1)


def test_peak_is_the_run_around_the_first_maximum(fam):
    for r in range(len(fam["status"])):
        lo, hi = fam["windows"][r, 0], fam["windows"][r, 2]
        y, thr = fam["onsets"][r], fam["picks"][r, 0]
        first = lo + int(np.argmax(y[lo:hi]))
        if not y[first] > thr:
            assert fam["status"][r] == pr.NOTHING_ABOVE
            continue
        a = first
        while a - 1 >= lo and y[a - 1] > thr:
            a -= 1
        b = first + 1
        while b < hi and y[b] > thr:
            b += 1
        if b - a < 2:
            assert fam["status"][r] == pr.ONE_SAMPLE
        else:
            assert (fam["picks"][r, 5], fam["picks"][r, 6]) == (a - 1, b + 1), r


def test_designed_rows_give_the_statuses_they_are_built_for():
    d = pr.designed_rows()
    _, status = pr.pick_rows(d["onsets"], d["windows"], d["row_group"], d["sampling_rate"], d["halfwidth"])
    assert dict(zip(d["names"], status)) == dict(zip(d["names"], d["expected"]))
    assert set(status) == {0, 1, 2, 3, 4, 6}


# -- the solver against SciPy -----------------------------------------------------------------------------------------
def test_solver_reaches_the_tight_scipy_minimum(fam):
    """Every converged row within 1e-6 of curve_fit(jac=analytic, ftol=xtol=gtol=1e-15): amplitude and sigma
    relative, mean in samples.  The reference's default call is further from that minimum than the bound."""
    status, picks, rate = fam["status"], fam["picks"], fam["sampling_rate"]
    assert not np.any(status == pr.NOT_CONVERGED)
    worst = default_worst = 0.0
    rows = np.flatnonzero(np.isin(status, (pr.PICKED, pr.MEAN_OUTSIDE)))
    assert len(rows) >= 100
    for r in rows:
        tight, default = fam["tight"][r], fam["default"][r]
        assert not isinstance(tight, Exception), (r, tight)
        x, y, p0 = pr.fit_inputs(fam["onsets"][r], int(picks[r, 5]), int(picks[r, 6]), rate, fam["halfwidth"][r])
        popt, iterations, converged = pr.lm_fit(x, y, p0)
        assert converged and iterations == picks[r, 7]
        worst = max(worst, pr.fit_distance(popt, tight, rate))
        if not isinstance(default, Exception):
            default_worst = max(default_worst, pr.fit_distance(default, tight, rate))
    print(f"\nrestatement to tight fit: {worst:.3e}; default curve_fit to tight fit: {default_worst:.3e}")
    assert worst <= RTOL
    assert default_worst > RTOL


def test_solver_has_the_analytic_jacobian():
    x = np.arange(100, 130) / 50.0
    p = np.array([7.0, 2.31, 0.07])
    jac = pr.gaussian_jac(x, *p)
    for k in range(3):
        h = 1e-7 * max(1.0, abs(p[k]))
        up, down = p.copy(), p.copy()
        up[k] += h
        down[k] -= h
        numeric = (pr.gaussian_1d(x, *up) - pr.gaussian_1d(x, *down)) / (2 * h)
        np.testing.assert_allclose(jac[:, k], numeric, rtol=1e-6, atol=1e-7)


# -- pick_windows ---------------------------------------------------------------------------------------------------------
def test_pick_windows_hand_cases():
    from quakemigrate_amd.picks import pick_windows

    # overlap: P and S windows meet at int((100 + 141) / 2) = 120
    w = pick_windows([100, 141], [30, 40], 451, [0, 0])
    assert w.dtype == np.int32 and w.tolist() == [[70, 100, 120], [120, 141, 181]]
    # no overlap: untouched
    assert pick_windows([100, 300], [30, 40], 451, [0, 0]).tolist() == [[70, 100, 130], [260, 300, 340]]
    # one phase: both ends clipped
    assert pick_windows([20], [30], 40, [5]).tolist() == [[0, 20, 40]]
    # three phases: only the first is clipped below, only the last above
    w = pick_windows([10, 60, 430], [30, 30, 30], 451, [7, 7, 7])
    assert w.tolist() == [[0, 10, 35], [35, 60, 90], [400, 430, 451]]
    # rows of two stations interleaved, phase order as they appear; rows of other stations do not interact
    w = pick_windows([100, 50, 141, 90], [30, 60, 40, 60], 200, [0, 1, 0, 1])
    assert w.tolist() == [[70, 100, 120], [0, 50, 70], [120, 141, 181], [70, 90, 150]]
    # the midpoint truncates towards zero like int(), also for an odd sum
    assert pick_windows([101, 140], [40, 40], 451, [0, 0])[0, 2] == 120
    # the picks_ref statement of the reference's rule agrees
    assert pr.distinguish_windows([[-20, 10, 40], [30, 60, 90], [400, 430, 460]], 451) == w_list(
        pick_windows([10, 60, 430], [30, 30, 30], 451, [7, 7, 7]))
    # a window the reference's slices would wrap
    with pytest.raises(ValueError, match="negative"):
        pick_windows([100, -60], [30, 20], 451, [0, 0])
    with pytest.raises(ValueError):
        pick_windows([100, 120], [30], 451, [0, 0])


def w_list(w):
    return [[int(v) for v in row] for row in w]


# -- DevicePicker on a stand-in engine ----------------------------------------------------------------------------------------
class RestatedEngine:
    """``Engine.pick_phases`` answered by the restatement."""

    def pick_phases(self, onsets, windows, row_group, sampling_rate, halfwidth, threshold_mode=0,
                    mad_multiplier=8.0, thresholds=None):
        self.mode = threshold_mode
        return pr.pick_rows(onsets, windows, row_group, sampling_rate, halfwidth, threshold_mode, mad_multiplier,
                            thresholds)


class Halfwidths:
    def gaussian_halfwidth(self, phase):
        return {"P": 5.0, "S": 10.0}[phase]


@pytest.mark.parametrize("method", ["MAD", "percentile"])
def test_device_picker_returns_the_references_table(fam, method):
    """The reference's loop (gaussian.py:171-228) written out on the restatement's pieces: windows from the origin
    time and the traveltimes, thresholds by the picker's method, -1 where no pick is made."""
    from quakemigrate_amd.picks import DevicePicker

    rows = np.concatenate([np.arange(0, 6), 80 + np.arange(0, 6)])
    onsets, rate, mw, fraction = fam["onsets"][rows], 50, 1.0, 0.1
    keys = [f"ST{r % 80}_{'P' if r < 80 else 'S'}" for r in rows]
    start = dt.datetime(2024, 5, 17, 10, 0, 0)
    otime = start + dt.timedelta(seconds=1.0)
    traveltimes = (fam["windows"][rows, 1] / rate) - 1.0                 # the family's arrivals, as traveltimes
    picker = DevicePicker(Halfwidths(), threshold_method=method, percentile_pick_threshold=0.99, fraction_tt=fraction)
    eng = RestatedEngine()
    table = picker.pick(eng, onsets, keys, start, rate, otime, mw, traveltimes)
    assert eng.mode == (0 if method == "MAD" else 1)
    picked = 0
    for station in dict.fromkeys(k.split("_")[0] for k in keys):
        st_rows = [i for i, k in enumerate(keys) if k.split("_")[0] == station]
        raw = []
        for i in st_rows:
            arrival = int(round((1.0 + traveltimes[i]) * rate))
            half = int(round((traveltimes[i] * fraction + mw) * rate))
            raw.append([arrival - half, arrival, arrival + half])
        windows = pr.distinguish_windows(raw, onsets.shape[1])
        for i, window in zip(st_rows, windows):
            assert table["pick_windows"][i].tolist() == window
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                thr = pr.find_pick_threshold(onsets[i], windows, method, 8.0, 0.99)
            assert table["thresholds"][i] == thr
            status, out = pr.pick_row(onsets[i], window, thr, float(rate), Halfwidths().gaussian_halfwidth(keys[i][-1]))
            assert table["status"][i] == status
            assert table["ModelledTime"][i] == otime + dt.timedelta(seconds=float(traveltimes[i]))
            if status == 0:
                picked += 1
                assert table["PickTime"][i] == start + dt.timedelta(seconds=float(out[1]))
                assert (table["PickError"][i], table["SNR"][i]) == (out[2], out[0])
                assert table["Residual"][i] == (table["PickTime"][i] - table["ModelledTime"][i]).total_seconds()
            else:
                assert all(table[c][i] == -1 for c in ("PickTime", "PickError", "SNR", "Residual"))
    assert picked >= 4
    with pytest.raises(ValueError, match="fraction_tt"):
        DevicePicker(Halfwidths()).pick(eng, onsets, keys, start, rate, otime, mw, traveltimes)
    with pytest.raises(ValueError, match="threshold_method"):
        DevicePicker(Halfwidths(), threshold_method="mean")


# -- the C ABI and the binding ----------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_refuses_without_a_device(lib):
    import ctypes

    assert hasattr(lib.qmlib, "qm_engine_pick_phases")
    from conftest import ROOT

    assert "int qm_engine_pick_phases(" in (ROOT / "include" / "qmhip.h").read_text()
    picks, status = np.full((2, 8), 7.0), np.full(2, 7, dtype=np.int32)
    onsets, windows = np.ones((2, 50)), np.array([[5, 10, 20], [5, 10, 20]], dtype=np.int32)
    groups, half = np.zeros(2, dtype=np.int32), np.ones(2)
    vp = ctypes.c_void_p
    rc = lib.qmlib.qm_engine_pick_phases(vp(None), onsets.ctypes.data_as(vp), 0, 2, 50, windows.ctypes.data_as(vp),
                                         groups.ctypes.data_as(vp), 50.0, half.ctypes.data_as(vp), 0, 8.0, vp(None),
                                         picks.ctypes.data_as(vp), status.ctypes.data_as(vp))
    assert rc != 0 and b"NULL argument" in lib.qmlib.qm_last_error()
    assert np.all(picks == 7.0) and np.all(status == 7)


def test_binding_checks_shapes_and_types_before_the_call(lib):
    eng = lib.Engine.__new__(lib.Engine)                # no device here: the checks come before the C call
    eng._h, eng.device = None, 0
    onsets, windows = np.ones((2, 50)), np.array([[5, 10, 20], [5, 10, 20]], dtype=np.int32)
    groups, half = np.zeros(2, dtype=np.int32), np.ones(2)
    with pytest.raises(ValueError, match="windows of shape"):
        eng.pick_phases(onsets, windows[:1], groups, 50.0, half)
    with pytest.raises(ValueError, match="row_group of shape"):
        eng.pick_phases(onsets, windows, groups[:1], 50.0, half)
    with pytest.raises(ValueError, match="halfwidth of shape"):
        eng.pick_phases(onsets, windows, groups, 50.0, np.ones(3))
    with pytest.raises(ValueError, match="thresholds of shape"):
        eng.pick_phases(onsets, windows, groups, 50.0, half, threshold_mode=1, thresholds=np.ones(3))
    with pytest.raises(TypeError):
        eng.pick_phases(onsets.astype(np.float32), windows, groups, 50.0, half)
    with pytest.raises(ValueError, match="contiguous"):
        eng.pick_phases(np.ones((2, 100))[:, ::2], windows, groups, 50.0, half)
    with pytest.raises(lib.QMHipError, match="NULL argument"):      # the engine handle is NULL
        eng.pick_phases(onsets, windows, groups, 50.0, half)
