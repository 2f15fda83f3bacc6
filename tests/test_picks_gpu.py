# -*- coding: utf-8 -*-
"""
The phase-pick stage on the GPU (qm_engine_pick_phases, Engine.pick_phases, picks.DevicePicker,
MigrationScan.locate_compute's picker) against its NumPy restatement, tests/picks_ref.py, and against SciPy.

What is discrete -- the threshold's bits, the status, the fit range -- is held to the restatement exactly.  The
fitted values are held to the minimum itself, ``curve_fit`` with the analytic Jacobian and every tolerance at
1e-15, within the project's value tolerance of 1e-6 (amplitude and sigma relative, mean in samples); the
reference's default ``curve_fit`` call stops up to 1e-4 short of that minimum (ftol = 1.5e-8, forward differences),
so it is reported, not asserted.  tests/test_picks_host.py pins the restatement to SciPy and the reference's rules.
"""

import numpy as np
import pytest

import picks_ref as pr

pytestmark = pytest.mark.gpu

RTOL = 1e-6


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


def call(eng, d, rows=slice(None), **kw):
    return eng.pick_phases(d["onsets"][rows], d["windows"][rows], d["row_group"][rows], d["sampling_rate"],
                           d["halfwidth"][rows], **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    return np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def fam():
    return pr.family_results(n_stations=80)


@pytest.fixture(scope="module")
def fam_gpu(engine, fam):
    return call(engine, fam)


@pytest.fixture(scope="module")
def designed():
    d = pr.designed_rows()
    d["picks"], d["status"] = pr.pick_rows(d["onsets"], d["windows"], d["row_group"], d["sampling_rate"],
                                           d["halfwidth"])
    return d


def assert_discrete(got, want_picks, want_status, names=None):
    picks, status = got
    names = names if names is not None else list(range(len(status)))
    wrong = [names[r] for r in np.flatnonzero(status != want_status)]
    assert not wrong, ("status", wrong, status, want_status)
    wrong = [names[r] for r in np.flatnonzero(bits(picks[:, 0]) != bits(want_picks[:, 0]))]
    assert not wrong, ("threshold bits", wrong)
    assert np.array_equal(picks[:, 5:7], want_picks[:, 5:7]), "fit ranges"
    failed = status != 0
    assert np.all(picks[failed, 1:5] == -1.0)
    assert np.array_equal(picks[status == 0, 3], np.abs(picks[status == 0, 4]))
    assert np.all(picks[np.isin(status, (1, 2, 3, 6)), 7] == 0) and np.all(picks[np.isin(status, (0, 4, 5)), 7] >= 1)


def fitted_distances(d, picks, status, tight, default):
    """(row -> distance to the tight fit, rows left out, largest distance of the default call to the tight fit)."""
    rate, dist, left_out, default_worst = d["sampling_rate"], {}, [], 0.0
    for r in np.flatnonzero(status == 0):
        lo, hi = d["windows"][r, 0], d["windows"][r, 2]
        t, ref = tight[r], default[r]
        if isinstance(ref, Exception):
            left_out.append(int(r))                     # the reference made no pick here
            continue
        if min(abs(ref[1] * rate - lo), abs(ref[1] * rate - hi)) <= 1e-3:
            left_out.append(int(r))                     # its window test could go either way
            continue
        assert not isinstance(t, Exception), (r, t)
        dist[int(r)] = pr.fit_distance(picks[r, [1, 2, 4]], t, rate)
        default_worst = max(default_worst, pr.fit_distance(ref, t, rate))
    return dist, left_out, default_worst


# -- 1. discrete results -----------------------------------------------------------------------------------------
def test_threshold_status_and_fit_range_equal_the_restatement(fam, fam_gpu):
    assert_discrete(fam_gpu, fam["picks"], fam["status"])
    assert np.count_nonzero(fam["status"] == 0) >= 100 and np.count_nonzero(fam["status"] == 1) >= 10


# -- 2., 3. fitted values, rows left out ---------------------------------------------------------------------------
def test_fitted_values_are_the_least_squares_minimum(fam, fam_gpu):
    picks, status = fam_gpu
    dist, left_out, default_worst = fitted_distances(fam, picks, status, fam["tight"], fam["default"])
    worst = max(dist.values())
    its = picks[status == 0, 7]
    print(f"\npicked rows {len(dist)}, left out {len(left_out)}; largest distance to the tight fit {worst:.3e}; "
          f"the reference's default curve_fit is up to {default_worst:.3e} from it; iterations median "
          f"{np.median(its):.0f}, most {its.max():.0f}")
    assert len(left_out) <= 0.02 * len(status)
    assert worst <= RTOL, sorted(dist.items(), key=lambda kv: -kv[1])[:5]
    # the reference's own pick/no-pick decision on these rows
    for r in np.flatnonzero(np.isin(status, (0, 5))):
        ref = fam["default"][r]
        if isinstance(ref, Exception) or r in left_out:
            continue
        inside = fam["windows"][r, 0] < ref[1] * fam["sampling_rate"] < fam["windows"][r, 2]
        assert inside == (status[r] == 0), r


# -- 4. designed rows ----------------------------------------------------------------------------------------------
def test_designed_rows(engine, designed):
    """Every kind of row in one call (tests/picks_ref.py: designed_rows).  The row that cannot converge is a rising
    exponential up to the end of its window: the least-squares Gaussian has no minimum there (b, c -> infinity),
    the restatement spends its 200 iterations on it, and so must the kernel."""
    d = designed
    assert np.array_equal(d["status"], d["expected"]), "the restatement itself"
    assert set(d["expected"]) == {0, 1, 2, 3, 4, 6}
    got = call(engine, d)
    assert_discrete(got, d["picks"], d["status"], d["names"])
    picks, status = got
    lengths = picks[:, 6] - picks[:, 5]
    assert lengths[d["names"].index("run of two samples")] == 4
    assert lengths[d["names"].index("fit range of more than 64 points")] > 64
    assert lengths[d["names"].index("fit range of more than 256 points")] > 256
    assert picks[d["names"].index("no minimum: a rising exponential"), 7] == 200
    r = d["names"].index("tied maximum in two runs")
    assert picks[r, 5] == 287 and picks[r, 6] == 294                # the first of the two equal maxima
    r = d["names"].index("constant noise")
    assert picks[r, 0] == 1.25                                      # MAD 0: the threshold is the median
    tight, default = {}, {}
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r in np.flatnonzero(status == 0):
            x, y, p0 = pr.fit_inputs(d["onsets"][r], int(picks[r, 5]), int(picks[r, 6]), d["sampling_rate"],
                                     d["halfwidth"][r])
            tight[r], default[r] = pr.scipy_tight(x, y, p0), pr.scipy_default(x, y, p0)
    dist, left_out, _ = fitted_distances(d, picks, status, tight, default)
    print("\ndesigned rows: largest distance to the tight fit", max(dist.values()))
    assert not left_out
    assert max(dist.values()) <= RTOL, dist


def test_small_and_tied_noise_sets_have_numpys_threshold_bits(engine):
    """The median's selection at its edges (tests/picks_ref.py: noise_set_rows): noise sets of 0, 1, 2, 3, 4, 255, 256
    and 257 samples -- one pass of the workgroup's 256 threads, and one sample past it -- of distinct values, equal
    values, equal middle values, a middle value that repeats across the even split, and neighbouring bit patterns.
    tests/test_picks_host.py pins the restatement on these rows to the formula on sorted values."""
    d = pr.noise_set_rows()
    want_picks, want_status = pr.pick_rows(d["onsets"], d["windows"], d["row_group"], d["sampling_rate"],
                                           d["halfwidth"])
    assert 64 <= d["onsets"].shape[1] <= 600 and len(d["names"]) == 40
    got = call(engine, d)
    assert_discrete(got, want_picks, want_status, d["names"])
    empty = np.array([name.startswith("0 ") for name in d["names"]])
    assert np.all(np.isnan(got[0][empty, 0])) and np.all(np.isfinite(got[0][~empty, 0]))
    assert np.all(got[1] == 1)


# -- 5. modes and layouts ------------------------------------------------------------------------------------------
def test_given_thresholds_equal_the_mad_mode(engine, fam, fam_gpu):
    got = call(engine, fam, threshold_mode=1, thresholds=fam_gpu[0][:, 0].copy())
    assert same(got, fam_gpu)


def test_percentile_thresholds_go_through_mode_1(engine, fam):
    thresholds = np.array([pr.find_pick_threshold(fam["onsets"][r], fam["windows"][fam["row_group"] == g],
                                                  "percentile", percentile_pick_threshold=0.99)
                           for r, g in enumerate(fam["row_group"])])
    want = pr.pick_rows(fam["onsets"], fam["windows"], fam["row_group"], fam["sampling_rate"], fam["halfwidth"],
                        threshold_mode=1, thresholds_in=thresholds)
    assert_discrete(call(engine, fam, threshold_mode=1, thresholds=thresholds), *want)


def test_device_resident_rows_equal_host_rows(engine, fam, fam_gpu):
    import torch

    d_on = torch.from_numpy(fam["onsets"]).to("cuda:0")
    got = engine.pick_phases(d_on, fam["windows"], fam["row_group"], fam["sampling_rate"], fam["halfwidth"])
    assert same(got, fam_gpu)


def test_two_calls_are_bit_equal(engine, fam, fam_gpu, designed):
    assert same(call(engine, fam), fam_gpu)
    assert same(call(engine, designed), call(engine, designed))


def test_reused_engine_equals_a_fresh_one(lib, engine, fam, fam_gpu, designed):
    from quakemigrate_amd import synth

    case = synth.make_case("C2", step=0, grid=(26, 25, 14), n_samples=700)
    logged = np.ascontiguousarray(np.log(np.clip(case.onsets, 0.01, np.inf)))
    sos = np.array([[[0.2, 0.1, 0.05, 1.0, -0.5, 0.25]]])
    engine.load_lut(case.traveltimes)
    first = call(engine, designed)
    for _ in range(2):
        engine.detect(logged, case.fsmp, case.lsmp, case.available)
        assert same(call(engine, designed), first)
        engine.marginal_map(logged, case.fsmp, case.lsmp, case.available, 100, 200)
        assert same(call(engine, fam), fam_gpu)
        engine.preprocess(case.onsets[:5], np.zeros(5, dtype=np.int32), sos)
        assert same(call(engine, fam, rows=slice(0, 30)), call(engine, fam, rows=slice(0, 30)))
    fresh = lib.Engine(0)
    try:
        assert same(call(fresh, designed), first)
        assert same(call(fresh, fam), fam_gpu)
    finally:
        fresh.close()


def test_rows_of_two_events_share_a_call(engine, fam, fam_gpu):
    """Event A: stations 0..39, event B: stations 40..79 (P and S rows of each); B's groups renumbered from 0 in
    its single call, distinct from A's in the shared one."""
    n = len(fam["status"]) // 2
    a = np.concatenate([np.arange(0, 40), n + np.arange(0, 40)])
    b = np.concatenate([np.arange(40, 80), n + np.arange(40, 80)])
    both = call(engine, fam, rows=np.concatenate([a, b]))
    single_a = call(engine, fam, rows=a)
    d = dict(fam, row_group=fam["row_group"] - 40)
    single_b = call(engine, d, rows=b)
    assert same((both[0][:80], both[1][:80]), single_a)
    assert same((both[0][80:], both[1][80:]), single_b)
    assert same(both, (fam_gpu[0][np.concatenate([a, b])], fam_gpu[1][np.concatenate([a, b])]))


def test_longest_row_works_and_one_more_sample_is_refused(lib, engine):
    limit = engine.get("pick_lds_samples")
    assert limit >= 4096
    rng = np.random.default_rng(3)
    t = np.arange(limit, dtype=np.float64)
    onsets = 1.3 + 0.1 * rng.random((2, limit))
    centres = (limit - 40, limit // 2)
    for r, c in enumerate(centres):
        onsets[r] += 6.0 * np.exp(-((t - c) ** 2) / (2.0 * 5.0 ** 2))
    windows = np.array([[limit - 100, c, limit] if r == 0 else [c - 60, c, c + 60]
                        for r, c in enumerate(centres)], dtype=np.int32)
    args = (windows, np.array([0, 1], dtype=np.int32), 50.0, np.array([5.0, 5.0]))
    got = engine.pick_phases(onsets, *args)
    want = pr.pick_rows(onsets, windows, args[1], 50.0, args[3])
    assert_discrete(got, *want)
    assert np.all(got[1] == 0)
    assert np.max(np.abs(got[0][:, 2] - want[0][:, 2])) * 50.0 <= RTOL
    longer = np.concatenate([onsets, np.full((2, 1), 1.3)], axis=1)
    with pytest.raises(lib.QMHipError, match="LDS"):
        engine.pick_phases(longer, *args)


def test_refusals(lib, engine, fam):
    import ctypes

    d = {k: fam[k][:4].copy() for k in ("onsets", "windows", "row_group", "halfwidth")}
    T = d["onsets"].shape[1]

    def refused(match, **change):
        a = {**d, "sampling_rate": 50.0, **change}
        with pytest.raises(lib.QMHipError, match=match):
            engine.pick_phases(a["onsets"], a["windows"], a["row_group"], a["sampling_rate"], a["halfwidth"],
                               **{k: a[k] for k in ("threshold_mode",) if k in a})

    for bad, row in (((-1, 10, 50), 0), ((T - 50, T - 10, T + 1), 3), ((60, 55, 50), 2)):
        w = d["windows"].copy()
        w[row] = bad
        refused(f"row {row}: window", windows=w)
    refused("sampling_rate", sampling_rate=0.0)
    refused("sampling_rate", sampling_rate=-50.0)
    refused("threshold_mode 1 without", threshold_mode=1)
    refused("threshold_mode must be", threshold_mode=2)

    # what the binding cannot express: the C call itself, with outputs that must stay as they are
    vp = ctypes.c_void_p
    picks, status = np.full((4, 8), 7.0), np.full(4, 7, dtype=np.int32)
    ptr = {k: v.ctypes.data_as(vp) for k, v in d.items()}

    def raw(e=engine._h, onsets=ptr["onsets"], n_rows=4, t_samples=T, windows=ptr["windows"],
            groups=ptr["row_group"], rate=50.0, halfwidth=ptr["halfwidth"], mode=0, given=vp(None),
            out=picks.ctypes.data_as(vp), out_status=status.ctypes.data_as(vp)):
        return lib.qmlib.qm_engine_pick_phases(e, onsets, 0, n_rows, t_samples, windows, groups, rate, halfwidth, mode,
                                               8.0, given, out, out_status)

    for change, text in ((dict(e=vp(None)), "NULL"), (dict(onsets=vp(None)), "NULL"), (dict(windows=vp(None)), "NULL"),
                         (dict(groups=vp(None)), "NULL"), (dict(halfwidth=vp(None)), "NULL"),
                         (dict(out=vp(None)), "NULL"), (dict(out_status=vp(None)), "NULL"),
                         (dict(n_rows=0), "empty"), (dict(t_samples=0), "empty"),
                         (dict(t_samples=engine.get("pick_lds_samples") + 1), "LDS"), (dict(rate=0.0), "sampling_rate"),
                         (dict(mode=1), "without thresholds_in")):
        assert raw(**change) != 0, change
        assert text in lib.qmlib.qm_last_error().decode(), (change, lib.qmlib.qm_last_error())
    assert np.all(picks == 7.0) and np.all(status == 7)
    assert raw() == 0 and np.all(picks[:, 7] >= 0) and np.all(status < 7)


# -- 6. end to end ---------------------------------------------------------------------------------------------------
def test_locate_compute_with_a_picker_gives_the_restatements_table(lib, monkeypatch):
    """examples/locate_events.py with its DevicePicker: per located event the table equals the restatement's run on
    the same un-logged onsets, with the windows rebuilt by the reference's rules from the origin time and the
    traveltimes -- discrete columns equal, pick times within 1e-6 samples."""
    import importlib.util

    from conftest import ROOT
    from quakemigrate_amd import picks as picks_mod

    seen = []
    original = picks_mod.DevicePicker.pick

    def recording(self, engine, raw_onsets, keys, onset_starttime, sampling_rate, otime, marginal_window,
                  traveltimes, **kw):
        seen.append(dict(onsets=np.array(raw_onsets), keys=list(keys), start=onset_starttime, rate=sampling_rate,
                         otime=otime, mw=marginal_window, tt=np.array(traveltimes), halfwidth=np.array(
                             [self.onset.gaussian_halfwidth(k.rpartition("_")[2]) for k in keys]), kw=kw))
        return original(self, engine, raw_onsets, keys, onset_starttime, sampling_rate, otime, marginal_window,
                        traveltimes, **kw)

    monkeypatch.setattr(picks_mod.DevicePicker, "pick", recording)
    spec = importlib.util.spec_from_file_location("locate_events_picks", ROOT / "examples" / "locate_events.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    located, truth, record_start, rate = mod.run()
    assert len(located) == len(seen) == 4
    n_picked = 0
    for result, s in zip(located, seen):
        table = result["picks"]
        n_rows, T = s["onsets"].shape
        stations = [k.rpartition("_")[0] for k in s["keys"]]
        since = (s["otime"] - s["start"]).total_seconds()
        windows = np.zeros((n_rows, 3), dtype=np.int64)
        for station in dict.fromkeys(stations):
            rows = [r for r in range(n_rows) if stations[r] == station]
            raw = []
            for r in rows:
                arrival = int(round((since + s["tt"][r]) * int(rate)))
                half = int(round((s["tt"][r] * s["kw"]["fraction_tt"] + s["mw"]) * int(rate)))
                raw.append([arrival - half, arrival, arrival + half])
            for r, w in zip(rows, pr.distinguish_windows(raw, T)):
                windows[r] = w
        assert np.array_equal(table["pick_windows"], windows)
        assert windows[:, 0].min() >= 0 and windows[:, 2].max() <= T
        groups = np.array([list(dict.fromkeys(stations)).index(st) for st in stations], dtype=np.int32)
        want_picks, want_status = pr.pick_rows(s["onsets"], windows, groups, float(rate), s["halfwidth"])
        assert_discrete((table["fits"], table["status"]), want_picks, want_status)
        assert np.array_equal(bits(table["thresholds"]), bits(want_picks[:, 0]))
        ok = want_status == 0
        n_picked += int(ok.sum())
        assert np.max(np.abs(table["fits"][ok, 2] - want_picks[ok, 2])) * rate <= 1e-6
        np.testing.assert_allclose(table["fits"][ok, 1], want_picks[ok, 1], rtol=RTOL)
        np.testing.assert_allclose(table["fits"][ok, 3], want_picks[ok, 3], rtol=RTOL)
        assert list(table["Station"]) == stations and list(table["Phase"]) == [k[-1] for k in s["keys"]]
        for r in range(n_rows):
            assert abs((table["ModelledTime"][r] - s["otime"]).total_seconds() - s["tt"][r]) < 2e-6
            if ok[r]:
                assert abs((table["PickTime"][r] - s["start"]).total_seconds() - table["fits"][r, 2]) < 2e-6
                assert table["PickError"][r] == table["fits"][r, 3] and table["SNR"][r] == table["fits"][r, 1]
                assert table["Residual"][r] == (table["PickTime"][r] - table["ModelledTime"][r]).total_seconds()
            else:
                assert all(table[c][r] == -1 for c in ("PickTime", "PickError", "SNR", "Residual"))
    assert n_picked >= 2 * len(located) * 3             # the injected arrivals are picked on most rows
