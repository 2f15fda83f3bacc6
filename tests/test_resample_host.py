# -*- coding: utf-8 -*-
"""
Host checks of the resampling stage: the NumPy restatement the GPU tests compare against (tests/resample_ref.py) is
pinned to SciPy and to a direct evaluation of the interpolation expression, ``ResampleStage`` plans the reference's
documented case as the reference's rules say, and the C ABI carries the new symbols.  No GPU needed.
"""

import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT
import preprocess_ref as pr
import resample_ref as rr

NEW_SYMBOLS = ("qm_engine_resample", "qm_stream_set_resample_stage", "qm_stream_push_raw")


def test_restated_lowpass_is_scipys_forward_backward_bit_for_bit():
    signal = pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import butter_lowpass_sos

    sos = butter_lowpass_sos(25 / 1.0000005, 100)
    assert sos.shape == (1, 6) and sos[0, 3] == 1.0            # two corners: one section
    for n in (2, 64, 301, 2048):
        x = pr.noisy_traces(n, 3, n)
        both = signal.sosfilt(sos, signal.sosfilt(sos, x, axis=-1)[:, ::-1], axis=-1)[:, ::-1]
        assert np.array_equal(rr.lowpassed(x, sos, detrend_on=False), both)
        assert np.array_equal(rr.lowpassed(x[1], sos, detrend_on=False), both[1])


def test_lowpass_is_built_as_documented_and_refuses_a_corner_at_nyquist():
    signal = pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import butter_lowpass_sos

    z, p, k = signal.iirfilter(2, (50 / 2.000001) / 100.0, btype="lowpass", ftype="butter", output="zpk")
    assert np.array_equal(butter_lowpass_sos(50 / 2.000001, 200), signal.zpk2sos(z, p, k))
    assert butter_lowpass_sos(10.0, 100, corners=4).shape == (2, 6)
    for freq in (50.0, 60.0, 0.0):
        with pytest.raises(ValueError, match="Nyquist"):
            butter_lowpass_sos(freq, 100)


@pytest.mark.parametrize("n", [64, 301, 2048])
def test_restated_detrend_is_scipys_applied_twice(n):
    """The bound of tests/test_preprocess_host.py: 4 n 2^-53 max|x|."""
    signal = pytest.importorskip("scipy.signal")
    x = pr.noisy_traces(n + 5, 4, n)
    want = signal.detrend(signal.detrend(x, axis=-1, type="linear"), axis=-1, type="constant")
    bound = 4 * n * 2.0 ** -53 * np.max(np.abs(x))
    got = rr.lowpassed(x, np.array([[1.0, 0, 0, 1, 0, 0]]))    # (an identity section: the detrend alone)
    err = np.max(np.abs(got - want))
    print(f"n = {n}: max |restated - scipy| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("dtype", [np.int32, np.float64])
@pytest.mark.parametrize("u", [2, 3, 5])
def test_restated_upsample_is_the_expression_evaluated_by_numpy(u, dtype):
    for n in (1, 2, 3, 65, 601):
        x = rr.raw_traces(10 * u + n, [n], dtype)[0]
        assert x.dtype == dtype
        want = np.zeros((n - 1) * u + 1)
        want[::u] = x
        for i in range(1, u):                                   # whole-array arithmetic: NumPy's own rounding
            want[i::u] = (i / u) * x[1:] + ((u - i) / u) * x[:-1]
        got = rr.upsample(x, u)
        assert got.dtype == np.float64 and np.array_equal(got, want), (u, n)


def test_restated_pads_and_kept_slice():
    x = np.array([3, 5, 9], dtype=np.int32)
    assert np.array_equal(rr.kept_series(x, 2, 2, 1, 0, 8), [3, 3, 3, 4, 5, 7, 9, 9])
    assert np.array_equal(rr.kept_series(x, 2, 2, 1, 1, 5), [3, 3, 4, 5, 7])
    assert np.array_equal(rr.kept_series(x, 1, 0, 0, 1, 2), [5, 9])
    rec = np.array([rr.record(0, 3, up=2, pad_left=2, pad_right=1, out_first=1)])
    assert np.array_equal(rr.resample(x, rec, None, None, None, 6), [[3, 3, 4, 5, 7, 9]])


# -- the plan ----------------------------------------------------------------------------------------------------------
T = 501                                                         # 10 s at 50 Hz


def _plan(raw_rate, n_raw, first_offset, **kw):
    from quakemigrate_amd.preprocess import ResampleStage

    return ResampleStage(50, raw_rate, n_raw, first_offset, **kw)


def test_resample_stage_plans_the_documented_case():
    """40 / 50 / 100 Hz to 50 Hz with upfactor = 5."""
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import RESAMPLE_FIELDS, butter_lowpass_sos, cosine_taper_sides

    assert RESAMPLE_FIELDS == rr.FIELDS
    stage = _plan([50, 100, 40], [501, 1001, 401], [0.0, 0.0, 0.0], upfactor=5)
    a = stage.arrays(T)
    rec = {name: a["records"][:, k] for k, name in enumerate(RESAMPLE_FIELDS)}
    assert a["records"].dtype == np.int64 and a["t_samples"] == T and a["total_raw_samples"] == 1903
    assert list(rec["raw_offset"]) == [0, 501, 1502] and list(rec["n_raw"]) == [501, 1001, 401]
    assert list(rec["up"]) == [1, 1, 5] and list(rec["dec"]) == [1, 2, 4]
    assert list(rec["pad_left"]) == [0, 0, 0] and list(rec["pad_right"]) == [0, 0, 0]
    assert list(rec["up_first"]) == [0, 0, 0] and list(rec["n_up"]) == [501, 1001, 2001]
    assert list(rec["out_first"]) == [0, 0, 0]
    for n_up, d, o in zip(rec["n_up"], rec["dec"], rec["out_first"]):
        assert -(-n_up // d) - o == T                           # every planned length is t_samples
    # one low-pass per rate that is decimated (100 Hz; 40 x 5 = 200 Hz), one taper per kept length
    assert a["sos_lp"].shape == (2, 1, 6)
    assert np.array_equal(a["sos_lp"][rec["lowpass"][1]], butter_lowpass_sos(50 / 2.000001, 100))
    assert np.array_equal(a["sos_lp"][rec["lowpass"][2]], butter_lowpass_sos(50 / 2.000001, 200))
    assert a["taper_table"].dtype == np.int32 and a["taper_table"].shape == (2, 2)
    for i in (1, 2):
        left, right = rr.taper_of(a["taper_table"], a["taper_weights"], rec["taper"][i])
        want = cosine_taper_sides(int(rec["n_up"][i]))
        assert np.array_equal(left, want[0]) and np.array_equal(right, want[1])
    # traces that reach beyond the window are trimmed to it
    wide = _plan([50, 100, 40], [511, 1021, 409], [-0.1, -0.1, -0.1], upfactor=5).arrays(T)
    rec = {name: wide["records"][:, k] for k, name in enumerate(RESAMPLE_FIELDS)}
    assert list(rec["up_first"]) == [5, 0, 20] and list(rec["n_up"]) == [501, 1021, 2001]
    assert list(rec["out_first"]) == [0, 5, 0]
    # two stages that plan the same work are equal, and hashable
    assert stage == _plan((50, 100, 40), (501, 1001, 401), (0, 0, 0), upfactor=5) and hash(stage) == hash(stage)


def test_resample_stage_pads_only_strictly_inside_one_raw_sample():
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import resample_pads

    u = 5
    # starts 0.6 raw samples late and ends 0.4 early: 400 samples at 40 Hz
    late = _plan([40], [400], [0.6 / 40], upfactor=u).arrays(T)["records"][0]
    assert list(late[[2, 3, 4, 5, 6, 7, 10]]) == [u, round(0.6 * u), round(0.4 * u), 0, 2001, 4, 0]
    assert resample_pads(0.6 / 40, 0.4 / 40, 40, u) == (3, 2)
    assert resample_pads(0.0, 0.0, 40, u) == (0, 0)             # exactly on the window's start and end
    assert resample_pads(1.0 / 40, 1.0 / 40, 40, u) == (0, 0)   # a full raw sample inside
    assert resample_pads(-0.01, 3.0, 40, u) == (0, 0)           # reaching out of the window, floating inside it
    # a whole raw sample that arrives a rounding error short of one is still a whole sample (nanosecond stamps)
    short = 0.3 - (0.1 + 7 / 40)                                # 0.025 in exact arithmetic
    assert short < 1.0 / 40
    assert resample_pads(0.0, short, 40, u) == (0, 0)
    assert resample_pads(0.025 - 1e-12, 0.025 + 1e-12, 40, u) == (0, 0)
    assert resample_pads(0.025 - 2e-9, 0.0, 40, u) == (5, 0)
    on_time = _plan([40], [401], [0.0], upfactor=u).arrays(T)["records"][0]
    assert list(on_time[[3, 4]]) == [0, 0]
    # a trace a full raw sample late gets no pad -- and so cannot fill the window
    with pytest.raises(ValueError, match="trace 0.*the window holds 501"):
        _plan([40], [400], [1.0 / 40], upfactor=u).arrays(T)


def test_resample_stage_refuses_rates_it_cannot_reach():
    pytest.importorskip("scipy.signal")
    with pytest.raises(ValueError, match="trace 1: 40 Hz"):
        _plan([50, 40], [501, 401], [0.0, 0.0]).arrays(T)
    with pytest.raises(ValueError, match="trace 1: 40 Hz.*upfactor = 3"):
        _plan([50, 40], [501, 401], [0.0, 0.0], upfactor=3).arrays(T)
    with pytest.raises(ValueError, match="trace 0.*give 500 samples"):
        _plan([100], [999], [0.0]).arrays(T)
    with pytest.raises(ValueError, match="one entry per trace"):
        _plan([100, 50], [999], [0.0])


# -- the C ABI and the Python layer ------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_symbols():
    import __graft_entry__ as g

    g.build_engine()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qmhip.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(ROOT / "quakemigrate_amd" / "csrc" / "libqmhip.so"))
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"include/qmhip.h does not declare {name}"
        assert hasattr(lib, name), f"libqmhip.so does not export {name}"


def test_ctypes_argtypes_are_set():
    from quakemigrate_amd.core import lib

    assert len(lib.qmlib.qm_engine_resample.argtypes) == 18
    assert len(lib.qmlib.qm_stream_set_resample_stage.argtypes) == 14
    assert len(lib.qmlib.qm_stream_push_raw.argtypes) == 2
    for name in ("Engine", "EngineReplicas"):
        assert callable(getattr(getattr(lib, name), "resample"))
    from quakemigrate_amd.stream import StreamingDetector

    assert callable(StreamingDetector.push_raw) and callable(StreamingDetector.set_resample_stage)


def test_python_refusals_that_need_no_device():
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd.core import lib

    stage = _plan([50, 100], [501, 1001], [0.0, 0.0])
    a = stage.arrays(T)
    with pytest.raises(ValueError, match="t_samples"):
        lib.resample_arrays(stage)                              # a stage without the window length
    with pytest.raises(ValueError, match="planned for windows of 501"):
        lib.resample_arrays(a, 500)
    with pytest.raises(ValueError, match="records of shape"):
        lib.resample_arrays(dict(a, records=a["records"][:, :10]))
    with pytest.raises(ValueError, match="sos_lp of shape"):
        lib.resample_arrays(dict(a, sos_lp=a["sos_lp"][0]))
    records, total = a["records"], a["total_raw_samples"]
    good = [np.zeros(501, dtype=np.int32), np.zeros(1001, dtype=np.int32)]
    assert lib.pack_raw(good, records, total).shape == (1502,)
    with pytest.raises(ValueError, match="1 raw traces, the stage plans 2"):
        lib.pack_raw(good[:1], records, total)
    with pytest.raises(ValueError, match="raw trace 1 .*plans 1001"):
        lib.pack_raw([good[0], good[1][:-1]], records, total)
    with pytest.raises(TypeError, match="raw trace 1: expected int32"):
        lib.pack_raw([good[0], good[1].astype(np.float64)], records, total, np.int32)
    with pytest.raises(TypeError, match="int32 or float64"):
        lib.pack_raw(np.zeros(1502, dtype=np.float32), records, total)
    with pytest.raises(ValueError, match="at least 1502"):
        lib.pack_raw(np.zeros(1501), records, total)
