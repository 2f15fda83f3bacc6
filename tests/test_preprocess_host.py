# -*- coding: utf-8 -*-
"""
Host checks of the pre-processing stage: the NumPy restatement the GPU tests compare against
(tests/preprocess_ref.py) is pinned to SciPy, the Python helpers behave as documented, and the C ABI carries the new
symbols.  No GPU needed.
"""

import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT
import preprocess_ref as pr

NEW_SYMBOLS = ("qm_engine_preprocess", "qm_stream_set_onset_stage", "qm_stream_push_signals")


@pytest.mark.parametrize("rate", [20, 50, 100])
@pytest.mark.parametrize("corners", [1, 2, 3, 4])
def test_restated_sosfilt_is_scipys_bit_for_bit(rate, corners):
    signal = pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import butter_bandpass_sos

    sos = butter_bandpass_sos(0.1 * rate, 0.4 * rate, rate, corners)
    assert sos.shape == (corners, 6) and np.all(sos[:, 3] == 1.0)
    for n in (64, 301, 2048):
        x = pr.noisy_traces(100 * corners + n, 3, n)
        forward = signal.sosfilt(sos, x, axis=-1)
        assert np.array_equal(pr.sosfilt(sos, x), forward)
        both = signal.sosfilt(sos, forward[:, ::-1], axis=-1)[:, ::-1]
        assert np.array_equal(pr.sosfilt_zero_phase(sos, x), both)
        assert np.array_equal(pr.sosfilt_zero_phase(sos, x[0]), both[0])      # (a single trace as well)


@pytest.mark.parametrize("n", [64, 301, 2048])
def test_restated_detrend_is_scipys_applied_twice(n):
    signal = pytest.importorskip("scipy.signal")
    x = pr.noisy_traces(n, 4, n)
    want = signal.detrend(signal.detrend(x, axis=-1, type="linear"), axis=-1, type="constant")
    bound = 4 * n * 2.0 ** -53 * np.max(np.abs(x))
    err = np.max(np.abs(pr.detrend(x) - want))
    print(f"n = {n}: max |restated - scipy| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_restated_taper_weights_only_the_ends():
    x = np.ones((2, 10))
    y = pr.taper(x, [0.0, 0.5], [0.25, 0.125, 0.0])
    assert np.array_equal(y[0], [0.0, 0.5, 1, 1, 1, 1, 1, 0.25, 0.125, 0.0])
    assert np.array_equal(pr.taper(x, [], []), x)


def test_bandpass_refuses_a_corner_at_or_above_nyquist():
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import butter_bandpass_sos

    for highcut in (25.0, 30.0):
        with pytest.raises(ValueError, match="Nyquist"):
            butter_bandpass_sos(2.0, highcut, 50, 2)
    assert butter_bandpass_sos(2.0, 24.9, 50, 2).shape == (2, 6)


@pytest.mark.parametrize("npts,p", [(301, 0.05), (2049, 0.05), (700, 0.1), (10, 0.05), (64, 0.5)])
def test_cosine_taper_sides(npts, p):
    from quakemigrate_amd.preprocess import cosine_taper_sides

    left, right = cosine_taper_sides(npts, p)
    m = int(p * npts)
    assert left.shape == right.shape == (m,)
    for ramp in (left, right[::-1]):
        assert np.all(ramp >= 0.0) and np.all(ramp <= 1.0)
        assert np.all(np.diff(ramp) > 0.0)
    assert np.array_equal(left, right[::-1])
    if m:
        assert left[0] == 0.0


def test_onset_stage_arrays():
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import OnsetStage

    stage = OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 12.0, 2)},
                       sta_lta_windows={"P": (0.2, 1.0), "S": (0.3, 1.5)},
                       trace_row=(0, 1, 1, 2, 3, 3), trace_phase=("P", "S", "S", "P", "S", "S"),
                       row_phase=("P", "S", "P", "S"))
    a = stage.arrays(700, 50)
    assert a["sos"].shape == (2, 2, 6)
    assert a["trace_filter"].tolist() == [0, 1, 1, 0, 1, 1]
    assert a["nsta"].tolist() == [11, 16, 11, 16] and a["nlta"].tolist() == [51, 76, 51, 76]
    assert len(a["taper_left"]) == len(a["taper_right"]) == 35
    same = OnsetStage(filters={"P": [2.0, 16.0, 2], "S": [2.0, 12.0, 2]},
                      sta_lta_windows={"P": [0.2, 1.0], "S": [0.3, 1.5]},
                      trace_row=[0, 1, 1, 2, 3, 3], trace_phase=list("PSSPSS"), row_phase=list("PSPS"))
    assert same == stage and hash(same) == hash(stage)
    assert dataclasses_replace(stage, position="centred") != stage
    with pytest.raises(ValueError, match="envelope"):
        dataclasses_replace(stage, transform="env")
    with pytest.raises(ValueError, match="corners"):
        dataclasses_replace(stage, filters={"P": (2.0, 16.0, 2), "S": (2.0, 12.0, 4)})


def dataclasses_replace(obj, **changes):
    import dataclasses

    return dataclasses.replace(obj, **changes)


def test_header_declares_and_library_exports_the_new_symbols():
    import __graft_entry__ as g

    g.build_engine()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qmhip.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(ROOT / "quakemigrate_amd" / "csrc" / "libqmhip.so"))
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"include/qmhip.h does not declare {name}"
        assert hasattr(lib, name), f"libqmhip.so does not export {name}"
