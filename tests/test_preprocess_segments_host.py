# -*- coding: utf-8 -*-
"""
Host checks of the pre-processing of gappy traces: ``plan_segments`` against hand-written records and its refusals,
``OnsetStage(fill_gaps=...)``, the per-segment restatement the GPU tests compare against
(tests/preprocess_segments_ref.py) against the reference's own sequence in NumPy / SciPy order, and the C ABI's new
symbols.  No GPU needed.
"""

import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT
import preprocess_ref as pr
import preprocess_segments_ref as sr

NEW_SYMBOLS = ("qm_engine_preprocess_segments", "qm_stream_set_segment_feed", "qm_stream_push_segments")


def _weights(*lengths, p=0.05):
    from quakemigrate_amd.preprocess import cosine_taper_sides

    parts = [np.concatenate(cosine_taper_sides(n, p)) for n in lengths]
    return np.concatenate(parts) if parts else np.zeros(0)


def test_plan_gaps_at_the_start_in_the_middle_and_at_the_end():
    from quakemigrate_amd.preprocess import SEGMENT_FIELDS, plan_segments

    assert SEGMENT_FIELDS[:7] == ("trace", "first", "n", "fill_before", "fill_after", "w_offset", "m")
    # trace 0: a gap at the start; trace 1: one in the middle; trace 2: one at the end; trace 3: all three
    segments = [(0, 40, 260), (1, 0, 100), (1, 140, 160), (2, 0, 200), (3, 20, 100), (3, 160, 100)]
    records, weights = plan_segments(300, 4, segments)
    # distinct lengths in order of appearance: 260 (m 13, at 0), 100 (m 5, at 26), 160 (m 8, at 36), 200 (m 10, at 52)
    assert records.dtype == np.int64 and records.tolist() == [
        [0, 40, 260, 40, 0, 0, 13, 0],
        [1, 0, 100, 0, 0, 26, 5, 0],
        [1, 140, 160, 40, 0, 36, 8, 0],
        [2, 0, 200, 0, 100, 52, 10, 0],
        [3, 20, 100, 20, 0, 26, 5, 0],
        [3, 160, 100, 40, 40, 26, 5, 0],
    ]
    assert np.array_equal(weights, _weights(260, 100, 160, 200))


def test_plan_two_segments_one_sample_apart():
    from quakemigrate_amd.preprocess import plan_segments

    records, weights = plan_segments(301, 1, [(0, 0, 150), (0, 151, 150)])
    assert records.tolist() == [[0, 0, 150, 0, 0, 0, 7, 0], [0, 151, 150, 1, 0, 0, 7, 0]]
    assert np.array_equal(weights, _weights(150))


def test_plan_short_segments():
    from quakemigrate_amd.preprocess import plan_segments

    # 1, 19, 20 and 21 samples: m = 0, 0, 1, 1 -- the one-sample ramps weigh their sample with 0
    records, weights = plan_segments(100, 2, [(0, 0, 1), (0, 10, 19), (1, 5, 20), (1, 30, 21)])
    assert records.tolist() == [
        [0, 0, 1, 0, 0, 0, 0, 0],
        [0, 10, 19, 9, 71, 0, 0, 0],
        [1, 5, 20, 5, 0, 0, 1, 0],
        [1, 30, 21, 5, 49, 2, 1, 0],
    ]
    assert weights.tolist() == [0.0, 0.0, 0.0, 0.0]
    # the segments of several traces may come interleaved: a trace's own stay in ascending order
    mixed, _ = plan_segments(100, 2, [(1, 5, 20), (0, 0, 1), (1, 30, 21), (0, 10, 19)])
    assert sorted(mixed[:, :5].tolist()) == sorted(records[:, :5].tolist())


def test_plan_taper_percentage_and_tiling():
    from quakemigrate_amd.preprocess import plan_segments

    segments = [(0, 3, 64), (0, 70, 129), (1, 0, 200), (2, 199, 1)]
    records, weights = plan_segments(200, 3, segments, taper_percentage=0.1)
    assert records[:, 6].tolist() == [6, 12, 20, 0]
    assert np.array_equal(weights, _weights(64, 129, 200, p=0.1))
    covered = np.zeros((3, 200), dtype=int)
    for tr, first, n, before, after, *_ in records.tolist():
        covered[tr, first - before:first + n + after] += 1
    assert np.all(covered == 1)


@pytest.mark.parametrize("segments,text", [
    ([(0, 0, 50), (0, 40, 50), (1, 0, 100)], "segment 1: samples [40, 90) of trace 0 overlap, touch or precede"),
    ([(0, 0, 50), (0, 50, 50), (1, 0, 100)], "segment 1: samples [50, 100) of trace 0 overlap, touch or precede"),
    ([(0, 60, 40), (0, 0, 50), (1, 0, 100)], "segment 1: samples [0, 50) of trace 0 overlap, touch or precede"),
    ([(0, 0, 50), (1, 90, 11)], "segment 1: samples [90, 101) of trace 1 leave the window of 100"),
    ([(0, -1, 50), (1, 0, 100)], "segment 0: samples [-1, 49) of trace 0 leave the window of 100"),
    ([(0, 10, 0), (1, 0, 100)], "segment 0: samples [10, 10) of trace 0 leave the window of 100"),
    ([(0, 0, 50), (2, 0, 100)], "segment 1: trace 2 out of range (2 traces)"),
    ([(0, 0, 50)], "trace 1 has no segment"),
])
def test_plan_refusals(segments, text):
    from quakemigrate_amd.preprocess import plan_segments

    with pytest.raises(ValueError, match=re.escape(text)):
        plan_segments(100, 2, segments)


def test_onset_stage_fill_gaps():
    pytest.importorskip("scipy.signal")
    import dataclasses

    from quakemigrate_amd.preprocess import GAP_FILL_VALUE, OnsetStage

    stage = OnsetStage(filters={"P": (2.0, 16.0, 2)}, sta_lta_windows={"P": (0.2, 1.0)}, trace_row=(0, 1),
                       trace_phase=("P", "P"), row_phase=("P", "P"))
    gappy = dataclasses.replace(stage, fill_gaps=True)
    assert stage.fill_gaps is False and gappy != stage and hash(gappy) != hash(stage)
    plain, filled = stage.arrays(301, 50), gappy.arrays(301, 50)
    assert "second_taper" not in plain and "fill_value" not in plain
    assert set(filled) - set(plain) == {"second_taper", "fill_value"}
    assert filled["second_taper"] == 1
    assert filled["fill_value"] == GAP_FILL_VALUE == np.sqrt(np.finfo(float).tiny) == 2.0 ** -511 == sr.FILL
    for key in plain:
        assert np.array_equal(plain[key], filled[key])


def _case():
    from quakemigrate_amd.preprocess import butter_bandpass_sos, plan_segments

    T = 301
    segments = [(0, 0, T), (1, 0, 1), (1, T - 2, 2), (2, 5, 63), (2, 70, 64), (2, 136, 65), (2, 205, 90),
                (3, 0, 150), (3, 151, 150), (4, 17, 129), (5, 0, 19), (5, 30, 20), (5, 60, 21)]
    sos = np.stack([butter_bandpass_sos(2.0, 16.0, 50, 2), butter_bandpass_sos(1.0, 10.0, 50, 2)])
    trace_filter = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
    records, weights = plan_segments(T, 6, segments)
    return T, segments, sos, trace_filter, records, weights, sr.gappy_traces(7, 6, T, segments)


def test_restatement_is_within_the_stage_bound_of_the_reference_sequence():
    """Per segment |restated - reference order| <= ||h||_1^2 * 4 n * 2^-53 * max|x| with n the segment's length (the
    stage's bound, tests/test_preprocess_gpu.py: two passes of a filter whose forward response has l1 norm ||h||_1
    over a detrend whose sums round 4 n times); fills are 2^-511 exactly."""
    pytest.importorskip("scipy.signal")
    T, segments, sos, trace_filter, records, weights, x = _case()
    got = sr.preprocess_segments(x, trace_filter, sos, records, weights)
    want = sr.reference_order(x, trace_filter, sos, records, weights)
    assert not np.any(np.isnan(got)) and not np.any(np.isnan(want))
    data = np.zeros(x.shape, dtype=bool)
    for tr, first, n in segments:
        seg = slice(first, first + n)
        bound = pr.impulse_l1(sos[trace_filter[tr]], n) ** 2 * 4 * n * 2.0 ** -53 * np.max(np.abs(x[tr, seg]))
        err = np.max(np.abs(got[tr, seg] - want[tr, seg]))
        print(f"trace {tr} [{first}, {first + n}): max |restated - reference order| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        data[tr, seg] = True
    assert np.all(got[~data] == 2.0 ** -511) and np.all(want[~data] == 2.0 ** -511)
    assert np.count_nonzero(~data) > 0
    # the second taper is there: the ends of a tapered segment are exactly 0, as the reference's are
    assert got[0, 0] == 0.0 and got[0, T - 1] == 0.0


def test_restatement_without_second_taper_and_fill_is_the_gap_free_stage():
    pytest.importorskip("scipy.signal")
    from quakemigrate_amd.preprocess import cosine_taper_sides, plan_segments

    T, _, sos, _, _, _, _ = _case()
    x = pr.noisy_traces(3, 2, T)
    records, weights = plan_segments(T, 2, [(0, 0, T), (1, 0, T)])
    left, right = cosine_taper_sides(T)
    got = sr.preprocess_segments(x, [0, 1], sos, records, weights, second_taper=False)
    assert np.array_equal(got, pr.preprocess(x, [0, 1], sos, left, right, device_order=True))


def test_header_declares_and_library_exports_the_new_symbols():
    import __graft_entry__ as g

    g.build_engine()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qmhip.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(ROOT / "quakemigrate_amd" / "csrc" / "libqmhip.so"))
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"include/qmhip.h does not declare {name}"
        assert hasattr(lib, name), f"libqmhip.so does not export {name}"
