# -*- coding: utf-8 -*-
"""
Every owner of device memory gives all of it back (csrc/qm_engine.hpp: the owning handles): after engines, streams,
replicas and a group have been used and closed, the pool's count of bytes handed out on the device
(``Engine.get("pool_live_bytes")``: process-local, deterministic) is what it was before -- exactly, twice over, the
second time on recycled blocks -- and the second cycle's results are the first one's bit for bit.
"""

import numpy as np
import pytest

from quakemigrate_amd import synth
from test_gpu_parity import RTOL, SCREEN_NORM, _assert_series

pytestmark = pytest.mark.gpu

RATE = 50
TRACE_ROW = np.array([0, 1, 2, 3, 4, 4, 5, 6, 6, 7, 8, 8], dtype=np.int32)      # 9 rows (4 P, 5 S), 12 traces
TRACE_PHASE = tuple("PPPPSSSSSSSS")
RAW_RATE = (50, 100, 40, 100, 50, 40, 100, 40, 50, 100, 50, 40)                # pass-through, d = 2, u = 5 then d = 4
PUSHES = 4


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    assert _lib.qmlib.qm_device_count() >= 1, "no HIP device visible"
    return _lib


@pytest.fixture(scope="module")
def setup(oracle):
    import resample_ref as rr
    from quakemigrate_amd.preprocess import OnsetStage, ResampleStage

    case = synth.make_case("C2", grid=(12, 11, 9), rows=9, n_samples=130)
    other = synth.make_case("C2", step=2, grid=(10, 7, 8), rows=9, n_samples=130)      # the table cache's second table
    T = case.onsets.shape[1]
    onset = OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 12.0, 2)},
                       sta_lta_windows={"P": (0.2, 1.0), "S": (0.3, 1.5)}, trace_row=TRACE_ROW,
                       trace_phase=TRACE_PHASE, row_phase=tuple("PPPPSSSSS"), taper_pad=20)
    n_raw = [(T - 1) * r // RATE + 1 for r in RAW_RATE]
    resample = ResampleStage(RATE, RAW_RATE, n_raw, [0.0] * len(RAW_RATE), upfactor=5)
    raws = [rr.raw_traces(500 + 31 * k, n_raw, np.int32) for k in range(PUSHES)]
    return {
        "case": case, "other": other, "T": T, "onset": onset, "resample": resample, "raws": raws,
        "lon": oracle.log_onsets(case.onsets), "lon_other": oracle.log_onsets(other.onsets),
        "want": oracle.detect(case.onsets, case.traveltimes, case.fsmp, case.lsmp, case.available, threads=4),
        "want_other": oracle.detect(other.onsets, other.traveltimes, other.fsmp, other.lsmp, other.available,
                                    threads=4),
    }


def _engine_part(lib, s, results):
    case, other, lon = s["case"], s["other"], s["lon"]
    step = (case.fsmp, case.lsmp, case.available)
    ns = lon.shape[1] - case.fsmp - case.lsmp
    eng = lib.Engine(0)
    eng.load_lut(case.traveltimes)
    series = eng.detect(lon, *step)
    _assert_series(series, s["want"])
    vol = eng.migrate(lon, *step, np.zeros((eng.n_nodes, ns)))
    marg = eng.marginal_map(lon, *step, 3, ns - 3)
    np.testing.assert_allclose(marg.reshape(-1), vol[:, 3:ns - 3].sum(axis=1), rtol=1e-12)
    results += [*series, vol, marg]
    # the staged calls: the first raw step's traces resampled, filtered, turned into onset rows
    a = s["onset"].arrays(s["T"], RATE)
    signals = eng.resample(s["raws"][0], s["resample"], t_samples=s["T"])
    filtered = eng.preprocess(signals, a["trace_filter"], a["sos"], taper=(a["taper_left"], a["taper_right"]))
    raw_on, log_on = eng.onsets(filtered, a["trace_row"], a["nsta"], a["nlta"], taper_pad=a["taper_pad"],
                                min_onset_value=a["min_onset_value"])
    assert np.all(np.isfinite(log_on)) and np.ptp(raw_on) > 0
    results += [signals, filtered, raw_on, log_on]
    # the table cache, one slot: a miss with its load, another, a hit (the two trade places), an eviction
    assert not eng.select_table("a", capacity=1)
    eng.load_lut(case.traveltimes)
    assert not eng.select_table("b", capacity=1)
    eng.load_lut(other.traveltimes)
    _assert_series(eng.detect(s["lon_other"], other.fsmp, other.lsmp, other.available), s["want_other"])
    assert eng.select_table("a", capacity=1)
    hit = eng.detect(lon, *step)
    _assert_series(hit, s["want"])
    assert not eng.select_table("c", capacity=1)
    eng.load_lut(other.traveltimes)
    evicted = eng.detect(s["lon_other"], other.fsmp, other.lsmp, other.available)
    _assert_series(evicted, s["want_other"])
    assert (eng.get("table_hits"), eng.get("table_misses"), eng.get("table_evictions")) == (1, 3, 1)
    results += [*hit, *evicted]
    eng.close()

    eng = lib.Engine(0, tie_rule=1)
    eng.load_lut(case.traveltimes)
    tied = eng.detect(lon, *step)
    _assert_series(tied, s["want"])
    eng.close()
    eng = lib.Engine(0, screen=1)
    eng.load_lut(case.traveltimes)
    screened = eng.detect(lon, *step)
    eng.close()
    assert np.array_equal(screened[2], s["want"][2])
    np.testing.assert_allclose(screened[0], s["want"][0], rtol=RTOL)
    np.testing.assert_allclose(screened[1], s["want"][1], rtol=SCREEN_NORM)
    results += [*tied, *screened]


def _stream_part(lib, s, results, engine_first):
    from quakemigrate_amd.stream import StreamingDetector

    case = s["case"]
    eng = lib.Engine(0)
    eng.load_lut(case.traveltimes)
    det = StreamingDetector(eng, 9, s["T"], case.fsmp, case.lsmp, case.available, depth=2, steps_per_launch=2)
    a = s["onset"].arrays(s["T"], RATE)
    orphan = dict(a, trace_row=np.where(a["trace_row"] == 2, 1, a["trace_row"]).astype(np.int32))
    # (refused by the onset record's build, after the pre-processing record has taken its device arrays)
    with pytest.raises(lib.QMHipError, match="row 2 has no trace"):
        det.set_onset_stage(orphan)
    det.set_onset_stage(s["onset"], RATE)
    det.set_resample_stage(s["resample"])
    got = det.run(s["raws"])
    assert len(got) == PUSHES and np.ptp(got[0][0]) > 0
    results += [x for triple in got for x in triple]
    for closing in ((eng, det) if engine_first else (det, eng)):    # (the engine first: the stream is orphaned)
        closing.close()


def _replicas_part(lib, s, results):
    from quakemigrate_amd.stream import StreamingDetector

    case = s["case"]
    reps = lib.EngineReplicas([0, 0])
    reps.load_lut(case.traveltimes)
    det = StreamingDetector(reps, 9, s["T"], case.fsmp, case.lsmp, case.available, depth=2, steps_per_launch=1)
    got = det.run([s["lon"]] * 3)
    det.close()
    reps.close()
    for triple in got:
        _assert_series(triple, s["want"])
    results += [x for triple in got for x in triple]


def _group_part(lib, s, results):
    case, lon = s["case"], s["lon"]
    step = (case.fsmp, case.lsmp, case.available)
    ns = lon.shape[1] - case.fsmp - case.lsmp
    g = lib.EngineGroup([0, 0])
    g.load_lut(case.traveltimes)
    series = g.detect(lon, *step)
    marg = g.marginal_map(lon, *step, 3, ns - 3)
    g.close()
    _assert_series(series, s["want"])
    assert np.ptp(marg) > 0
    results += [*series, marg]


def test_everything_closed_leaves_the_pool_as_it_was(lib, setup):
    probe = lib.Engine(0)
    try:
        lib.release_cached_memory()
        base = probe.get("pool_live_bytes")
        cycles = []
        for cycle in range(2):
            results = []
            _engine_part(lib, setup, results)
            assert probe.get("pool_live_bytes") == base, ("engine", cycle)
            _stream_part(lib, setup, results, engine_first=cycle == 1)
            assert probe.get("pool_live_bytes") == base, ("stream", cycle)
            _replicas_part(lib, setup, results)
            assert probe.get("pool_live_bytes") == base, ("replicas", cycle)
            _group_part(lib, setup, results)
            assert probe.get("pool_live_bytes") == base, ("group", cycle)
            cycles.append([np.array(x) for x in results])
        assert len(cycles[0]) == len(cycles[1])
        for k, (first, second) in enumerate(zip(*cycles)):
            assert np.array_equal(first, second), k
    finally:
        probe.close()
