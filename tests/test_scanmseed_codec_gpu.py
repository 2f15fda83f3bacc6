# -*- coding: utf-8 -*-
"""
The .scanmseed codec on the GPU (include/qmhip.h: qm_engine_scanmseed_encode / _decode; kernels:
csrc/qm_scanmseed.hpp) against the Python codec of quakemigrate_amd/scanmseed.py and the reference's two benchmark
files.  Every comparison is exact -- bytes, integers, the bits of the descaled floats: there is no tolerance anywhere.
"""

import datetime as dt
import shutil

import numpy as np
import pytest

import scanmseed_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

T0 = dt.datetime(2014, 6, 29, 23, 59, 0)
GOLDEN_FILES = {"icequake_iceland_2014_180.scanmseed": 11, "volcanotectonic_iceland_2014_236.scanmseed": 87}


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


@pytest.fixture(scope="module")
def sm():
    from quakemigrate_amd import scanmseed

    return scanmseed


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def five(x):
    """Five channels of one length from one series: channel j is the series held at its first sample for j samples
    (j zero differences in front: the same widths at five alignments of the chain)."""
    x = np.asarray(x, dtype=np.int32)
    return {ch: np.concatenate([np.full(j, x[0], dtype=np.int32), x])[:len(x)]
            for j, ch in enumerate(("COA", "COA_N", "X", "Y", "Z"))}


def check_codec(engine, sm, series, rate=50.0):
    """Device encode == Python encode, byte for byte; device decode of those bytes == the series.  Returns the bytes."""
    want = sm.encode_scanmseed(T0, rate, series)
    got = sm.encode_scanmseed(T0, rate, series, engine=engine)
    assert len(got) == len(want)
    assert got == want, np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[:8]
    records = np.frombuffer(got, dtype=np.uint8).reshape(-1, sm.RECLEN)
    samples = [sm.parse_header(r.tobytes())[4] for r in records]
    offsets = np.concatenate([[0], np.cumsum(samples)[:-1]])
    ints, none = engine.scanmseed_decode(records, samples, offsets, int(np.sum(samples)))
    assert none is None
    assert np.array_equal(ints, np.concatenate([series[ch] for ch in sm.CHANNELS]))
    return got


# -- 1, 2: the reference's files ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDEN_FILES))
def test_golden_files_decode_and_encode_exactly(engine, sm, name):
    path = GOLDEN / name
    start, rate, cols = sm.read_scanmseed(path, 1000.0)
    for device in (False, True):
        g_start, g_rate, g_cols = sm.read_scanmseed(path, 1000.0, engine=engine, device=device)
        assert (g_start, g_rate) == (start, rate)
        for ch in sm.CHANNELS:
            resident = device and ch in ("COA", "COA_N")
            assert hasattr(g_cols[ch], "data_ptr") == resident and hasattr(g_cols["int"][ch], "data_ptr") == resident
            got_i = g_cols["int"][ch].cpu().numpy() if resident else g_cols["int"][ch]
            got_f = g_cols[ch].cpu().numpy() if resident else g_cols[ch]
            assert got_i.dtype == np.int32 and np.array_equal(got_i, cols["int"][ch])
            assert got_f.dtype == np.float64 and np.array_equal(bits(got_f), bits(cols[ch]))
    blob = path.read_bytes()
    assert len(blob) == GOLDEN_FILES[name] * sm.RECLEN
    assert sm.encode_scanmseed(start, rate, cols["int"], engine=engine) == blob


# -- 3, 4: widths and ends ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.designed_series()))
def test_designed_series(engine, sm, name):
    check_codec(engine, sm, five(ref.designed_series()[name]))


# -- 5: tile edges ------------------------------------------------------------------------------------------------------
def test_chain_enters_a_tile_at_every_offset_and_words_straddle_the_edges(engine, sm):
    tile = engine.get("scanmseed_tile")
    n = 3 * tile + 11
    wide = (1 << 29) - 1
    entries, straddles = set(), 0
    for shifts in (range(0, 5), range(5, 10)):
        series = {}
        for ch, lead in zip(sm.CHANNELS, shifts):
            # `lead` one-difference words in front shift the chain of seven-difference words behind them
            d = np.where(np.arange(n - 1) % 2 == 0, 7, -8)
            d[:lead] = np.where(np.arange(lead) % 2 == 0, wide, -wide)
            # ... and a run of other widths across the second edge
            d[2 * tile - 9:2 * tile + 9] = [300, -300, 20, -20, 100, -100, 16000, -16000, 5] * 2
            series[ch] = x = ref.from_differences(d)
            starts = ref.chain(ref.counts(ref.width_class(ref.differences(x))))
            for edge in (tile, 2 * tile, 3 * tile):
                at = starts[np.searchsorted(starts, edge)]
                if edge == tile:
                    entries.add(int(at - edge))
                straddles += int(at != edge)
        check_codec(engine, sm, series)
    assert entries == set(range(7)) and straddles >= 12


# -- 6: random differential ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_random_switching_widths(engine, sm, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(30_000, 40_001))
    classes = [(0, 1, 2), (0, 1, 2, 3, 4), (2, 3, 4, 5), (0, 1, 2, 3, 4, 5, 6), (0, 6)]
    series = {ch: ref.switching_walk(rng, n, classes=cl, max_run=int(rng.integers(2, 60)))
              for ch, cl in zip(sm.CHANNELS, classes)}
    first = check_codec(engine, sm, series)
    assert sm.encode_scanmseed(T0, 50.0, series, engine=engine) == first        # the same bytes on every run
    # device-resident input
    import torch

    stacked = torch.from_numpy(np.stack([series[ch] for ch in sm.CHANNELS])).to(f"cuda:{engine.device}")
    out = engine.scanmseed_encode(stacked)
    assert sm.fill_headers(out["records"], out["n_records"], out["rec_first"], out["rec_count"], T0, 50.0) == first


# -- 7: refusals --------------------------------------------------------------------------------------------------------
def test_encode_refuses_by_name(engine, lib, sm):
    base = np.zeros((5, 3000), dtype=np.int32)
    x = base.copy()
    x[3, 2500:] = 1 << 29                                       # a difference of 2^29 at Y[2500]
    with pytest.raises(lib.QMHipError, match=r"channel Y, sample 2500: difference does not fit 30 bits"):
        engine.scanmseed_encode(x)
    x = base.copy()
    x[1, :2] = [-(1 << 31), (1 << 31) - 1]                      # (a 32-bit subtraction would see -1)
    x[1, 2:] = (1 << 31) - 1
    with pytest.raises(lib.QMHipError, match=r"channel COA_N, sample 1: difference does not fit 30 bits"):
        engine.scanmseed_encode(x)
    f = np.array(list(sm.scale_factors(1000.0).values()))
    clips = [sm.COA_CLIP, sm.COA_CLIP, None, None, None]
    y = np.ones((5, 3000))
    y[2, 2999] = np.nan
    with pytest.raises(lib.QMHipError, match=r"channel X, sample 2999 is NaN"):
        engine.scanmseed_encode(y, f, clips)
    y = np.ones((5, 3000))
    y[4, 17] = -2147.483649                                     # x 1e6: one below int32
    with pytest.raises(lib.QMHipError, match=r"channel Z, sample 17: the scaled value is outside int32"):
        engine.scanmseed_encode(y, f, clips)
    y[4, :] = -2147.0
    y[4, 17] = -2147.483648                                     # ... and the lowest int32 itself is taken
    engine.scanmseed_encode(y, f, clips)
    # the engine goes on working after a refusal
    check_codec(engine, sm, five(ref.designed_series()["n8"]))


def test_decode_refuses_by_record(engine, lib, sm):
    series = five(ref.switching_walk(np.random.default_rng(7), 9000, classes=(0, 1, 2, 3)))
    blob = sm.encode_scanmseed(T0, 50.0, series)
    good = np.frombuffer(blob, dtype=np.uint8).reshape(-1, sm.RECLEN)
    samples = np.array([sm.parse_header(r.tobytes())[4] for r in good])
    offsets = np.concatenate([[0], np.cumsum(samples)[:-1]])
    total = int(samples.sum())
    assert len(good) >= 8

    def python_raises(records, counts, k, text):
        with pytest.raises(ValueError, match=text):
            sm.steim2_decode(records[k, sm.DATA_OFFSET:].tobytes(), int(counts[k]))

    # the reverse integration constant of record 3, one bit flipped
    bad = good.copy()
    bad[3, sm.DATA_OFFSET + 8 + 3] ^= 1
    python_raises(bad, samples, 3, "reverse integration constant mismatch")
    with pytest.raises(lib.QMHipError, match=r"record 3: STEIM2 reverse integration constant mismatch"):
        engine.scanmseed_decode(bad, samples, offsets, total)
    # an invalid pair in record 5: code 2 with dnib 0 on the first data word of frame 1
    bad = good.copy()
    word0 = int.from_bytes(bad[5, sm.DATA_OFFSET + 64:sm.DATA_OFFSET + 68].tobytes(), "big")
    word0 = (word0 & ~(3 << 28)) | (2 << 28)
    bad[5, sm.DATA_OFFSET + 64:sm.DATA_OFFSET + 68] = np.frombuffer(word0.to_bytes(4, "big"), dtype=np.uint8)
    bad[5, sm.DATA_OFFSET + 68] &= 0x3f
    python_raises(bad, samples, 5, "invalid STEIM2 code 2 / dnib 0")
    with pytest.raises(lib.QMHipError, match=r"record 5: invalid STEIM2 code / dnib pair"):
        engine.scanmseed_decode(bad, samples, offsets, total)
    # both at once: the smaller record index is named
    bad[3, sm.DATA_OFFSET + 8 + 3] ^= 1
    with pytest.raises(lib.QMHipError, match=r"record 3: STEIM2 reverse"):
        engine.scanmseed_decode(bad, samples, offsets, total)
    # ... but an invalid pair BEHIND the record's last difference is not looked at, as in the Python
    last = len(good) - 1
    bad = good.copy()
    assert not bad[last, sm.RECLEN - 64:].any()
    bad[last, sm.RECLEN - 64:sm.RECLEN - 60] = 0xff             # codes 3 on the last frame's (unused, zero) words ...
    bad[last, sm.RECLEN - 60] = 0xc0                            # ... whose dnib 3 is invalid under code 3
    assert np.array_equal(sm.steim2_decode(bad[last, sm.DATA_OFFSET:].tobytes(), int(samples[last])),
                          sm.steim2_decode(good[last, sm.DATA_OFFSET:].tobytes(), int(samples[last])))
    ints, _ = engine.scanmseed_decode(bad, samples, offsets, total)
    assert np.array_equal(ints, np.concatenate([series[ch] for ch in sm.CHANNELS]))
    # a sample count larger than the record holds: one more than it has, and more than any record can have
    for extra in (1, 7000):
        counts = samples.copy()
        counts[6] += extra
        python_raises(good, counts, 6, "fewer differences than samples")
        with pytest.raises(lib.QMHipError, match=r"record 6 holds fewer differences than samples"):
            engine.scanmseed_decode(good, counts, offsets, total + extra)
    # the front end maps the record to the file's
    with pytest.raises(ValueError, match=r"record 3: STEIM2 reverse integration constant mismatch.*record 3 of the file"):
        bad = good.copy()
        bad[3, sm.DATA_OFFSET + 8 + 3] ^= 1
        sm._read_with_engine(bad.tobytes(), 1000.0, engine, False)
    # the engine goes on working after a refusal
    ints, _ = engine.scanmseed_decode(good, samples, offsets, total)
    assert np.array_equal(ints, np.concatenate([series[ch] for ch in sm.CHANNELS]))


# -- 8: quantise --------------------------------------------------------------------------------------------------------
def test_float_flavour_quantises_like_numpy(engine, sm):
    ucf = 1000.0
    rng = np.random.default_rng(8)
    n = 5000
    k = np.arange(n)
    # exact ties of both parities: (2 k + 1) / 64 x 1e5 = 3125 k + 1562.5, (2 k + 1) / 128 x 1e6 = 15625 k + 7812.5
    coa = (2 * (k % 400) + 1) / 64.0
    coa[:2] = [0.0, -0.0]
    coa_n = 1.0 + rng.uniform(0, 0.5, n)
    # up to the 21474 clip and across it in steps a 30-bit difference holds, values at and above it, down again
    top = [21474.0, 21474.00001, 21474.5, 3e4, 1e9, np.inf, 21473.999995, 21473.99999]
    coa[940:1000] = np.linspace(coa[939], 21473.9, 60)
    coa[1000:1400] = np.linspace(21473.9, 21474.1, 400)
    coa[1400:1408] = top
    coa[1408:1468] = np.linspace(21473.9, coa[1468], 60)
    coa_n[1900:2000] = np.linspace(coa_n[1899], 21473.0, 100)
    coa_n[2000:2003] = [21474.0, 5e4, 21473.999999]
    coa_n[2003:2103] = np.linspace(21473.0, coa_n[2103], 100)
    coord = np.stack([((2 * (k % 300) + 1) / 128.0) * np.where(k % 2, -1, 1),
                      -64.5 + np.cumsum(rng.uniform(-1e-5, 1e-5, n)),
                      (2 * (k % 50) + 1) / 128.0 - 0.25], axis=1)  # negative coordinates; ties on Z x 1e3 x ucf too
    want = sm.quantise(coa, coa_n, coord, ucf)
    assert (want["COA"] % 2 == 0).sum() > 100 and (want["COA"] % 2 == 1).sum() > 100
    assert want["COA"].max() == 2147400000 and want["X"].min() < 0 and want["Y"].min() < 0
    stacked = np.ascontiguousarray(np.stack([coa, coa_n, coord[:, 0], coord[:, 1], coord[:, 2]]))
    factors = [sm.scale_factors(ucf)[ch] for ch in sm.CHANNELS]
    clips = [sm.COA_CLIP, sm.COA_CLIP, None, None, None]
    out = engine.scanmseed_encode(stacked, factors, clips)
    got = sm.fill_headers(out["records"], out["n_records"], out["rec_first"], out["rec_count"], T0, 50.0)
    assert got == sm.encode_scanmseed(T0, 50.0, want)
    import torch

    out = engine.scanmseed_encode(torch.from_numpy(stacked).to(f"cuda:{engine.device}"), factors, clips)
    assert sm.fill_headers(out["records"], out["n_records"], out["rec_first"], out["rec_count"], T0, 50.0) == got


# -- 9: front end -------------------------------------------------------------------------------------------------------
def test_sink_with_an_engine_writes_the_same_files(engine, sm, tmp_path):
    rate, n = 50, 3000
    sinks = [sm.CoalescenceSink(tmp_path / "host", rate), sm.CoalescenceSink(tmp_path / "device", rate, engine=engine)]
    t0 = dt.datetime(2024, 2, 29, 23, 57, 30)                   # the third step crosses midnight
    rng = np.random.default_rng(3)
    for i in range(4):
        coa = 2.0 + np.cumsum(rng.uniform(-0.01, 0.01, n))
        coa[1000:1300] += np.minimum(np.arange(300), 299 - np.arange(300)) * 160.0   # a peak beyond the 21474 clip
        coa_n = 1.0 + rng.uniform(0, 0.5, n)
        coord = np.cumsum(rng.uniform(-0.01, 0.01, (n, 3)), axis=0)
        for sink in sinks:
            if i == 1:
                sink.empty(t0, 60.0, i, "gap", 1000.0)
            else:
                sink.append(t0 + dt.timedelta(seconds=60 * i), coa, coa_n, coord, 1000.0)
    for sink in sinks:
        sink.write()
        assert [p.name for p in sink.files] == ["2024_060.scanmseed", "2024_061.scanmseed"]
    for a, b in zip(sinks[0].files, sinks[1].files):
        assert a.read_bytes() == b.read_bytes() and a.stat().st_size >= 5 * sm.RECLEN


BENCHMARKS = {
    "icequake": dict(scan="icequake_iceland_2014_180.scanmseed", csv="icequake_iceland_2014_180_TriggeredEvents.csv",
                     day="2014_180.scanmseed", mw=0.06, mei=0.12, threshold=2.15,
                     start=dt.datetime(2014, 6, 29, 18, 42, 5), end=dt.datetime(2014, 6, 29, 18, 42, 15), region=None),
    "volcanotectonic": dict(scan="volcanotectonic_iceland_2014_236.scanmseed",
                            csv="volcanotectonic_iceland_2014_236_TriggeredEvents.csv", day="2014_236.scanmseed",
                            mw=0.75, mei=1.5, threshold=1.85, start=dt.datetime(2014, 8, 24, 0, 1, 0),
                            end=dt.datetime(2014, 8, 24, 0, 11, 0), region=[-17.15, 64.72, 0.0, -16.65, 64.93, 14.0]),
}


@pytest.mark.parametrize("name", sorted(BENCHMARKS))
def test_trigger_on_the_device_resident_read_gives_the_same_events(engine, sm, tmp_path, name):
    from quakemigrate_amd import trigger

    b = BENCHMARKS[name]
    shutil.copyfile(GOLDEN / b["scan"], tmp_path / b["day"])
    t = trigger.DeviceTrigger(marginal_window=b["mw"], min_event_interval=b["mei"], normalise_coalescence=True,
                              static_threshold=b["threshold"])
    t0, rate, cols = sm.read_scanmseed(tmp_path / b["day"], 1000.0)
    host = t.trigger_series(engine, t0, rate, cols, b["start"], b["end"], region=b["region"])
    host_last = t.last
    resident = t.trigger(tmp_path, b["start"], b["end"], 1000.0, region=b["region"], engine=engine)
    assert len(resident) == len(host) > 0
    assert resident == host                                     # every column of every event, floats by value
    for key in ("n_candidates", "n_events", "first_sample", "last_sample"):
        assert t.last[key] == host_last[key]
    assert np.array_equal(t.last["events_i"], host_last["events_i"])
    assert np.array_equal(bits(t.last["events_f"]), bits(host_last["events_f"]))
    recorded = trigger.read_triggered_events(GOLDEN / b["csv"])
    assert [e["EventID"] for e in resident] == [e["EventID"] for e in recorded]
