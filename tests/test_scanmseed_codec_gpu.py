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


# -- 10: past one trip of the compose and quantise loops ----------------------------------------------------------------
# sms_compose_kernel carries the chain's state (entry offset, word index) from one chunk of "scanmseed_compose_chunk"
# tiles to the next; sms_quantise_kernel strides a grid of at most QUANT_GRID threads per channel over the samples.  The
# series below are (chunk + 3) tiles + 11 samples long: two trips of the compose loop, three of the quantiser's.  Every
# test asserts on the restatement alone, before the device is asked, what makes it able to fail.
QUANT_GRID = 4096 * 256                                         # (qm_scanmseed.hip: the quantise launch's cap)
MIXED = [300, -300, 20, -20, 100, -100, 16000, -16000, 5] * 2


def long_shape(engine):
    tile, chunk = engine.get("scanmseed_tile"), engine.get("scanmseed_compose_chunk")
    return tile, chunk, (chunk + 3) * tile + 11


def encode_equals(engine, stacked, want):
    """One encode call (a NumPy array or a device tensor) against the restatement's dict; returns the engine's."""
    got = engine.scanmseed_encode(stacked)
    assert np.array_equal(got["n_records"], want["n_records"])
    assert got["records"].shape == want["records"].shape
    assert np.array_equal(got["records"], want["records"]), np.argwhere(got["records"] != want["records"])[:8]
    assert np.array_equal(got["rec_first"], want["rec_first"]) and np.array_equal(got["rec_count"], want["rec_count"])
    return got


def decodes_back(engine, out, stacked):
    counts = out["rec_count"].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]])
    ints, none = engine.scanmseed_decode(out["records"], out["rec_count"], offsets, int(counts.sum()))
    assert none is None and np.array_equal(ints, stacked.ravel())


def restated(rows, edge):
    """The rows' chains walked once: (encode_channels' dict, per row (entry offset into the tile at `edge`, word index
    there), the counts of the words from there on)."""
    chains = [ref.trace_chain(x) for x in rows]
    at = [int(np.searchsorted(starts, edge)) for _, _, starts in chains]
    state = [(int(starts[k] - edge), k) for (_, _, starts), k in zip(chains, at)]
    late = sum(np.bincount(count[starts[k:]], minlength=8) for (_, count, starts), k in zip(chains, at))
    return ref.encode_channels(rows, chains), state, late


@pytest.fixture(scope="module")
def long_chains(engine):
    """
    C1's two calls, built and restated once: [(stacked (5, n) int32, encode_channels' dict, [(entry, word)] * 5)].
    Words of seven 4-bit differences behind `lead` one-difference words, as in the tile-edge test above: the chain
    enters tile `chunk` at offset lead % 7 (6 for no lead).  A run of other widths takes at most three differences a
    word and gathers every chain that reaches it into three alignments, so where it lies ACROSS position chunk x tile
    the tile is entered at 0, 1 or 2 whatever the lead.  Hence: the run lies across (chunk + 1) x tile in every channel,
    across chunk x tile in the second call's last two (leads 8 and 9, whose offsets 1 and 2 the first call has), and
    eight positions behind chunk x tile in the others, whose seven-difference words straddle that position.
    """
    tile, chunk, n = long_shape(engine)
    wide = (1 << 29) - 1
    calls = []
    for shifts in (range(0, 5), range(5, 10)):
        rows = []
        for lead in shifts:
            d = np.where(np.arange(n - 1) % 2 == 0, 7, -8)
            d[:lead] = np.where(np.arange(lead) % 2 == 0, wide, -wide)
            at = chunk * tile - 9 if lead >= 8 else chunk * tile + 8
            d[at:at + len(MIXED)] = MIXED
            d[(chunk + 1) * tile - 9:(chunk + 1) * tile + 9] = MIXED
            rows.append(ref.from_differences(d))
        if shifts[0] == 5:                                      # one word per sample: 943 samples per record
            rows[2] = ref.from_differences(np.where(np.arange(n - 1) % 2 == 0, wide, -wide), first=-(1 << 28))
        stacked = np.ascontiguousarray(np.stack(rows))
        want, state, _ = restated(stacked, chunk * tile)
        calls.append((stacked, want, state))
    return calls


def test_long_chain_carries_entry_offset_and_word_index_across_a_compose_chunk(engine, long_chains):
    tile, chunk, n = long_shape(engine)
    assert n > chunk * tile + 2 * tile                          # tiles chunk .. chunk + 3 belong to the second trip
    state = [s for _, _, states in long_chains for s in states]
    print("entry offsets, word indices at tile", chunk, ":", state)
    assert {e for e, _ in state} == set(range(7))               # a dropped `e` (0 again) shows in six of them
    assert min(w for _, w in state) > 65_535                    # ... a dropped or 16-bit `w` in every channel
    assert sum(e != 0 for e, _ in state) >= 4                   # words that straddle position chunk x tile
    wide_records = long_chains[1][1]["n_records"]
    print("records per channel:", [c[1]["n_records"].tolist() for c in long_chains])
    assert wide_records[2] == -(-n // ref.REC_WORDS) and wide_records[2] > 2000
    for stacked, want, _ in long_chains:
        decodes_back(engine, encode_equals(engine, stacked, want), stacked)


CLASS_SETS = [(0, 1, 2), (0, 1, 2, 3, 4), (2, 3, 4, 5), (0, 1, 2, 3, 4, 5, 6), (0, 6)]


@pytest.fixture(scope="module")
def long_walks(engine):
    """C2's series, built and restated once: (stacked (5, n) int32, encode_channels' dict, word histogram late)."""
    tile, chunk, n = long_shape(engine)
    rng = np.random.default_rng(2014)
    rows = [ref.folded_switching_walk(rng, n, classes=cl, max_run=int(rng.integers(2, 60))) for cl in CLASS_SETS]
    stacked = np.ascontiguousarray(np.stack(rows))
    want, _, late = restated(stacked, chunk * tile)
    return stacked, want, late


def test_long_random_widths(engine, long_walks):
    stacked, want, late = long_walks
    print("words of 1..7 differences in tiles at or beyond the compose chunk:", late[1:].tolist())
    assert late[0] == 0 and late[1:].min() > 0                  # all seven layouts behind the carried state
    decodes_back(engine, encode_equals(engine, stacked, want), stacked)
    import torch

    encode_equals(engine, torch.from_numpy(stacked).to(f"cuda:{engine.device}"), want)


def test_long_float_input_quantises_past_the_grid(engine, sm):
    """test_float_flavour_quantises_like_numpy's 5000 samples, repeated over the whole length: the same ties, clips,
    zeros and negative coordinates in the quantiser's second and third trip."""
    _, _, n = long_shape(engine)
    assert n > 2 * QUANT_GRID + 5000
    ucf, m = 1000.0, 5000
    rng = np.random.default_rng(8)
    k = np.arange(m)
    coa = (2 * (k % 400) + 1) / 64.0
    coa[:2] = [0.0, -0.0]
    coa_n = 1.0 + rng.uniform(0, 0.5, m)
    coa[940:1000] = np.linspace(coa[939], 21473.9, 60)
    coa[1000:1400] = np.linspace(21473.9, 21474.1, 400)
    coa[1400:1408] = [21474.0, 21474.00001, 21474.5, 3e4, 1e9, np.inf, 21473.999995, 21473.99999]
    coa[1408:1468] = np.linspace(21473.9, coa[1468], 60)
    coa_n[1900:2000] = np.linspace(coa_n[1899], 21473.0, 100)
    coa_n[2000:2003] = [21474.0, 5e4, 21473.999999]
    coa_n[2003:2103] = np.linspace(21473.0, coa_n[2103], 100)
    block = np.stack([coa, coa_n, ((2 * (k % 300) + 1) / 128.0) * np.where(k % 2, -1, 1),
                      -64.5 + np.cumsum(rng.uniform(-1e-5, 1e-5, m)), (2 * (k % 50) + 1) / 128.0 - 0.25])
    stacked = np.ascontiguousarray(np.tile(block, (1, -(-n // m)))[:, :n])
    stacked[3] += np.repeat(np.arange(-(-n // m)) % 7, m)[:n] * 1e-3           # (the repeats differ on Y)
    want = sm.quantise(stacked[0], stacked[1], stacked[2:].T, ucf)
    at = np.arange(n)
    scaled = np.minimum(stacked[0], sm.COA_CLIP) * 1e5
    tie = scaled - np.floor(scaled) == 0.5
    for trip in (1, 2):                                         # ties whose lower neighbour is odd, and is even
        late = tie & (at >= trip * QUANT_GRID) & (at < (trip + 1) * QUANT_GRID)
        up, down = int((late & (want["COA"] > scaled)).sum()), int((late & (want["COA"] < scaled)).sum())
        print("COA ties in trip", trip, "of the quantiser's grid, rounded up / down:", up, down)
        assert up > 100 and down > 100
    scaled = stacked[2] * 1e6
    tie = (scaled - np.floor(scaled) == 0.5) & (at >= QUANT_GRID)
    below, above = int((tie & (scaled < 0)).sum()), int((tie & (scaled > 0)).sum())
    print("X ties beyond the grid, negative / positive:", below, above)
    assert below > 100 and above > 100
    clipped = np.flatnonzero((stacked[0] > sm.COA_CLIP) & (want["COA"] == 2147400000))
    print("clipped COA samples beyond", 2 * QUANT_GRID, ":", int((clipped > 2 * QUANT_GRID).sum()))
    assert clipped.max() > 2 * QUANT_GRID and want["X"][2 * QUANT_GRID:].min() < 0 and want["Y"].min() < 0
    expect = ref.encode_channels(np.stack([want[ch] for ch in sm.CHANNELS]))
    factors = [sm.scale_factors(ucf)[ch] for ch in sm.CHANNELS]
    clips = [sm.COA_CLIP, sm.COA_CLIP, None, None, None]
    import torch

    for series in (stacked, torch.from_numpy(stacked).to(f"cuda:{engine.device}")):
        got = engine.scanmseed_encode(series, factors, clips)
        assert np.array_equal(got["n_records"], expect["n_records"])
        assert np.array_equal(got["records"], expect["records"])
        assert np.array_equal(got["rec_first"], expect["rec_first"])
        assert np.array_equal(got["rec_count"], expect["rec_count"])


def test_long_refusals_name_late_positions(engine, lib, sm, long_chains):
    tile, chunk, n = long_shape(engine)
    edge = chunk * tile
    assert edge > 2_000_000 > QUANT_GRID + 1                    # every position below lies in a second trip
    x = np.zeros((5, n), dtype=np.int32)
    x[3, edge + 5:] = 1 << 29
    with pytest.raises(lib.QMHipError, match=rf"channel Y, sample {edge + 5}: difference does not fit 30 bits"):
        engine.scanmseed_encode(x)
    # one step on each side of the compose chunk's edge: X's lies further into its channel and still comes first
    x = np.zeros((5, n), dtype=np.int32)
    x[2, edge + 7:] = 1 << 29
    x[4, edge - 7:] = 1 << 29
    assert 2 * n + edge + 7 < 4 * n + edge - 7
    with pytest.raises(lib.QMHipError, match=rf"channel X, sample {edge + 7}: difference does not fit 30 bits"):
        engine.scanmseed_encode(x)
    x = np.zeros((5, n), dtype=np.int32)
    x[1, edge + 7:] = 1 << 29
    x[0, edge - 7:] = 1 << 29
    with pytest.raises(lib.QMHipError, match=rf"channel COA, sample {edge - 7}: difference does not fit 30 bits"):
        engine.scanmseed_encode(x)
    del x
    f = np.array(list(sm.scale_factors(1000.0).values()))
    clips = [sm.COA_CLIP, sm.COA_CLIP, None, None, None]
    y = np.ones((5, n))
    y[4, 2_000_000] = np.nan
    with pytest.raises(lib.QMHipError, match=r"channel Z, sample 2000000 is NaN"):
        engine.scanmseed_encode(y, f, clips)
    y[4, 2_000_000] = 1.0
    y[1, QUANT_GRID + 1] = -3e4                                 # x 1e5: below int32 (the clip bounds the other side)
    with pytest.raises(lib.QMHipError,
                       match=rf"channel COA_N, sample {QUANT_GRID + 1}: the scaled value is outside int32"):
        engine.scanmseed_encode(y, f, clips)
    del y
    # the engine goes on working after the refusals
    stacked, want, _ = long_chains[0]
    encode_equals(engine, stacked, want)


def test_long_file_to_device_to_trigger(engine, sm, tmp_path, long_walks):
    import trigger_ref as tr

    stacked, _, _ = long_walks
    ucf, period = 1000.0, 20_000_000
    stride = engine.get("trigger_merge_stride")
    series = {ch: stacked[j] for j, ch in enumerate(sm.CHANNELS)}
    path = tmp_path / "2014_180.scanmseed"
    sm.write_scanmseed(path, dt.datetime(2014, 6, 29), 50.0, series, engine=engine)
    f = sm.scale_factors(ucf)
    coa, coa_n = series["COA"] / f["COA"], series["COA_N"] / f["COA_N"]
    # COA is a random walk: it crosses its median some hundreds of times, and with a marginal window of one sample most
    # of those runs are events of their own
    threshold, mw_ns, mei_ns = float(np.median(coa)), period, 2 * period
    par = dict(trigger_on=0, method="static", value=threshold)
    want = tr.trigger_series(coa, coa_n, 0, None, tr.STATIC, threshold, 1, period, mw_ns, mei_ns)
    print("threshold", threshold, "candidates", want["n_candidates"], "events", want["n_events"])
    assert want["n_events"] > stride and want["n_candidates"] > want["n_events"]
    _, rate, host = sm.read_scanmseed(path, ucf, engine=engine)
    _, _, dev = sm.read_scanmseed(path, ucf, engine=engine, device=True)
    assert rate == 50.0 and hasattr(dev["COA"], "data_ptr") and not hasattr(host["COA"], "data_ptr")
    assert np.array_equal(bits(host["COA"]), bits(coa)) and np.array_equal(bits(host["COA_N"]), bits(coa_n))
    for ch in sm.CHANNELS:
        assert np.array_equal(host["int"][ch], series[ch])
    answers = [engine.trigger_series(c["COA"], c["COA_N"], period, mw_ns, mei_ns, want_candidates=True, **par)
               for c in (dev, host)]
    for got in answers:
        assert (got["n_candidates"], got["n_events"]) == (want["n_candidates"], want["n_events"])
        assert np.array_equal(got["candidates"], want["candidates"])
        assert np.array_equal(got["events_i"], want["events_i"])
        assert np.array_equal(bits(got["events_f"]), bits(want["events_f"]))
        assert np.array_equal(bits(got["thresholds"]), bits(want["thresholds"]))
