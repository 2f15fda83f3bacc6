# -*- coding: utf-8 -*-
"""
The .scanmseed codec without a GPU: the NumPy restatement of the chain formulation (tests/scanmseed_ref.py) against the
Python codec byte for byte, the linearised ``steim2_encode`` against the bytes of the encoder it replaced, and the C
ABI's new symbols as far as they answer without a device.
"""

import ctypes
import datetime as dt
import hashlib
import json
import re

import numpy as np
import pytest

import scanmseed_ref as ref
from conftest import GOLDEN, ROOT

T0 = dt.datetime(2014, 6, 29)
GOLDEN_FILES = {"icequake_iceland_2014_180.scanmseed": 11, "volcanotectonic_iceland_2014_236.scanmseed": 87}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_engine()
    from quakemigrate_amd.core import lib as _lib

    return _lib


def restated_trace(sm, x, station="COA", rate=50.0):
    records, first, count = ref.encode_trace(x)
    n_records = [len(records) if ch == station else 0 for ch in sm.CHANNELS]
    return sm.fill_headers(records, n_records, first, count, T0, rate)


@pytest.mark.parametrize("name", sorted(GOLDEN_FILES))
def test_restatement_rewrites_the_golden_files(name):
    from quakemigrate_amd import scanmseed as sm

    blob = (GOLDEN / name).read_bytes()
    assert len(blob) == GOLDEN_FILES[name] * sm.RECLEN
    start, rate, cols = sm.read_scanmseed(GOLDEN / name)
    series = np.stack([cols["int"][ch] for ch in sm.CHANNELS])
    out = ref.encode_channels(series)
    assert int(out["n_records"].sum()) == GOLDEN_FILES[name]
    assert sm.fill_headers(out["records"], out["n_records"], out["rec_first"], out["rec_count"], start, rate) == blob
    assert sm.encode_scanmseed(start, rate, cols["int"]) == blob        # (the Python re-encodes them exactly)


@pytest.mark.parametrize("name", sorted(ref.designed_series()))
def test_restatement_equals_the_python_on_the_designed_series(name):
    from quakemigrate_amd import scanmseed as sm

    x = ref.designed_series()[name]
    want = sm.write_trace(sm.Trace("COA", "NW", T0, 50.0, x))
    assert restated_trace(sm, x) == want
    # ... and the first record's payload is what steim2_encode gives on the whole trace
    payload, n = sm.steim2_encode(x, int(x[0]))
    assert want[sm.DATA_OFFSET:sm.RECLEN] == payload
    assert np.array_equal(np.concatenate([d for *_, d in sm.read_records(want)]), x)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_the_python_on_switching_walks(seed):
    from quakemigrate_amd import scanmseed as sm

    x = ref.switching_walk(np.random.default_rng(seed), 40_000 - seed, classes=(0, 1, 2, 3, 4, 5, 6))
    assert restated_trace(sm, x) == sm.write_trace(sm.Trace("COA", "NW", T0, 50.0, x))


def test_folded_walk_keeps_its_classes_and_equals_the_python():
    """The vectorised builder of the long GPU cases: a quarter of 30 011 steps of up to 2^29 would leave int32 many
    times over, the folded series stays inside +-2^30 and comes near it; no difference outside 30 bits, every class
    asked for present, the same series for the same seed; the restatement on it equals the Python encoder."""
    from quakemigrate_amd import scanmseed as sm

    n = 30_011
    x = ref.folded_switching_walk(np.random.default_rng(5), n, classes=(0, 2, 4, 6), max_run=30)
    assert x.dtype == np.int32 and len(x) == n
    assert (1 << 29) < np.abs(x.astype(np.int64)).max() <= (1 << 30)
    assert np.array_equal(x, ref.folded_switching_walk(np.random.default_rng(5), n, classes=(0, 2, 4, 6), max_run=30))
    cls = ref.width_class(ref.differences(x))
    assert cls.max() == 6 and set(np.unique(cls)) >= {0, 2, 4, 6}
    # runs of one class: words of 7, 5, 3 and 1 differences all occur on the chain
    count = ref.counts(cls)
    assert np.bincount(count[ref.chain(count)], minlength=8)[[1, 3, 5, 7]].min() > 0
    assert restated_trace(sm, x) == sm.write_trace(sm.Trace("COA", "NW", T0, 50.0, x))


def test_restatement_refuses_what_the_python_refuses():
    from quakemigrate_amd import scanmseed as sm

    for x in ([0, 1 << 29], [-(1 << 31), (1 << 31) - 1]):
        x = np.array(x, dtype=np.int32)
        with pytest.raises(OverflowError):
            ref.encode_trace(x)
        with pytest.raises(OverflowError):
            sm.write_trace(sm.Trace("COA", "NW", T0, 50.0, x))


def test_linearised_encoder_writes_the_parents_bytes():
    """200 000 samples: the digest was recorded from the encoder that converted the whole rest of the trace for
    every record (tests/golden/scanmseed_parent_200k.json)."""
    from quakemigrate_amd import scanmseed as sm

    want = json.loads((GOLDEN / "scanmseed_parent_200k.json").read_text())
    x = ref.switching_walk(np.random.default_rng(2014), want["samples"])
    blob = sm.write_trace(sm.Trace("COA", "NW", T0, 50.0, x))
    assert len(blob) == want["bytes"]
    assert hashlib.sha256(blob).hexdigest() == want["sha256"]


def test_encoder_converts_a_record_and_its_look_ahead_only():
    """steim2_encode touches 6601 + 7 samples however long the rest of the trace is; `left` stays exact at the end."""
    from quakemigrate_amd import scanmseed as sm

    class Counting:
        def __init__(self, data):
            self.data, self.touched = data, 0

        def __len__(self):
            return len(self.data)

        def __getitem__(self, key):
            part = self.data[key]
            self.touched += np.size(part)
            return part

    x = ref.from_differences(np.where(np.arange(49_999) % 2 == 0, 7, -8))
    counted = Counting(x)
    payload, n = sm.steim2_encode(counted, int(x[0]))
    assert n == 6601 and counted.touched == 6601 + 7
    assert payload == sm.steim2_encode(x[:6601 + 7], int(x[0]))[0]
    # a trace that ends inside the look-ahead: the last words shrink under count <= left
    for tail in range(1, 8):
        short = x[:6601 - 7 + tail]
        assert sm.steim2_encode(short, int(short[0]))[1] == len(short)


def test_symbols_are_declared_and_exported(lib):
    import subprocess

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qmhip.h").read_text(), flags=re.S)
    so = ROOT / "quakemigrate_amd" / "csrc" / "libqmhip.so"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", str(so)], text=True).split()
    for name in ("qm_engine_scanmseed_encode", "qm_engine_scanmseed_decode", "qm_engine_trigger_resident"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in exported, name
        assert getattr(lib.qmlib, name).argtypes is not None


def test_calls_refuse_a_null_engine_by_name(lib):
    x = np.zeros((5, 8), dtype=np.int32)
    n_records = np.zeros(5, dtype=np.int64)
    records = np.zeros((5, 4096), dtype=np.uint8)
    first, count = np.zeros(5, dtype=np.int32), np.zeros(5, dtype=np.int32)
    vp = ctypes.c_void_p
    rc = lib.qmlib.qm_engine_scanmseed_encode(None, x.ctypes.data_as(vp), 0, 0, 8, None, None, 5,
                                              n_records.ctypes.data_as(vp), records.ctypes.data_as(vp),
                                              first.ctypes.data_as(vp), count.ctypes.data_as(vp))
    assert rc != 0 and b"qm_engine_scanmseed_encode: NULL argument" in lib.qmlib.qm_last_error()
    offset, out = np.zeros(5, dtype=np.int64), np.zeros(40, dtype=np.int32)
    rc = lib.qmlib.qm_engine_scanmseed_decode(None, records.ctypes.data_as(vp), 5, count.ctypes.data_as(vp),
                                              offset.ctypes.data_as(vp), None, 40, out.ctypes.data_as(vp), None, 0)
    assert rc != 0 and b"qm_engine_scanmseed_decode: NULL argument" in lib.qmlib.qm_last_error()
    assert not records.any() and not out.any() and not n_records.any()


def test_binding_checks_shapes_and_dtypes_before_the_call(lib):
    eng = object.__new__(lib.Engine)                # no device: every check below fires before the handle is used
    eng._h, eng.device = None, 0
    with pytest.raises(TypeError, match="NumPy array or a device tensor"):
        eng.scanmseed_encode([[0] * 5] * 5)
    with pytest.raises(ValueError, match=r"\(5, n\) expected"):
        eng.scanmseed_encode(np.zeros((4, 10), dtype=np.int32))
    with pytest.raises(ValueError, match=r"\(5, n\) expected"):
        eng.scanmseed_encode(np.zeros(10, dtype=np.int32))
    with pytest.raises(TypeError, match="int32 or float64"):
        eng.scanmseed_encode(np.zeros((5, 10), dtype=np.int64))
    with pytest.raises(ValueError, match="no samples"):
        eng.scanmseed_encode(np.zeros((5, 0), dtype=np.int32))
    with pytest.raises(ValueError, match="C-contiguous"):
        eng.scanmseed_encode(np.zeros((10, 5), dtype=np.int32).T)
    with pytest.raises(ValueError, match="need factors"):
        eng.scanmseed_encode(np.zeros((5, 10)))
    with pytest.raises(ValueError, match=r"\(5,\) expected"):
        eng.scanmseed_encode(np.zeros((5, 10)), factors=[1.0] * 4)
    records = np.zeros((2, 4096), dtype=np.uint8)
    with pytest.raises(TypeError, match="NumPy array expected"):
        eng.scanmseed_decode(records.tobytes(), [1, 1], [0, 1], 2)
    with pytest.raises(TypeError, match="uint8"):
        eng.scanmseed_decode(records.astype(np.int8), [1, 1], [0, 1], 2)
    with pytest.raises(ValueError, match=r"\(n_records, 4096\)"):
        eng.scanmseed_decode(records.reshape(4, 2048), [1] * 4, [0] * 4, 4)
    with pytest.raises(ValueError, match=r"\(2,\) expected"):
        eng.scanmseed_decode(records, [1, 1, 1], [0, 1], 2)
    with pytest.raises(ValueError, match=r"rec_factor of shape"):
        eng.scanmseed_decode(records, [1, 1], [0, 1], 2, rec_factor=[1.0])
    with pytest.raises(ValueError, match="n_total must be positive"):
        eng.scanmseed_decode(records, [1, 1], [0, 1], 0)
    # the front end: five channels of one length, an integer rate
    from quakemigrate_amd import scanmseed as sm

    series = {ch: np.zeros(4, dtype=np.int32) for ch in sm.CHANNELS}
    series["Z"] = np.zeros(5, dtype=np.int32)
    with pytest.raises(ValueError, match="of one length"):
        sm.encode_scanmseed(T0, 50.0, series, engine=eng)
    with pytest.raises(ValueError, match="device=True needs an engine"):
        sm.read_scanmseed(GOLDEN / sorted(GOLDEN_FILES)[0], device=True)
