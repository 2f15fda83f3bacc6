# -*- coding: utf-8 -*-
"""
The engine's tunables through ``Engine.config`` / ``Engine.get`` (the record and its table: csrc/qm_config.hpp): every
case of tests/tunables_cases.py with the whole refusal text, the forwarding of groups and replicas, and a table's
layout not depending on the tables the engine held before.
"""

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (first: it puts the repository root on sys.path)
import tunables_cases as tc  # noqa: E402
from test_call_sequences import LAYOUT_KEYS  # noqa: E402
from test_gpu_parity import NORM  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    assert _lib.qmlib.qm_device_count() >= 1, "no HIP device visible"
    return _lib


def _walk(lib, eng, keys):
    """Every probe of ``keys`` on ``eng`` (no table resident): the refusal text, or the read-back."""
    for key in keys:
        for value, want in tc.CASES[key]:
            if isinstance(want, str):
                with pytest.raises(lib.QMHipError) as err:
                    eng.config(key, value)
                assert str(err.value) == want, (key, value)
            else:
                eng.config(key, value)
                assert eng.get(key) == tc.ENGINE_READS_LAST_LAUNCH.get(key, want), (key, value)


def test_every_case_as_it_was_before_the_record(lib):
    """The keys that could be read before the tunables became one record: this test passed unchanged on the
    engine as it was, with its two chains."""
    eng = lib.Engine(0)
    _walk(lib, eng, [k for k in tc.CASES if k not in tc.NEWLY_READABLE])
    with pytest.raises(lib.QMHipError) as err:
        eng.config("no_such_key", 1)
    assert str(err.value) == "unknown config key 'no_such_key'"
    with pytest.raises(lib.QMHipError) as err:
        eng.get("no_such_key")
    assert str(err.value) == "unknown key 'no_such_key'"
    # a refused value changes nothing
    for key in ("waves", "lds_bytes", "chunk_bytes", "shift"):
        before = eng.get(key)
        with pytest.raises(lib.QMHipError):
            eng.config(key, -5)
        assert eng.get(key) == before, key
    eng.close()


def test_fresh_engine_reads_the_defaults(lib):
    eng = lib.Engine(0)
    for key, want in tc.DEFAULTS.items():
        if key not in tc.NEWLY_READABLE:
            assert eng.get(key) == tc.ENGINE_READS_LAST_LAUNCH.get(key, want), key
    eng.close()


def test_the_nine_keys_read_back(lib):
    eng = lib.Engine(0)
    for key in tc.NEWLY_READABLE:
        assert eng.get(key) == tc.DEFAULTS[key], key
    _walk(lib, eng, tc.NEWLY_READABLE)
    eng.close()


def test_brick_x_fills_in_the_other_two(lib):
    eng = lib.Engine(0)
    for what, key, value in tc.BRICK_FILL_STEPS:
        if what == "set":
            eng.config(key, value)
        else:
            assert eng.get(key) == value, (key, value)
    eng.close()


def test_group_and_replicas_forward(lib):
    group = lib.EngineGroup([0, 0])
    with pytest.raises(lib.QMHipError) as err:
        group.config("waves", 17)
    assert str(err.value) == "waves must be 1..16"
    with pytest.raises(lib.QMHipError) as err:
        group.config("screen", 1)
    assert str(err.value) == ("qm_group_config: screen = 1 is not available on an engine group (the screened "
                              "detect has no partial form)")
    group.config("shift", 0)
    assert group.get("shift") == 0 and group.lead.get("shift") == 0
    group.close()
    reps = lib.EngineReplicas([0, 0])
    with pytest.raises(lib.QMHipError) as err:
        reps.config("waves", 0)
    assert str(err.value) == "waves must be 1..16"
    reps.config("chunk_bytes", 1 << 21)
    assert [r.get("chunk_bytes") for r in reps.replicas] == [1 << 21, 1 << 21]
    assert reps.get("chunk_bytes") == 1 << 21
    reps.close()


def _layout(eng):
    family = "wide" if eng.get("shift_wide_tiles") > 0 else eng.get("last_kernel")
    read = {"family": family, "waves": eng.get("waves"), "lds_bytes": eng.get("lds_bytes")}
    read.update({k: eng.get(k) for k in LAYOUT_KEYS[family]})
    return read


def test_layout_with_one_of_waves_and_lds_bytes_set_does_not_depend_on_earlier_tables(lib):
    """With exactly one of waves / lds_bytes set by the user, the other one is what a fresh engine takes -- not what
    the layout search of an EARLIER table left behind.  (Before the tunables became one record the search kept its
    choice in the tunables themselves: the long-lived engine below reported lds_bytes = 163840, the 44-row table's,
    where the fresh one reports 81920.)"""
    from quakemigrate_amd import synth

    grid = (6, 5, 4)
    big = synth.make_case("C2", step=0, grid=grid, rows=44, n_samples=300)
    small = synth.make_case("C2", step=0, grid=grid, rows=10, n_samples=300)
    lon = np.ascontiguousarray(np.log(np.clip(small.onsets, 0.01, np.inf)))

    old = lib.Engine(0, brick_x=2, brick_y=2, brick_z=2)
    old.load_lut(big.traveltimes)
    old.config("waves", 8)
    old.load_lut(small.traveltimes)
    fresh = lib.Engine(0, brick_x=2, brick_y=2, brick_z=2, waves=8)
    fresh.load_lut(small.traveltimes)
    got = old.detect(lon, small.fsmp, small.lsmp, small.available)
    want = fresh.detect(lon, small.fsmp, small.lsmp, small.available)
    print("long-lived:", _layout(old), "fresh:", _layout(fresh))
    assert _layout(old) == _layout(fresh)
    assert fresh.get("waves") == 8 and fresh.get("lds_bytes") == 80 * 1024
    assert got[0].shape == (300,)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    np.testing.assert_allclose(got[1], want[1], rtol=NORM)
    old.close()
    fresh.close()
