# -*- coding: utf-8 -*-
"""Engine replicas, host side (include/qmhip.h parts 2 and 3): the refusals of qm_stream_create_replicas that touch
no device, the front end's empty list, and the new symbols in the header."""

import ctypes
import pathlib

import pytest

from quakemigrate_amd.core import lib


def _create(engines, n):
    out = ctypes.c_void_p()
    rc = lib.qmlib.qm_stream_create_replicas(engines, n, 400, 10, 10, 8, 0, 1, 2, ctypes.byref(out))
    return rc, out, lib.qmlib.qm_last_error().decode()


def test_null_array_is_refused():
    rc, out, msg = _create(None, 2)
    assert rc != 0 and out.value is None
    assert "NULL argument" in msg and "qm_stream_create_replicas" in msg


def test_no_engines_is_refused():
    arr = (ctypes.c_void_p * 1)()
    rc, out, msg = _create(arr, 0)
    assert rc != 0 and out.value is None
    assert "at least one engine" in msg


@pytest.mark.parametrize("n", [1, 3])
def test_null_entry_is_refused(n):
    arr = (ctypes.c_void_p * n)()
    rc, out, msg = _create(arr, n)
    assert rc != 0 and out.value is None
    assert "replica 0 is NULL" in msg


def test_replicas_of_no_device_raise_value_error():
    with pytest.raises(ValueError):
        lib.EngineReplicas([])


def test_replica_symbols_are_declared():
    header = (pathlib.Path(lib.__file__).resolve().parents[2] / "include" / "qmhip.h").read_text()
    for name in ("qm_engine_table_digest", "qm_stream_create_replicas"):
        assert f"{name}(" in header
        assert hasattr(lib.qmlib, name)
