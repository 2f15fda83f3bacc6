# -*- coding: utf-8 -*-
"""Engine groups, host side (include/qmhip.h part 4): the partition plan against distributed.py's column
partition, the flat z-run rule, and the refusals of qm_group_create that touch no device."""

import ctypes

import pytest

from quakemigrate_amd import distributed as qd
from quakemigrate_amd.core import lib


def _flat_range(boxes, ny, nz):
    return [((x0 * ny + y0) * nz + z0, (x0 * ny + y0) * nz + z0 + (x1 - x0) * (y1 - y0) * (z1 - z0))
            for x0, x1, y0, y1, z0, z1 in boxes]


@pytest.mark.parametrize("grid", [(21, 17, 18), (2, 3, 20), (201, 201, 101)])
@pytest.mark.parametrize("n_parts", range(1, 10))
def test_plan_is_the_column_partition(grid, n_parts):
    nx, ny, nz = grid
    covered = []
    for part in range(n_parts):
        got = lib.group_plan(nx, ny, nz, n_parts, part)
        want = qd.column_boxes(*qd.shard_columns(nx, ny, n_parts, part), ny)
        assert [b[:4] for b in got] == [tuple(w) for w in want], (part, got, want)
        assert all(b[4:] == (0, nz) for b in got)
        covered += _flat_range(got, ny, nz)
    # every node once, ascending: the boxes of all parts tile [0, N)
    assert covered[0][0] == 0 and covered[-1][1] == nx * ny * nz
    assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
    assert all(lo < hi for lo, hi in covered)


def test_more_parts_than_columns_leaves_parts_empty():
    plans = [lib.group_plan(2, 3, 20, 9, p) for p in range(9)]
    assert sum(1 for p in plans if not p) == 3 and all(len(p) <= 1 for p in plans)


@pytest.mark.parametrize("n", [1, 5, 31, 32, 1000, 80_011])
@pytest.mark.parametrize("n_parts", [1, 2, 3, 7, 8])
def test_flat_table_is_cut_into_balanced_z_runs(n, n_parts):
    runs = []
    for part in range(n_parts):
        got = lib.group_plan(1, 1, n, n_parts, part)
        base, extra = divmod(n, n_parts)
        z0 = part * base + min(part, extra)
        z1 = z0 + base + (1 if part < extra else 0)
        assert got == ([(0, 1, 0, 1, z0, z1)] if z1 > z0 else []), (part, got)
        runs += _flat_range(got, 1, n)
    assert runs[0][0] == 0 and runs[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(runs, runs[1:]))


def test_plan_refuses_bad_arguments():
    boxes, nb = (ctypes.c_int32 * 18)(), ctypes.c_int32()
    assert lib.qmlib.qm_group_plan(4, 4, 4, 2, 2, boxes, ctypes.byref(nb)) != 0
    assert b"part" in lib.qmlib.qm_last_error()
    assert lib.qmlib.qm_group_plan(0, 4, 4, 2, 0, boxes, ctypes.byref(nb)) != 0
    assert lib.qmlib.qm_group_plan(4, 4, 4, 0, 0, boxes, ctypes.byref(nb)) != 0


@pytest.mark.parametrize("ids", [[], [-1], [0, -3]])
def test_group_create_refuses_without_touching_a_device(ids):
    h = ctypes.c_void_p()
    arr = (ctypes.c_int32 * max(len(ids), 1))(*ids)
    assert lib.qmlib.qm_group_create(arr, len(ids), ctypes.byref(h)) != 0
    assert h.value is None
    msg = lib.qmlib.qm_last_error().decode()
    assert ("at least one device" in msg) if not ids else ("negative" in msg)
    with pytest.raises(lib.QMHipError):
        lib.EngineGroup(ids)


def test_group_symbols_are_declared():
    import pathlib

    header = (pathlib.Path(lib.__file__).resolve().parents[2] / "include" / "qmhip.h").read_text()
    for name in ("qm_group_plan", "qm_group_create", "qm_group_destroy", "qm_group_config", "qm_group_get",
                 "qm_group_load_lut", "qm_group_table_select", "qm_group_detect", "qm_group_marginal",
                 "qm_group_migrate", "qm_group_find_max_coa", "qm_group_synchronize", "qm_group_n_parts",
                 "qm_group_part_info"):
        assert f"{name}(" in header
        assert hasattr(lib.qmlib, name)
