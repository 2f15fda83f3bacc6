# -*- coding: utf-8 -*-
"""
The grid eikonal solver on the GPU (include/qmhip.h: qm_engine_tt_eikonal3d; kernels: csrc/qm_traveltimes.hpp) against
its NumPy restatement (tests/traveltimes3d_ref.py, pinned to its serial form and to closed forms by
tests/test_traveltimes3d_host.py).  Every float has the restatement's bits and every integer is equal: the kernel runs
the restatement's operations in its order, so there is no tolerance anywhere in this file.

A thread of the plane launch takes one node at most (the launch covers the plane's rectangle), so there is no second
trip to test; the 24 x 24 x 24 case has planes of more than one workgroup.
"""

import numpy as np
import pytest

import traveltimes3d_ref as t3
import traveltimes_ref as tr
from test_traveltimes3d_host import SMALL, small_case

pytestmark = pytest.mark.gpu

LL, SPACING = SMALL["ll"], SMALL["spacing"]


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


def bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(engine, case, tol=t3.TOL, device=False, slowness_on_device=False, want=None):
    """One call against the restatement: grids, rounds and status."""
    ll, spacing, count, sources, s0, slowness, row_model = case
    want = t3.solve(*case, tol=tol) if want is None else want
    given = slowness
    if slowness_on_device:
        import torch

        given = torch.as_tensor(np.ascontiguousarray(slowness), device=f"cuda:{engine.device}")
    got = engine.traveltimes_eikonal3d(ll, spacing, count, sources, s0, given, row_model, tol=tol, device=device)
    assert tuple(got[0].shape) == (len(s0),) + tuple(count)
    assert np.array_equal(got[2], want[2]) and not want[2].any()
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(bits(got[0]), bits(want[0]))
    return got, want


def random_slowness(count, seed, models=1):
    return np.random.default_rng(seed).uniform(0.25, 1.0 / 3.0, size=(models,) + tuple(count))


def upper_corner(count):
    return tuple(l + (n - 1) * s for l, s, n in zip(LL, SPACING, count))


# -- the scheme --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [0.0, t3.TOL])
def test_small_case_has_the_restatements_bits(engine, tol):
    """7 x 6 x 5, anisotropic spacing, a source off the nodes, random slowness: strict and at the default tolerance."""
    check(engine, small_case(), tol=tol)
    assert engine.get("tt_ns_eikonal3d") > 0


PLACEMENTS = {
    "on_a_node": tuple(l + i * s for l, s, i in zip(LL, SPACING, (2, 1, 3))),
    "on_a_cell_face": (LL[0] + 2 * SPACING[0], 1.13, 0.71),
    "ll_corner": LL,
    "ur_corner": upper_corner((6, 5, 5)),           # the clipped cell
}


@pytest.mark.parametrize("where", list(PLACEMENTS))
def test_source_placements(engine, where):
    count = (6, 5, 5)
    source = PLACEMENTS[where]
    cell = t3.source_cell(LL, SPACING, count, source)
    assert np.all(cell >= 0) and np.all(cell <= np.array(count) - 2)
    if where == "ur_corner":
        assert tuple(cell) == tuple(n - 2 for n in count)
    (got, _, _), _ = check(engine, (LL, SPACING, count, [source], [0.3], random_slowness(count, 11), [0]))
    if where != "on_a_cell_face":                   # the source is a node: T = 0 there and nowhere else
        assert np.count_nonzero(got[0] == 0.0) == 1


@pytest.mark.parametrize("count", [(2, 9, 8), (9, 2, 8)])
def test_an_axis_of_two_nodes(engine, count):
    source = tuple(l + f * (n - 1) * s for l, s, n, f in zip(LL, SPACING, count, (0.37, 0.41, 0.29)))
    check(engine, (LL, SPACING, count, [source], [0.28], random_slowness(count, 12), [0]))


def layered_case():
    """Four rows over two models on 12 x 11 x 10: model 0 homogeneous, model 1 with a low-velocity layer and a fast
    block (head waves); four different sources."""
    count = (12, 11, 10)
    ix, _, iz = np.meshgrid(*(np.arange(n) for n in count), indexing="ij")
    v = np.where(iz < 3, 4.0, np.where(iz < 5, 2.0, 5.0))
    v = np.where((ix >= 8) & (iz >= 2), 6.5, v)
    slowness = np.stack([np.full(count, 0.25), 1.0 / v])
    sources = [(0.13, 1.71, 0.83), (2.9, 0.6, 1.3), (4.41, 3.97, 2.05), (-0.6, 4.1, 0.25)]
    row_model = [0, 1, 0, 1]
    s0 = [0.25, 0.5, 0.25, 0.25]
    return LL, SPACING, count, sources, s0, slowness, row_model


_LAYERED = {}


def layered_solution():
    if not _LAYERED:
        _LAYERED["want"] = t3.solve(*layered_case())
    return _LAYERED["want"]


def test_four_rows_over_two_models(engine):
    want = layered_solution()
    assert len(set(want[1].tolist())) > 1, want[1]          # the rows settle after different round counts
    assert want[1][1] > want[1][0]                          # ... the layered model later than the homogeneous one
    check(engine, layered_case(), want=want)


def test_planes_of_more_than_one_workgroup(engine):
    """24 x 24 x 24, one row: the largest plane has 432 nodes and its rectangle 576 cells."""
    count = (24, 24, 24)
    assert 432 > engine.get("tt_plane_threads")
    z = LL[2] + np.arange(24) * SPACING[2]
    slowness = np.broadcast_to(1.0 / (3.0 + 0.6 * z), (1,) + count)
    check(engine, (LL, SPACING, count, [(3.13, 2.71, 1.23)], [1.0 / (3.0 + 0.6 * 1.23)], slowness, [0]))


def test_host_and_device_sides_give_equal_bits(engine):
    want = t3.solve(*small_case())
    for slowness_on_device in (False, True):
        for device in (False, True):
            (got, _, _), _ = check(engine, small_case(), device=device, slowness_on_device=slowness_on_device, want=want)
            assert hasattr(got, "is_cuda") == device


# -- one engine, every travel-time call ---------------------------------------------------------------------------------
H = 0.125
GRID = ((-3.0, 1.5, -1.0), (0.5, 0.4, 0.25), (13, 11, 9))


def _tt_calls():
    """The calls of the interleaving test, by name: a function of an engine that returns the arrays to compare."""
    nz = 45
    z = np.arange(nz) * H
    sec_slow = np.array([1.0 / (3.0 + 0.6 * z), 1.0 / np.where(z < 1.5, 4.0, np.where(z < 2.5, 2.0, 5.0))])
    zs, s0 = np.array([0.925, 0.0375]), np.array([1.0 / (3.0 + 0.6 * 0.925), 0.25])
    stations = np.array([[-1.0, 3.5, 0.0], [0.77, 4.13, 0.33]])
    rng = np.random.default_rng(5)
    hand_made = rng.uniform(0.0, 9.0, size=(2, 70, 40))
    big, small = layered_case(), small_case()

    def eikonal(case):
        return lambda e: e.traveltimes_eikonal3d(*case, device=False)

    return {
        "eikonal_big": eikonal(big),
        "eikonal_small": eikonal(small),
        "homogeneous_big": lambda e: (e.traveltimes_homogeneous(*GRID, np.repeat(stations, 2, axis=0), [5.0, 2.9, 5.0, 2.9]),),
        "homogeneous_small": lambda e: (e.traveltimes_homogeneous(LL, SPACING, (5, 4, 3), stations[:1] * 0.1, [4.0]),),
        "sections_lds": lambda e: e.traveltime_sections(sec_slow, zs, 67, H, source_slowness=s0),
        "sections_scratch": lambda e: e.traveltime_sections(sec_slow[:1], zs[:1], 31, H, source_slowness=s0[:1],
                                                            force_scratch=True),
        "sweep": lambda e: (e.sweep_sections(hand_made, *GRID, stations[:, :2], [1, 0], [[0.0, -1.25], [0.0, -1.25]], H),),
    }


def test_between_the_other_travel_time_calls_on_one_engine(lib):
    """The call shares TravelTimeStage's buffers with the three others: on one engine, larger before smaller and the
    reverse, every result equals a fresh engine's."""
    calls = _tt_calls()
    fresh = {}
    for name, call in calls.items():
        eng = lib.Engine(0)
        try:
            fresh[name] = [np.array(a, copy=True) for a in call(eng)]
        finally:
            eng.close()
    order = ["eikonal_big", "homogeneous_big", "eikonal_small", "sections_lds", "eikonal_big", "sweep", "eikonal_small",
             "sections_scratch", "homogeneous_small", "eikonal_small", "eikonal_big"]
    eng = lib.Engine(0)
    try:
        for sequence in (order, order[::-1]):
            for step, name in enumerate(sequence):
                got = calls[name](eng)
                assert len(got) == len(fresh[name])
                for a, b in zip(got, fresh[name]):
                    a = np.asarray(a)
                    assert a.dtype == b.dtype and a.shape == b.shape, (step, name)
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (step, name)
    finally:
        eng.close()
    # and the fresh engines' eikonal results are the restatement's
    assert np.array_equal(bits(fresh["eikonal_big"][0]), bits(layered_solution()[0]))


# -- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(engine, lib):
    import torch

    ll, spacing, count, sources, s0, slowness, row_model = small_case()
    layered = layered_case()
    with pytest.raises(lib.QMHipError, match=r"row 0: not settled after 1 rounds"):
        engine.traveltimes_eikonal3d(*layered[:3], layered[3][:2], layered[4][:2], layered[5], [1, 1], max_iters=1)
    for axis, beyond in ((0, LL[0] - 0.01), (2, upper_corner(count)[2] + 0.01), (1, np.nan)):
        outside = list(sources[0])
        outside[axis] = beyond
        with pytest.raises(lib.QMHipError, match=r"row 0: source at .* outside the grid"):
            engine.traveltimes_eikonal3d(ll, spacing, count, [outside], s0, slowness, row_model)
    for bad in (0.0, np.nan):
        broken = slowness.copy()
        broken[0, 3, 2, 1] = bad
        node = (3 * count[1] + 2) * count[2] + 1
        for given in (broken, torch.as_tensor(broken, device=f"cuda:{engine.device}")):
            with pytest.raises(lib.QMHipError, match=rf"model 0: slowness (0|nan|-nan) at node {node} "):
                engine.traveltimes_eikonal3d(ll, spacing, count, sources, s0, given, row_model)
    with pytest.raises(lib.QMHipError, match=r"row 0: slowness .* at the source"):
        engine.traveltimes_eikonal3d(ll, spacing, count, sources, [0.0], slowness, row_model)
    with pytest.raises(lib.QMHipError, match=r"axis 1: 1 nodes"):
        engine.traveltimes_eikonal3d(ll, spacing, (7, 1, 5), [(0.13, 0.5, 0.83)], s0, np.full((1, 7, 1, 5), 0.3), [0])
    for model in (-1, 1):
        with pytest.raises(lib.QMHipError, match=rf"row 0: model {model} of 1"):
            engine.traveltimes_eikonal3d(ll, spacing, count, sources, s0, slowness, [model])
    check(engine, small_case())                     # and the engine goes on


# -- end to end --------------------------------------------------------------------------------------------------------
STATIONS = {"ST0": (0.13, 1.71, 0.83), "ST1": (1.0, 1.3, 0.5), "ST2": (1.9, 2.4, 1.37)}     # ST1: on a node
E2E_COUNT = (8, 7, 6)


def _rows(stations, n_ph):
    return np.repeat(np.array(list(stations.values())), n_ph, axis=0), np.tile(np.arange(n_ph), len(stations))


def test_compute_traveltimes_3d_serves_the_restatements_table(engine):
    """compute_traveltimes(method="3d") -> set_traveltime_grids -> serve -> download_lut equals rint(restatement *
    rate)."""
    from quakemigrate_amd import traveltimes as tt

    gx, gy, gz = tr.grid_xyz(LL, SPACING, E2E_COUNT)
    vp = 3.0 + 0.6 * gz + 0.8 * np.exp(-((gx - 0.5) ** 2 + (gy - 1.5) ** 2 + (gz - 0.9) ** 2))
    velocity = {"P": vp, "S": vp / 1.73}
    phases = ("P", "S")
    lut = tt.compute_traveltimes(engine, LL, SPACING, E2E_COUNT, STATIONS, "3d", phases=phases, velocity=velocity)
    assert list(lut) == list(STATIONS) and all(list(lut[s]) == list(phases) for s in lut)
    grids = [lut[s][ph] for s in lut for ph in phases]
    assert all(g.is_cuda and tuple(g.shape) == E2E_COUNT for g in grids)

    sources, row_model = _rows(STATIONS, 2)
    s0 = np.array([1.0 / tt.trilinear(velocity[ph], LL, SPACING, E2E_COUNT, [xyz])[0]
                   for xyz in STATIONS.values() for ph in phases])
    slowness = np.stack([1.0 / velocity[ph] for ph in phases])
    want, _, status = t3.solve(LL, SPACING, E2E_COUNT, sources, s0, slowness, row_model)
    assert not status.any()
    for g, w in zip(grids, want):
        assert np.array_equal(bits(g), bits(w))

    rate = 50.0
    engine.set_traveltime_grids(grids)
    engine.serve(rate, np.arange(len(grids)))
    table = engine.download_lut()
    assert np.array_equal(table, np.stack([np.rint(w * rate).astype(np.int32) for w in want], axis=-1))

    # the same volumes from the device, and the sources moved to the reference's nodes
    import torch

    on_device = {ph: torch.as_tensor(v, device=f"cuda:{engine.device}") for ph, v in velocity.items()}
    again = tt.compute_traveltimes(engine, LL, SPACING, E2E_COUNT, STATIONS, "3d", phases=phases, velocity=on_device,
                                   device=False)
    device_slowness = torch.stack([1.0 / on_device[ph] for ph in phases]).cpu().numpy()
    want_again = t3.solve(LL, SPACING, E2E_COUNT, sources, s0, device_slowness, row_model)[0]
    for r, (s, ph) in enumerate((s, ph) for s in STATIONS for ph in phases):
        assert np.array_equal(bits(again[s][ph]), bits(want_again[r]))
    snapped = tt.compute_traveltimes(engine, LL, SPACING, E2E_COUNT, STATIONS, "3d", phases=("P",), velocity=velocity,
                                     device=False, snap_to_node=True)
    idx, nodes = tt.nearest_node(LL, SPACING, E2E_COUNT, list(STATIONS.values()))
    s0_nodes = 1.0 / tt.trilinear(vp, LL, SPACING, E2E_COUNT, nodes)
    want_snapped = t3.solve(LL, SPACING, E2E_COUNT, nodes, s0_nodes, slowness[:1], [0, 0, 0])[0]
    for r, s in enumerate(STATIONS):
        assert np.array_equal(bits(snapped[s]["P"]), bits(want_snapped[r]))
        assert snapped[s]["P"][tuple(idx[r])] == 0.0


def test_compute_traveltimes_1d_on_the_grid(engine):
    """method="1d", solver="grid" equals the restatement on the model spread over the grid's depths by
    model_velocity, linear and as blocks."""
    from quakemigrate_amd import traveltimes as tt

    vmod = {"Depth": np.array([-3.0, 0.5, 2.0]), "Vp": np.array([3.2, 4.9, 6.1]), "Vs": np.array([1.8, 2.8, 3.5])}
    phases = ("P", "S")
    depths = LL[2] + np.arange(E2E_COUNT[2]) * SPACING[2]
    sources, row_model = _rows(STATIONS, 2)
    for block_model in (False, True):
        lut = tt.compute_traveltimes(engine, LL, SPACING, E2E_COUNT, STATIONS, "1d", phases=phases, vmod=vmod,
                                     solver="grid", block_model=block_model, device=False)
        slowness = np.stack([np.broadcast_to(1.0 / tt.model_velocity(vmod, ph, depths, block_model), E2E_COUNT)
                             for ph in phases])
        s0 = np.array([1.0 / tt.model_velocity(vmod, ph, xyz[2], block_model) for xyz in STATIONS.values() for ph in phases])
        want, _, status = t3.solve(LL, SPACING, E2E_COUNT, sources, s0, slowness, row_model)
        assert not status.any()
        for r, (s, ph) in enumerate((s, ph) for s in STATIONS for ph in phases):
            assert np.array_equal(bits(lut[s][ph]), bits(want[r])), (block_model, s, ph)


# -- the stage clock ---------------------------------------------------------------------------------------------------
def test_stage_clock(lib):
    eng = lib.Engine(0)
    try:
        assert eng.get("tt_ns_eikonal3d") == 0
        eng.traveltimes_eikonal3d(*small_case(), device=False)
        assert eng.get("tt_ns_eikonal3d") > 0
        assert eng.get("tt_ns_sections") == 0 and eng.get("tt_ns_sweep") == 0 and eng.get("tt_ns_homogeneous") == 0
    finally:
        eng.close()
