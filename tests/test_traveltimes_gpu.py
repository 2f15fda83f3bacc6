# -*- coding: utf-8 -*-
"""
Travel-time tables on the GPU (include/qmhip.h: qm_engine_tt_homogeneous / _tt_sections / _tt_sweep; kernels:
csrc/qm_traveltimes.hpp) against their NumPy restatement (tests/traveltimes_ref.py, pinned to closed forms and SciPy by
tests/test_traveltimes_host.py).  Every float has the restatement's bits and every integer is equal: the kernels run
the restatement's operations in its order, so there is no tolerance anywhere in this file.
"""

import numpy as np
import pytest

import traveltimes_ref as tr

pytestmark = pytest.mark.gpu

# the 3-D grid: non-cubic spacing, negative ll_corner z; its depths are negative, zero and exact multiples of H
LL = (-3.0, 1.5, -1.0)
SPACING = (0.5, 0.4, 0.25)
COUNT = (23, 19, 17)
STATIONS = np.array([
    [-1.0, 3.5, 0.0],           # on a node (4, 5, 4): d = 0 under it
    [0.77, 4.13, 0.33],         # between nodes
    [-5.2, 2.0, 0.1],           # outside the grid horizontally
    [2.0, 6.0, -2.3],           # above the grid
    [-3.0, 1.5, -1.0],          # at a corner
])
VELOCITIES = (5.0, 2.9)
# A row's nodes past one pass of the per-node kernels' launch grid.  (130 x 67 x 33, 287 430 nodes, would not be: the
# grid of 2048 x 256 threads strides over ONE row's nodes, row after row, so the row itself has to exceed it.)
BIG_COUNT = (130, 67, 65)
H = 0.125                       # the sections' spacing


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


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


# -- a. homogeneous ----------------------------------------------------------------------------------------------------
def _rows():
    xyz = np.repeat(STATIONS, len(VELOCITIES), axis=0)
    vel = np.tile(VELOCITIES, len(STATIONS))
    return xyz, vel


@pytest.mark.parametrize("device", [False, True])
def test_homogeneous_has_the_restatements_bits(engine, device):
    xyz, vel = _rows()
    got = engine.traveltimes_homogeneous(LL, SPACING, COUNT, xyz, vel, device=device)
    assert tuple(got.shape) == (len(vel),) + COUNT
    for r in range(len(vel)):
        want = tr.homogeneous(LL, SPACING, COUNT, xyz[r], vel[r])
        assert np.array_equal(bits(got[r]), bits(want)), r
    assert host(got[0])[4, 5, 4] == 0.0             # the station on a node
    assert engine.get("tt_ns_homogeneous") > 0


def test_homogeneous_past_one_pass_of_the_launch_grid(engine):
    xyz, vel = STATIONS[1:3], np.array(VELOCITIES)
    threads = engine.get("tt_grid_blocks") * engine.get("tt_grid_threads")
    assert int(np.prod(BIG_COUNT)) > threads        # (the grid strides over a row's nodes, row after row)
    got = engine.traveltimes_homogeneous(LL, SPACING, BIG_COUNT, xyz, vel)
    for r in range(len(vel)):
        assert np.array_equal(bits(got[r]), bits(tr.homogeneous(LL, SPACING, BIG_COUNT, xyz[r], vel[r]))), r


def test_homogeneous_refusals(engine, lib):
    with pytest.raises(lib.QMHipError, match="row 1: velocity"):
        engine.traveltimes_homogeneous(LL, SPACING, COUNT, STATIONS[:2], [5.0, 0.0])
    with pytest.raises(lib.QMHipError, match="row 0: station"):
        engine.traveltimes_homogeneous(LL, SPACING, COUNT, [[np.nan, 0.0, 0.0]], [5.0])
    with pytest.raises(lib.QMHipError, match="node_spacing"):
        engine.traveltimes_homogeneous(LL, (0.5, 0.0, 0.25), COUNT, STATIONS[:1], [5.0])


# -- b. sections -------------------------------------------------------------------------------------------------------
def models(nz):
    """Velocity per depth row: homogeneous, gradient, three blocks 3.0 / 5.0 / 6.5 (head waves), a low-velocity layer."""
    z = np.arange(nz) * H
    top = z[-1]
    return {
        "homogeneous": np.full(nz, 4.0),
        "gradient": 3.0 + 0.6 * z,
        "blocks": np.where(z < 0.3 * top, 3.0, np.where(z < 0.6 * top, 5.0, 6.5)),
        "low_velocity": np.where(z < 0.3 * top, 4.0, np.where(z < 0.5 * top, 2.0, 5.0)),
    }


def source_depths(nz):
    """On a row, between rows, in the top cell, in the bottom cell."""
    return [7 * H, 7.4 * H, 0.3 * H, (nz - 2 + 0.6) * H]


def section_inputs(nz, names=None, depths=None):
    slowness, zs, s0 = [], [], []
    for name, v in models(nz).items():
        if names is not None and name not in names:
            continue
        for d in (source_depths(nz) if depths is None else depths):
            slowness.append(1.0 / v)
            zs.append(d)
            s0.append(1.0 / np.interp(d, np.arange(nz) * H, v))
    return np.array(slowness), np.array(zs), np.array(s0)


_SOLVED = {}


def solved(nr, nz):
    """The restatement on the sixteen sections (4 models x 4 source depths) of a shape, computed once."""
    if (nr, nz) not in _SOLVED:
        slowness, zs, s0 = section_inputs(nz)
        _SOLVED[nr, nz] = (slowness, zs, s0) + tuple(tr.solve_sections(slowness, zs, s0, nr, H))
    return _SOLVED[nr, nz]


def check_sections(engine, nr, nz, **kwargs):
    slowness, zs, s0, T, rounds, status = solved(nr, nz)
    got_T, got_rounds, got_status = engine.traveltime_sections(slowness, zs, nr, H, source_slowness=s0, **kwargs)
    assert np.array_equal(host(got_status), status) and not status.any()
    assert np.array_equal(host(got_rounds), rounds)
    assert np.array_equal(bits(got_T), bits(T))
    return got_T


@pytest.mark.parametrize("shape", [(67, 45), (45, 67)])
def test_sections_have_the_restatements_bits(engine, shape):
    """Diagonal counts that are no multiples of 64; sixteen sections of four models in one launch."""
    nr, nz = shape
    check_sections(engine, nr, nz)
    rounds = solved(nr, nz)[4].reshape(4, 4)
    assert rounds[3].min() > 2                      # the low-velocity layer takes more than one round of work
    assert engine.get("tt_ns_sections") > 0


@pytest.mark.parametrize("side", ["under", "over"])
def test_sections_on_both_sides_of_the_lds_limit(engine, side):
    limit = engine.get("tt_lds_nodes")
    nz = 125
    nr = limit // nz + (1 if side == "over" else 0)
    assert nr != nz and ((nr * nz > limit) == (side == "over")) and (nr + 1) * nz > limit
    check_sections(engine, nr, nz)


def test_lds_and_scratch_forms_give_equal_bits(engine):
    nr, nz = 67, 45
    assert nr * nz <= engine.get("tt_lds_nodes")
    a = check_sections(engine, nr, nz)
    b = check_sections(engine, nr, nz, force_scratch=True)
    assert np.array_equal(bits(a), bits(b))
    c = check_sections(engine, nr, nz, force_scratch=True, device=True)
    assert np.array_equal(bits(a), bits(c))


def test_strict_iteration_has_the_restatements_bits(engine):
    """tol = 0: a value is taken whenever it is below the old one at all.  More rounds, the same agreement."""
    nr, nz = 45, 67
    slowness, zs, s0 = section_inputs(nz, names=("gradient", "low_velocity"), depths=[7.4 * H, 0.3 * H])
    T, rounds, status = tr.solve_sections(slowness, zs, s0, nr, H, tol=0.0)
    default_rounds = solved(nr, nz)[4].reshape(4, 4)[[1, 3]][:, [1, 2]].reshape(-1)
    assert not status.any() and np.all(rounds > default_rounds)
    for force_scratch in (False, True):
        got = engine.traveltime_sections(slowness, zs, nr, H, source_slowness=s0, tol=0.0, force_scratch=force_scratch)
        assert np.array_equal(got[2], status) and np.array_equal(got[1], rounds)
        assert np.array_equal(bits(got[0]), bits(T))


def test_diagonals_longer_than_one_pass_of_the_workgroup(engine):
    """515 x 514: the longest diagonals (514 nodes, two of them per sweep) exceed the workgroup's 512 threads, so the
    kernel's walk along a diagonal (``ip += threads``) takes its second trip; the largest diagonal of the other cases
    has 125 nodes.  Above the LDS limit: the scratch form.
    Two sections in one launch, the gradient and the low-velocity model, the source between rows.  The restatement
    settles in 7 and 8 rounds (about 4 s on a CPU); the kernel's time is printed (``-s``)."""
    nr, nz = 515, 514
    threads = engine.get("tt_section_threads")
    assert min(nr, nz) > threads
    assert nr * nz > engine.get("tt_lds_nodes")
    slowness, zs, s0 = section_inputs(nz, names=("gradient", "low_velocity"), depths=[7.4 * H])
    assert slowness.shape == (2, nz)
    T, rounds, status = tr.solve_sections(slowness, zs, s0, nr, H)
    got_T, got_rounds, got_status = engine.traveltime_sections(slowness, zs, nr, H, source_slowness=s0)
    print(f"\n{nr} x {nz}, 2 sections: rounds {rounds.tolist()}, status {status.tolist()}, kernel "
          f"{engine.get('tt_ns_sections') / 1e6:.1f} ms")
    assert np.array_equal(got_status, status) and not status.any()
    assert np.array_equal(got_rounds, rounds)
    assert np.array_equal(bits(got_T), bits(T))


def test_sections_refusals(engine, lib):
    nr, nz = 67, 45
    slowness, zs, s0 = section_inputs(nz, names=("gradient", "low_velocity"), depths=[7.4 * H])
    with pytest.raises(lib.QMHipError, match=r"section 0: not settled after 1 rounds"):
        engine.traveltime_sections(slowness[1:], zs[1:], nr, H, source_slowness=s0[1:], max_iters=1)    # low velocity
    ok = engine.traveltime_sections(slowness, zs, nr, H, source_slowness=s0)
    assert not ok[2].any()
    for bad in (0.0, -0.25, np.nan, np.inf):
        broken = slowness.copy()
        broken[1, 17] = bad
        with pytest.raises(lib.QMHipError, match=r"section 1: slowness .* in row 17"):
            engine.traveltime_sections(broken, zs, nr, H, source_slowness=s0)
    for depth in (-0.01, (nz - 1) * H, (nz + 3) * H, np.nan):
        with pytest.raises(lib.QMHipError, match=r"section 1: source at depth"):
            engine.traveltime_sections(slowness, [zs[0], depth], nr, H, source_slowness=s0)
    with pytest.raises(lib.QMHipError, match=r"section 0: slowness .* at the source"):
        engine.traveltime_sections(slowness, zs, nr, H, source_slowness=[0.0, s0[1]])


# -- c. sweep ----------------------------------------------------------------------------------------------------------
# Two section spacings.  H divides the grid's z spacing: every depth is an exact multiple of it -- negative ones and
# zero among them -- and the fraction along z is 0 at every node.  H_OFF does not: the depths from -1.0 up are
# negative and positive non-multiples (np.remainder adds the spacing back for the negative ones), the fraction along
# z takes values all over (0, 1), and off a multiple of the spacing the origin shifts the cell against the fraction.
H_OFF = 0.07
SPACINGS = [H, H_OFF]


def _section_plan(h=H):
    """The sections of STATIONS on the grid, as the planner lays them out (z0 a multiple of h)."""
    from quakemigrate_amd import traveltimes as tt

    return tt.plan_sections(LL, SPACING, COUNT, STATIONS, h)


def _origins(plan, h, z0_on_multiple):
    """(x0, z0) per station; off the multiples the origin lies 0.4 h higher, which keeps every cell inside sections
    that have a row to spare."""
    return np.column_stack([np.zeros(len(STATIONS)), plan["z0"] - (0.0 if z0_on_multiple else 0.4 * h)])


def check_sweep(engine, sections, origins, row_section, h, device=False):
    got = engine.sweep_sections(sections, LL, SPACING, COUNT, STATIONS[:, :2], row_section, origins, h, device=device)
    sec = host(sections)
    for r in range(len(STATIONS)):
        want = tr.sweep(LL, SPACING, COUNT, STATIONS[r, :2], sec[row_section[r]], origins[r][0], origins[r][1], h)
        assert np.array_equal(bits(got[r]), bits(want)), r
    return got


def check_fractions(h, origins, z0_on_multiple):
    """What the spacing puts in front of the kernel: see SPACINGS."""
    depth = tr.grid_xyz(LL, SPACING, COUNT)[2][0, 0, :]
    fz = np.remainder(depth, h) / h
    if h == H:
        assert np.all(fz == 0.0) and depth.min() < 0.0 and np.any(depth == 0.0)
    else:
        assert np.any((depth < 0.0) & (fz > 0.0)) and np.any((depth > 0.0) & (fz > 0.0))
        assert fz.min() < 0.2 and fz.max() > 0.8 and np.any(fz == 0.0)      # (depth 0 is a node)
        # off a multiple, the cell of the floor and the cell the fraction belongs to part at some depths
        if not z0_on_multiple:
            offset = (depth - origins[0, 1]) / h
            assert np.any(np.floor(offset) != np.rint(offset - fz))


@pytest.mark.parametrize("z0_on_multiple", [True, False])
@pytest.mark.parametrize("h", SPACINGS)
def test_sweep_of_the_solvers_sections(engine, h, z0_on_multiple):
    from quakemigrate_amd import traveltimes as tt

    plan = _section_plan(h)
    vmod = {"Depth": [-3.0, 0.5, 2.0], "Vp": [3.2, 4.9, 6.1]}
    rows = np.arange(plan["nz"]) * h
    slowness = np.array([1.0 / tt.model_velocity(vmod, "P", z0 + rows) for z0 in plan["z0"]])
    s0 = 1.0 / tt.model_velocity(vmod, "P", STATIONS[:, 2])
    sections, _, _ = engine.traveltime_sections(slowness, plan["source_depth"], plan["nr"], h, source_slowness=s0,
                                                device=True)
    origins = _origins(plan, h, z0_on_multiple)     # (the planner's margin of 5 rows is the row to spare)
    got = check_sweep(engine, sections, origins, np.arange(len(STATIONS)), h, device=True)
    check_fractions(h, origins, z0_on_multiple)
    assert np.all(np.isfinite(host(got)))
    assert engine.get("tt_ns_sweep") > 0


@pytest.mark.parametrize("z0_on_multiple", [True, False])
@pytest.mark.parametrize("h", SPACINGS)
def test_sweep_of_hand_made_sections(engine, h, z0_on_multiple):
    """Random sections from the host: all four corners of a cell differ, so a corner taken from the wrong place shows
    wherever its weight is not 0.  With z0 off the multiples of h the reference's remainder rule shows: the fractions
    are those of the coordinates, the cell that of the offsets."""
    plan = _section_plan(h)
    rng = np.random.default_rng(20261020)
    sections = rng.uniform(0.0, 9.0, size=(3, plan["nr"], plan["nz"] + 1))
    origins = _origins(plan, h, z0_on_multiple)
    got = check_sweep(engine, sections, origins, np.array([2, 0, 1, 1, 2]), h)
    check_fractions(h, origins, z0_on_multiple)
    assert np.all(np.isfinite(got))


def test_sweep_refuses_a_node_outside_its_section(engine, lib):
    plan = _section_plan()
    sections = np.ones((1, plan["nr"], plan["nz"]))
    origins = np.column_stack([np.zeros(len(STATIONS)), plan["z0"]])
    origins[3, 1] = LL[2] + 3 * H                   # row 3's section now starts below the grid's first depths
    d, z = tr.distances_depths(LL, SPACING, COUNT, STATIONS[3, :2])
    first = tr.outside(d, z, origins[3, 0], origins[3, 1], H, plan["nr"], plan["nz"])[0]
    with pytest.raises(lib.QMHipError, match=rf"row 3: node {first} .* lies outside section 0"):
        engine.sweep_sections(sections, LL, SPACING, COUNT, STATIONS[:, :2], np.zeros(5, dtype=np.int32), origins, H)
    origins[3, 1] = plan["z0"][3]
    short = np.ones((1, plan["nr"] - 8, plan["nz"]))    # the far corner's distance now leaves the columns
    with pytest.raises(lib.QMHipError, match=r"row \d: node \d+ .* lies outside section 0"):
        engine.sweep_sections(short, LL, SPACING, COUNT, STATIONS[:, :2], np.zeros(5, dtype=np.int32), origins, H)
    with pytest.raises(lib.QMHipError, match=r"row 2: section 4 of 1"):
        engine.sweep_sections(sections.tolist(), LL, SPACING, COUNT, STATIONS[:, :2], [0, 0, 4, 0, 0], origins, H)


# -- end to end --------------------------------------------------------------------------------------------------------
def test_compute_traveltimes_serves_the_restatements_table(engine):
    """compute_traveltimes(method="1d", device=True) -> set_traveltime_grids -> serve -> download_lut equals
    rint(grid * rate) of the restatement's grids."""
    from quakemigrate_amd import traveltimes as tt

    vmod = {"Depth": np.array([-3.0, 0.5, 2.0]), "Vp": np.array([3.2, 4.9, 6.1]), "Vs": np.array([1.8, 2.8, 3.5])}
    stations = {f"ST{i}": tuple(xyz) for i, xyz in enumerate(STATIONS)}
    phases = ("P", "S")
    lut = tt.compute_traveltimes(engine, LL, SPACING, COUNT, stations, "1d", phases=phases, vmod=vmod, section_dx=H,
                                 device=True)
    assert list(lut) == list(stations) and all(list(lut[s]) == list(phases) for s in lut)
    grids = [lut[s][ph] for s in lut for ph in phases]
    assert all(g.is_cuda and tuple(g.shape) == COUNT for g in grids)

    plan = tt.plan_sections(LL, SPACING, COUNT, STATIONS, H)
    rows = np.arange(plan["nz"]) * H
    slowness = np.array([1.0 / tt.model_velocity(vmod, ph, plan["z0"][i] + rows)
                         for i in range(len(STATIONS)) for ph in phases])
    s0 = np.array([1.0 / tt.model_velocity(vmod, ph, STATIONS[i, 2]) for i in range(len(STATIONS)) for ph in phases])
    sections = tr.solve_sections(slowness, np.repeat(plan["source_depth"], 2), s0, plan["nr"], H)[0]
    want = [tr.sweep(LL, SPACING, COUNT, STATIONS[r // 2, :2], sections[r], 0.0, plan["z0"][r // 2], H)
            for r in range(len(sections))]
    for g, w in zip(grids, want):
        assert np.array_equal(bits(g), bits(w))

    rate = 50.0
    engine.set_traveltime_grids(grids)
    engine.serve(rate, np.arange(len(grids)))
    table = engine.download_lut()
    expected = np.stack([np.rint(w * rate).astype(np.int32) for w in want], axis=-1)
    assert np.array_equal(table, expected)

    host_lut = tt.compute_traveltimes(engine, LL, SPACING, COUNT, stations, "homogeneous", vp=5.0, vs=2.9, device=False)
    assert np.array_equal(bits(host_lut["ST1"]["S"]), bits(tr.homogeneous(LL, SPACING, COUNT, STATIONS[1], 2.9)))
