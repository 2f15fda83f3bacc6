# -*- coding: utf-8 -*-
"""
CPU checks of tests/shift_layout.py: the designed travel-time tables reach what tests/test_shift_windows.py relies
on -- every window register, every quad count and alignment of the shift-reuse schedule, bricks exactly on the LDS
limit -- and the recipe tables of the older GPU tests do not (the gap those tables close).  Same seeds as on the GPU.
"""

import itertools

import numpy as np
import pytest

import shift_layout as sl

C = sl.constants()
TOP = {False: 4 * C["kShiftNqMax"] - 4, True: 4 * C["kShiftNqMax"] - C["kShiftWideSpl"]}   # nq = NQMAX: 20 and 18
# the largest offset each roster table must reach on (256-sample tiles, wide tiles) -- stated here, not taken from the
# designers: the tables made for the wide tiles hold 18 on both kinds (their launches run 256-sample tiles too)
REACH = {"n30": (20, None), "n29": (20, None), "n41": (20, None), "n70": (20, None), "w30": (18, 18), "w41": (None, 18),
         "neg29": (18, 18)}


def _layouts(name, kind):
    narrow, wide, direct = sl.case_layouts(name, kind)
    return [L for L in (narrow, wide) if L is not None], direct


def test_every_flavour_runs_on_a_table_that_reaches_the_top_of_its_window():
    """every workgroup shape is launched on at least one table whose layout of that shape holds the top offset"""
    for kind in ("4", "8", "12", "rows8", "rows2", "rows4"):
        assert any(k == kind and REACH[n][0] == TOP[False] for n, k in sl.CASES), kind
    for kind in ("wide", "wide_rows"):
        assert any(k == kind and REACH[n][1] == TOP[True] for n, k in sl.CASES), kind


def test_constants_come_from_the_generated_header():
    assert C["kShiftNqMax"] == 6 and C["kShiftNqMin"] <= C["kShiftNqMax"], C
    assert TOP == {False: 20, True: 18}
    assert sl.plane_bytes("4") % 16 == 0 and sl.plane_bytes("8") % 16 == 0 and sl.plane_bytes("wide") % 16 == 0
    text = sl.INC.read_text()
    for name in ("kShiftPlane", "kShiftPlane8"):
        assert f"constexpr int {name} = {C[name]};" in text


@pytest.mark.parametrize("name,kind", sl.CASES)
def test_every_window_register_is_consumed_by_every_node_position(name, kind):
    """Offset coverage: (node position 0..7) x (offset 0..20) on 256-sample tiles, x (0..18) on wide tiles; the top
    offset at NQMAX quads in both row parities (the loop alternates between two register windows by row).  The
    tables of M_WIDE also run 256-sample tiles (the tile behind the wide ones): those reach 18, which the tables of
    M_NARROW cover to 20."""
    layouts, _ = _layouts(name, kind)
    for L in layouts:
        top = REACH[name][int(L.wide)]
        assert L.top_offset() == top and top <= TOP[L.wide], (name, kind, L.wide, L.top_offset())
        seen = np.zeros((8, top + 1), dtype=bool)
        for pos in range(8):
            offs = L.off[:, pos, :][np.broadcast_to(L.valid[:, pos, None], L.off[:, pos, :].shape)]
            seen[pos, np.unique(offs)] = True
        assert seen.all(), (name, kind, L.wide, np.argwhere(~seen)[:8])
        for parity in (0, 1):
            rows = np.arange(L.S) % 2 == parity
            for pos in range(8):
                at_top = (L.off[:, pos, :] == top) & L.valid[:, pos, None] & (L.nq == L.nq_max) & rows[None, :]
                assert at_top.any(), (name, kind, L.wide, pos, parity)
        assert len(sl.witness_targets(L, (top - 1, top))) == 32
        assert len(sl.witness_targets(L, (top - 1, top), parities=None)) == 16


@pytest.mark.parametrize("name,kind", sl.CASES)
def test_every_quad_count_transition_and_alignment(name, kind):
    layouts, direct = _layouts(name, kind)
    for L in layouts:
        assert set(np.unique(L.nq)) == set(range(2, L.nq_max + 1)), (name, kind, np.unique(L.nq))
        cls = np.where(L.nq <= 4, 4, L.nq)                       # quads 5 and 6 are fetched behind branches
        pairs = set(zip(cls[:, :-1].ravel().tolist(), cls[:, 1:].ravel().tolist()))
        assert pairs == set(itertools.product((4, 5, 6), repeat=2)), (name, kind, sorted(pairs))
        lead = L.dmin - L.e0                                      # samples of the window in front of the first add
        if L.wide:
            assert set(np.unique(lead)) == {0, 1} and set(np.unique(L.e0 % 4)) == {0, 2}
        else:
            assert set(np.unique(lead)) == {0, 1, 2, 3} and set(np.unique(L.e0 % 4)) == {0}
    assert direct == 0, (name, kind, direct)                      # a cap: no brick leaves for the direct kernel


def test_noise_limits_of_the_register_window():
    """m = 20 (18 on wide tiles) is the largest noise whose windows hold NQMAX quads; one more overflows."""
    grid, rows = (9, 11, 13), 12
    for wide, m in ((False, sl.M_NARROW), (True, sl.M_WIDE)):
        at = sl.Layout(sl.noise_table(grid, rows, m, 7), (8, 8, 8), wide)
        assert at.top_offset() == TOP[wide] == m and at.nq.max() == at.nq_max and not at.over.any()
        past = sl.Layout(sl.noise_table(grid, rows, m + 1, 7), (8, 8, 8), wide)
        assert past.nq.max() == past.nq_max + 1 and past.over.any()
    # a noise the wide tiles cannot hold is fine on 256-sample tiles, and lowering m loses the top registers
    assert not sl.Layout(sl.noise_table(grid, rows, sl.M_NARROW, 7), (8, 8, 8), False).over.any()
    assert sl.Layout(sl.noise_table(grid, rows, sl.M_NARROW, 7), (8, 8, 8), True).over.any()
    assert sl.Layout(sl.noise_table(grid, rows, 18, 7), (8, 8, 8), False).top_offset() == 18


def test_negative_entries_count_as_zero():
    tt = sl.table("neg29")
    assert (tt == -3).sum() >= 6 and (tt == sl.INT32_MIN).sum() >= 6
    L = sl.Layout(tt, (8, 8, 8))
    assert np.array_equal(L.lo, sl.Layout(np.maximum(tt, 0), (8, 8, 8)).lo) and (L.off >= 0).all()


@pytest.mark.parametrize("name", list(sl.BOUNDARIES))
def test_boundary_tables_sit_exactly_on_the_limit(name):
    """Brick 0: run + zero row = plane_bytes / 16 (fits); brick 1: one slot more (direct kernel); brick 2: far below
    the limit with ONE group at NQMAX + 1 quads (direct); brick 3: the same group at exactly NQMAX (fits).  Odd row
    counts: bricks 0 and 1 would both fit without the padding row's zero window."""
    spec = sl.BOUNDARIES[name]
    tt, limit = sl.boundary(name)
    assert limit * 16 == sl.plane_bytes(spec.kind)
    narrow, wide, direct = sl.engine_layouts(tt, spec.kind, spec.brick)
    L = wide if spec.kind == "wide" else narrow
    assert L.nbricks == 4
    total = (L.run + L.zero)[:, 0]
    assert total[0] == limit and total[1] == limit + 1 and total[2] < limit and total[3] < limit
    assert L.overflow[:, 0].tolist() == [False, False, True, False]
    nq_of_brick = [L.nq[L.brick_of_group == b].max() for b in range(4)]
    assert nq_of_brick[2] == L.nq_max + 1 and nq_of_brick[3] == L.nq_max
    assert (L.nq[L.brick_of_group == 2] > L.nq_max).sum() == 1
    assert L.fits(sl.plane_bytes(spec.kind)).tolist() == sl.BOUNDARY_FIT and direct == 2
    if spec.rows % 2:
        assert (L.zero[:, 0] == L.zero_slots).all() and L.run[1, 0] <= limit < L.run[1, 0] + L.zero_slots
    else:
        assert (L.zero == 0).all()
    if spec.kind == "wide":                                       # the 256-sample tiles' windows are not what binds
        assert narrow.fits(sl.plane_bytes("8")).tolist() == [True, True, True, True]


def test_recipe_tables_of_the_older_gpu_tests_stop_short_of_the_top_registers():
    """A record of the gap the designed tables close: the homogeneous-velocity recipes behind SHIFT_SHAPES /
    WIDE_SHAPES (tests/test_gpu_parity.py) never consume the window's last registers -- offsets stay <= 18 of 20 on
    256-sample tiles and <= 16 of 18 on wide tiles in the groups that stay on the shift-reuse loops (8x8x8 bricks).
    If a change to quakemigrate_amd.synth moves this, this test says so."""
    from quakemigrate_amd import synth
    from test_gpu_parity import SHIFT_SHAPES, WIDE_SHAPES

    shapes = {(s[0], s[1], s[2]) for s in SHIFT_SHAPES} | {(s[0], s[1], s[2]) for s in WIDE_SHAPES}
    reach = {False: 0, True: 0}
    for recipe, grid, rows in sorted(shapes):
        tt = synth.make_case(recipe, step=1, grid=grid, rows=rows, n_samples=64).traveltimes
        for wide in (False, True):
            L = sl.Layout(tt, (8, 8, 8), wide)
            ok = (L.nq <= L.nq_max)[:, None, :] & L.valid[:, :, None]
            reach[wide] = max(reach[wide], int((L.off * ok).max()))
    assert reach[False] <= 18 < TOP[False] and reach[True] <= 16 < TOP[True], reach
