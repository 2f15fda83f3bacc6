# -*- coding: utf-8 -*-
"""
The generated shift-reuse loops (csrc/gen_shift_asm.py -> qm_shift_asm.inc) at the TOP of their register windows.

The recipe tables of tests/test_gpu_parity.py (quakemigrate_amd.synth: homogeneous velocities) never make an add
consume the last registers of a 24-double window: window offsets stay <= 18 of 20 (wide tiles: 16 of 18), so the
sixth quad's second half -- the 8-wave shape's far plane, the last ds_read_b64s of a tail tile's row, the wide
tiles' second conditional read -- could be dropped or mis-addressed without a test noticing.  Here every flavour of
the loops runs on tables DESIGNED with the NumPy restatement of the schedule (tests/shift_layout.py, checked on the
CPU by tests/test_shift_layout.py): bounded-noise tables that reach offset 20 (18) at six quads for every node
position with no brick on the direct kernel, and boundary tables whose bricks sit exactly on and one slot past the
LDS limit.

Reference: oracle.detect, oracle.c_migrate and the time sum of the oracle's volume.  Bounds: those of
tests/test_gpu_parity.py (indices equal, max_coa and stored values TIGHT, max_norm_coa and the marginal map NORM,
the round-2 engine's bits where the older shift tests ask for them).  Every case first proves by the engine's
read-outs that the flavour it is there for has run.
"""

import numpy as np
import pytest

import shift_layout as sl
from test_gpu_parity import NORM, TIGHT, _assert_series

pytestmark = pytest.mark.gpu
FSMP = 30


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    assert _lib.qmlib.qm_device_count() >= 1, "no HIP device visible"
    return _lib


def _brick_cfg(kind):
    """the brick shape is fixed so that the restatement knows it (the row-block forms have their own)"""
    if kind in sl.BLOCK_FORMS:
        return {}
    bx, by, bz = sl.BRICKS.get(kind, (8, 8, 8))
    return {"brick_x": bx, "brick_y": by, "brick_z": bz}


# Which generated loop a case is there for, and how the engine is brought to it.  Per case: table (shift_layout.TABLES),
# workgroup shape (shift_layout.plane_bytes), engine configuration, scanned samples, the samples [t_lo, t_hi) that the
# tile kind under test computes (the witness events go there), calls ("d" detect, "v" volume, "m" marginal map),
# loop flavours (shift_lazy), expected read-outs.
#
#   shift_groups_detect / _lazy, _volume, _marginal        "w4"      4 waves, <= 32 rows
#   shift_groups_detect8 / _lazy, _volume8, _marginal8     "w8"      33-64 rows: plane B through the far-plane register
#   shift_groups_detect3                                   "w12"     shift_waves = 12
#   shift_tail{1,2,3}_{detect,volume,marginal}             "tail*"   remainders of 61 / 125 / 190 samples (4 and 8 waves)
#   shift_group_rows8                                      "rows8"   > 64 rows, shift_rows_direct = 0
#   shift_group_rows / _lazy, shift_group_rows_volume      "rows2", "rows4"   shift_rows_direct = 1 and 2
#   shift_wide_detect / _lazy                              "wide"    shift_wide = 1
#   shift_wide_rows / _lazy                                "wide_rows"   shift_wide_rows = 2
#   shift_wide_detect_bmax / _bmax_lazy, stack_shift_bricks_kernel<4> / <8>: TIE_CASES below (tie_rule = 1)
FLAVOURS = {
    "w4": dict(table="n30", kind="4", cfg={"shift_waves": 4, "shift_tail": 0}, ns=300, span=(0, 300), calls="dvm",
               lazy=(0, 1), expect={"shift_waves": 4, "shift_tail_spl": 0, "shift_row_blocks": 1}),
    "w8": dict(table="n41", kind="8", cfg={"shift_tail": 0}, ns=300, span=(0, 300), calls="dvm", lazy=(0, 1),
               expect={"shift_waves": 8, "shift_tail_spl": 0, "shift_row_blocks": 1}),
    "w8-even-pairs": dict(table="n29", kind="8", cfg={"shift_waves": 8}, ns=512, span=(0, 512), calls="d",
                          lazy=(0, 1), expect={"shift_waves": 8, "shift_tail_spl": 0}),
    "w12": dict(table="n30", kind="12", cfg={"shift_waves": 12}, ns=512, span=(0, 512), calls="d", lazy=(0,),
                expect={"shift_waves": 12, "shift_tail_spl": 0}),
    "tail1": dict(table="n29", kind="4", cfg={"shift_waves": 4}, ns=317, span=(256, 317), calls="dvm", lazy=(0, 1),
                  expect={"shift_waves": 4, "shift_tail_spl": 1}),
    "tail2": dict(table="n29", kind="4", cfg={"shift_waves": 4}, ns=381, span=(256, 381), calls="dvm", lazy=(0,),
                  expect={"shift_waves": 4, "shift_tail_spl": 2}),
    "tail3": dict(table="n29", kind="4", cfg={"shift_waves": 4}, ns=446, span=(256, 446), calls="dvm", lazy=(0,),
                  expect={"shift_waves": 4, "shift_tail_spl": 3}),
    "tail2-8-waves": dict(table="n41", kind="8", cfg={}, ns=125, span=(0, 125), calls="dvm", lazy=(0,),
                          expect={"shift_waves": 8, "shift_tail_spl": 2}),
    "tail3-8-waves": dict(table="n41", kind="8", cfg={}, ns=446, span=(256, 446), calls="dvm", lazy=(1,),
                          expect={"shift_waves": 8, "shift_tail_spl": 3}),
    "rows8": dict(table="n70", kind="rows8", cfg={"shift": 1, "shift_rows_direct": 0}, ns=512, span=(0, 512),
                  calls="d", lazy=(0,), expect={"shift_waves": 8, "shift_row_blocks": 2}),
    "rows2": dict(table="n70", kind="rows2", cfg={"shift_rows_direct": 1}, ns=300, span=(0, 300), calls="dv",
                  lazy=(0, 1), expect={"shift_waves": 8, "shift_row_blocks": 3}),
    "rows4": dict(table="n70", kind="rows4", cfg={"shift_rows_direct": 2}, ns=300, span=(0, 300), calls="dv",
                  lazy=(0, 1), expect={"shift_waves": 4, "shift_row_blocks": 3}),
    "wide": dict(table="w30", kind="wide", cfg={"shift_wide": 1}, ns=768, span=(0, 768), calls="d", lazy=(0, 1),
                 expect={"shift_waves": 8, "shift_wide_tiles": 2, "shift_tail_spl": 0, "shift_wide_row_blocks": 1}),
    "wide-and-tail": dict(table="w30", kind="wide", cfg={"shift_wide": 1}, ns=500, span=(0, 384), calls="d",
                          lazy=(0, 1), expect={"shift_waves": 8, "shift_wide_tiles": 1, "shift_tail_spl": 2}),
    "wide_rows": dict(table="w41", kind="wide_rows", cfg={"shift_wide": 1, "shift_wide_rows": 2}, ns=600,
                      span=(0, 600), calls="d", lazy=(0, 1),
                      expect={"shift_waves": 8, "shift_wide_tiles": 2, "shift_wide_row_blocks": 3}),
    "negative-entries": dict(table="neg29", kind="4", cfg={"shift_waves": 4}, ns=512, span=(0, 512), calls="dv",
                             lazy=(0, 1), expect={"shift_waves": 4}),
    "negative-entries-wide": dict(table="neg29", kind="wide", cfg={"shift_wide": 1}, ns=768, span=(0, 768),
                                  calls="d", lazy=(0, 1), expect={"shift_waves": 8, "shift_wide_tiles": 2}),
}


def _schedule_readouts(eng, kind, narrow, wide, direct):
    """the engine's summary of its schedule against the restatement's integers"""
    if kind in ("wide", "wide_rows"):
        assert eng.get("shift_wide_ok") == 1
        assert eng.get("shift_wide_operands_per_add_x1000") == wide.operands_x1000(), \
            (eng.get("shift_wide_operands_per_add_x1000"), wide.operands_x1000())
        assert eng.get("shift_wide_direct_bricks") == direct
    else:
        assert eng.get("shift_ok") == 1
        assert eng.get("shift_operands_per_add_x1000") == narrow.operands_x1000(), \
            (eng.get("shift_operands_per_add_x1000"), narrow.operands_x1000())
        assert eng.get("shift_wide_bricks") == direct
        assert eng.get("shift_brick_nodes") == int(np.prod(narrow.brick))


def _ran(eng, kind, lazy, expect):
    wide = kind in ("wide", "wide_rows")
    got = {k: eng.get(k) for k in expect}
    assert eng.get("last_kernel") == 3 and eng.get("last_kernel_j") == (6 if wide else 4), \
        (eng.get("last_kernel"), eng.get("last_kernel_j"))
    assert got == expect, (got, expect)
    if lazy is not None:
        assert eng.get("shift_lazy") == lazy


def _witnessed_case(oracle, spec, threads=8):
    """table, layouts, onsets with one event per (node position, top offset) inside the tile kind under test, the
    oracle's volume and series -- after proving ON THE ORACLE that each target node wins its sample"""
    tt = sl.table(spec["table"])
    narrow, wide, direct = sl.case_layouts(spec["table"], spec["kind"])
    L = wide if wide is not None else narrow
    top = L.top_offset()
    assert direct == 0 and int(L.nq.max()) == L.nq_max and top == (sl.TABLES[spec["table"]].m)
    # (both row parities per (node position, offset) wherever the tile kind under test holds 32 events apart)
    few = spec["span"][1] - spec["span"][0] < 100
    targets = sl.witness_targets(L, (top - 1, top), parities=None if few else (0, 1))
    lsmp, ns = int(tt.max()) + 20, spec["ns"]
    onsets, t_k = sl.witness_onsets(tt, targets, FSMP, lsmp, ns, spec["span"][0], spec["span"][1],
                                    seed=sl.TABLES[spec["table"]].seed + ns)
    avail = tt.shape[-1]
    ref = oracle.c_migrate(onsets, tt, FSMP, lsmp, avail, threads=threads)
    want = oracle.c_find_max_coa(ref, threads=2)
    for (node, row, pos, off), t in zip(targets, t_k):
        assert want[2][t] == node, ("the oracle's maximum is not the witness node", node, row, pos, off, t, want[2][t])
    return tt, (narrow, wide, direct), oracle.log_onsets(onsets), lsmp, avail, ref.reshape(-1, ns), want


@pytest.mark.parametrize("name", list(FLAVOURS))
def test_every_loop_flavour_at_the_top_of_its_register_window(lib, oracle, name):
    spec = FLAVOURS[name]
    tt, (narrow, wide, direct), lon, lsmp, avail, flat, want = _witnessed_case(oracle, spec)
    kind, ns, cfg = spec["kind"], spec["ns"], {**spec["cfg"], **_brick_cfg(spec["kind"])}
    old = lib.Engine(0, shift=0, **_brick_cfg(kind))
    old.load_lut(tt)
    round2 = old.detect(lon, FSMP, lsmp, avail)
    assert old.get("last_kernel") != 3
    n_nodes = flat.shape[0]
    for lazy in spec["lazy"]:
        eng = lib.Engine(0, shift_lazy=lazy, **cfg)
        eng.load_lut(tt)
        got = eng.detect(lon, FSMP, lsmp, avail)
        _ran(eng, kind, lazy, spec["expect"])
        _schedule_readouts(eng, kind, narrow, wide, direct)
        _assert_series(got, want)
        assert np.array_equal(got[2], round2[2]) and np.array_equal(got[0], round2[0])     # same bits
        np.testing.assert_allclose(got[1], round2[1], rtol=NORM)
        # a batch of two steps is its steps (the row-block kernels take them one by one: same bits)
        other = np.ascontiguousarray(np.roll(lon, 7, axis=1))
        one = eng.detect(other, FSMP, lsmp, avail)
        two = eng.detect_batch(np.stack([lon, other]), FSMP, lsmp, avail)
        for i in range(3):
            assert np.array_equal(two[i][0], got[i]) and np.array_equal(two[i][1], one[i]), (name, lazy, i)
        narrow_expect = {k: v for k, v in spec["expect"].items() if not k.startswith("shift_wide")}
        if "v" in spec["calls"]:
            vol = np.full((n_nodes, ns), np.nan)
            series = (np.full(ns, np.nan), np.full(ns, np.nan), np.full(ns, -1, dtype=np.int64))
            eng.migrate(lon, FSMP, lsmp, avail, vol, scan_out=series)
            _ran(eng, kind, None, narrow_expect)
            _assert_series(series, want)
            np.testing.assert_allclose(vol, flat, rtol=TIGHT)
            vol2 = np.full((n_nodes, ns), np.nan)
            old.migrate(lon, FSMP, lsmp, avail, vol2)
            assert old.get("last_kernel") != 3 and np.array_equal(vol, vol2)              # every stored value
            assert np.array_equal(series[0], round2[0]) and np.array_equal(series[2], round2[2])
        if "m" in spec["calls"]:
            t_lo, t_hi = spec["span"]
            for i0, i1 in ((0, ns), (t_lo + (t_hi - t_lo) // 4, t_hi - (t_hi - t_lo) // 4), (ns - 1, ns)):
                s2 = (np.full(ns, np.nan), np.full(ns, np.nan), np.full(ns, -1, dtype=np.int64))
                m = eng.marginal_map(lon, FSMP, lsmp, avail, i0, i1, scan_out=s2)
                _ran(eng, kind, None, narrow_expect)
                np.testing.assert_allclose(m.reshape(-1), flat[:, i0:i1].sum(axis=-1), rtol=NORM)
                _assert_series(s2, want)
                assert np.array_equal(s2[0], round2[0]) and np.array_equal(s2[2], round2[2])
        eng.close()
    old.close()


# tie_rule = 1: the fused detect leaves a row of maxima per brick -- stack_shift_bricks_kernel<4> / <8> on 256-sample
# tiles, the wide tiles' own loop flavours (shift_wide_detect_bmax / _bmax_lazy) -- and the refinement picks the
# index by the reference's scalar-exp rule
TIE_CASES = {
    "bricks-4-waves": dict(table="n30", kind="4", cfg={"shift_waves": 4}, ns=512, span=(0, 512), lazy=(0,),
                           expect={"shift_waves": 4}),
    "bricks-8-waves": dict(table="n41", kind="8", cfg={}, ns=512, span=(0, 512), lazy=(0,), expect={"shift_waves": 8}),
    "wide-bmax": dict(table="w30", kind="wide", cfg={"shift_wide": 1}, ns=768, span=(0, 768), lazy=(0, 1),
                      expect={"shift_waves": 8, "shift_wide_tiles": 2}),
}


@pytest.mark.parametrize("name", list(TIE_CASES))
def test_tie_rule_flavours_at_the_top_of_the_register_window(lib, oracle, name):
    spec = TIE_CASES[name]
    tt, (narrow, wide, direct), lon, lsmp, avail, flat, want = _witnessed_case(oracle, spec)
    kind, cfg = spec["kind"], {**spec["cfg"], **_brick_cfg(spec["kind"])}
    rule = oracle.np_argmax_exp_rule(lon, tt, FSMP, lsmp, avail, prelogged=True)
    nbricks = (wide if wide is not None else narrow).nbricks
    for lazy in spec["lazy"]:
        base = lib.Engine(0, shift_lazy=lazy, **cfg)
        base.load_lut(tt)
        a0, b0, c0 = base.detect(lon, FSMP, lsmp, avail)
        base.close()
        eng = lib.Engine(0, tie_rule=1, shift_lazy=lazy, **cfg)
        eng.load_lut(tt)
        a, b, c = eng.detect(lon, FSMP, lsmp, avail)
        _ran(eng, kind, lazy if kind == "wide" else None, spec["expect"])
        assert eng.get("tie_brick_rows") == nbricks, (eng.get("tie_brick_rows"), nbricks)
        assert eng.get("tie_overflow_samples") == 0
        _schedule_readouts(eng, kind, narrow, wide, direct)
        eng.close()
        assert np.array_equal(c, rule), np.flatnonzero(c != rule)[:8]
        assert np.array_equal(a, a0)                                       # the default engine's bits
        np.testing.assert_allclose(b, b0, rtol=1e-13)
        _assert_series((a, b, c0), want)


@pytest.mark.parametrize("name", list(sl.BOUNDARIES))
def test_bricks_exactly_on_and_one_slot_past_the_lds_limit(lib, oracle, name):
    """Four bricks of a fixed shape: run + zero row = plane_bytes / 16 (stays), one slot more (direct kernel), one
    group at seven quads (direct kernel), that group at exactly six (stays) -- the predicted two bricks run on the
    direct kernel beside the shift-reuse loops, the launch's partial sets fold to the oracle's series, and a batch of
    two steps is its steps."""
    from quakemigrate_amd import synth

    spec = sl.BOUNDARIES[name]
    tt, limit = sl.boundary(name)
    narrow, wide, direct = sl.engine_layouts(tt, spec.kind, spec.brick)
    assert direct == 2
    S, ns = spec.rows, 500 if spec.kind == "wide" else 400
    lsmp = int(tt.max()) + 20
    rng = np.random.default_rng(spec.seed)
    flat_tt = tt.reshape(-1, S).astype(np.int64)
    nodes = rng.integers(0, flat_tt.shape[0], size=4)
    arrivals = [FSMP + int(t0) + flat_tt[n] for n, t0 in zip(nodes, (40, 150, 260, ns - 30))]
    onsets = synth.synthetic_onsets(rng, S, FSMP + ns + lsmp, arrivals)
    lon = oracle.log_onsets(onsets)
    want = oracle.detect(onsets, tt, FSMP, lsmp, S, threads=4)
    bricks = dict(brick_x=spec.brick[0], brick_y=spec.brick[1], brick_z=spec.brick[2])
    cfg = {"4": {"shift_waves": 4}, "8": {"shift_waves": 8}, "wide": {"shift_wide": 1}}[spec.kind]
    old = lib.Engine(0, shift=0, **bricks)
    old.load_lut(tt)
    round2 = old.detect(lon, FSMP, lsmp, S)
    assert old.get("last_kernel") != 3
    old.close()
    for lazy in (0, 1):
        eng = lib.Engine(0, shift_lazy=lazy, **cfg, **bricks)
        eng.load_lut(tt)
        got = eng.detect(lon, FSMP, lsmp, S)
        _ran(eng, spec.kind, lazy, {"shift_waves": 8 if spec.kind != "4" else 4,
                                    "shift_wide_tiles": 1 if spec.kind == "wide" else 0})
        _schedule_readouts(eng, spec.kind, narrow, wide, direct)
        _assert_series(got, want)
        assert np.array_equal(got[2], round2[2]) and np.array_equal(got[0], round2[0])
        np.testing.assert_allclose(got[1], round2[1], rtol=NORM)
        other = np.ascontiguousarray(np.roll(lon, 7, axis=1))
        one = eng.detect(other, FSMP, lsmp, S)
        two = eng.detect_batch(np.stack([lon, other]), FSMP, lsmp, S)
        for i in range(3):
            assert np.array_equal(two[i][0], got[i]) and np.array_equal(two[i][1], one[i]), (name, lazy, i)
        eng.close()
