# -*- coding: utf-8 -*-
"""
The engine's read-outs (``qm_engine_get``, csrc/qm_engine.hip) and the two per-stage clocks behind the
``trigger_ns_<stage>`` and ``scanmseed_ns_<stage>`` keys, pinned as the library answered them BEFORE the read-outs
became a table and the two clocks one ``StageClock`` (csrc/qm_engine.hpp).

``KEYS`` is every key the former ``else if`` chain answered, copied from it, the tunables of ``config_get`` behind
them.  tests/golden/readouts_parent.json holds their values on the small mixed table of
tools/record_stack_launches.py after ``load_lut`` and one ``detect``; this file wrote it from that commit's library
(``QM_HIP_LIB=/path/to/libqmhip.so python tests/test_readouts_gpu.py tests/golden/readouts_parent.json COMMIT``), and
the file names the keys it leaves out: what follows the machine or the clock.

The clocks: which stages report a time and which report 0 is what a call ran; the times themselves are not compared.
"""

import json
import sys

import numpy as np
import pytest

from conftest import ROOT                          # (first: it puts the repository root on sys.path)

sys.path.insert(0, str(ROOT / "tools"))
import record_stack_launches as rec                 # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN_PATH = ROOT / "tests" / "golden" / "readouts_parent.json"

TRIGGER_STAGES = ("smooth", "stats", "runs", "compact", "peaks", "merge")
SCANMSEED_STAGES = ("quantise", "scan", "compose", "pack", "frame", "decode")
TRIGGER_NS = tuple(f"trigger_ns_{s}" for s in TRIGGER_STAGES)
SCANMSEED_NS = tuple(f"scanmseed_ns_{s}" for s in SCANMSEED_STAGES)
# the chain, top to bottom
READOUTS = (
    "brick_x", "brick_y", "brick_z", "samples_per_lane", "waves", "lds_bytes", "screened_steps", "fallback_steps",
    "last_candidates", "screen_pairs", "screen_big", "screen_brick_nodes", "last_kernel", "last_kernel_j", "shift_ok",
    "shift_waves", "shift_lazy", "shift_tail_spl", "shift_wide_ok", "shift_wide_row_blocks", "shift_wide_tiles",
    "shift_wide_brick_nodes", "shift_wide_direct_bricks", "shift_wide_operands_per_add_x1000", "steps_per_launch",
    "pick_lds_samples", "amp_lds_samples", "trigger_max_radius") + TRIGGER_NS + (
    "trigger_smooth_tile", "trigger_run_block", "trigger_merge_stride", "scanmseed_tile",
    "scanmseed_compose_chunk") + SCANMSEED_NS + (
    "tie_brick_rows", "tie_refined_steps", "tie_overflow_samples", "tie_pairs", "table_hits", "table_misses",
    "table_evictions", "table_digests", "tables_parked", "table_bytes", "tables_parked_bytes", "pool_live_bytes",
    "shift_row_blocks", "shift_brick_nodes", "shift_wide_bricks", "shift_operands_per_add_x1000", "pair_brick_nodes",
    "pair_wide_bricks", "pair_tile", "n_bricks", "n_wide_bricks", "mean_span", "n_cu", "n_nodes", "n_rows", "nx", "ny",
    "nz")
# ... and what falls through to config_get: the tunables (csrc/qm_config.hip)
TUNABLES = (
    "groups", "rounds", "force_direct", "generic", "exact", "scan_waves", "chunk_bytes", "pair", "screen",
    "screen_brick16", "shift", "shift_tail", "shift_rows_direct", "shift_wide", "shift_wide_rows", "stream_pull",
    "stream_stamps", "preproc_skew", "tie_rule", "tie_sets", "trigger_timing", "log_timing")
KEYS = READOUTS + TUNABLES
# What the golden file leaves out.  The machine: the CU count, the process's pool, and shift_lazy -- the detect loop's
# flavour follows the launch's group count, which follows the CU count.  The clock: every stage time.
LEFT_OUT = ("n_cu", "pool_live_bytes", "shift_lazy") + TRIGGER_NS + SCANMSEED_NS

PERIOD, MW, MEI = 20_000_000, 10 ** 9, 2 * 10 ** 9
WEIGHTS = np.array([0.05, 0.25, 0.4, 0.25, 0.05])


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    assert _lib.qmlib.qm_device_count() >= 1, "no HIP device visible"
    return _lib


@pytest.fixture()
def engine(lib):
    eng = lib.Engine(0)
    yield eng
    eng.close()


def answers(eng):
    return {k: eng.get(k) for k in KEYS}


def after_one_detect(lib):
    """Every key on the mixed table, after load_lut and one detect."""
    c = rec.case_of(rec.MIXED)
    eng = lib.Engine(0, **rec._engine_cfg(rec.MIXED))
    try:
        eng.load_lut(c.tt)
        ns = 401
        eng.detect(c.lon, c.fsmp0, c.t_samples - c.fsmp0 - ns, c.tt.shape[-1])
        return answers(eng)
    finally:
        eng.close()


def test_every_name_answers_on_a_fresh_engine_and_an_unknown_one_is_refused(lib, engine):
    got = answers(engine)
    assert list(got) == list(KEYS) and all(isinstance(v, int) for v in got.values())
    with pytest.raises(lib.QMHipError) as refusal:
        engine.get("no_such_key")
    assert str(refusal.value) == "unknown key 'no_such_key'"


def test_values_after_a_detect_are_the_parents(lib):
    golden = json.loads(GOLDEN_PATH.read_text())
    assert golden["left_out"] == list(LEFT_OUT)
    got = after_one_detect(lib)
    assert list(got) == list(KEYS)
    assert {k: v for k, v in got.items() if k not in LEFT_OUT} == golden["values"]
    assert set(golden["values"]) | set(LEFT_OUT) == set(KEYS)


def one_peak(height):
    x = np.full(4096, 1.0)
    x[2000:2010] = height
    x[2005] = height + 1.0
    return x


def trigger(eng, x):
    return eng.trigger_series(x, x.copy(), PERIOD, MW, MEI, method="static", value=2.0, weights=WEIGHTS)


def test_trigger_clock(engine):
    times = lambda: [engine.get(k) for k in TRIGGER_NS]             # noqa: E731
    smooth, stats, runs, compact, peaks, merge = range(6)
    engine.config("trigger_timing", 1)
    assert trigger(engine, one_peak(9.0))["n_events"] == 1
    t = times()
    print("trigger_timing = 1, one peak:", t)
    assert all(t[k] > 0 for k in (smooth, runs, compact, peaks, merge)) and t[stats] == 0
    # a series that stays under the threshold: no candidates, the three stages behind the count did not run
    assert trigger(engine, one_peak(1.2))["n_candidates"] == 0
    t = times()
    print("trigger_timing = 1, under the threshold:", t)
    assert t[smooth] > 0 and t[runs] > 0 and t[stats] == 0
    assert (t[compact], t[peaks], t[merge]) == (0, 0, 0)
    engine.config("trigger_timing", 0)
    assert trigger(engine, one_peak(9.0))["n_events"] == 1
    assert times() == [0] * 6


def test_scanmseed_clock(lib, engine):
    times = lambda: [engine.get(k) for k in SCANMSEED_NS]           # noqa: E731
    quantise, scan, compose, pack, frame, decode = range(6)
    rng = np.random.default_rng(5)
    ints = np.cumsum(rng.integers(-200, 201, (5, 3000)), axis=1).astype(np.int32)
    enc = engine.scanmseed_encode(ints)
    t = times()
    print("int32 encode:", t)
    assert t[quantise] == 0 and t[decode] == 0 and all(t[k] > 0 for k in (scan, compose, pack, frame))
    engine.scanmseed_encode(ints.astype(np.float64) / 8.0, factors=np.full(5, 8.0))
    t = times()
    print("float64 encode:", t)
    assert t[quantise] > 0 and t[decode] == 0 and all(t[k] > 0 for k in (scan, compose, pack, frame))
    offsets = np.concatenate([[0], np.cumsum(enc["rec_count"])[:-1]])
    out, _ = engine.scanmseed_decode(enc["records"], enc["rec_count"], offsets, 5 * 3000)
    assert np.array_equal(out.reshape(5, 3000), ints)
    t = times()
    print("decode:", t)
    assert t[decode] > 0 and t[:decode] == [0] * 5
    # a refused encode leaves the times of the call before
    before = times()
    bad = ints.copy()
    bad[2, 1500:] += 1 << 30
    with pytest.raises(lib.QMHipError, match="does not fit 30 bits"):
        engine.scanmseed_encode(bad)
    assert times() == before


if __name__ == "__main__":
    from quakemigrate_amd.core import lib as _lib

    values = after_one_detect(_lib)
    record = {"commit": sys.argv[2] if len(sys.argv) > 2 else None,
              "case": "tools/record_stack_launches.py: the mixed table, load_lut and one detect of 401 samples",
              "left_out": list(LEFT_OUT),
              "values": {k: v for k, v in values.items() if k not in LEFT_OUT}}
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(record, indent=1) + "\n")
    print(f"{len(record['values'])} read-outs recorded in {sys.argv[1]}")
