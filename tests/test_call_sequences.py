# -*- coding: utf-8 -*-
"""
One engine for the life of a process: call sequences against fresh engines.

DESIGN.md section 0 and include/qmhip.h promise that the kernel a call runs and the bits it returns depend on the
table, the configuration and the call -- not on what the engine did before.  MigrationScan, the drop-in symbols
and the sharded detectors rely on it: they keep ONE engine whose scratch only grows, whose layouts are built at the
first launch that takes them and parked with their table, and whose record of the last launch later calls read.

* ``test_walk``: a seeded plan (tests/sequence_plan.py; its coverage is checked on the CPU by
  tests/test_sequence_plan.py) drives one long-lived engine of each flavour through loads, selects, every kind of
  launch at scan lengths across every tile boundary, stream changes and pool releases.  Every distinct request is
  also evaluated ONCE on a fresh engine of the flavour (make, load, one call, close), that result is held to the CPU
  oracle at the suite's bounds (the tie_rule = 1 index series to oracle.np_argmax_exp_rule on every sample), and at every step the long-lived engine's outputs -- the three series, every stored
  volume value, the marginal map, the partial sets, the read-outs of the launch and of the brick layout it ran on
  (``LAYOUT_KEYS``) -- must be ``np.array_equal`` to it.
* ``test_walk_with_a_poisoned_pool``: the ``engine`` and ``tie_rule`` walks, shorter, in a child process each with
  ``QM_HIP_POOL_POISON=1`` (every block the device pool hands out starts as 0xFF bytes).
* ``test_tie_partial_after_an_intervening_call`` and ``test_screen_and_tie_rule_exclude_each_other``: the two
  faults the walk's subject had when this file was written (qm_engine_tie_partial trusted launch state that any
  other call overwrites; ``screen = 1`` silently dropped the refinement of ``tie_rule = 1``).

* ``test_group_load_after_a_partial_miss_keeps_every_box_engine_keyed``: what the walk found besides (group_3, seed
  20261016, step 53).  A group's ``select_table`` can still miss where one engine would hit -- its box engines park
  and evict on their own (``run_walk`` says where) --, which costs a rebuild and never a wrong table.

Wall time on one MI355X, one visit: this file 32 s (25 tests; 12 s of it the two poisoned-pool children, mostly
their start-up, 6 s each the first walk, which also builds the tables and the oracle's series the others reuse, and
the tie_rule walk with its rule evaluations) beside 103 s of tests/test_gpu_parity.py (254 tests) on the parent
commit's library.
"""

import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, RTOL, load_golden       # (first: it puts the repository root on sys.path)
import sequence_plan as sp                          # noqa: E402
from test_gpu_parity import NORM, SCREEN_NORM, TIGHT   # noqa: E402

pytestmark = pytest.mark.gpu
MARGINAL = 1e-12                    # marginal maps, as tests/test_group_gpu.py and test_gpu_parity.py hold them
CHUNK_SMALL, CHUNK_WHOLE = 1 << 20, 4 << 30        # "chunk_bytes": several time chunks / one
RULE_CHUNK = 256                    # oracle.np_argmax_exp_rule is evaluated per chunk of this many onset positions
RULE_CACHE_ENV = "QM_SEQUENCE_RULE_CACHE"       # a file of evaluated chunks handed to the poisoned-pool children


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    assert _lib.qmlib.qm_device_count() >= 1, "no HIP device visible"
    return _lib


# ------------------------------------------------------------------------------------------------ inputs, oracle
@functools.lru_cache(maxsize=None)
def _logged(table):
    tt, onsets, fsmp0, t_samples = sp.table_case(table)
    return np.ascontiguousarray(np.log(np.clip(onsets, 0.01, np.inf)))


def _step(table, k):
    """The logged onsets of step k of a detect_batch (k = 0: the table's own)."""
    lon = _logged(table)
    return lon if k == 0 else np.ascontiguousarray(np.roll(lon, sp.BATCH_SHIFT * k, axis=1))


_ORACLE = {}


def _oracle_series(oracle, table, fsmp, ns, k):
    key = ("series", table, fsmp, ns, k)
    if key not in _ORACLE:
        tt, _, _, t_samples = sp.table_case(table)
        _ORACLE[key] = oracle.detect(_step(table, k), tt, fsmp, t_samples - fsmp - ns, tt.shape[-1], threads=8,
                                     prelogged=True)
    return _ORACLE[key]


# tie_rule = 1 is held to oracle.np_argmax_exp_rule on EVERY sample.  That NumPy restatement costs about half a
# second per hundred samples of these tables, so it is evaluated once per table and onset POSITION: a scan sample k
# stacks the onsets at fsmp + k + delay whatever fsmp and the scan length are, so its index is a function of the
# position fsmp + k alone, and step j of a detect_batch (the rows rolled by BATCH_SHIFT * j) reads at position p what
# the table's own onsets hold at p - BATCH_SHIFT * j.  Chunks of RULE_CHUNK positions, evaluated when first needed.
_RULE = {}


def _rule_chunk(oracle, table, c):
    if (table, c) not in _RULE:
        tt, _, _, t_samples = sp.table_case(table)
        lon, lmax = _logged(table), int(tt.max())
        p0, p1 = c * RULE_CHUNK, min((c + 1) * RULE_CHUNK, t_samples - lmax)
        assert p1 > p0, (table, c)
        piece = np.ascontiguousarray(lon[:, p0:p1 + lmax])
        _RULE[(table, c)] = oracle.np_argmax_exp_rule(piece, tt, 0, lmax, tt.shape[-1], prelogged=True)
    return _RULE[(table, c)]


def _oracle_rule(oracle, table, fsmp, ns, k):
    """The reference's arg-max rule on near-ties (what tie_rule = 1 is specified as) for every sample of the scan
    (fsmp, ns) over step k's onsets."""
    tt = sp.table_case(table)[0]
    shift = sp.BATCH_SHIFT * k
    # (no element the roll wrapped round is read: every read lies at or behind fsmp; delays are not negative)
    assert fsmp >= shift and int(tt.min()) >= 0
    p0, p1 = fsmp - shift, fsmp - shift + ns
    pieces = [_rule_chunk(oracle, table, c) for c in range(p0 // RULE_CHUNK, (p1 - 1) // RULE_CHUNK + 1)]
    first = (p0 // RULE_CHUNK) * RULE_CHUNK
    out = np.concatenate(pieces)[p0 - first:p1 - first]
    assert out.size == ns
    return out


def _check_rule_positions(oracle):
    """The position argument above, checked once against direct evaluations: a scan with another pre-pad, and a
    rolled step's."""
    table = "c3_70"
    tt, _, fsmp0, t_samples = sp.table_case(table)
    for fsmp, k, ns in ((fsmp0 + 41, 0, 40), (fsmp0, 3, 40)):
        lsmp = t_samples - fsmp - ns
        direct = oracle.np_argmax_exp_rule(_step(table, k), tt, fsmp, lsmp, tt.shape[-1], prelogged=True)
        assert np.array_equal(direct, _oracle_rule(oracle, table, fsmp, ns, k)), (fsmp, k)


def _save_rule_cache(path):
    np.savez(path, **{f"{t}|{c}": v for (t, c), v in _RULE.items()})


def _load_rule_cache(path):
    with np.load(path) as z:
        for name in z.files:
            t, c = name.split("|")
            _RULE[(t, int(c))] = z[name]


@functools.lru_cache(maxsize=2)
def _oracle_volume_cached(table, fsmp, ns, accumulate=False):
    """The oracle's volume (n_nodes, ns); ``accumulate``: stacked on top of sequence_plan.accumulate_prefill, the
    reference's ``+=`` (migratelib.c:57: the volume's content joins the stack, then the exp)."""
    from oracle import qm_oracle

    tt, _, _, t_samples = sp.table_case(table)
    lsmp = t_samples - fsmp - ns
    if not accumulate:
        return qm_oracle.c_migrate(_logged(table), tt, fsmp, lsmp, tt.shape[-1], threads=8,
                                   prelogged=True).reshape(-1, ns)
    start = sp.accumulate_prefill(tt[..., 0].size, ns)
    return qm_oracle.c_migrate(_logged(table), tt, fsmp, lsmp, tt.shape[-1], threads=8, prelogged=True,
                               initial=start).reshape(-1, ns)


# ------------------------------------------------------------------------------------------------ one request
def _make(lib, flavour):
    cls, arg, cfg, _ = sp.FLAVOURS[flavour]
    return getattr(lib, cls)(arg, **cfg)


def _nan_series(shape):
    return (np.full(shape, np.nan), np.full(shape, np.nan), np.full(shape, -1, dtype=np.int64))


def _get(lib, eng, key):
    try:
        return eng.get(key)
    except lib.QMHipError as e:         # (a group whose box engines ran different kernels says so: that text is
        return str(e)                   # a function of the launch as well)


# The layout the launch ran on, by the stacking kernel's family (last_kernel): brick size and the bricks that do not
# fit it.  Only the family the launch TOOK: a long-lived engine legitimately still holds an older layout in the others.
LAYOUT_KEYS = {
    0: ("n_bricks", "n_wide_bricks"),                                   # round-2 kernels: chunked ...
    1: ("n_bricks", "n_wide_bricks"),                                   # ... and exact-row-count
    2: ("pair_tile", "pair_brick_nodes", "pair_wide_bricks"),           # paired
    3: ("shift_brick_nodes", "shift_wide_bricks"),                      # shift-reuse, 256-sample tiles
    "wide": ("shift_wide_brick_nodes", "shift_wide_direct_bricks"),     # shift-reuse with wide tiles in front
}
SCREEN_LAYOUT_KEYS = ("screen_brick_nodes", "screen_pairs")


def _swept_steps(lib, eng):
    """Detect steps that went through the screening sweep so far, screened or redone in float64."""
    return _get(lib, eng, "screened_steps") + _get(lib, eng, "fallback_steps")


def _run(lib, eng, req):
    """One request on ``eng`` (its table is resident): a dict of everything the call wrote, outputs pre-filled with
    NaN / -1, and the launch's read-outs."""
    out = {}
    sweeps = req.kind in ("detect", "detect_batch", "detect_partial") and _get(lib, eng, "screen") == 1
    swept = _swept_steps(lib, eng) if sweeps else 0
    if req.kind == "find_max_coa":
        series = _nan_series(req.ns)
        eng.find_max_coa(sp.fmc_volume(req.ns), req.ns, sp.FMC_NODES, out=series)
        out["series"] = series
        return out                      # (no stacking launch: the read-outs keep the last one's)
    import torch

    tt, _, _, _ = sp.table_case(req.table)
    lon, rows, n_nodes = _logged(req.table), tt.shape[-1], tt[..., 0].size
    fsmp, lsmp = sp.pads(req)
    ns = req.ns
    if req.kind == "detect":
        out["series"] = eng.detect(lon, fsmp, lsmp, rows, out=_nan_series(ns))
    elif req.kind == "detect_batch":
        steps = np.stack([_step(req.table, k) for k in range(req.args[0])])
        out["series"] = eng.detect_batch(steps, fsmp, lsmp, rows, out=_nan_series((req.args[0], ns)))
    elif req.kind == "detect_partial":
        dev = torch.device("cuda", 0)
        part = (torch.full((ns,), float("nan"), dtype=torch.float64, device=dev),
                torch.full((ns,), -1, dtype=torch.int64, device=dev),
                torch.full((ns,), float("nan"), dtype=torch.float64, device=dev))
        torch.cuda.synchronize()        # (the fills ran on torch's stream, the engine may be on its own)
        eng.detect_partial(lon, fsmp, lsmp, rows, part)
        out["series"] = eng.finalize(part[0], part[1], part[2], 1, ns, n_nodes, out=_nan_series(ns))
        eng.synchronize()
        out["partial"] = tuple(p.cpu().numpy() for p in part)
    elif req.kind == "migrate_host":
        scan, chunked, accumulate = req.args
        eng.config("chunk_bytes", CHUNK_SMALL if chunked else CHUNK_WHOLE)
        vol = sp.accumulate_prefill(n_nodes, ns) if accumulate else np.full((n_nodes, ns), np.nan)
        series = _nan_series(ns) if scan else None
        eng.migrate(lon, fsmp, lsmp, rows, vol, scan_out=series, accumulate=accumulate)
        out["volume"] = vol
        if scan:
            out["series"] = series
    elif req.kind == "migrate_device":
        vol = torch.full((n_nodes, ns), float("nan"), dtype=torch.float64, device=torch.device("cuda", 0))
        series = _nan_series(ns) if req.args[0] else None
        torch.cuda.synchronize()
        eng.migrate(lon, fsmp, lsmp, rows, vol, scan_out=series)
        eng.synchronize()
        out["volume"] = vol.cpu().numpy()
        if series is not None:
            out["series"] = series
    elif req.kind == "marginal_map":
        series = _nan_series(ns)
        out["map"] = eng.marginal_map(lon, fsmp, lsmp, rows, req.args[0], req.args[1],
                                      out=np.full(tt.shape[:3], np.nan), scan_out=series)
        out["series"] = series
    else:
        raise AssertionError(f"unknown kind {req.kind}")
    # Read-outs of THIS launch (include/qmhip.h: they describe the last launch whatever its family -- after one that
    # is not shift-reuse the three shift_* values are 0 on the long-lived engine as on the fresh one).
    # steps_per_launch describes the last detect_batch: it is compared where this call was one.
    keys = ["last_kernel", "last_kernel_j", "tie_brick_rows", "shift_wide_tiles", "shift_tail_spl", "shift_lazy"]
    read = {k: _get(lib, eng, k) for k in keys}
    if req.kind == "detect_batch":
        read["steps_per_launch"] = _get(lib, eng, "steps_per_launch")
    # ... and of the layout it ran on: a table that comes back from parking, or is loaded over another, has the
    # layout a fresh engine builds (a group whose box engines disagree on the family: as before, the text alone)
    family = read["last_kernel"]
    if family == 3 and read["shift_wide_tiles"] != 0:
        family = "wide" if isinstance(read["shift_wide_tiles"], int) else None
    read.update({k: _get(lib, eng, k) for k in LAYOUT_KEYS.get(family, ())})
    if sweeps and _swept_steps(lib, eng) > swept:
        read.update({k: _get(lib, eng, k) for k in SCREEN_LAYOUT_KEYS})
    out["readouts"] = read
    return out


def _check_series(got, want, norm, what):
    a, b, c = got
    ra, rb, rc = want
    if rc is not None:
        assert np.array_equal(c, rc), f"{what}: argmax differs at {np.flatnonzero(c != rc)[:8]}"
    np.testing.assert_allclose(a, ra, rtol=RTOL, err_msg=what)
    np.testing.assert_allclose(b, rb, rtol=RTOL, err_msg=what)
    np.testing.assert_allclose(a, ra, rtol=TIGHT, err_msg=what)
    np.testing.assert_allclose(b, rb, rtol=max(TIGHT, norm), err_msg=what)


def _check_against_oracle(oracle, flavour, req, out):
    """The fresh engine's result of a request against the CPU oracle, at the suite's bounds."""
    what = f"fresh {flavour} engine, {req}"
    group = sp.is_group(flavour)
    for name, arrays in out.items():
        if name != "readouts":
            for x in (arrays if isinstance(arrays, tuple) else (arrays,)):
                assert not np.isnan(x).any() and not (x.dtype == np.int64 and (x < 0).any()), \
                    f"{what}: {name} holds elements nobody wrote"
    if req.kind == "find_max_coa":
        want = oracle.c_find_max_coa(sp.fmc_volume(req.ns), threads=4)
        a, b, c = out["series"]
        assert np.array_equal(c, want[2]) and np.array_equal(a, want[0]), what
        np.testing.assert_allclose(b, want[1], rtol=NORM if group else TIGHT, err_msg=what)
        return
    fsmp, _ = sp.pads(req)
    ns = req.ns
    screened = flavour == "screen" and req.kind in ("detect", "detect_batch", "detect_partial")
    norm = SCREEN_NORM if screened else NORM
    # tie_rule = 1 refines every FINAL series (not the partial sets a finalize folds): the index series is the
    # reference's rule's, the values are unchanged
    ruled = flavour == "tie_rule" and req.kind != "detect_partial"
    if "series" in out:
        steps = req.args[0] if req.kind == "detect_batch" else 1
        for k in range(steps):
            got = out["series"] if req.kind != "detect_batch" else tuple(s[k] for s in out["series"])
            wa, wb, wc = _oracle_series(oracle, req.table, fsmp, ns, k)
            _check_series(got, (wa, wb, None if ruled else wc), norm, f"{what}, step {k}")
            if ruled:
                rule = _oracle_rule(oracle, req.table, fsmp, ns, k)
                assert np.array_equal(got[2], rule), \
                    f"{what}, step {k}: tie_rule index differs at samples {np.flatnonzero(got[2] != rule)[:8]}"
    if "volume" in out or "map" in out:
        ref = _oracle_volume_cached(req.table, fsmp, ns, req.kind == "migrate_host" and req.args[2])
        if "map" in out:
            want = ref[:, req.args[0]:req.args[1]].sum(axis=1).reshape(out["map"].shape)
            np.testing.assert_allclose(out["map"], want, rtol=MARGINAL, err_msg=what)
        else:
            np.testing.assert_allclose(out["volume"], ref, rtol=TIGHT, err_msg=what)


def _same(got, fresh, what):
    """Bit equality of everything a call wrote, and of its read-outs."""
    assert set(got) == set(fresh), what
    for name in got:
        if name == "readouts":
            assert got[name] == fresh[name], f"{what}: read-outs {got[name]} on the long-lived engine, " \
                                             f"{fresh[name]} on a fresh one"
            continue
        g = got[name] if isinstance(got[name], tuple) else (got[name],)
        f = fresh[name] if isinstance(fresh[name], tuple) else (fresh[name],)
        for i, (x, y) in enumerate(zip(g, f)):
            if not np.array_equal(x, y):
                bad = np.flatnonzero(np.asarray(x != y).reshape(-1))
                rel = np.max(np.abs((x - y).reshape(-1)[bad] / np.where(y.reshape(-1)[bad] == 0, 1,
                                                                          y.reshape(-1)[bad])))
                raise AssertionError(f"{what}: {name}[{i}] differs from the fresh engine's in {len(bad)} of {x.size} "
                                     f"elements (first at {bad[:6]}, largest relative difference {rel:.3g})")


# family of the stacking kernel a roster table reaches on a FRESH engine of the plain flavour, after a detect of its
# longest scan: (last_kernel, shift_waves, shift_row_blocks) -- a roster entry must not stop covering its family
FAMILIES = {
    "c3_30": (3, 4, 1),                 # shift-reuse, two 4-wave workgroups per CU
    "c3_44": (3, 8, 1),                 # shift-reuse, one 8-wave workgroup per CU
    "c3_70": (3, 8, 3),                 # shift-reuse on row blocks (70 rows: three blocks)
    "c2_11": None,                      # (no shift-reuse layout: _check_family)
    "c3_30m": (3, 4, 1),
}


_FAMILIES_CHECKED = []


def _check_families(lib):
    """Once per process: every roster table reaches its family on a fresh plain engine, and the 384-sample wide
    tiles are reached on a fresh ``shift_wide = 1`` engine (these grids are too small for the automatic choice)."""
    if _FAMILIES_CHECKED:
        return
    for table in sp.TABLES:
        tt = sp.table_case(table)[0]
        longest = [r for r in sp.roster(table)["detect"] if r.ns == sp.TABLES[table].lengths[-1]][0]
        eng = lib.Engine(0)
        eng.load_lut(tt)
        _run(lib, eng, longest)
        family = (eng.get("last_kernel"), eng.get("shift_waves"), eng.get("shift_row_blocks"))
        assert eng.get("shift_wide_tiles") == 0, table
        volume_kernel = None
        if table == "c2_11":            # a device volume of 401 samples: whole tiles of the table's own length
            _run(lib, eng, sp.roster(table)["migrate_device"][2])
            volume_kernel = eng.get("last_kernel")
        eng.close()
        if table == "c2_11":
            # incoherent: no shift-reuse layout -- the fused detect on the exact-row-count kernel (1), the volume on
            # the paired one (2)
            assert (family[0], volume_kernel) == (1, 2), (table, family, volume_kernel)
            continue
        assert family == FAMILIES[table], (table, family)
        # wide tiles: at least ns // 384 of them from 384 samples on (what is left behind them runs as a tail tile,
        # a pulled-back 256-sample tile or one more wide tile), none below
        wide = lib.Engine(0, shift_wide=1)
        wide.load_lut(tt)
        for req in sp.roster(table)["detect"]:
            _run(lib, wide, req)
            got = wide.get("shift_wide_tiles") if wide.get("last_kernel") == 3 else 0
            if req.ns < 384:
                assert got == 0, (table, req.ns, got)
            else:
                assert got >= req.ns // 384 and (wide.get("last_kernel"), wide.get("last_kernel_j")) == (3, 6), \
                    (table, req.ns, got, wide.get("last_kernel_j"))
        wide.close()
    _FAMILIES_CHECKED.append(True)


# ------------------------------------------------------------------------------------------------ the walk
def run_walk(lib, oracle, flavour, seed=None, steps=None):
    seed = sp.SEEDS[flavour] if seed is None else seed
    plan = sp.make_plan(flavour, seed, steps)
    _check_families(lib)
    if flavour == "tie_rule" and not _RULE:
        _check_rule_positions(oracle)
    import torch

    memo = {}
    side = torch.cuda.Stream()

    def fresh(req):
        if req not in memo:
            e2 = _make(lib, flavour)
            try:
                if req.table:
                    e2.load_lut(sp.table_case(req.table)[0])
                memo[req] = _run(lib, e2, req)
            finally:
                e2.close()
            _check_against_oracle(oracle, flavour, req, memo[req])
        return memo[req]

    eng = _make(lib, flavour)
    came_back = 0
    try:
        for i, op in enumerate(plan):
            try:
                if op.op == "load":
                    eng.load_lut(sp.table_case(op.table)[0])
                elif op.op == "select":
                    resident = eng.select_table(op.table, capacity=op.arg)
                    came_back += bool(resident and op.expect)
                    if sp.is_group(flavour) and op.expect and not resident:
                        # A group's box engines park and evict on their own, and a box engine that exists for only
                        # some of the grids' shapes has parked fewer tables than the model's engine, so a cache of
                        # one can drop the very table the others kept (seed 20261016, group_3, step 48: the third
                        # box of the 20 x 21 x 22 grid).  The group then says "not resident" and the caller loads:
                        # a rebuild the single engine would not need, never a wrong table.  The reverse -- resident
                        # where the model has lost the table -- stays an error.
                        eng.load_lut(sp.table_case(op.table)[0])
                    else:
                        assert resident == op.expect, f"select_table says resident={resident}, the model {op.expect}"
                elif op.op == "set_stream":
                    eng.synchronize()
                    eng.set_stream(side.cuda_stream if op.arg == "torch" else None)
                elif op.op == "release":
                    lib.release_cached_memory()
                else:
                    want = fresh(op.arg)
                    _same(_run(lib, eng, op.arg), want, f"{op.arg}")
            except Exception as e:
                raise AssertionError(f"flavour {flavour}, seed {seed}, step {i} of {len(plan)}: {e}\n"
                                     f"operations up to it:\n{sp.format_ops(plan[:i + 1])}") from e
    finally:
        eng.close()
    # (a group may miss where the model hits, see above -- but tables do come back from parking on it as well)
    hits = sum(1 for op in plan if op.op == "select" and op.expect)
    assert hits == 0 or came_back >= 1, (came_back, hits)
    return len(plan), len(memo)


@pytest.mark.parametrize("flavour", list(sp.FLAVOURS))
def test_walk(lib, oracle, flavour):
    """A long-lived engine's outputs equal a fresh engine's, bit for bit, at every step of the flavour's plan."""
    t0 = time.time()
    steps, requests = run_walk(lib, oracle, flavour)
    print(f"\nwalk {flavour}: {steps} steps, {requests} distinct requests, {time.time() - t0:.1f} s")


def test_walk_with_a_poisoned_pool(lib, tmp_path):
    """The engine and tie_rule walks once more, shorter, with QM_HIP_POOL_POISON=1 (read once per process: a child
    each, one at a time, under a time limit; the second only if the first passed)."""
    env = dict(os.environ, QM_HIP_POOL_POISON="1")
    if _RULE:                           # (the rule's chunks this process evaluated: the same values, not twice)
        cache = tmp_path / "rule_chunks.npz"
        _save_rule_cache(cache)
        env[RULE_CACHE_ENV] = str(cache)
    for flavour in ("engine", "tie_rule"):
        done = subprocess.run([sys.executable, os.path.abspath(__file__), flavour, str(sp.POISON_STEPS)], env=env,
                              cwd=str(ROOT), timeout=600, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert done.returncode == 0, f"poisoned-pool walk {flavour}: exit {done.returncode}\n{done.stdout[-6000:]}"
        assert f"walk {flavour} ok" in done.stdout, done.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ pinned faults
def _near_tie_halves(lib, oracle, **cfg):
    """near_ties_bricks cut at its mirror plane into two tie_rule = 1 engines (a node and its mirror image live on
    different engines), and what the protocol needs."""
    import torch

    g = load_golden("near_ties_bricks")
    tt, fsmp, lsmp, avail = g["traveltimes"], int(g["fsmp"]), int(g["lsmp"]), int(g["available"])
    nx, ny, nz = tt.shape[:3]
    lon = np.ascontiguousarray(oracle.log_onsets(g["onsets"]))
    ns = lon.shape[1] - fsmp - lsmp
    half = nx // 2
    engines, tables = [], []
    for x0, x1 in ((0, half), (half, nx)):
        eng = lib.Engine(0, tie_rule=1, **cfg)
        tables.append((np.ascontiguousarray(tt[x0:x1]), x0 * ny * nz))
        eng.load_lut(tables[-1][0], node_offset=tables[-1][1])
        engines.append(eng)
    return dict(g=g, lon=lon, fsmp=fsmp, lsmp=lsmp, avail=avail, ns=ns, n_total=nx * ny * nz, engines=engines,
                tables=tables, dev=torch.device("cuda", 0))


def _sharded_tie_detect(h, between=None):
    """detect_partial into packed[r] -> finalize_packed -> tie_partial into tie_packed[r] -> tie_fold, the exchange
    emulated by torch.stack; ``between(engine 0)`` runs after engine 0's detect_partial, before its tie_partial.
    Returns the index series, or the QMHipError engine 0's tie_partial raised."""
    import torch

    from quakemigrate_amd.core.lib import QMHipError

    ns, dev = h["ns"], h["dev"]
    packed = [torch.full((3, ns), float("nan"), dtype=torch.float64, device=dev) for _ in h["engines"]]
    torch.cuda.synchronize()
    for r, eng in enumerate(h["engines"]):
        p = packed[r]
        eng.detect_partial(h["lon"], h["fsmp"], h["lsmp"], h["avail"], (p[0], p[1].view(torch.int64), p[2]))
        eng.synchronize()
    gathered = torch.stack(packed).contiguous()
    out = (torch.full((ns,), float("nan"), dtype=torch.float64, device=dev),
           torch.full((ns,), float("nan"), dtype=torch.float64, device=dev),
           torch.full((ns,), -1, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    fold = h["engines"][1]
    fold.finalize_packed(gathered, 2, ns, h["n_total"], out=out)
    fold.synchronize()
    if between is not None:
        between(h["engines"][0])
        h["engines"][0].synchronize()
    ties = [torch.zeros((2, ns), dtype=torch.float64, device=dev) for _ in h["engines"]]
    torch.cuda.synchronize()
    for r, eng in enumerate(h["engines"]):
        try:
            eng.tie_partial(h["lon"], h["fsmp"], h["lsmp"], h["avail"], gathered, 2, ties[r])
        except QMHipError as e:
            assert r == 0, "the engine nobody disturbed refused"
            return e
        eng.synchronize()
    fold.tie_fold(torch.stack(ties).contiguous(), 2, ns, out[2])
    fold.synchronize()
    return out[2].cpu().numpy()


def _interleavings(h):
    """name -> what runs on engine 0 between its detect_partial and its tie_partial, all at the same ns."""
    import torch

    lon, fsmp, lsmp, avail, ns = h["lon"], h["fsmp"], h["lsmp"], h["avail"], h["ns"]
    tt0, off0 = h["tables"][0]
    n_nodes = tt0[..., 0].size
    rolled = np.ascontiguousarray(np.roll(lon, 7, axis=1))

    # (the calls in between stack OTHER onsets, the rows rolled by seven samples: the sets they leave are not the
    # step's)
    def marginal(e):
        e.marginal_map(rolled, fsmp, lsmp, avail, 0, ns, scan_out=_nan_series(ns))

    def migrate_device(e):
        vol = torch.zeros((n_nodes, ns), dtype=torch.float64, device=h["dev"])
        torch.cuda.synchronize()
        e.migrate(rolled, fsmp, lsmp, avail, vol, scan_out=_nan_series(ns))

    def migrate_host_chunks(e):
        e.config("chunk_bytes", CHUNK_SMALL)
        e.migrate(rolled, fsmp, lsmp, avail, np.zeros((n_nodes, ns)), scan_out=_nan_series(ns))
        e.config("chunk_bytes", CHUNK_WHOLE)

    def detect_batch(e):
        e.detect_batch(np.stack([rolled, lon]), fsmp, lsmp, avail)

    def detect_rolled(e):
        e.detect(rolled, fsmp, lsmp, avail)

    def find_max_coa(e):                # (a volume of small values: its sets replace the first sixteen in d_pmax)
        e.find_max_coa(np.ascontiguousarray(np.random.default_rng(3).uniform(1e-9, 1e-6, size=(4096, ns))), ns, 4096)

    def load_other_table(e):            # another table of the same shape (the half mirrored in y)
        e.load_lut(np.ascontiguousarray(tt0[:, ::-1]), node_offset=off0)
        e.load_lut(tt0, node_offset=off0)

    def select_away_and_back(e):
        assert e.select_table("spare", capacity=4) is False
        e.load_lut(np.ascontiguousarray(tt0[:, ::-1]), node_offset=off0)
        assert e.select_table("half", capacity=4) is True

    return [("marginal_map", marginal), ("migrate_device_scan_out", migrate_device),
            ("migrate_host_chunks", migrate_host_chunks), ("detect_batch_2", detect_batch),
            ("detect_rolled", detect_rolled), ("find_max_coa_same_ns", find_max_coa),
            ("load_lut_same_shape", load_other_table), ("select_table_away_and_back", select_away_and_back)]


INTERLEAVINGS = ["marginal_map", "migrate_device_scan_out", "migrate_host_chunks", "detect_batch_2", "detect_rolled",
                 "find_max_coa_same_ns", "load_lut_same_shape", "select_table_away_and_back"]


@pytest.mark.parametrize("cfg", [{}, {"tie_sets": 0}], ids=["brick-rows", "sets-of-bricks"])
@pytest.mark.parametrize("name", INTERLEAVINGS)
def test_tie_partial_after_an_intervening_call(lib, oracle, name, cfg):
    """qm_engine_tie_partial refines the sets its engine's LAST detect_partial left in the engine's scratch.  A call
    in between overwrites them (every stacking launch, find_max_coa) or re-describes them (the last launch's record,
    another table): the only acceptable outcomes are a QMHipError that asks for detect_partial first, or the
    correct index series -- never another one -- and after a refusal the engine works as before.  Both forms of
    the refinement: from the rows of maxima per brick (d_bmax), and from the workgroups' sets (``tie_sets = 0``:
    d_pmax itself, which a volume scan overwrites)."""
    h = _near_tie_halves(lib, oracle, **cfg)
    try:
        h["engines"][0].select_table("half", capacity=4)          # (engine 0's table has a key: it can be parked)
        h["engines"][0].load_lut(*h["tables"][0][:1], node_offset=h["tables"][0][1])
        idx_scalar = h["g"]["idx_scalar"]
        base = _sharded_tie_detect(h)
        assert isinstance(base, np.ndarray) and np.array_equal(base, idx_scalar), "the undisturbed protocol"
        between = dict(_interleavings(h))[name]
        got = _sharded_tie_detect(h, between)
        if isinstance(got, Exception):
            assert "detect_partial" in str(got), str(got)
        else:
            wrong = np.flatnonzero(got != idx_scalar)
            assert wrong.size == 0, (f"tie_partial after {name}: a different index series, {wrong.size} of "
                                     f"{got.size} samples (first {wrong[:6]})")
        again = _sharded_tie_detect(h)
        assert isinstance(again, np.ndarray) and np.array_equal(again, idx_scalar), f"the engine after {name}"
    finally:
        for e in h["engines"]:
            e.close()


def test_screen_and_tie_rule_exclude_each_other(lib, oracle):
    """``screen = 1`` with ``tie_rule = 1`` (include/qmhip.h, the tie_rule row): the screened detect has no near-tie
    refinement, so every detect call of such an engine is REFUSED with an error that names the two keys -- it used
    to return the default rule's indices in silence --, nothing is counted as refined, and the engine's volume
    launches (which never screen) keep refining."""
    g = load_golden("near_ties_bricks")
    tt, fsmp, lsmp, avail = g["traveltimes"], int(g["fsmp"]), int(g["lsmp"]), int(g["available"])
    lon = np.ascontiguousarray(oracle.log_onsets(g["onsets"]))
    ns = lon.shape[1] - fsmp - lsmp
    eng = lib.Engine(0, screen=1, tie_rule=1)
    eng.load_lut(tt)
    import torch

    part = (torch.zeros(ns, dtype=torch.float64, device="cuda"), torch.zeros(ns, dtype=torch.int64, device="cuda"),
            torch.zeros(ns, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    for call in (lambda: eng.detect(lon, fsmp, lsmp, avail),
                 lambda: eng.detect_batch(np.stack([lon, lon]), fsmp, lsmp, avail),
                 lambda: eng.detect_partial(lon, fsmp, lsmp, avail, part)):
        with pytest.raises(lib.QMHipError) as err:
            call()
        assert "screen" in str(err.value) and "tie_rule" in str(err.value), str(err.value)
    assert eng.get("tie_refined_steps") == 0
    series = _nan_series(ns)
    eng.marginal_map(lon, fsmp, lsmp, avail, 0, ns, scan_out=series)
    assert np.array_equal(series[2], g["idx_scalar"]) and eng.get("tie_refined_steps") == 1
    # either key alone keeps its meaning
    eng.config("screen", 0)
    a, b, c = eng.detect(lon, fsmp, lsmp, avail)
    assert np.array_equal(c, g["idx_scalar"]) and eng.get("tie_refined_steps") == 2
    eng.config("screen", 1)
    eng.config("tie_rule", 0)
    a1, b1, c1 = eng.detect(lon, fsmp, lsmp, avail)
    assert np.array_equal(a1, a) and eng.get("tie_refined_steps") == 2 and eng.get("screened_steps") >= 1
    assert 0.03 < np.mean(c1 != g["idx_scalar"]) < 0.2          # (the default rule is the other one)
    eng.close()


def test_group_load_after_a_partial_miss_keeps_every_box_engine_keyed(lib, oracle):
    """Found by the group_3 walk (seed 20261016, step 53).  Three parts cut the 16 x 16 x 12 grid into 2 + 3 + 2 boxes
    and the other two grids into one box each, so the second and third box engines see only the first table.  A
    cache of one then evicts that table on the first box engines while the others keep it parked: the group's
    select misses, and its load used to land ON TOP of the table those engines had just brought back -- a foreign
    load, which took their key away (qm_engine_load_lut), so they never parked the table again and the group
    rebuilt it at every later select whatever the capacity."""
    x, y, z = (sp.table_case(t)[0] for t in ("c3_70", "c3_30", "c2_11"))
    assert [len(lib.group_plan(*x.shape[:3], 3, p)) for p in range(3)] == [2, 3, 2]
    assert [len(lib.group_plan(*y.shape[:3], 3, p)) for p in range(3)] == [1, 1, 1]
    assert [len(lib.group_plan(*z.shape[:3], 3, p)) for p in range(3)] == [1, 1, 1]
    g = lib.EngineGroup([0, 0, 0])
    try:
        for key, tt, cap in (("x", x, 1), ("y", y, 1), ("z", z, 1), ("x", x, 1), ("y", y, 4)):
            assert g.select_table(key, capacity=cap) is False, key
            g.load_lut(tt)
        assert g.select_table("x", capacity=4) is True        # parked by EVERY box engine, the cache has room
        req = sp.roster("c3_70")["detect"][2]
        got = _run(lib, g, req)
        fresh = lib.EngineGroup([0, 0, 0])
        fresh.load_lut(x)
        want = _run(lib, fresh, req)
        fresh.close()
        _check_against_oracle(oracle, "group_3", req, want)
        _same(got, want, "the table that came back")
    finally:
        g.close()


if __name__ == "__main__":              # the poisoned-pool child: one walk, exit status 0 only if it held
    from quakemigrate_amd.core import lib as _lib
    from oracle import qm_oracle as _oracle

    _flavour, _steps = sys.argv[1], int(sys.argv[2])
    assert os.environ.get("QM_HIP_POOL_POISON") == "1"
    if os.environ.get(RULE_CACHE_ENV):
        _load_rule_cache(os.environ[RULE_CACHE_ENV])
    _n, _m = run_walk(_lib, _oracle, _flavour, steps=_steps)
    print(f"walk {_flavour} ok: {_n} steps, {_m} distinct requests")
