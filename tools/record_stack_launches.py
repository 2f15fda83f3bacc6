# -*- coding: utf-8 -*-
"""
What every stacking launch of a fixed matrix decides and returns, as a JSON record.

``python tools/record_stack_launches.py [--last-launch-rule] OUT.json [COMMIT]`` walks the matrix on the library
the package loads (another build: ``QM_HIP_LIB=/path/to/libqmhip.so``) and writes the record; tests/test_stack_plan_gpu.py replays the matrix
and compares with tests/golden/stack_launches_parent.json, which this script wrote from the commit before the
launch plan became one record (``StackPlan``, csrc/qm_engine.hpp).  The Python binding and the C ABI are the same on
both sides, so one script drives both libraries.

The matrix: the five roster tables of tests/sequence_plan.py with their whole ``roster()`` under fourteen
configurations, a fresh engine per (table, configuration); one table whose incoherent corner sends some bricks to the
direct kernel beside the shift-reuse one; one three-part ``EngineGroup`` pass.  Per (table, configuration, kind) the
record holds the read-outs after every request and ONE digest -- SHA-256, 16 hex digits -- over the bytes of
everything the kind's requests wrote (the three series, the volume or the map).  Group counts have no read-out: they
fix the order of the sum over the nodes, so the bits of ``max_norm_coa`` pin them.  They follow the CU count, which
the record names.  A call the engine refuses is recorded by its refusal.

``--last-launch-rule`` is for a library from BEFORE that record only (the golden file was written with it): such a
library kept ``shift_lazy`` / ``shift_tail_spl`` / ``shift_wide_tiles`` from an earlier shift-reuse launch through
launches of the other families, where a fresh engine reports 0 (include/qmhip.h: the read-outs describe the LAST
launch), and the option stores the fresh engine's 0 there.  Without it -- the default, and what the replay does --
every read-out is stored as the library gives it.  The rule's other half, ``last_kernel`` = 0 after a launch of the
direct kernel alone, needs no such help here: of direct-only launches the matrix holds the ``force_direct`` engines,
whose every launch is one; a direct-only launch behind an LDS one is tests/test_call_sequences.py's to compare.
"""

import collections
import hashlib
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import sequence_plan as sp                                          # noqa: E402
from quakemigrate_amd import synth                                  # noqa: E402

READOUTS = ("last_kernel", "last_kernel_j", "shift_waves", "shift_lazy", "shift_tail_spl", "shift_wide_tiles",
            "tie_brick_rows")
SHIFT_ONLY = ("shift_lazy", "shift_tail_spl", "shift_wide_tiles")
CONFIGS = ({}, {"tie_rule": 1}, {"tie_rule": 1, "tie_sets": 0}, {"shift_wide": 1}, {"shift_wide": 1, "tie_rule": 1},
           {"shift": 0}, {"shift_lazy": 0}, {"shift_lazy": 1, "groups": 7}, {"shift_waves": 8}, {"force_direct": 1},
           {"pair": 2}, {"exact": 0}, {"generic": 1}, {"samples_per_lane": 2})
MIXED_CONFIGS = ({}, {"tie_rule": 1})
MIXED = "mixed"                     # the table with an incoherent corner: LDS and direct launch side by side
GROUP = "c3_30"                     # the table of the group pass
CHUNK_SMALL, CHUNK_WHOLE = 1 << 20, 4 << 30
Case = collections.namedtuple("Case", "tt lon fsmp0 t_samples")
_CASES = {}


def case_of(table):
    """Table, logged onsets, pre-pad and row length of a matrix table, built once."""
    if table not in _CASES:
        if table == MIXED:
            c = synth.make_case("C3", step=2, grid=(24, 20, 18), rows=12, n_samples=401)
            tt = c.traveltimes.copy()
            corner = tt[:6, :5, :7]
            tt[:6, :5, :7] = np.random.default_rng(404).integers(0, c.lsmp, size=corner.shape)
            onsets, fsmp0 = np.ascontiguousarray(c.onsets), int(c.fsmp)
        else:
            tt, onsets, fsmp0, _ = sp.table_case(table)
        _CASES[table] = Case(tt, np.ascontiguousarray(np.log(np.clip(onsets, 0.01, np.inf))), fsmp0, onsets.shape[1])
    return _CASES[table]


def requests_of(table):
    """kind -> requests, in the order they run on the (table, configuration)'s engine."""
    if table != MIXED:
        return sp.roster(table)
    return collections.OrderedDict([("detect", [sp.Request("detect", table, 0, 401, ())]),
                                    ("marginal_map", [sp.Request("marginal_map", table, 0, 401, (100, 301))]),
                                    ("migrate_device", [sp.Request("migrate_device", table, 0, 401, (True,))])])


def _nan_series(shape):
    return (np.full(shape, np.nan), np.full(shape, np.nan), np.full(shape, -1, dtype=np.int64))


def run_request(eng, req):
    """One request on ``eng``: the arrays the call wrote, in a fixed order."""
    import torch

    if req.kind == "find_max_coa":
        series = _nan_series(req.ns)
        eng.find_max_coa(sp.fmc_volume(req.ns), req.ns, sp.FMC_NODES, out=series)
        return list(series)
    c = case_of(req.table)
    rows, n_nodes, ns = c.tt.shape[-1], c.tt[..., 0].size, req.ns
    fsmp = c.fsmp0 + req.fsmp_off
    lsmp = c.t_samples - fsmp - ns
    dev = torch.device("cuda", 0)
    if req.kind == "detect":
        return list(eng.detect(c.lon, fsmp, lsmp, rows, out=_nan_series(ns)))
    if req.kind == "detect_batch":
        steps = np.stack([np.roll(c.lon, sp.BATCH_SHIFT * k, axis=1) for k in range(req.args[0])])
        return list(eng.detect_batch(steps, fsmp, lsmp, rows, out=_nan_series((req.args[0], ns))))
    if req.kind == "detect_partial":
        part = (torch.full((ns,), float("nan"), dtype=torch.float64, device=dev),
                torch.full((ns,), -1, dtype=torch.int64, device=dev),
                torch.full((ns,), float("nan"), dtype=torch.float64, device=dev))
        torch.cuda.synchronize()        # (the fills ran on torch's stream, the engine is on its own)
        eng.detect_partial(c.lon, fsmp, lsmp, rows, part)
        series = eng.finalize(part[0], part[1], part[2], 1, ns, n_nodes, out=_nan_series(ns))
        eng.synchronize()
        return list(series) + [p.cpu().numpy() for p in part]
    if req.kind == "migrate_host":
        scan, chunked, accumulate = req.args
        eng.config("chunk_bytes", CHUNK_SMALL if chunked else CHUNK_WHOLE)
        vol = sp.accumulate_prefill(n_nodes, ns) if accumulate else np.full((n_nodes, ns), np.nan)
        series = _nan_series(ns) if scan else None
        eng.migrate(c.lon, fsmp, lsmp, rows, vol, scan_out=series, accumulate=accumulate)
        return [vol] + (list(series) if scan else [])
    if req.kind == "migrate_device":
        vol = torch.full((n_nodes, ns), float("nan"), dtype=torch.float64, device=dev)
        series = _nan_series(ns) if req.args[0] else None
        torch.cuda.synchronize()
        eng.migrate(c.lon, fsmp, lsmp, rows, vol, scan_out=series)
        eng.synchronize()
        return [vol.cpu().numpy()] + (list(series) if series is not None else [])
    assert req.kind == "marginal_map", req
    series = _nan_series(ns)
    out = eng.marginal_map(c.lon, fsmp, lsmp, rows, req.args[0], req.args[1], out=np.full(c.tt.shape[:3], np.nan),
                           scan_out=series)
    return [out] + list(series)


def read_outs(lib, eng, req, last_launch_rule):
    def get(key):
        try:
            return eng.get(key)
        except lib.QMHipError as e:     # (a group whose box engines differ says so: a function of the launches too)
            return str(e)

    got = [get(k) for k in READOUTS]
    if last_launch_rule and got[0] != 3:
        got = [0 if k in SHIFT_ONLY else v for k, v in zip(READOUTS, got)]
    if req.kind == "detect_batch":
        got.append(get("steps_per_launch"))
    return got


def walk(lib, table, cfg, group=False, last_launch_rule=False):
    """{kind: {"readouts": [...], "digest": ...}} of every request of ``table`` on ONE fresh engine with ``cfg``."""
    out = collections.OrderedDict()
    try:
        eng = lib.EngineGroup([0, 0, 0], **cfg) if group else lib.Engine(0, **dict(_engine_cfg(table), **cfg))
    except lib.QMHipError as e:
        return {"refused": str(e)}
    try:
        eng.load_lut(case_of(table).tt)
        for kind, reqs in requests_of(table).items():
            if group and kind not in sp.GROUP_KINDS:
                continue
            sha, reads = hashlib.sha256(), []
            for req in reqs:
                try:
                    for x in run_request(eng, req):
                        sha.update(np.ascontiguousarray(x).tobytes())
                    reads.append(read_outs(lib, eng, req, last_launch_rule))
                except lib.QMHipError as e:
                    reads.append({"refused": str(e)})
            out[kind] = {"readouts": reads, "digest": sha.hexdigest()[:16]}
        if table == MIXED:
            # (this entry must not stop covering the split launch)
            direct, nodes = eng.get("shift_wide_bricks"), eng.get("shift_brick_nodes")
            assert 0 < direct and direct * nodes < eng.get("n_nodes"), (direct, nodes)
            out["direct_bricks"] = direct
    finally:
        eng.close()
    return out


def _engine_cfg(table):
    return {"brick_x": 4, "brick_y": 4, "brick_z": 4} if table == MIXED else {}


def matrix():
    """(name, table, configuration, group) of every engine of the matrix."""
    for table in list(sp.TABLES) + [MIXED]:
        for cfg in (MIXED_CONFIGS if table == MIXED else CONFIGS):
            yield f"{table}|{json.dumps(cfg, sort_keys=True)}", table, cfg, False
    yield f"{GROUP}|group_3", GROUP, {}, True


def n_cu(lib):
    eng = lib.Engine(0)
    try:
        return eng.get("n_cu")
    finally:
        eng.close()


def main(argv):
    from quakemigrate_amd.core import lib

    rule = "--last-launch-rule" in argv
    argv = [a for a in argv if a != "--last-launch-rule"]

    record = collections.OrderedDict([("commit", argv[2] if len(argv) > 2 else None), ("n_cu", n_cu(lib)),
                                      ("readouts", list(READOUTS) + ["steps_per_launch (detect_batch)"]),
                                      ("entries", collections.OrderedDict())])
    for name, table, cfg, group in matrix():
        record["entries"][name] = walk(lib, table, cfg, group, last_launch_rule=rule)
    lines = ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in record["entries"].items())
    head = ", ".join(f"{json.dumps(k)}: {json.dumps(record[k])}" for k in ("commit", "n_cu", "readouts"))
    pathlib.Path(argv[1]).write_text("{" + head + ', "entries": {\n' + lines + "\n}}\n")
    print(f"{len(record['entries'])} engines recorded in {argv[1]}")


if __name__ == "__main__":
    main(sys.argv)
