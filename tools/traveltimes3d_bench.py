# -*- coding: utf-8 -*-
"""
The grid eikonal solver (include/qmhip.h: qm_engine_tt_eikonal3d) on two geometries of BASELINE.md: config C3's
201 x 201 x 101 grid with 30 stations x 2 phases = 60 rows over two models, and the Icequake-sized 71 x 64 x 57 grid
with 12 stations x 2 phases.  The model is a 1-D one spread over the grid's depths, so the sections + sweep path can
solve the same problem beside it.

One JSON line per geometry and path, times from the stage's HIP events ("tt_ns_<stage>", for eikonal3d first launch
to last with the per-round flag read-backs inside), medians of `--calls`:
  eikonal3d       all rows in one call: call_ms, rounds (min, max over rows; the call runs the max), launches
                  (8 (nx + ny + nz - 2) per round, the first and the last pass), ms_per_round, us_per_launch
  eikonal3d_one_row   the SAME launch train with one row in it: what the train costs when the planes are nearly empty.
                  `train_share` = one_row call_ms / all-rows call_ms: near 1, the launch train bounds the call; near
                  0, the arithmetic of the rows does.  (Both calls run the same number of rounds only if the one row
                  is the slowest to settle: rounds are printed for both, and ms_per_round is the figure to compare.)
  host_ms         the host clock around the whole call (staging, the slowness check and the synchronise included),
                  and host_share_outside = 1 - call_ms / host_ms
  sections+sweep  the same 1-D model through qm_engine_tt_sections and qm_engine_tt_sweep, sections at a fifth of the
                  node spacing (the reference's nlloc_dx proportion): their two stage times
and beside them, on the CPU, the NumPy restatement (tests/traveltimes3d_ref.py) at a REDUCED size, one row: the
restatement is the tests' oracle, not a baseline.  No pass/fail threshold on any time.

    python tools/traveltimes3d_bench.py [--calls 10] [--out profiles/traveltimes3d_bench.txt]
"""

import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import traveltimes3d_ref as t3  # noqa: E402
from quakemigrate_amd import traveltimes as tt  # noqa: E402
from quakemigrate_amd.core import lib  # noqa: E402

GEOMETRIES = {
    "C3": dict(count=(201, 201, 101), spacing=(0.5, 0.5, 0.5), stations=30),
    "icequake": dict(count=(71, 64, 57), spacing=(0.025, 0.025, 0.025), stations=12),
}
PHASES = ("P", "S")
VMOD = {"Depth": [0.0, 4.0, 15.0, 35.0], "Vp": [4.0, 5.6, 6.4, 7.9], "Vs": [2.3, 3.2, 3.7, 4.5]}
REDUCED = (41, 41, 21)


def timed(eng, steps, calls):
    """`steps`: (stage key, call) pairs run in this order.  Medians over `calls` of each step's stage time (ms), read
    right after its call -- the next call of the stage zeroes the clocks of the stages it does not run --, and of the
    host clock around all of them (ms)."""
    import torch

    def run():
        return [(call(), eng.get(key) / 1e6)[1] for key, call in steps]

    run()                       # warm-up
    stage, host = [], []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stage.append(run())
        host.append((time.perf_counter() - t0) * 1e3)
    return np.median(np.array(stage), axis=0), float(np.median(host))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--geometries", default="C3,icequake")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "traveltimes3d_bench.txt"))
    a = ap.parse_args()
    if lib.qmlib.qm_device_count() < 1:
        raise SystemExit("traveltimes3d_bench: no HIP device visible")
    import torch

    eng = lib.Engine(0)
    lines = []

    def emit(**fields):
        lines.append(json.dumps(fields))
        print(lines[-1], flush=True)

    for name in a.geometries.split(","):
        geo = GEOMETRIES[name]
        count, spacing, ll = geo["count"], geo["spacing"], (0.0, 0.0, 0.0)
        rng = np.random.default_rng(5)
        extent = [(n - 1) * s for n, s in zip(count, spacing)]
        xyz = np.c_[rng.uniform(0, extent[0], geo["stations"]), rng.uniform(0, extent[1], geo["stations"]),
                    rng.uniform(0, extent[2] * 0.05, geo["stations"])]
        n_ph = len(PHASES)
        n_rows = geo["stations"] * n_ph
        depths = ll[2] + np.arange(count[2]) * spacing[2]
        slowness = np.stack([np.broadcast_to(1.0 / tt.model_velocity(VMOD, ph, depths), count) for ph in PHASES])
        slowness = torch.as_tensor(np.ascontiguousarray(slowness), device=f"cuda:{eng.device}")
        s0 = np.array([1.0 / tt.model_velocity(VMOD, ph, z) for z in xyz[:, 2] for ph in PHASES])
        sources, row_model = np.repeat(xyz, n_ph, axis=0), np.tile(np.arange(n_ph), geo["stations"])
        per_round = 8 * (sum(count) - 2)
        kept = {}

        def solve(rows):
            kept["out"] = eng.traveltimes_eikonal3d(ll, spacing, count, sources[:rows], s0[:rows], slowness,
                                                    row_model[:rows], device=True)

        for label, rows in (("eikonal3d", n_rows), ("eikonal3d_one_row", 1)):
            (ms,), host = timed(eng, [("tt_ns_eikonal3d", lambda: solve(rows))], a.calls)
            rounds = kept["out"][1]
            launches = per_round * int(rounds.max()) + 2
            kept[label] = ms
            emit(geometry=name, path=label, grid=count, rows=rows, models=n_ph, call_ms=round(float(ms), 3),
                 rounds_min_max=[int(rounds.min()), int(rounds.max())], launches=launches,
                 ms_per_round=round(float(ms) / int(rounds.max()), 3), us_per_launch=round(float(ms) * 1e3 / launches, 3),
                 host_ms=round(host, 3), host_share_outside=round(1.0 - float(ms) / host, 3))
        emit(geometry=name, train_share=round(float(kept["eikonal3d_one_row"] / kept["eikonal3d"]), 3))
        del kept["out"]

        dx = spacing[0] / 5
        plan = tt.plan_sections(ll, spacing, count, xyz, dx)
        depth_rows = np.arange(plan["nz"]) * dx
        sec_slow = np.array([1.0 / tt.model_velocity(VMOD, ph, plan["z0"][i] + depth_rows)
                             for i in range(geo["stations"]) for ph in PHASES])
        zs = np.repeat(plan["source_depth"], n_ph)
        origins = np.repeat(np.column_stack([np.zeros(geo["stations"]), plan["z0"]]), n_ph, axis=0)

        def sections():
            kept["sections"] = eng.traveltime_sections(sec_slow, zs, plan["nr"], dx, source_slowness=s0, device=True)[0]

        def sweep():
            eng.sweep_sections(kept["sections"], ll, spacing, count, sources[:, :2], np.arange(n_rows), origins, dx,
                               device=True)

        (sec_ms, sweep_ms), host = timed(eng, [("tt_ns_sections", sections), ("tt_ns_sweep", sweep)], a.calls)
        emit(geometry=name, path="sections+sweep", rows=n_rows, section_shape=[plan["nr"], plan["nz"]], section_spacing=dx,
             sections_ms=round(float(sec_ms), 3), sweep_ms=round(float(sweep_ms), 3), host_ms=round(host, 3))

    # the oracle, on the CPU, reduced
    count = REDUCED
    depths = np.arange(count[2]) * 0.5
    slow = np.broadcast_to(1.0 / tt.model_velocity(VMOD, "P", depths), (1,) + count)
    t0 = time.perf_counter()
    _, rounds, _ = t3.solve((0.0, 0.0, 0.0), (0.5, 0.5, 0.5), count, [(7.3, 11.1, 0.2)],
                            [1.0 / tt.model_velocity(VMOD, "P", 0.2)], slow, [0])
    emit(host="numpy restatement (the oracle, not a baseline)", reduced_grid=count, rows=1, rounds=int(rounds[0]),
         numpy_ms=round((time.perf_counter() - t0) * 1e3, 1))
    eng.close()
    pathlib.Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
