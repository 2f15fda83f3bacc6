# -*- coding: utf-8 -*-
"""
The C3 detect step on an engine group (include/qmhip.h part 4) beside one Engine: host onsets in, host series
out, for a single ``Engine``, ``EngineGroup([0])``, ``EngineGroup([0, 0])`` and -- on a box with more GPUs --
``EngineGroup(range(G))``.  Each configuration is warmed up, then timed call by call with a host clock around
calls that end in a device synchronise (every call here returns host arrays), and the device time of every
part's share of the last step comes from its own HIP events (``EngineGroup.part_info``; ``Engine.last_kernel_ms``
for the single engine).  Results must equal the single engine's (argmax and max_coa bit for bit).  One JSON line
per configuration.

    python tools/group_bench.py [--samples 1536] [--rows 30] [--warmup 3] [--steps 10]
"""

import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from quakemigrate_amd import synth  # noqa: E402
from quakemigrate_amd.core import lib  # noqa: E402


def run(eng, lon, case, warmup, steps):
    out = (np.zeros(case.n_samples), np.zeros(case.n_samples), np.zeros(case.n_samples, dtype=np.int64))
    for _ in range(warmup):
        eng.detect(lon, case.fsmp, case.lsmp, case.available, out=out)
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        eng.detect(lon, case.fsmp, case.lsmp, case.available, out=out)
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=1536)
    ap.add_argument("--rows", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    n_dev = lib.qmlib.qm_device_count()
    if n_dev < 1:
        raise SystemExit("group_bench: no HIP device visible")
    case = synth.make_case("C3", step=0, rows=args.rows, n_samples=args.samples)
    lon = np.ascontiguousarray(np.log(np.clip(case.onsets, 0.01, np.inf)))
    head = dict(grid=list(case.grid), rows=args.rows, n_samples=case.n_samples, devices_visible=n_dev,
                warmup=args.warmup, steps=args.steps)

    single = lib.Engine(0)
    single.load_lut(case.traveltimes)
    want, times = run(single, lon, case, args.warmup, args.steps)
    print(json.dumps(dict(head, config="Engine(0)", median_ms=round(statistics.median(times), 3),
                          min_ms=round(min(times), 3), kernel_ms=[round(single.last_kernel_ms(), 3)])), flush=True)
    single.close()

    configs = [[0], [0, 0]] + ([list(range(n_dev))] if n_dev > 1 else [])
    for devices in configs:
        g = lib.EngineGroup(devices)
        g.load_lut(case.traveltimes)
        got, times = run(g, lon, case, args.warmup, args.steps)
        same = bool(np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0]))
        norm = float(np.max(np.abs(got[1] - want[1]) / np.abs(want[1])))
        parts = [g.part_info(p) for p in range(len(devices))]
        print(json.dumps(dict(head, config=f"EngineGroup({devices})", median_ms=round(statistics.median(times), 3),
                              min_ms=round(min(times), 3),
                              part_ms=[round(p["last_ms"], 3) for p in parts],
                              part_nodes=[p["node_range"][1] - p["node_range"][0] for p in parts],
                              part_boxes=[len(p["boxes"]) for p in parts],
                              bit_equal=same, max_norm_rel=norm)), flush=True)
        g.close()
        if not same:
            raise SystemExit(f"group_bench: EngineGroup({devices}) differs from the single engine")


if __name__ == "__main__":
    main()
