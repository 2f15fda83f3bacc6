# -*- coding: utf-8 -*-
"""
The travel-time stage (include/qmhip.h: qm_engine_tt_homogeneous / _tt_sections / _tt_sweep) on the geometry of
BASELINE config C3: a 201 x 201 x 101 grid, 30 stations x 2 phases, sections at a fifth of the node spacing.

One JSON line per launch, times from the stage's HIP events ("tt_ns_<stage>"), medians of `--calls`:
  homogeneous   60 rows in one launch; `stream_fraction`: its bytes per second over the 4.8 TB/s store stream that
                tools/diag_write_bw.py measured
  sections      60 sections of nr x nz nodes in one launch (tau in engine scratch at this size), with the rounds taken
  sweep         60 rows in one launch, the sections resident; `stream_fraction` as above
and beside them, on this machine's CPU, the NumPy restatement (tests/traveltimes_ref.py):
  numpy_homogeneous_row_ms / numpy_sweep_row_ms   one row, median of `--host-repeats`; x 60 for the whole table
  numpy_sections_reduced_ms                       the section restatement on `reduced_shape`, 8 sections -- a REDUCED
                                                  size: the restatement is the tests' oracle, not a baseline
No pass/fail threshold on any time.

    python tools/traveltimes_bench.py [--calls 10] [--host-repeats 3] [--out profiles/traveltimes_bench.txt]
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
import traveltimes_ref as tr  # noqa: E402
from quakemigrate_amd import traveltimes as tt  # noqa: E402
from quakemigrate_amd.core import lib  # noqa: E402

COUNT, SPACING, LL = (201, 201, 101), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)
N_STATIONS, PHASES = 30, ("P", "S")
VMOD = {"Depth": [0.0, 4.0, 15.0, 35.0], "Vp": [4.0, 5.6, 6.4, 7.9], "Vs": [2.3, 3.2, 3.7, 4.5]}
STORE_STREAM = 4.8e12           # bytes per second, tools/diag_write_bw.py
REDUCED = (143, 52)


def median_ms(eng, key, call, calls):
    call()                      # warm-up
    times = []
    for _ in range(calls):
        call()
        times.append(eng.get(key) / 1e6)
    return float(np.median(times)), [round(min(times), 4), round(max(times), 4)]


def host_ms(call, repeats):
    call()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "traveltimes_bench.txt"))
    a = ap.parse_args()
    if lib.qmlib.qm_device_count() < 1:
        raise SystemExit("traveltimes_bench: no HIP device visible")
    rng = np.random.default_rng(5)
    extent = [(n - 1) * s for n, s in zip(COUNT, SPACING)]
    xyz = np.c_[rng.uniform(0, extent[0], N_STATIONS), rng.uniform(0, extent[1], N_STATIONS), np.zeros(N_STATIONS)]
    n_ph, dx = len(PHASES), SPACING[0] / 5
    rows_xyz = np.repeat(xyz, n_ph, axis=0)
    nodes, n_rows = int(np.prod(COUNT)), N_STATIONS * n_ph
    grid_bytes = nodes * n_rows * 8
    eng = lib.Engine(0)
    lines = []

    def emit(**fields):
        lines.append(json.dumps(fields))
        print(lines[-1], flush=True)

    vel = np.tile([5.0, 2.9], N_STATIONS)
    ms, span = median_ms(eng, "tt_ns_homogeneous",
                         lambda: eng.traveltimes_homogeneous(LL, SPACING, COUNT, rows_xyz, vel, device=True), a.calls)
    emit(launch="homogeneous", grid=COUNT, rows=n_rows, kernel_ms=round(ms, 4), kernel_ms_min_max=span,
         bytes=grid_bytes, stream_fraction=round(grid_bytes / (ms * 1e-3) / STORE_STREAM, 3))

    plan = tt.plan_sections(LL, SPACING, COUNT, xyz, dx)
    depth_rows = np.arange(plan["nz"]) * dx
    slowness = np.array([1.0 / tt.model_velocity(VMOD, ph, plan["z0"][i] + depth_rows)
                         for i in range(N_STATIONS) for ph in PHASES])
    s0 = np.array([1.0 / tt.model_velocity(VMOD, ph, xyz[i, 2]) for i in range(N_STATIONS) for ph in PHASES])
    zs = np.repeat(plan["source_depth"], n_ph)
    solved = {}

    def solve():
        solved["out"] = eng.traveltime_sections(slowness, zs, plan["nr"], dx, source_slowness=s0, device=True)

    ms, span = median_ms(eng, "tt_ns_sections", solve, a.calls)
    sections, rounds, _ = solved["out"]
    rounds = rounds.cpu().numpy()
    emit(launch="sections", sections=n_rows, shape=[plan["nr"], plan["nz"]], spacing=dx,
         lds=bool(plan["nr"] * plan["nz"] <= eng.get("tt_lds_nodes")), kernel_ms=round(ms, 3), kernel_ms_min_max=span,
         rounds_min_max=[int(rounds.min()), int(rounds.max())])

    origins = np.repeat(np.column_stack([np.zeros(N_STATIONS), plan["z0"]]), n_ph, axis=0)
    ms, span = median_ms(eng, "tt_ns_sweep",
                         lambda: eng.sweep_sections(sections, LL, SPACING, COUNT, rows_xyz[:, :2], np.arange(n_rows),
                                                    origins, dx, device=True), a.calls)
    emit(launch="sweep", grid=COUNT, rows=n_rows, kernel_ms=round(ms, 4), kernel_ms_min_max=span, bytes=grid_bytes,
         stream_fraction=round(grid_bytes / (ms * 1e-3) / STORE_STREAM, 3))

    section0 = sections[0].cpu().numpy()
    hom = host_ms(lambda: tr.homogeneous(LL, SPACING, COUNT, xyz[0], 5.0), a.host_repeats)
    swp = host_ms(lambda: tr.sweep(LL, SPACING, COUNT, xyz[0, :2], section0, 0.0, plan["z0"][0], dx), a.host_repeats)
    nr, nz = REDUCED
    red = host_ms(lambda: tr.solve_sections(slowness[:8, :nz], np.full(8, 0.2), s0[:8], nr, dx), 1)
    emit(host="numpy restatement", numpy_homogeneous_row_ms=hom, numpy_homogeneous_table_ms=round(hom * n_rows, 1),
         numpy_sweep_row_ms=swp, numpy_sweep_table_ms=round(swp * n_rows, 1), numpy_sections_reduced_ms=red,
         reduced_shape=list(REDUCED), reduced_sections=8)
    eng.close()
    pathlib.Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
