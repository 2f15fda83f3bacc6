# -*- coding: utf-8 -*-
"""
The phase-pick launch (include/qmhip.h: qm_engine_pick_phases) beside the host loop it replaces, and its share of a
located event.

Rows: the seeded family of tests/picks_ref.py (smoothed noise around 1.3, one asymmetric bump per row, taper pads of
ones), P and S rows per station: 30 and 60 rows of 451 samples (a C3-sized and a BASELINE configs[3]-sized table at
50 Hz, marginal window 2 s) and 60 rows of 4096.

Per shape one JSON line:
  kernel_ms            the launch alone: HIP events around it (qm_engine_last_kernel_ms), median of `--calls` calls
  wall_host_ms         host clock around Engine.pick_phases with the onsets on the host: copies in, launch, copies
                       back, synchronise; median
  wall_device_ms       the same with the onsets resident on the device (what qm_engine_onsets leaves there)
  host_loop_ms         the reference's per-row work on this machine's CPU: threshold (median and MAD), peak and its
                       default scipy.optimize.curve_fit call, rows one after the other as GaussianPicker does; median
                       of `--host-repeats` passes
  host_fit_ms          ... the curve_fit calls of that loop alone
  ratio                host_loop_ms / wall_host_ms
  picked, iterations   rows with a pick, the solver's iterations (median, most)
With --locate (default) two more lines: per located event of examples/locate_events.py on a C3-sized grid
(201 x 201 x 101 nodes, 30 rows), the host clock between consecutive events handed to on_event -- without a picker
(what locate_compute did before it had one) and with the DevicePicker -- and what the former plus the host loop of
a 30-row table would come to.

    python tools/pick_bench.py [--calls 50] [--host-repeats 3] [--no-locate] > profiles/pick_bench.txt
"""

import argparse
import importlib.util
import json
import pathlib
import sys
import time
import warnings

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import picks_ref as pr  # noqa: E402
from quakemigrate_amd.core import lib  # noqa: E402

SHAPES = ((30, 451), (60, 451), (60, 4096))


def host_loop_ms(fam):
    """(whole loop, curve_fit alone) in ms for one pass over the rows."""
    fit = 0.0
    t0 = time.perf_counter()
    for r in range(len(fam["onsets"])):
        group = fam["windows"][fam["row_group"] == fam["row_group"][r]]
        thr = pr.find_pick_threshold(fam["onsets"][r], group, "MAD", 8.0)
        lo, hi = fam["windows"][r, 0], fam["windows"][r, 2]
        try:
            peak = pr.find_peak(fam["onsets"][r][lo:hi], thr)
        except pr.NoOnsetPeak:
            continue
        x, y, p0 = pr.fit_inputs(fam["onsets"][r], lo + peak[0] - 1, lo + peak[1] + 1, fam["sampling_rate"],
                                 fam["halfwidth"][r])
        t1 = time.perf_counter()
        try:
            pr.scipy_default(x, y, p0)
        except (ValueError, RuntimeError):
            pass
        fit += time.perf_counter() - t1
    return (time.perf_counter() - t0) * 1e3, fit * 1e3


def bench_shape(eng, n_rows, t_samples, calls, host_repeats):
    import torch

    fam = pr.family(seed=7, n_stations=n_rows // 2, t_samples=t_samples)
    args = (fam["windows"], fam["row_group"], fam["sampling_rate"], fam["halfwidth"])
    d_on = torch.from_numpy(fam["onsets"]).to(f"cuda:{eng.device}")
    picks, status = eng.pick_phases(fam["onsets"], *args)                # warm-up: code object, buffers
    eng.pick_phases(d_on, *args)
    kernel, wall_host, wall_dev = [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        eng.pick_phases(fam["onsets"], *args)
        wall_host.append((time.perf_counter() - t0) * 1e3)
        kernel.append(eng.last_kernel_ms())
        t0 = time.perf_counter()
        eng.pick_phases(d_on, *args)
        wall_dev.append((time.perf_counter() - t0) * 1e3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host_loop_ms(fam)
        host = [host_loop_ms(fam) for _ in range(host_repeats)]
    loop, fit = float(np.median([h[0] for h in host])), float(np.median([h[1] for h in host]))
    its = picks[status == 0, 7]
    out = dict(rows=n_rows, t_samples=t_samples, kernel_ms=round(float(np.median(kernel)), 4),
               kernel_ms_min_max=[round(min(kernel), 4), round(max(kernel), 4)],
               wall_host_ms=round(float(np.median(wall_host)), 4), wall_device_ms=round(float(np.median(wall_dev)), 4),
               host_loop_ms=round(loop, 3), host_fit_ms=round(fit, 3),
               ratio=round(loop / float(np.median(wall_host)), 1), picked=int((status == 0).sum()),
               iterations=[int(np.median(its)), int(its.max())] if len(its) else [0, 0])
    print(json.dumps(out), flush=True)
    return out


def locate_ms(with_picker, n_events):
    """ms between consecutive located events of the example on a C3-sized grid (the first one, which loads the
    table, left out)."""
    spec = importlib.util.spec_from_file_location("locate_events", ROOT / "examples" / "locate_events.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    stamps = []
    mod.run(grid=(201, 201, 101), rows=30, n_events=n_events, with_picker=with_picker,
            on_event=lambda result: stamps.append(time.perf_counter()))
    return [round(v * 1e3, 3) for v in np.diff(stamps)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--no-locate", action="store_true")
    ap.add_argument("--events", type=int, default=7)
    a = ap.parse_args()
    if lib.qmlib.qm_device_count() < 1:
        raise SystemExit("pick_bench: no HIP device visible")
    eng = lib.Engine(0)
    results = [bench_shape(eng, n, t, a.calls, a.host_repeats) for n, t in SHAPES]
    eng.close()
    if not a.no_locate:
        without, with_picks = locate_ms(False, a.events), locate_ms(True, a.events)
        base, picked = float(np.median(without)), float(np.median(with_picks))
        host = results[0]["host_loop_ms"]
        print(json.dumps(dict(locate="C3-sized grid, 30 rows", ms_between_events_without_picker=without,
                              ms_between_events_with_device_picker=with_picks)), flush=True)
        print(json.dumps(dict(locate_event_ms=round(base, 3), locate_event_with_device_picks_ms=round(picked, 3),
                              device_picks_share=round((picked - base) / picked, 3),
                              locate_event_plus_host_loop_ms=round(base + host, 3),
                              host_loop_share=round(host / (base + host), 3))), flush=True)


if __name__ == "__main__":
    main()
