# -*- coding: utf-8 -*-
"""
The continuous stream fed with GAPPY traces (include/qmhip.h: qm_stream_set_segment_feed, qm_stream_push_segments)
beside the gap-free stream and beside the host path such timesteps took before: the geometry of
tools/resample_bench.py -- 45 component traces (one per P row, two per S row of C3's 30 rows) in windows of 7862
samples at 50 Hz on a 101 x 101 x 51 grid, seeded noise ~1e3 on a ramp and an offset with a burst each.

Every figure is printed as it is measured; nothing is asserted or concluded from them here.  One JSON line:
  ms_per_step_signals            push_signals, the gap-free stage of this build: host clock from the first push to
                                 the last pop of `--steps` timesteps at one timestep per launch, after `--warm`
                                 launches of the same stream; median of `--repeats` windows
  ms_per_step_segments_gap_free  (a) push_segments with one segment per trace (the planning of the records inside the
                                 clock), the same traces
  ms_per_step_segments_3         (b) push_segments with 3 segments per trace
  ms_per_step_host               (c) the host path: per timestep and segment scipy.signal.detrend twice, the cosine
                                 taper, sosfilt forward and backward, the taper again, the fill, then the library's
                                 CPU STA/LTA per trace, the root-mean-square over a row's components, clip and
                                 logarithm, and push of the log-onsets -- all inside the clock (obspy's per-trace
                                 overhead not included); the 3-segment layout
  segment_kernel_ms              qm_engine_preprocess_segments' launch alone on the 3-segment layout, HIP events
                                 (qm_engine_last_kernel_ms), median of `--calls` calls; segment_kernel_gap_free_ms: on
                                 the one-segment layout

The line goes to stdout and to `--out` (default profiles/segments_bench.txt).

    python tools/segments_bench.py [--steps 12] [--repeats 10]
"""

import argparse
import dataclasses
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from quakemigrate_amd.core import lib  # noqa: E402
from quakemigrate_amd.preprocess import GAP_FILL_VALUE, OnsetStage, plan_segments  # noqa: E402
from quakemigrate_amd.stream import StreamingDetector  # noqa: E402

SCAN_RATE = 50


def traces(seed, case, trace_row):
    t_samples = case.onsets.shape[1]
    rng = np.random.default_rng(seed)
    t = np.arange(t_samples, dtype=np.float64)
    x = (1e3 * rng.standard_normal((len(trace_row), t_samples)) + rng.uniform(-3, 3, (len(trace_row), 1)) * t
         + rng.uniform(-5e3, 5e3, (len(trace_row), 1)))
    for i, row in enumerate(trace_row):
        at = int(np.argmax(case.onsets[row]))
        n = min(50, t_samples - at)
        x[i, at:at + n] += 3e4 * rng.standard_normal(n) * np.exp(-np.arange(n) / 15.0)
    return np.ascontiguousarray(x)


def three_segments(seed, n_traces, t_samples):
    """Per trace a late start, two gaps of 5-200 samples and an early end."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_traces):
        cuts = (rng.integers(t_samples // 5, 2 * t_samples // 5), rng.integers(3 * t_samples // 5, 4 * t_samples // 5))
        g = rng.integers(5, 200, size=4)
        out += [(i, int(g[0]), int(cuts[0] - g[0])), (i, int(cuts[0] + g[1]), int(cuts[1] - cuts[0] - g[1])),
                (i, int(cuts[1] + g[2]), int(t_samples - cuts[1] - g[2] - g[3]))]
    return out


def host_onsets(x, segments, a, t_samples, n_rows):
    """calculate_onsets for gappy traces with NumPy, SciPy and the library's CPU STA/LTA: the log-onsets."""
    from scipy.signal import detrend, sosfilt

    records, weights = plan_segments(t_samples, len(x), segments)
    f = np.full(x.shape, GAP_FILL_VALUE)

    def taper(y, off, m):
        y[:m] *= weights[off:off + m]
        y[len(y) - m:] *= weights[off + m:off + 2 * m]

    for tr, first, n, _, _, off, m, _ in records.tolist():
        y = detrend(detrend(x[tr, first:first + n], type="linear"), type="constant")
        sos = a["sos"][a["trace_filter"][tr]]
        taper(y, off, m)
        y = sosfilt(sos, sosfilt(sos, y)[::-1])[::-1].copy()
        taper(y, off, m)
        f[tr, first:first + n] = y
    squares = np.zeros((n_rows, t_samples))
    for i, row in enumerate(a["trace_row"]):
        squares[row] += lib.overlapping_sta_lta(f[i] * f[i], int(a["nsta"][row]), int(a["nlta"][row])) ** 2
    onsets = np.sqrt(squares)
    pad = int(a["taper_pad"])
    if pad > 0:
        onsets[:, :pad] = 1.0
        onsets[:, -pad:] = 1.0
    return np.log(np.clip(np.clip(onsets, a["min_onset_value"], np.inf), 0.01, np.inf))


def timed_stream(eng, case, rows, t_samples, feed, push, steps, warm, repeats, **stages):
    sd = StreamingDetector(eng, rows, t_samples, case.fsmp, case.lsmp, case.available, depth=3, steps_per_launch=1,
                           **stages)

    def run(n):
        popped = 0
        for i in range(n):
            while not push(sd, feed(i)):
                sd.pop(1)
                popped += 1
        sd.flush()
        sd.pop(n - popped)

    run(warm)
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(steps)
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    sd.close()
    return ms


def main():
    from quakemigrate_amd import synth

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segments_bench.txt"))
    ap.add_argument("--grid", nargs=3, type=int, default=[101, 101, 51])
    ap.add_argument("--t-samples", type=int, default=7862, help="samples per window (C3's own: 7862)")
    ap.add_argument("--pool", type=int, default=3, help="distinct windows, cycled")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    if lib.qmlib.qm_device_count() < 1:
        raise SystemExit("segments_bench: no HIP device visible")
    probe = synth.make_case("C3", step=0, grid=tuple(args.grid), table=False)
    pads = probe.onsets.shape[1] - synth.CONFIGS["C3"]["n_samples"]
    cases = [synth.make_case("C3", step=s, grid=tuple(args.grid), n_samples=args.t_samples - pads, table=(s == 0))
             for s in range(args.pool)]
    case = cases[0]
    rows, t_samples = case.onsets.shape
    n_p = rows // 2
    trace_row = list(range(n_p)) + [r for r in range(n_p, rows) for _ in range(2)]
    plain = OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 16.0, 2)},
                       sta_lta_windows={"P": (0.2, 1.0), "S": (0.2, 1.0)}, trace_row=trace_row,
                       trace_phase=["P"] * n_p + ["S"] * (2 * (rows - n_p)),
                       row_phase=["P"] * n_p + ["S"] * (rows - n_p), taper_pad=20)
    gappy = dataclasses.replace(plain, fill_gaps=True)
    a = gappy.arrays(t_samples, SCAN_RATE)
    n = len(trace_row)
    wins = [traces(200 + s, c, trace_row) for s, c in enumerate(cases)]
    whole = [(i, 0, t_samples) for i in range(n)]
    three = [three_segments(300 + s, n, t_samples) for s in range(args.pool)]

    eng = lib.Engine(0)
    kernel = {}
    for name, segments in (("gap_free", whole), ("3", three[0])):
        records, weights = plan_segments(t_samples, n, segments)
        eng.preprocess_segments(wins[0], a["trace_filter"], a["sos"], records, weights)   # (first call: allocations)
        ms = []
        for _ in range(args.calls):
            eng.preprocess_segments(wins[0], a["trace_filter"], a["sos"], records, weights)
            ms.append(eng.last_kernel_ms())
        kernel[name] = ms
    eng.load_lut(case.traveltimes)
    common = dict(steps=args.steps, warm=args.warm, repeats=args.repeats)
    pool = len(wins)
    sig_ms = timed_stream(eng, case, rows, t_samples, lambda i: wins[i % pool],
                          lambda sd, w: sd.push_signals(w), onset_stage=plain, sampling_rate=SCAN_RATE, **common)
    free_ms = timed_stream(eng, case, rows, t_samples, lambda i: (wins[i % pool], whole),
                           lambda sd, w: sd.push_segments(*w), onset_stage=gappy, sampling_rate=SCAN_RATE,
                           max_segments=4 * n, **common)
    three_ms = timed_stream(eng, case, rows, t_samples, lambda i: (wins[i % pool], three[i % pool]),
                            lambda sd, w: sd.push_segments(*w), onset_stage=gappy, sampling_rate=SCAN_RATE,
                            max_segments=4 * n, **common)
    host_ms = timed_stream(eng, case, rows, t_samples,
                           lambda i: host_onsets(wins[i % pool], three[i % pool], a, t_samples, rows),
                           lambda sd, w: sd.push(w), **common)
    eng.close()
    med = lambda v: round(float(np.median(v)), 4)           # noqa: E731
    line = dict(
        grid=list(case.grid), rows=rows, traces=n, t_samples=t_samples, steps_per_launch=1, steps=args.steps,
        warmup_launches=args.warm, repeats=args.repeats,
        ms_per_step_signals=med(sig_ms), ms_per_step_signals_all=[round(v, 4) for v in sig_ms],
        ms_per_step_segments_gap_free=med(free_ms), ms_per_step_segments_gap_free_all=[round(v, 4) for v in free_ms],
        ms_per_step_segments_3=med(three_ms), ms_per_step_segments_3_all=[round(v, 4) for v in three_ms],
        ms_per_step_host=med(host_ms), ms_per_step_host_all=[round(v, 4) for v in host_ms],
        segment_kernel_ms=med(kernel["3"]), segment_kernel_gap_free_ms=med(kernel["gap_free"]))
    text = json.dumps(line)
    print(text, flush=True)
    with open(args.out, "w") as out:
        out.write(text + "\n")


if __name__ == "__main__":
    main()
