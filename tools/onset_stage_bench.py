# -*- coding: utf-8 -*-
"""
The continuous stream with WAVEFORMS going in (include/qmhip.h: qm_stream_set_onset_stage, qm_stream_push_signals)
beside the stream that takes log-onsets: C1-, E1- and C3-sized streams at 1 and 8 timesteps per launch, each once
with pre-made log-onsets pushed (what the host plugin path pushes after ITS pre-processing) and once with the
resampled component traces pushed (detrend, taper, zero-phase band-pass and STA/LTA in the launch).  Traces: one per
P row, two per S row (36 for C1 and E1, 45 for C3), seeded noise ~1e3 on a ramp and an offset with a burst each.

Per (configuration, K) one JSON line:
  ms_per_step_onsets / ms_per_step_signals   host clock from the first push to the last pop of the timed steps (the
                                             pop synchronises), after `--warm` launches of the same stream; the
                                             median of `--repeats` such windows and their spread
  preprocess_kernel_ms / onset_kernels_ms    the two stages alone on the K x n_traces traces of one launch, device
                                             arrays in and out: host clock around `--kernel-calls` enqueued calls
                                             ending in a synchronise, per call (the staged call's small coefficient
                                             copies are inside)
  preprocess_plain_ms                        the same with "preproc_skew" = 0 (every section on one lane)
  host_preprocess_ms                         SciPy detrend x2 + taper + sosfilt x2 of one timestep's traces on this
                                             machine's CPU (what the host plugin path spends per timestep before it
                                             can push; obspy's per-trace overhead not included)
  equal                                      the signal stream's series are array_equal to the log-onset stream's
                                             (whose log-onsets are the staged calls' output)

    python tools/onset_stage_bench.py [--configs C1 E1 C3] [--warm 32] [--repeats 3] > profiles/onset_stage_bench.txt
"""

import argparse
import json
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from quakemigrate_amd import synth  # noqa: E402
from quakemigrate_amd.core import lib  # noqa: E402
from quakemigrate_amd.preprocess import OnsetStage  # noqa: E402
from quakemigrate_amd.stream import StreamingDetector  # noqa: E402

STEPS = {"C1": 800, "E1": 96, "C3": 24}


def stage_for(rows, t_samples, rate):
    """P rows (first half) one trace each, S rows two; the reference's default filters and windows."""
    n_p = rows // 2
    trace_row = list(range(n_p)) + [r for r in range(n_p, rows) for _ in range(2)]
    stage = OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 16.0, 2)} if rate <= 100 else
                       {"P": (10.0, 100.0, 2), "S": (10.0, 100.0, 2)},
                       sta_lta_windows={"P": (0.2, 1.0), "S": (0.2, 1.0)} if rate <= 100 else
                       {"P": (0.01, 0.25), "S": (0.05, 0.5)},
                       trace_row=trace_row, trace_phase=["P"] * n_p + ["S"] * (2 * (rows - n_p)),
                       row_phase=["P"] * n_p + ["S"] * (rows - n_p), taper_pad=20)
    return stage, stage.arrays(t_samples, rate)


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


def host_preprocess_ms(x, a, repeats=3):
    from scipy.signal import detrend, sosfilt

    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        for i in range(len(x)):
            y = detrend(detrend(x[i], type="linear"), type="constant")
            y[:len(a["taper_left"])] *= a["taper_left"]
            y[len(y) - len(a["taper_right"]):] *= a["taper_right"]
            sos = a["sos"][a["trace_filter"][i]]
            sosfilt(sos, sosfilt(sos, y)[::-1])
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def timed_stream(eng, case, a, rows, t_samples, k, wins, push, steps, warm, repeats):
    sd = StreamingDetector(eng, rows, t_samples, case.fsmp, case.lsmp, case.available, depth=3, steps_per_launch=k,
                           onset_stage=a if push == "signals" else None)
    sd.run(wins[i % len(wins)] for i in range(warm * k))
    ms, got = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = sd.run(wins[i % len(wins)] for i in range(steps))
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    sd.close()
    return ms, got


def stage_kernels_ms(eng, a, x, rows, k, calls):
    """(preprocess skewed, preprocess plain, onset kernels) ms per call on the k x n_traces traces of one launch."""
    import torch

    dev = f"cuda:{eng.device}"
    n, t_samples = x.shape
    d_in = torch.from_numpy(np.ascontiguousarray(np.tile(x, (k, 1)))).to(dev)
    d_f = torch.empty_like(d_in)
    d_log = torch.empty((k * rows, t_samples), dtype=torch.float64, device=dev)
    tf = np.tile(a["trace_filter"], k)
    tr = np.concatenate([a["trace_row"] + s * rows for s in range(k)]).astype(np.int32)
    nsta, nlta = np.tile(a["nsta"], k), np.tile(a["nlta"], k)

    def pre():
        eng.preprocess(d_in, tf, a["sos"], taper=(a["taper_left"], a["taper_right"]), out=d_f)

    def ons():
        eng.onsets(d_f, tr, nsta, nlta, taper_pad=a["taper_pad"], min_onset_value=a["min_onset_value"],
                   log_out=d_log)

    def per_call(fn):
        fn()
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        eng.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    skewed = per_call(pre)
    eng.config("preproc_skew", 0)
    plain = per_call(pre)
    eng.config("preproc_skew", 1)
    pre()
    return skewed, plain, per_call(ons)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", nargs="+", default=["C1", "E1", "C3"])
    ap.add_argument("--ks", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--pool", type=int, default=3, help="distinct windows, cycled")
    ap.add_argument("--warm", type=int, default=32, help="launches run before the clock starts")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-calls", type=int, default=10)
    args = ap.parse_args()
    if lib.qmlib.qm_device_count() < 1:
        raise SystemExit("onset_stage_bench: no HIP device visible")
    for name in args.configs:
        rate = synth.CONFIGS[name]["rate"]
        cases = [synth.make_case(name, step=s, table=(s == 0)) for s in range(args.pool)]
        case = cases[0]
        rows, t_samples = case.onsets.shape
        stage, a = stage_for(rows, t_samples, rate)
        sigs = [traces(100 + s, c, a["trace_row"]) for s, c in enumerate(cases)]
        eng = lib.Engine(0)
        eng.load_lut(case.traveltimes)
        logged = []
        for x in sigs:                                      # the staged calls' log-onsets: what the other stream pushes
            f = eng.preprocess(x, a["trace_filter"], a["sos"], taper=(a["taper_left"], a["taper_right"]))
            logged.append(eng.onsets(f, a["trace_row"], a["nsta"], a["nlta"], taper_pad=a["taper_pad"],
                                     min_onset_value=a["min_onset_value"])[1])
        host_ms = host_preprocess_ms(sigs[0], a)
        for k in args.ks:
            steps = max(k, STEPS.get(name, 48) // k * k)
            warm = args.warm if name != "C3" else max(2, args.warm // 8)
            on_ms, on_got = timed_stream(eng, case, a, rows, t_samples, k, logged, "onsets", steps, warm, args.repeats)
            sg_ms, sg_got = timed_stream(eng, case, a, rows, t_samples, k, sigs, "signals", steps, warm, args.repeats)
            equal = all(all(np.array_equal(p, q) for p, q in zip(g, w)) for g, w in zip(sg_got, on_got))
            skewed, plain, ons = stage_kernels_ms(eng, a, sigs[0], rows, k, args.kernel_calls)
            print(json.dumps(dict(
                config=name, grid=list(case.grid), rows=rows, traces=len(a["trace_row"]), t_samples=t_samples,
                n_sections=int(a["sos"].shape[1]), steps_per_launch=k, steps=steps, warmup_launches=warm,
                ms_per_step_onsets=round(float(np.median(on_ms)), 4), ms_per_step_onsets_all=[round(v, 4) for v in on_ms],
                ms_per_step_signals=round(float(np.median(sg_ms)), 4),
                ms_per_step_signals_all=[round(v, 4) for v in sg_ms],
                preprocess_kernel_ms=round(skewed, 4), preprocess_plain_ms=round(plain, 4),
                onset_kernels_ms=round(ons, 4), host_preprocess_ms=round(host_ms, 3), equal=bool(equal))), flush=True)
            if not equal:
                raise SystemExit("onset_stage_bench: the signal stream differs from the log-onset stream")
        eng.close()


if __name__ == "__main__":
    main()
