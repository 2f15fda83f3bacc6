# -*- coding: utf-8 -*-
"""
The resampling stage (include/qmhip.h: qm_engine_resample, qm_stream_set_resample_stage, qm_stream_push_raw) beside
SciPy doing the same work on the host: 45 raw int32 traces -- 22 at 100 Hz (2 x the 50 Hz scan rate, decimated by 2),
5 at 40 Hz (0.8 x: upsampled by 5, decimated by 4), 18 at the scan rate (passed through) -- in windows of 7500
output samples, seeded noise ~1e3 on a ramp and an offset with a burst each.  C3's 30 rows on a reduced grid
(`--grid`): what is measured here does not depend on the grid, and the stream's step should not hide it.

Every figure is printed as it is measured; nothing is concluded from them here.  One JSON line per section:
  stage    kernel_ms            the launch alone: HIP events around it (qm_engine_last_kernel_ms), median of `--calls`
                                calls, host arrays in and out; kernel_plain_ms: the same with "preproc_skew" = 0
           call_ms              the whole call by the host clock (raw bytes in, float64 traces out, synchronised), median
           host_scipy_ms        the same stage on this machine's CPU: per trace the interpolation expression in NumPy,
                                scipy.signal.detrend twice, the cosine taper, sosfilt forward and backward, [::d];
                                median of `--host-repeats` passes (obspy's per-trace overhead not included)
           max_abs_diff         device against that host pass (the filter's bits are equal; the detrend's sums differ
                                in order)
  stream   ms_per_step_raw      host clock from the first push to the last pop of `--steps` timesteps, push_raw (the
                                resampling in the launch), after `--warm` launches; median of `--repeats` windows
           ms_per_step_signals  the same stream fed by push_signals with traces resampled beforehand (the pipeline alone)
           ms_per_step_signals_host_resampled
                                push_signals with the SciPy resampling of every timestep inside the clock: what a
                                caller without the stage pays per timestep (push_signals and everything behind it is
                                the code of the commit before the stage, unchanged by it)
           equal                push_raw's series are array_equal to those of Engine.resample + push_signals
  parent   (with `--parent-tree DIR`, a built checkout of the commit before the stage: `git archive` of it into DIR,
           `build_engine()` there) the two push_signals figures again, measured by a child process that imports the
           package and loads the library of THAT tree: parent_ms_per_step_signals, _host_resampled; parent_equal: its
           series hash to what this build's push_signals stream gave on the same traces.  Without the option the
           push_signals figures above come from this build only, whose push_signals path the stage did not touch.

The lines go to stdout and to `--out` (default profiles/resample_bench.txt).

    python tools/resample_bench.py [--steps 12] [--repeats 10] [--parent-tree parent_build]
"""

import argparse
import hashlib
import json
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
# (the child of `--parent-tree` imports the package of that tree, not of this one)
TREE = pathlib.Path(sys.argv[sys.argv.index("--child") + 1]).resolve() if "--child" in sys.argv else ROOT
sys.path.insert(0, str(TREE))
from quakemigrate_amd.core import lib  # noqa: E402
from quakemigrate_amd.stream import StreamingDetector  # noqa: E402

SCAN_RATE = 50
RESAMPLE_FIELDS = ("raw_offset", "n_raw", "up", "pad_left", "pad_right", "up_first", "n_up", "dec", "lowpass", "taper",
                   "out_first")


def raw_rates(n_traces):
    """Half at twice the scan rate, every tenth (even ones) at 0.8 x, the others at the scan rate."""
    rates = [100 if i % 2 else 50 for i in range(n_traces)]
    for i in range(0, n_traces, 10):
        rates[i] = 40
    return rates


def raw_traces(seed, case, trace_row, rates, n_raw):
    rng = np.random.default_rng(seed)
    out = []
    for i, (row, rate, n) in enumerate(zip(trace_row, rates, n_raw)):
        x = 1e3 * rng.standard_normal(n) + rng.uniform(-3, 3) * np.arange(n) * SCAN_RATE / rate + rng.uniform(-5e3, 5e3)
        at = int(np.argmax(case.onsets[row])) * rate // SCAN_RATE
        m = min(50 * rate // SCAN_RATE, n - at)
        x[at:at + m] += 3e4 * rng.standard_normal(m) * np.exp(-np.arange(m) * SCAN_RATE / (15.0 * rate))
        out.append(np.rint(x).astype(np.int32))
    return out


def host_resample(traces, a, t_samples):
    """The stage with NumPy and SciPy, trace by trace."""
    from scipy.signal import detrend, sosfilt

    out = np.empty((len(traces), t_samples))
    for i, (x, rec) in enumerate(zip(traces, a["records"])):
        r = dict(zip(RESAMPLE_FIELDS, (int(v) for v in rec)))
        u, d = r["up"], r["dec"]
        y = x.astype(np.float64)
        if u > 1:
            up = np.zeros((len(x) - 1) * u + 1)
            up[::u] = x
            for k in range(1, u):
                up[k::u] = (k / u) * x[1:] + ((u - k) / u) * x[:-1]
            y = np.concatenate([np.full(r["pad_left"], float(x[0])), up, np.full(r["pad_right"], float(x[-1]))])
        y = y[r["up_first"]:r["up_first"] + r["n_up"]]
        if d > 1:
            y = detrend(detrend(y, type="linear"), type="constant")
            off, m = (int(v) for v in a["taper_table"][r["taper"]])
            y[:m] *= a["taper_weights"][off:off + m]
            y[len(y) - m:] *= a["taper_weights"][off + m:off + 2 * m]
            sos = a["sos_lp"][r["lowpass"]]
            y = sosfilt(sos, sosfilt(sos, y)[::-1])[::-1][::d]
        out[i] = y[r["out_first"]:r["out_first"] + t_samples]
    return out


def median_ms(fn, repeats):
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms


def series_hash(results):
    h = hashlib.sha256()
    for triple in results:
        for series in triple:
            h.update(np.ascontiguousarray(series).tobytes())
    return h.hexdigest()[:16]


def child(path):
    """The two push_signals streams on the package and library of TREE, from the arrays the parent process left in
    `path`; one JSON line."""
    z = np.load(path, allow_pickle=False)
    a = {k[2:]: z[k] for k in z.files if k.startswith("a_")}
    onset = {k[2:]: (z[k] if z[k].ndim else z[k].item()) for k in z.files if k.startswith("o_")}
    fsmp, lsmp, available, rows, t_samples, steps, warm, repeats = (int(v) for v in z["ints"])
    case = argparse.Namespace(fsmp=fsmp, lsmp=lsmp, available=available)
    bounds = z["raw_bounds"]
    raws = [[w[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1)] for w in z["packed"]]
    eng = lib.Engine(0)
    eng.load_lut(z["traveltimes"])
    sig_ms, got = timed_stream(eng, case, rows, t_samples, list(z["signals"]), steps, warm, repeats, onset_stage=onset)
    host_ms, _ = timed_stream(eng, case, rows, t_samples, raws, steps, warm, repeats, onset_stage=onset,
                              prepare=lambda traces: host_resample(traces, a, t_samples))
    eng.close()
    print(json.dumps(dict(tree=str(TREE.name), sig_ms=sig_ms, host_ms=host_ms, series=series_hash(got))), flush=True)


def timed_stream(eng, case, rows, t_samples, windows, steps, warm, repeats, prepare=None, **stages):
    sd = StreamingDetector(eng, rows, t_samples, case.fsmp, case.lsmp, case.available, depth=3, steps_per_launch=1,
                           **stages)
    feed = (lambda i: windows[i % len(windows)]) if prepare is None else (lambda i: prepare(windows[i % len(windows)]))
    sd.run(feed(i) for i in range(warm))
    ms, got = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = sd.run(feed(i) for i in range(steps))
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    sd.close()
    return ms, got


def main():
    from quakemigrate_amd import synth
    from quakemigrate_amd.preprocess import OnsetStage, ResampleStage

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resample_bench.txt"))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the commit before the stage")
    ap.add_argument("--grid", nargs=3, type=int, default=[101, 101, 51])
    ap.add_argument("--t-samples", type=int, default=7500, help="output samples per window")
    ap.add_argument("--pool", type=int, default=3, help="distinct windows, cycled")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    if lib.qmlib.qm_device_count() < 1:
        raise SystemExit("resample_bench: no HIP device visible")
    # (a window is the scan's samples between the pads the table asks for: the scan is sized so that the window holds
    # --t-samples)
    probe = synth.make_case("C3", step=0, grid=tuple(args.grid), table=False)
    pads = probe.onsets.shape[1] - synth.CONFIGS["C3"]["n_samples"]
    cases = [synth.make_case("C3", step=s, grid=tuple(args.grid), n_samples=args.t_samples - pads, table=(s == 0))
             for s in range(args.pool)]
    case = cases[0]
    rows, t_samples = case.onsets.shape
    if t_samples != args.t_samples:
        raise SystemExit(f"resample_bench: windows of {t_samples} samples, {args.t_samples} asked for")
    n_p = rows // 2
    trace_row = list(range(n_p)) + [r for r in range(n_p, rows) for _ in range(2)]
    onset = OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 16.0, 2)},
                       sta_lta_windows={"P": (0.2, 1.0), "S": (0.2, 1.0)}, trace_row=trace_row,
                       trace_phase=["P"] * n_p + ["S"] * (2 * (rows - n_p)),
                       row_phase=["P"] * n_p + ["S"] * (rows - n_p), taper_pad=20)
    rates = raw_rates(len(trace_row))
    n_raw = [(t_samples - 1) * r // SCAN_RATE + 1 for r in rates]
    stage = ResampleStage(SCAN_RATE, rates, n_raw, [0.0] * len(rates), upfactor=5)
    a = stage.arrays(t_samples)
    raws = [raw_traces(200 + s, c, trace_row, rates, n_raw) for s, c in enumerate(cases)]
    packed = [np.concatenate(r) for r in raws]

    out = open(args.out, "w")

    def emit(**line):
        text = json.dumps(line)
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    eng = lib.Engine(0)
    eng.resample(packed[0], a)                              # (first call: allocations)
    kernel, call = [], []
    for skew in (1, 0):
        eng.config("preproc_skew", skew)
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            device = eng.resample(packed[0], a)
            if skew:
                call.append((time.perf_counter() - t0) * 1e3)
            ms.append(eng.last_kernel_ms())
        kernel.append(ms)
    eng.config("preproc_skew", 1)
    host_ms, host_all = median_ms(lambda: host_resample(raws[0], a, t_samples), args.host_repeats)
    host = host_resample(raws[0], a, t_samples)
    emit(**dict(
        section="stage", traces=len(rates), at_100_hz=rates.count(100), at_40_hz=rates.count(40),
        at_50_hz=rates.count(50), t_samples=t_samples, raw_samples=int(a["total_raw_samples"]), raw_dtype="int32",
        kernel_ms=round(float(np.median(kernel[0])), 4), kernel_ms_all=[round(v, 4) for v in kernel[0]],
        kernel_plain_ms=round(float(np.median(kernel[1])), 4), call_ms=round(float(np.median(call)), 4),
        call_ms_all=[round(v, 4) for v in call], host_scipy_ms=round(host_ms, 3),
        host_scipy_ms_all=[round(v, 3) for v in host_all],
        max_abs_diff=float(np.max(np.abs(device - host))), max_abs_value=float(np.max(np.abs(host)))))

    eng.load_lut(case.traveltimes)
    signals = [eng.resample(p, a) for p in packed]
    common = dict(onset_stage=onset, sampling_rate=SCAN_RATE)
    run = lambda windows, **kw: timed_stream(eng, case, rows, t_samples, windows, args.steps, args.warm,  # noqa: E731
                                             args.repeats, **kw, **common)
    raw_ms, raw_got = run(packed, resample_stage=stage)
    sig_ms, sig_got = run(signals)
    host_ms, _ = run(raws, prepare=lambda traces: host_resample(traces, a, t_samples))
    equal = all(all(np.array_equal(p, q) for p, q in zip(g, w)) for g, w in zip(raw_got, sig_got))
    eng.close()
    med = lambda v: round(float(np.median(v)), 4)           # noqa: E731
    emit(**dict(
        section="stream", grid=list(case.grid), rows=rows, traces=len(rates), t_samples=t_samples, steps_per_launch=1,
        steps=args.steps, warmup_launches=args.warm, repeats=args.repeats,
        ms_per_step_raw=med(raw_ms), ms_per_step_raw_all=[round(v, 4) for v in raw_ms],
        ms_per_step_signals=med(sig_ms), ms_per_step_signals_all=[round(v, 4) for v in sig_ms],
        ms_per_step_signals_host_resampled=med(host_ms),
        ms_per_step_signals_host_resampled_all=[round(v, 4) for v in host_ms], equal=bool(equal)))
    if not equal:
        raise SystemExit("resample_bench: the raw stream differs from the signal stream")
    if args.parent_tree:
        oa = onset.arrays(t_samples, SCAN_RATE)
        bounds = np.concatenate([[0], np.cumsum(n_raw)])
        with tempfile.TemporaryDirectory() as tmp:
            path = str(pathlib.Path(tmp) / "inputs.npz")
            np.savez(path, traveltimes=case.traveltimes, signals=np.stack(signals), packed=np.stack(packed),
                     raw_bounds=bounds, ints=np.array([case.fsmp, case.lsmp, case.available, rows, t_samples, args.steps,
                                                       args.warm, args.repeats]),
                     **{"a_" + k: np.asarray(v) for k, v in a.items()}, **{"o_" + k: np.asarray(v) for k, v in oa.items()})
            done = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), "--child", args.parent_tree,
                                   path], check=True, capture_output=True, text=True, timeout=600)
        got = json.loads(done.stdout.strip().splitlines()[-1])
        emit(section="parent", tree=got["tree"], steps=args.steps, repeats=args.repeats,
             parent_ms_per_step_signals=med(got["sig_ms"]), parent_ms_per_step_signals_all=[round(v, 4) for v in got["sig_ms"]],
             parent_ms_per_step_signals_host_resampled=med(got["host_ms"]),
             parent_ms_per_step_signals_host_resampled_all=[round(v, 4) for v in got["host_ms"]],
             parent_equal=bool(got["series"] == series_hash(sig_got)))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 2])
    else:
        main()
