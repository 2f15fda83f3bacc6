# -*- coding: utf-8 -*-
"""
The amplitude stage (include/qmhip.h: qm_engine_measure_amplitudes) beside the SciPy loop it replaces.

Traces: 30 x 3 and 400 x 3 component traces of 80 s at 100 Hz (seeded noise with a P and an S wavelet), the band-pass
on (2 - 16 Hz, four corners), three windows each: 5 s of noise, a P and an S window of a few seconds.

Per shape one JSON line:
  kernel_ms            the two launches alone: HIP events around them (qm_engine_last_kernel_ms), median of `--calls`
  wall_host_ms         host clock around Engine.measure_amplitudes with the traces on the host: copies in, launches,
                       copies back, synchronise; median
  wall_device_ms       the same with the traces resident on the device
  windows_only_ms      kernel_ms of the same call without the filter: the window launch alone
  scipy_loop_ms        the reference's per-trace work on this machine's CPU, one trace after the other as
                       Amplitude.get_amplitudes does, as far as the stage takes it over: scipy.signal.detrend, taper,
                       sosfilt; per window detrend, two find_peaks, the pairing rules and the RMS (the filter gain by
                       sosfreqz stays on the host on both sides and is not timed; obspy's and pandas' own overheads
                       are not in it either); median of `--host-repeats` passes
  ratio                scipy_loop_ms / wall_host_ms

    python tools/amplitude_bench.py [--calls 10] [--host-repeats 10] [--out profiles/amplitude_bench.txt]
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
import amplitudes_ref as ar  # noqa: E402
from quakemigrate_amd.core import lib  # noqa: E402
from quakemigrate_amd.preprocess import butter_bandpass_sos, cosine_taper_sides  # noqa: E402

RATE, SECONDS = 100.0, 80.0
STATIONS = (30, 400)


def family(n_stations, seed=3):
    rng = np.random.default_rng(seed)
    n = int(RATE * SECONDS)
    t = np.arange(n) / RATE
    traces, recs = [], []
    for s in range(n_stations):
        p_at, s_at = 20.0 + 10.0 * rng.random(), 35.0 + 15.0 * rng.random()
        for _ in range(3):
            x = 3e-7 * rng.standard_normal(n) + 1e-9 * t
            for j, at in enumerate((p_at, s_at)):
                since = np.clip(t - at, 0.0, None)
                x += (1 + 2 * j) * 2e-5 * since * np.exp(-2.0 * since) * np.sin(2 * np.pi * (6.0 - j) * since)
            k = len(traces)
            traces.append(x)
            p0, p1, s0, s1 = (int(v * RATE) for v in (p_at - 1.5, p_at + 1.5, s_at - 2.0, s_at + 4.0))
            recs += [[k, p0 - 500, p0, 0], [k, p0, p1, 1], [k, s0, s1, 1]]
    packed, offsets = ar.pack(traces)
    left, right = cosine_taper_sides(n)
    sos = butter_bandpass_sos(2.0, 16.0, RATE, 4)
    trecs = np.stack([offsets, np.full(len(traces), n), np.zeros(len(traces)), np.zeros(len(traces))], axis=1)
    return dict(traces=traces, packed=packed, trecs=trecs.astype(np.int64), recs=np.array(recs, dtype=np.int64),
                sos=sos[None], table=np.array([[0, len(left)]], dtype=np.int32), weights=np.concatenate([left, right]),
                left=left, right=right)


def scipy_loop_ms(fam):
    from scipy import signal

    sos = fam["sos"][0]
    t0 = time.perf_counter()
    measured = 0
    for k, x in enumerate(fam["traces"]):
        y = signal.detrend(x, type="linear")
        y[:len(fam["left"])] *= fam["left"]
        y[len(y) - len(fam["right"]):] *= fam["right"]
        y = signal.sosfilt(sos, y)
        for _, lo, hi, kind in fam["recs"][3 * k:3 * k + 3]:
            w = signal.detrend(y[lo:hi], type="linear")
            if kind == 1:
                peaks, troughs = signal.find_peaks(w, prominence=0.0)[0], signal.find_peaks(-w, prominence=0.0)[0]
                measured += ar.pair(w, peaks, troughs)[0] == 0
            np.sqrt(np.mean(np.square(w)))
    return (time.perf_counter() - t0) * 1e3, measured


def bench(eng, n_stations, calls, host_repeats):
    import torch

    fam = family(n_stations)
    kw = dict(sos=fam["sos"], taper_table=fam["table"], taper_weights=fam["weights"])
    d_x = torch.from_numpy(fam["packed"]).to(f"cuda:{eng.device}")
    values, index = eng.measure_amplitudes(fam["packed"], fam["trecs"], fam["recs"], **kw)      # warm-up
    eng.measure_amplitudes(d_x, fam["trecs"], fam["recs"], **kw)
    kernel, wall_host, wall_dev, windows = [], [], [], []
    plain = fam["trecs"].copy()
    plain[:, 2:] = -1
    for _ in range(calls):
        t0 = time.perf_counter()
        eng.measure_amplitudes(fam["packed"], fam["trecs"], fam["recs"], **kw)
        wall_host.append((time.perf_counter() - t0) * 1e3)
        kernel.append(eng.last_kernel_ms())
        t0 = time.perf_counter()
        eng.measure_amplitudes(d_x, fam["trecs"], fam["recs"], **kw)
        wall_dev.append((time.perf_counter() - t0) * 1e3)
        eng.measure_amplitudes(d_x, plain, fam["recs"])
        windows.append(eng.last_kernel_ms())
    scipy_loop_ms(fam)
    host = [scipy_loop_ms(fam) for _ in range(host_repeats)]
    loop = float(np.median([h[0] for h in host]))
    out = dict(stations=n_stations, traces=3 * n_stations, samples=int(RATE * SECONDS), windows=len(fam["recs"]),
               kernel_ms=round(float(np.median(kernel)), 4), kernel_ms_min_max=[round(min(kernel), 4), round(max(kernel), 4)],
               windows_only_ms=round(float(np.median(windows)), 4),
               wall_host_ms=round(float(np.median(wall_host)), 4), wall_device_ms=round(float(np.median(wall_dev)), 4),
               scipy_loop_ms=round(loop, 3), ratio=round(loop / float(np.median(wall_host)), 1),
               measured=int(np.sum(index[fam["recs"][:, 3] == 1, 0] == 0)), scipy_measured=host[0][1])
    return json.dumps(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "amplitude_bench.txt"))
    a = ap.parse_args()
    if lib.qmlib.qm_device_count() < 1:
        raise SystemExit("amplitude_bench: no HIP device visible")
    eng = lib.Engine(0)
    lines = []
    for n in STATIONS:
        lines.append(bench(eng, n, a.calls, a.host_repeats))
        print(lines[-1], flush=True)
    eng.close()
    pathlib.Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
