# -*- coding: utf-8 -*-
"""
The trigger stage (include/qmhip.h: qm_engine_trigger) on a day of coalescence beside its NumPy restatement on the
host.

Series: a day at 50 Hz (4 320 000 samples) of quantised noise with bursts on it (several hundred events), and the
worst case for the run kernels, flags alternating sample by sample (n / 2 candidates).  MAD threshold over 3600 s,
smoothing on (sigma 0.2 s, truncated at 4 sigma), as a user of the reference's Trigger would set a noisy day up.

Per case one JSON line:
  wall_ms              host clock around Engine.trigger_series: copies in, the launch sequence with its two read-backs
                       of counts, copies back; median of `--calls` calls
  sequence_ms          HIP events around the launch sequence (qm_engine_last_kernel_ms), median
  stage_us             per stage, HIP events around its kernels ("trigger_timing": smooth, stats, runs = count + scan,
                       compact, peaks, merge), median
  host_ms              tests/trigger_ref.trigger_series on this machine's CPU, once (`--no-host` leaves it out: the
                       restatement loops over the candidates in Python and takes minutes on the alternating case)
  candidates, events

    python tools/trigger_bench.py [--calls 20] [--no-host] > profiles/trigger_bench.txt
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
import trigger_ref as tr  # noqa: E402
from quakemigrate_amd.core import lib  # noqa: E402

RATE, DAY = 50, 86400 * 50
PERIOD, MW, MEI = 20_000_000, 2_000_000_000, 4_000_000_000
STAGES = ("smooth", "stats", "runs", "compact", "peaks", "merge")


def noisy_day(n_bursts=600, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.gamma(2.0, 0.5, (2, DAY))
    for at in rng.integers(0, DAY - 400, n_bursts):
        x[:, at:at + 300] += rng.uniform(6.0, 20.0) * np.hanning(300)
    return np.round(x, 5)


def alternating_day():
    x = np.ones((2, DAY))
    x[:, ::2] = 3.0
    return x


def bench(eng, name, x, calls, host, **kw):
    coa, coa_n = np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1])
    eng.config("trigger_timing", 1)
    out = eng.trigger_series(coa, coa_n, PERIOD, MW, MEI, max_events=DAY, **kw)         # warm-up: code objects, buffers
    wall, seq, stage = [], [], {s: [] for s in STAGES}
    for _ in range(calls):
        t0 = time.perf_counter()
        eng.trigger_series(coa, coa_n, PERIOD, MW, MEI, max_events=DAY, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        seq.append(eng.last_kernel_ms())
        for s in STAGES:
            stage[s].append(eng.get(f"trigger_ns_{s}") / 1e3)
    eng.config("trigger_timing", 0)
    line = dict(case=name, samples=len(coa), candidates=out["n_candidates"], events=out["n_events"],
                wall_ms=round(float(np.median(wall)), 3), sequence_ms=round(float(np.median(seq)), 3),
                stage_us={s: round(float(np.median(v)), 1) for s, v in stage.items()})
    if host:
        t0 = time.perf_counter()
        ref = tr.trigger_series(coa, coa_n, kw.get("trigger_on", 0), kw.get("weights"),
                                {"static": 0, "mad": 1, "median_ratio": 2}[kw.get("method", "static")],
                                kw.get("value", 1.5), kw.get("chunk_samples", 1), PERIOD, MW, MEI)
        line["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        line["equal"] = bool(np.array_equal(ref["events_i"], out["events_i"]))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if lib.qmlib.qm_device_count() < 1:
        raise SystemExit("trigger_bench: no HIP device visible")
    eng = lib.Engine(0)
    _, w = tr.gaussian_weights(0.2 * RATE, 4.0)
    bench(eng, "noisy day, MAD 3600 s x 8, smoothing on", noisy_day(), a.calls, not a.no_host, method="mad", value=8.0,
          chunk_samples=3600 * RATE, weights=w)
    bench(eng, "noisy day, static 4.0", noisy_day(), a.calls, not a.no_host, value=4.0)
    bench(eng, "alternating flags, static 2.0", alternating_day(), max(a.calls // 4, 1), False, value=2.0)
    eng.close()


if __name__ == "__main__":
    main()
