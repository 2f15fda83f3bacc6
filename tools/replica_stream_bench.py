# -*- coding: utf-8 -*-
"""
The continuous detect stream on engine replicas (include/qmhip.h: qm_stream_create_replicas) beside the stream on
one Engine: a stream of pre-made, seeded, logged windows through ``StreamingDetector`` for ``Engine(0)``,
``EngineReplicas([0])``, ``[0, 0]`` and -- on a box with more GPUs -- ``range(G)``, in two configurations: C3 at
one timestep per launch (slots above 1 MB: the copy path) and C1 at eight (the pull path).  The host clock runs
from the first push to the last pop of the timed steps (the pop synchronises).  Each stream first runs past its
first 256 launches (the one-off stall of the command processor around launch 180 of a process's first stream that
bench.py's step_with_copies leg warms past).  Every timed step's three series must equal the Engine stream's
(array_equal).  ``digest_ms``: the first ``table_digest()`` of the configuration (every replica's), host clock
around a synchronising call.  One JSON line per (configuration, engine set).  ``--stamps``: "stream_stamps" on every engine; each lane's digest of its launches is
read from stderr and the largest gap between launches reported.

    python tools/replica_stream_bench.py [--c3-steps 48] [--c1-steps 800] [--pool 6] [--warm 256] [--stamps]
"""

import argparse
import json
import os
import pathlib
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from quakemigrate_amd import synth  # noqa: E402
from quakemigrate_amd.core import lib  # noqa: E402
from quakemigrate_amd.stream import StreamingDetector  # noqa: E402


def windows(name, pool, **size):
    cases = [synth.make_case(name, step=s, table=(s == 0), **size) for s in range(pool)]
    wins = [np.ascontiguousarray(np.log(np.clip(c.onsets, 0.01, np.inf))) for c in cases]
    return cases[0], wins


def close_reading_stderr(sd):
    """Close the stream; with "stream_stamps" on, each lane prints its digest to stderr then: the largest gaps."""
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            sd.close()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    sys.stderr.write(text)
    return [float(v) for v in re.findall(r"gap between launches us median [0-9.]+ p90 [0-9.]+ max ([0-9.]+)", text)]


def measure(eng, case, wins, k, steps, warm, stamps):
    """(ms per step, the timed steps' results, digest ms, largest launch gaps in us)."""
    t0 = time.perf_counter()
    eng.table_digest()
    digest_ms = (time.perf_counter() - t0) * 1e3
    if stamps:
        eng.config("stream_stamps", 1)
    rows, t_samples = wins[0].shape
    sd = StreamingDetector(eng, rows, t_samples, case.fsmp, case.lsmp, case.available, depth=3, steps_per_launch=k)
    sd.run(wins[i % len(wins)] for i in range(warm * k))
    t0 = time.perf_counter()
    got = sd.run(wins[i % len(wins)] for i in range(steps))
    ms = (time.perf_counter() - t0) / steps * 1e3
    gaps = close_reading_stderr(sd)
    return ms, got, digest_ms, gaps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--c3-steps", type=int, default=48)
    ap.add_argument("--c1-steps", type=int, default=800)
    ap.add_argument("--pool", type=int, default=6, help="distinct windows, cycled")
    ap.add_argument("--warm", type=int, default=256, help="launches run before the clock starts")
    ap.add_argument("--stamps", action="store_true")
    args = ap.parse_args()
    n_dev = lib.qmlib.qm_device_count()
    if n_dev < 1:
        raise SystemExit("replica_stream_bench: no HIP device visible")
    sets = [None, [0], [0, 0]] + ([list(range(n_dev))] if n_dev > 1 else [])
    for name, k, steps in (("C3", 1, args.c3_steps), ("C1", 8, args.c1_steps)):
        case, wins = windows(name, args.pool)
        head = dict(config=name, grid=list(case.grid), rows=int(wins[0].shape[0]), n_samples=case.n_samples,
                    steps_per_launch=k, depth=3, steps=steps, mb_per_step=round(wins[0].nbytes / 1e6, 3),
                    devices_visible=n_dev)
        want, base_ms = None, None
        for devices in sets:
            eng = lib.Engine(0) if devices is None else lib.EngineReplicas(devices)
            eng.load_lut(case.traveltimes)
            ms, got, digest_ms, gaps = measure(eng, case, wins, k, steps, args.warm, args.stamps)
            eng.close()
            line = dict(head, engines="Engine(0)" if devices is None else f"EngineReplicas({devices})",
                        ms_per_step=round(ms, 4), warmup_launches=args.warm, digest_ms=round(digest_ms, 3))
            if devices is None:
                want, base_ms = got, ms
            else:
                same = len(got) == len(want) and all(
                    all(np.array_equal(x, y) for x, y in zip(g, w)) for g, w in zip(got, want))
                line.update(vs_engine=round(ms / base_ms, 4), equal_to_engine_stream=bool(same))
                if not same:
                    print(json.dumps(line), flush=True)
                    raise SystemExit(f"replica_stream_bench: {line['engines']} differs from the Engine stream")
            if gaps:
                line["max_gap_between_launches_us"] = max(gaps)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
