# -*- coding: utf-8 -*-
"""
The .scanmseed codec (include/qmhip.h: qm_engine_scanmseed_encode / _decode) on a day file beside the Python codec.

Series: a day at 50 Hz, 4 320 000 samples on each of the five channels, seeded.  Detect-like widths: COA and COA_N are
random walks with uniform steps of +-300 counts (10-bit differences, a few narrower); X, Y and Z hold a grid node's
coordinate for runs of 1 .. 200 samples and jump by +-(1 .. 40) cells of 500 000 (X, Y) or 250 000 (Z) counts between
them (zeros, i.e. 4-bit words of seven, broken by single 30-bit differences).  The float64 flavour gets the same series
divided by the channels' factors.

One JSON line per case, medians of `--calls` calls after a warm-up:
  wall_ms      host clock around the Engine call: copies in, launches, the read-back of counts, copies back
  sequence_ms  HIP events around the launch sequence (qm_engine_last_kernel_ms)
  stage_us     HIP events around every launch ("scanmseed_ns_<stage>")
Cases: encode from int32 / float64 on the host and from a device-resident int32 tensor; decode (int32 and descaled
float64) to the host and to the device; then the whole front end once each way (encode_scanmseed with the headers'
Python loop, read_scanmseed with header parsing), checked against each other.
Python codec: this build's linearised encoder and the decoder on the full day (once), and -- `--parent-tree DIR`, a
checkout of the parent commit, e.g. `git worktree add parent_build HEAD~1` -- the parent's codec in a child process at
216 000 and 108 000 samples per channel; its day figure is an EXTRAPOLATION: t = a n + b n^2 through the two points for
the encoder (it converts the whole rest of the trace for every record), n / 216 000 times the measurement for the
decoder.

    python tools/scanmseed_bench.py [--calls 10] [--parent-tree parent_build] [--no-python] > profiles/scanmseed_bench.txt
"""

import argparse
import datetime as dt
import json
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from quakemigrate_amd import scanmseed as sm  # noqa: E402

RATE, DAY = 50, 86400 * 50
T0 = dt.datetime(2014, 8, 24)
ENCODE_STAGES = ("quantise", "scan", "compose", "pack", "frame")
PARENT_SAMPLES = (108_000, 216_000)


def day_series(n=DAY, seed=50):
    rng = np.random.default_rng(seed)
    rows = []
    for base in (200_000, 150_000):                             # COA, COA_N: +-300 steps, kept positive
        walk = np.cumsum(rng.integers(-300, 301, n))
        rows.append(base + walk - walk.min())
    for cell in (500_000, 500_000, 250_000):                    # X, Y, Z: a node's coordinate, held, then a jump
        runs = rng.integers(1, 201, n // 50)
        runs = runs[:np.searchsorted(np.cumsum(runs), n) + 1]
        node = np.clip(np.cumsum(rng.integers(-40, 41, len(runs))), -1000, 1000)
        rows.append(np.repeat(node * cell, runs)[:n])
    return np.ascontiguousarray(np.stack(rows).astype(np.int32))


def median_calls(eng, call, calls, stages):
    call()                                                      # warm-up: code objects, buffers
    wall, seq, stage = [], [], {s: [] for s in stages}
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        seq.append(eng.last_kernel_ms())
        for s in stages:
            stage[s].append(eng.get(f"scanmseed_ns_{s}") / 1e3)
    return dict(wall_ms=round(float(np.median(wall)), 3), sequence_ms=round(float(np.median(seq)), 3),
                stage_us={s: round(float(np.median(v)), 1) for s, v in stage.items() if np.median(v) > 0})


PARENT_CHILD = """
import sys, time, json, datetime as dt
import numpy as np
sys.path.insert(0, sys.argv[1])
from quakemigrate_amd import scanmseed as sm
x = np.load(sys.argv[2])
out = {}
for n in (%d, %d):
    t0 = time.perf_counter()
    blobs = [sm.write_trace(sm.Trace(ch, "NW", dt.datetime(2014, 8, 24), 50.0, row[:n])) for ch, row in zip(sm.CHANNELS, x)]
    enc = time.perf_counter() - t0
    t0 = time.perf_counter()
    for blob in blobs:
        for _ in sm.read_records(blob):
            pass
    out[n] = (enc, time.perf_counter() - t0)
print(json.dumps(out))
""" % PARENT_SAMPLES


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--samples", type=int, default=DAY)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--no-python", action="store_true")
    a = ap.parse_args()
    import torch

    from quakemigrate_amd.core import lib

    if lib.qmlib.qm_device_count() < 1:
        raise SystemExit("scanmseed_bench: no HIP device visible")
    eng = lib.Engine(0)
    n = a.samples
    x = day_series(n)
    factors = np.array([sm.scale_factors(1000.0)[ch] for ch in sm.CHANNELS])
    clips = [sm.COA_CLIP, sm.COA_CLIP, None, None, None]
    xf = np.ascontiguousarray(x / factors[:, None])
    assert np.array_equal(np.round(xf * factors[:, None]).astype(np.int32), x)
    xd = torch.from_numpy(x).to(f"cuda:{eng.device}")
    series = {ch: x[c] for c, ch in enumerate(sm.CHANNELS)}

    out = eng.scanmseed_encode(x)
    print(json.dumps(dict(series="day", samples_per_channel=n, records=[int(v) for v in out["n_records"]],
                          file_bytes=int(out["records"].nbytes))), flush=True)
    for name, call in (("encode, int32 on the host", lambda: eng.scanmseed_encode(x)),
                       ("encode, float64 on the host", lambda: eng.scanmseed_encode(xf, factors, clips)),
                       ("encode, int32 on the device", lambda: eng.scanmseed_encode(xd))):
        print(json.dumps(dict(case=name, **median_calls(eng, call, a.calls, ENCODE_STAGES))), flush=True)
    assert np.array_equal(eng.scanmseed_encode(xf, factors, clips)["records"], out["records"])
    records, counts = out["records"], out["rec_count"]
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rec_factor = np.repeat(factors, out["n_records"])
    for name, device in (("decode to the host", False), ("decode to the device", True)):
        call = lambda: eng.scanmseed_decode(records, counts, offsets, 5 * n, rec_factor=rec_factor, device=device)  # noqa: E731
        print(json.dumps(dict(case=name, **median_calls(eng, call, a.calls, ("decode",)))), flush=True)
    ints, _ = eng.scanmseed_decode(records, counts, offsets, 5 * n)
    assert np.array_equal(ints.reshape(5, n), x)

    # the whole front end, once each way
    t0 = time.perf_counter()
    blob = sm.encode_scanmseed(T0, RATE, series, engine=eng)
    front_enc = time.perf_counter() - t0
    path = pathlib.Path(tempfile.gettempdir()) / "scanmseed_bench_day.scanmseed"
    path.write_bytes(blob)
    t0 = time.perf_counter()
    _, _, cols = sm.read_scanmseed(path, 1000.0, engine=eng, device=True)
    front_dec = time.perf_counter() - t0
    assert all(np.array_equal(np.asarray(cols["int"][ch].cpu() if hasattr(cols["int"][ch], "cpu") else cols["int"][ch]),
                              series[ch]) for ch in sm.CHANNELS)
    print(json.dumps(dict(case="front end: encode_scanmseed(engine) with the headers' Python loop; read_scanmseed(engine, "
                               "device=True) with header parsing", encode_ms=round(front_enc * 1e3, 1),
                          decode_ms=round(front_dec * 1e3, 1))), flush=True)

    if not a.no_python:
        t0 = time.perf_counter()
        py_blob = sm.encode_scanmseed(T0, RATE, series)
        py_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        for _ in sm.read_records(py_blob):
            pass
        py_dec = time.perf_counter() - t0
        print(json.dumps(dict(case="Python codec of this build (linearised encoder), the full day, this box's CPU",
                              encode_s=round(py_enc, 2), decode_s=round(py_dec, 2),
                              bytes_equal_to_the_device=bool(py_blob == blob))), flush=True)
    path.unlink()
    if a.parent_tree:
        tree = pathlib.Path(a.parent_tree).resolve()
        if not (tree / "quakemigrate_amd" / "scanmseed.py").is_file():
            raise SystemExit(f"scanmseed_bench: {tree} holds no quakemigrate_amd/scanmseed.py")
        npy = pathlib.Path(tempfile.gettempdir()) / "scanmseed_bench_parent.npy"
        np.save(npy, x[:, :PARENT_SAMPLES[1]])
        got = json.loads(subprocess.check_output([sys.executable, "-c", PARENT_CHILD, str(tree), str(npy)], text=True))
        npy.unlink()
        (n1, (e1, d1)), (n2, (e2, d2)) = sorted((int(k), v) for k, v in got.items())
        b = (e2 / n2 - e1 / n1) / (n2 - n1)                     # t = a n + b n^2 through the two points
        a_lin = e1 / n1 - b * n1
        print(json.dumps(dict(case="Python codec of the parent commit, child process, this box's CPU, five channels",
                              measured={str(n1): dict(encode_s=round(e1, 2), decode_s=round(d1, 2)),
                                        str(n2): dict(encode_s=round(e2, 2), decode_s=round(d2, 2))},
                              EXTRAPOLATED_to_the_day=dict(samples_per_channel=n,
                                                           encode_s=round(a_lin * n + b * n * n, 0),
                                                           decode_s=round(d2 * n / n2, 1),
                                                           model="encode a n + b n^2 through the two points, decode "
                                                                 "linear"))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
