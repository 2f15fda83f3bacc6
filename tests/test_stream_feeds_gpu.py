# -*- coding: utf-8 -*-
"""
Which call a stream accepts in which state, and what it says where it refuses, pinned as the library answered BEFORE
the refusals came from one feed table (csrc/qm_stream.hip: ``kFeedTable``, ``may_set``, ``may_push``).

Seven calls, always with valid, full-size arguments -- the three ``set_*`` calls and the four pushes of
``StreamingDetector`` -- so a call accepted by mistake computes on zeros and never reads past a buffer.  A script is a
sequence of them on a fresh stream made without stages: every sequence of 1 to 3 calls, and every sequence of 4 that
starts with ``set_onset_stage`` (742 scripts).  The streams hold two timesteps per launch and two slots, so a script's
first push sits in a half-filled slot -- the ``fill_n > 0`` half of "before the first push" -- and its second launches.
After each call the script records ``"ok"``, ``"full"`` (a push that found every slot un-popped) or the exception's
class and full text.

tests/golden/stream_feeds_parent.json holds every script's outcomes; this file wrote it from the parent commit's
library (``QM_HIP_LIB=/path/to/libqmhip.so python tests/test_stream_feeds_gpu.py tests/golden/stream_feeds_parent.json COMMIT``).
"""

import itertools
import json
import sys
import time

import numpy as np
import pytest

from conftest import ROOT                          # (first: it puts the repository root on sys.path)

pytestmark = pytest.mark.gpu
GOLDEN_PATH = ROOT / "tests" / "golden" / "stream_feeds_parent.json"

ROWS, T, FSMP, LSMP, RATE = 4, 256, 16, 16, 50
TRACE_ROW = (0, 1, 2, 2, 3, 3)                      # 4 rows (2 P, 2 S), 6 traces
RAW_RATE = (50, 100, 40, 100, 50, 40)               # pass-through, d = 2, u = 5 then d = 4
SETS = ("set_onset_stage", "set_resample_stage", "set_segment_feed")
PUSHES = ("push", "push_signals", "push_raw", "push_segments")
CALLS = SETS + PUSHES


def scripts():
    out = [s for n in (1, 2, 3) for s in itertools.product(CALLS, repeat=n)]
    return out + [(SETS[0],) + s for s in itertools.product(CALLS, repeat=3)]


def arguments():
    """Every call's arguments, made once: the stages as the dicts the C ABI takes, the pushes' zero-filled inputs."""
    from quakemigrate_amd.preprocess import OnsetStage, ResampleStage, plan_segments

    n = len(TRACE_ROW)
    onset = OnsetStage(filters={"P": (2.0, 16.0, 2), "S": (2.0, 12.0, 2)},
                       sta_lta_windows={"P": (0.2, 1.0), "S": (0.3, 1.5)}, trace_row=TRACE_ROW,
                       trace_phase=tuple("PPSSSS"), row_phase=tuple("PPSS"), taper_pad=20, fill_gaps=True)
    resample = ResampleStage(RATE, RAW_RATE, [(T - 1) * r // RATE + 1 for r in RAW_RATE], [0.0] * n, upfactor=5)
    records, weights = plan_segments(T, n, [(i, 0, T) for i in range(n)])      # one segment per trace
    return {
        "set_onset_stage": (onset.arrays(T, RATE),),
        "set_resample_stage": (resample.arrays(T), np.int32),
        "set_segment_feed": (),
        "push": (np.zeros((ROWS, T)),),
        "push_signals": (np.zeros((n, T)),),
        "push_raw": (np.zeros(resample.total_raw_samples, dtype=np.int32),),
        "push_segments": (np.zeros((n, T)), records, weights),
    }


def outcomes(lib):
    """script (call names joined by ">") -> the outcome of each of its calls, on one engine."""
    from quakemigrate_amd.stream import StreamingDetector

    args = arguments()
    table = np.random.default_rng(7).integers(0, LSMP + 1, size=(5, 4, 3, ROWS)).astype(np.int32)
    got = {}
    eng = lib.Engine(0)
    try:
        eng.load_lut(table)
        for script in scripts():
            det = StreamingDetector(eng, ROWS, T, FSMP, LSMP, ROWS, depth=2, steps_per_launch=2)
            try:
                trail = []
                for call in script:
                    try:
                        accepted = getattr(det, call)(*args[call])
                        trail.append("full" if call in PUSHES and not accepted else "ok")
                    except Exception as e:  # noqa: BLE001
                        trail.append(f"{type(e).__name__}: {e}")
                got[">".join(script)] = trail
            finally:
                det.close()
    finally:
        eng.close()
    return got


def test_every_script_ends_as_it_did_on_the_parent():
    from quakemigrate_amd.core import lib

    assert lib.qmlib.qm_device_count() >= 1, "no HIP device visible"
    golden = json.loads(GOLDEN_PATH.read_text())["scripts"]
    assert list(golden) == [">".join(s) for s in scripts()] and len(golden) == 742
    t0 = time.perf_counter()
    got = outcomes(lib)
    print(f"{len(got)} scripts in {time.perf_counter() - t0:.2f} s")
    differing = [s for s in golden if got[s] != golden[s]]
    assert not differing, (f"{len(differing)} scripts differ from the parent's; the first: {differing[0]}\n"
                           f"  parent: {golden[differing[0]]}\n  now:    {got[differing[0]]}")
    # (the record is not vacuous: calls are accepted, refused and in every one of the five forms)
    said = {text for trail in golden.values() for text in trail}
    for form in ("ok", "has no", "comes first", "already (it is set once)", "is set before the first push",
                 "one stream, one kind of input"):
        assert any(form in text for text in said), form


if __name__ == "__main__":
    from quakemigrate_amd.core import lib as _lib

    t0 = time.perf_counter()
    record = {"commit": sys.argv[2] if len(sys.argv) > 2 else None,
              "case": f"{ROWS} rows, {len(TRACE_ROW)} traces, windows of {T} samples; streams of 2 slots x 2 steps",
              "scripts": outcomes(_lib)}
    print(f"{len(record['scripts'])} scripts in {time.perf_counter() - t0:.2f} s")
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(record, indent=0) + "\n")
    print(f"recorded in {sys.argv[1]}")
