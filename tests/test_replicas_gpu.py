# -*- coding: utf-8 -*-
"""
Engine replicas on the GPU (include/qmhip.h: qm_engine_table_digest, qm_stream_create_replicas;
quakemigrate_amd.core.EngineReplicas): the continuous pipeline split by time over several engines that hold the
same table.  ``[0, 0]`` is two replicas on GPU 0, the form a one-GPU box can test.  Every timestep is the single
engine's bit for bit: the same kernels on the same table.
"""

import itertools

import numpy as np
import pytest

from conftest import load_golden
from quakemigrate_amd import synth

pytestmark = pytest.mark.gpu
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    assert _lib.qmlib.qm_device_count() >= 1, "no HIP device visible"
    return _lib


DEVICE_LISTS = [
    pytest.param([0], id="0"),
    pytest.param([0, 0], id="0,0"),
    pytest.param([0, 0, 0], id="0,0,0"),
    pytest.param("multi", id="multi-gpu"),
]


def _devices(spec):
    if spec != "multi":
        return spec
    from quakemigrate_amd.core import lib as _lib

    n = _lib.qmlib.qm_device_count()
    if n < 2:
        pytest.skip("one HIP device: the multi-GPU list needs two or more")
    return list(range(min(n, 3)))


# ------------------------------------------------------------------------------ digest
def _mix(z):
    """splitmix64's finalizer on uint64 arrays (wrapping)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _mix_int(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def np_digest(table, node_offset=0):
    """qm_engine_table_digest restated: table as lut_download returns it, (nx, ny, nz, n_rows)."""
    nx, ny, nz, rows = table.shape
    v = np.ascontiguousarray(table, dtype=np.int32).reshape(-1).view(np.uint32).astype(np.uint64)
    i = np.arange(v.size, dtype=np.uint64)
    h = int(_mix(_mix(i) + v).sum(dtype=np.uint64))
    for f in (nx, ny, nz, rows, node_offset):
        h = _mix_int((h + (f & MASK)) & MASK)
    return h


def _case(grid, rows=12, n_samples=300, step=2):
    if grid == "flat":
        c = synth.make_case("C3", step=step, grid=(21, 17, 18), rows=rows, n_samples=n_samples)
        c.traveltimes = np.ascontiguousarray(c.traveltimes.reshape(1, 1, -1, c.traveltimes.shape[-1]))
        return c
    return synth.make_case("C3", step=step, grid=grid, rows=rows, n_samples=n_samples)


@pytest.mark.parametrize("grid", [pytest.param((21, 17, 18), id="21x17x18"), pytest.param((2, 3, 20), id="2x3x20"),
                                  pytest.param("flat", id="flat")])
def test_digest_equals_numpy_restatement(lib, grid):
    tt = _case(grid).traveltimes
    eng = lib.Engine(0)
    eng.load_lut(tt)
    d = eng.table_digest()
    assert d == np_digest(eng.download_lut()) == np_digest(tt)
    assert eng.get("table_digests") == 1
    assert eng.table_digest() == d and eng.get("table_digests") == 1        # cached
    # another node offset is another digest (the shape fields are folded in)
    eng.load_lut(tt, node_offset=7)
    assert eng.table_digest() == np_digest(tt, node_offset=7) != d
    eng.close()


def test_digest_identifies_the_table(lib):
    tt = _case((21, 17, 18)).traveltimes
    a, b = lib.Engine(0), lib.Engine(0)
    a.load_lut(tt)
    b.load_lut(tt)
    assert a.table_digest() == b.table_digest()
    other = tt.copy()
    other[3, 4, 5, 6] += 1
    b.load_lut(other)
    assert b.table_digest() != a.table_digest()
    assert b.table_digest() == np_digest(other)
    # a table served on the device equals the same int32 table loaded
    rate = 50
    rng = np.random.default_rng(11)
    grids = [rng.uniform(0.0, 3.0, (9, 8, 7)) for _ in range(5)]
    a.set_traveltime_grids(grids)
    a.serve(rate, [0, 2, 4])
    b.load_lut(np.ascontiguousarray(np.rint(np.stack([grids[r] * rate for r in (0, 2, 4)], axis=-1)),
                                    dtype=np.int32))
    assert np.array_equal(a.download_lut(), b.download_lut())
    assert a.table_digest() == b.table_digest()
    a.close()
    b.close()


def test_digest_survives_a_table_select_round_trip(lib):
    tt = _case((21, 17, 18)).traveltimes
    other = np.ascontiguousarray(tt[::-1])
    eng = lib.Engine(0)
    assert not eng.select_table("A")
    eng.load_lut(tt)
    da = eng.table_digest()
    assert not eng.select_table("B")
    eng.load_lut(other)
    db = eng.table_digest()
    assert db != da and eng.get("table_digests") == 2
    assert eng.select_table("A")
    assert eng.table_digest() == da
    assert eng.select_table("B")
    assert eng.table_digest() == db
    assert eng.get("table_digests") == 2                                     # the parked tables were not rehashed
    eng.close()


# ------------------------------------------------------------------------------ the stream
GRID, ROWS, NS, STEPS = (23, 20, 19), 10, 300, 11


@pytest.fixture(scope="module")
def stream_case(oracle):
    cases = [synth.make_case("C1", step=s, grid=GRID, rows=ROWS, n_samples=NS, table=(s == 0)) for s in range(STEPS)]
    c0 = cases[0]
    wins = [oracle.log_onsets(c.onsets) for c in cases]
    return c0, wins


_REF = {}


def _reference(lib, stream_case, k, pull):
    """StreamingDetector(Engine) and per-step Engine.detect over the windows, and the stacking launches a
    detect_batch of m steps logs (computed once per (k, pull); the engine is closed before replicas are made)."""
    from quakemigrate_amd.stream import StreamingDetector

    if (k, pull) not in _REF:
        c0, wins = stream_case
        eng = lib.Engine(0, stream_pull=pull, log_timing=1)
        eng.load_lut(c0.traveltimes)
        single = [eng.detect(w, c0.fsmp, c0.lsmp, c0.available) for w in wins]
        sd = StreamingDetector(eng, ROWS, wins[0].shape[1], c0.fsmp, c0.lsmp, c0.available, depth=2,
                               steps_per_launch=k)
        streamed = sd.run(wins)
        sd.close()
        calls = {}
        for m in sorted({k, STEPS % k or k}):
            eng.kernel_log()
            eng.detect_batch(np.stack(wins[:m]), c0.fsmp, c0.lsmp, c0.available)
            calls[m] = eng.kernel_log()[1]
        eng.close()
        _REF[(k, pull)] = (single, streamed, calls)
    return _REF[(k, pull)]


def _same(got, want):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        for x, y in zip(g, w):
            assert np.array_equal(x, y), j


def _drive(sd, wins, sizes):
    """Push every window, popping in the given sizes (cycled) whenever the ring is full, then flush and drain."""
    got = []
    sizes = itertools.cycle(sizes)

    def take():
        n = min(next(sizes), sd.pending()[0])
        a, b, c = sd.pop(n)
        got.extend((a[j], b[j], c[j]) for j in range(n))

    for w in wins:
        while not sd.push(w):
            take()
    sd.flush()
    while sd.pending()[0]:
        take()
    return got


@pytest.mark.parametrize("pull", [0, 1])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("devices", DEVICE_LISTS)
def test_replicated_stream_equals_the_single_engine(lib, stream_case, devices, k, pull):
    from quakemigrate_amd.stream import StreamingDetector

    devices = _devices(devices)
    single, streamed, calls = _reference(lib, stream_case, k, pull)
    c0, wins = stream_case
    rep = lib.EngineReplicas(devices, stream_pull=pull, log_timing=1)
    rep.load_lut(c0.traveltimes)
    for r in rep.replicas:
        r.kernel_log()
    sd = StreamingDetector(rep, ROWS, wins[0].shape[1], c0.fsmp, c0.lsmp, c0.available, depth=2,
                           steps_per_launch=k)
    got = _drive(sd, wins, [2, 5, 1, 4])
    _same(got, single)
    _same(got, streamed)
    # launch j (K steps; the last one holds the rest) ran on replica j mod n, and each replica logged its share
    n = len(devices)
    sizes = [min(k, STEPS - j * k) for j in range(-(-STEPS // k))]
    for r, eng in enumerate(rep.replicas):
        mine = sizes[r::n]
        assert eng.kernel_log()[1] == sum(calls[m] for m in mine), (r, mine)
        assert mine, "every replica ran launches"
    sd.close()
    rep.close()


def test_back_pressure_counts_every_replicas_slots(lib, stream_case):
    from quakemigrate_amd.stream import StreamingDetector

    single = _reference(lib, stream_case, 2, 0)[0]
    c0, wins = stream_case
    n, depth, k = 2, 2, 2
    rep = lib.EngineReplicas([0] * n)
    rep.load_lut(c0.traveltimes)
    sd = StreamingDetector(rep, ROWS, wins[0].shape[1], c0.fsmp, c0.lsmp, c0.available, depth=depth,
                           steps_per_launch=k)
    for w in wins[:n * depth * k]:
        assert sd.push(w)
    assert sd.pending() == (n * depth * k, 0)
    assert not sd.push(wins[8])                          # every replica's slots hold un-popped results
    first = sd.pop(1)                                    # part of the oldest launch: its slot stays taken
    assert not sd.push(wins[8])
    second = sd.pop(1)                                   # the oldest launch is popped: one launch is free
    assert sd.push(wins[8]) and sd.push(wins[9])
    assert not sd.push(wins[10])
    assert sd.pending() == (n * depth * k, 0)
    rest = sd.pop(n * depth * k)
    got = [tuple(x[0] for x in first), tuple(x[0] for x in second)] + \
          [tuple(x[j] for x in rest) for j in range(n * depth * k)]
    _same(got, single[:len(got)])
    sd.close()
    rep.close()


def test_refusals_on_a_device(lib, stream_case):
    import ctypes

    from quakemigrate_amd.stream import StreamingDetector

    c0, wins = stream_case
    T = wins[0].shape[1]
    rep = lib.EngineReplicas([0, 0])
    rep.load_lut(c0.traveltimes)
    other = c0.traveltimes.copy()
    other[1, 2, 3, 4] += 1                               # same shape, one element off
    rep.replicas[1].load_lut(other)
    with pytest.raises(lib.QMHipError, match="replica 1 holds another table than replica 0"):
        StreamingDetector(rep, ROWS, T, c0.fsmp, c0.lsmp, c0.available)
    with pytest.raises(lib.QMHipError, match="replica 1 holds another table than replica 0"):
        rep.table_digest()
    rep.replicas[1].load_lut(np.ascontiguousarray(c0.traveltimes[:-1]))
    with pytest.raises(lib.QMHipError, match="another shape"):
        StreamingDetector(rep, ROWS, T, c0.fsmp, c0.lsmp, c0.available)
    # the same engine twice
    h = rep.replicas[0]._h.value
    arr = (ctypes.c_void_p * 2)(h, h)
    out = ctypes.c_void_p()
    assert lib.qmlib.qm_stream_create_replicas(arr, 2, T, c0.fsmp, c0.lsmp, c0.available, 0, 1, 2,
                                               ctypes.byref(out)) != 0
    assert out.value is None and b"same engine" in lib.qmlib.qm_last_error()
    # ... and a replica without a table
    fresh = lib.Engine(0)
    arr = (ctypes.c_void_p * 2)(h, fresh._h.value)
    assert lib.qmlib.qm_stream_create_replicas(arr, 2, T, c0.fsmp, c0.lsmp, c0.available, 0, 1, 2,
                                               ctypes.byref(out)) != 0
    assert b"replica 1 holds no travel-time table" in lib.qmlib.qm_last_error()
    fresh.close()
    # with the table made equal again, the stream goes
    rep.replicas[1].load_lut(c0.traveltimes)
    sd = StreamingDetector(rep, ROWS, T, c0.fsmp, c0.lsmp, c0.available)
    _same(sd.run(wins[:3]), _reference(lib, stream_case, 1, 0)[0][:3])
    sd.close()
    rep.close()


def test_table_changed_under_the_stream(lib, stream_case):
    from quakemigrate_amd.stream import StreamingDetector

    single = _reference(lib, stream_case, 1, 0)[0]
    c0, wins = stream_case
    rep = lib.EngineReplicas([0, 0])
    assert not rep.select_table("A")
    rep.load_lut(c0.traveltimes)
    sd = StreamingDetector(rep, ROWS, wins[0].shape[1], c0.fsmp, c0.lsmp, c0.available, depth=3)
    assert sd.push(wins[0]) and sd.push(wins[1])         # one launch on each replica
    assert not rep.replicas[0].select_table("B")
    rep.replicas[0].load_lut(np.ascontiguousarray(c0.traveltimes[::-1]))     # same shape, other delays
    with pytest.raises(lib.QMHipError, match="changed under the stream"):
        sd.push(wins[2])                                 # replica 0's launch is refused; the window waits
    with pytest.raises(lib.QMHipError, match="changed under the stream"):
        sd.flush()
    assert sd.pending() == (2, 1)
    assert rep.replicas[0].select_table("A")             # the stream's table again
    assert sd.push(wins[3]) and sd.push(wins[4])         # the waiting launch goes out first
    sd.flush()
    assert sd.pending() == (5, 0)
    a, b, c = sd.pop(5)
    _same([(a[j], b[j], c[j]) for j in range(5)], single[:5])
    sd.close()
    rep.close()


def test_closing_the_replicas_first(lib, stream_case):
    from quakemigrate_amd.stream import StreamingDetector

    c0, wins = stream_case
    rep = lib.EngineReplicas([0, 0])
    rep.load_lut(c0.traveltimes)
    sd = StreamingDetector(rep, ROWS, wins[0].shape[1], c0.fsmp, c0.lsmp, c0.available, depth=2)
    assert sd.push(wins[0]) and sd.push(wins[1]) and sd.push(wins[2])
    rep.close()                                          # the lanes are orphaned, not dangling
    for call in (lambda: sd.push(wins[3]), sd.flush, sd.pending, lambda: sd.pop(1)):
        with pytest.raises(lib.QMHipError, match="destroyed"):
            call()
    sd.close()
    sd.close()


def _script(lib, eng, stream_case):
    """One fixed sequence of stream calls on ``eng`` (depth 2, three steps per launch).  Returns the log -- per
    operation its name, what it returned, its error text and ``pending()`` behind it -- and the popped timesteps.
    Two things in an error text belong to the handle, not to the protocol, and are levelled: the constructor's own
    function name, and the tables' serial numbers (``#7``), which are unique in the process."""
    import re

    from quakemigrate_amd.stream import StreamingDetector

    c0, wins = stream_case
    T = wins[0].shape[1]
    log, popped = [], []

    def text(exc):
        return re.sub(r"#\d+", "#n", str(exc).replace("qm_stream_create_replicas", "qm_stream_create"))

    def do(name, call, sd=None):
        value = err = pend = None
        try:
            value = call()
        except lib.QMHipError as exc:
            err = text(exc)
        if isinstance(value, tuple):                    # a pop: the series go to `popped`, their count to the log
            popped.extend((value[0][j], value[1][j], value[2][j]) for j in range(len(value[0])))
            value = len(value[0])
        if sd is not None:
            try:
                pend = sd.pending()
            except lib.QMHipError as exc:
                pend = text(exc)
        log.append((name, value, err, pend))

    assert not eng.select_table("A")
    eng.load_lut(c0.traveltimes)
    do("create, too many steps per launch",
       lambda: StreamingDetector(eng, ROWS, T, c0.fsmp, c0.lsmp, c0.available, depth=2, steps_per_launch=5000) and None)
    sd = StreamingDetector(eng, ROWS, T, c0.fsmp, c0.lsmp, c0.available, depth=2, steps_per_launch=3)
    for j in range(6):
        do(f"fill the ring {j}", lambda: sd.push(wins[j]), sd)
    do("refused push", lambda: sd.push(wins[6]), sd)
    do("partial pop", lambda: sd.pop(2), sd)
    do("refused push, slot partly popped", lambda: sd.push(wins[6]), sd)
    do("pop that frees a slot", lambda: sd.pop(1), sd)
    do("push 6", lambda: sd.push(wins[6]), sd)
    do("push 7", lambda: sd.push(wins[7]), sd)
    do("over-pop", lambda: sd.pop(4), sd)
    do("flush a partly filled launch", sd.flush, sd)
    do("flush nothing", sd.flush, sd)
    do("pop 5", lambda: sd.pop(5), sd)
    do("push 8", lambda: sd.push(wins[8]), sd)
    do("push 9", lambda: sd.push(wins[9]), sd)
    assert not eng.select_table("B")
    eng.load_lut(np.ascontiguousarray(c0.traveltimes[::-1]))    # same shape, other delays
    do("table changed: the filling push", lambda: sd.push(wins[10]), sd)
    do("table changed: the next push", lambda: sd.push(wins[0]), sd)
    do("table changed: flush", sd.flush, sd)
    assert eng.select_table("A")
    do("recovery: push", lambda: sd.push(wins[0]), sd)
    do("recovery: push again", lambda: sd.push(wins[1]), sd)
    do("recovery: flush", sd.flush, sd)
    do("recovery: pop", lambda: sd.pop(5), sd)
    do("push before the engine closes", lambda: sd.push(wins[2]), sd)
    eng.close()
    do("engine closed: push", lambda: sd.push(wins[3]), sd)
    do("engine closed: flush", sd.flush, sd)
    do("engine closed: pop", lambda: sd.pop(1), sd)
    sd.close()
    sd.close()
    return log, popped


def test_one_script_two_handles(lib, stream_case):
    """A stream on ``Engine(0)`` and one on ``EngineReplicas([0])`` are the same thing: after every operation of one
    script -- the ring filled, a refused push, a partial pop, a pop that frees a slot, an over-pop, a flush of a partly
    filled launch, a table change under the stream with its refusals and the recovery, the engine closed first -- the
    return value, ``pending()`` and any error's text are the same, and all popped series are equal."""
    single = _reference(lib, stream_case, 3, 0)[0]
    log_e, popped_e = _script(lib, lib.Engine(0), stream_case)
    log_r, popped_r = _script(lib, lib.EngineReplicas([0]), stream_case)
    for e, r in zip(log_e, log_r):
        assert e == r
    assert len(log_e) == len(log_r)
    _same(popped_r, popped_e)
    _same(popped_e, single[:8] + [single[j] for j in (8, 9, 10, 0, 1)])
    # the script is what it says it is: the refusals refuse, and for the reasons named
    by_name = {name: (value, err, pend) for name, value, err, pend in log_e}
    assert "steps_per_launch must be in 1..4096" in by_name["create, too many steps per launch"][1]
    assert by_name["refused push"] == (False, None, (6, 0))
    assert by_name["refused push, slot partly popped"] == (False, None, (4, 0))
    assert by_name["push 7"] == (True, None, (3, 2))
    assert "4 steps asked for, 3 launched" in by_name["over-pop"][1] and by_name["over-pop"][2] == (3, 2)
    assert by_name["flush a partly filled launch"] == (None, None, (5, 0))
    for name in ("table changed: the filling push", "table changed: the next push", "table changed: flush"):
        assert "changed under the stream" in by_name[name][1] and by_name[name][2] == (0, 3), name
    assert by_name["recovery: push again"] == (True, None, (3, 2))
    assert by_name["recovery: pop"] == (5, None, (0, 0))
    for name in ("engine closed: push", "engine closed: flush", "engine closed: pop"):
        assert "destroyed" in by_name[name][1] and "destroyed" in by_name[name][2], name


def test_a_stage_on_every_lane_or_on_none(lib, stream_case):
    """A lane whose engine is gone refuses the onset stage; the lane before it keeps nothing of it."""
    from quakemigrate_amd.preprocess import OnsetStage
    from quakemigrate_amd.stream import StreamingDetector

    c0, wins = stream_case
    T = wins[0].shape[1]
    stage = OnsetStage(filters={"P": (2.0, 16.0, 2)}, sta_lta_windows={"P": (0.2, 1.0)}, trace_row=tuple(range(ROWS)),
                       trace_phase=tuple("P" * ROWS), row_phase=tuple("P" * ROWS), taper_pad=20)
    rep = lib.EngineReplicas([0, 0])
    rep.load_lut(c0.traveltimes)
    sd = StreamingDetector(rep, ROWS, T, c0.fsmp, c0.lsmp, c0.available, depth=2, steps_per_launch=3)
    rep.replicas[1].close()
    lib.release_cached_memory()
    before = rep.replicas[0].get("pool_live_bytes")
    with pytest.raises(lib.QMHipError, match="destroyed"):
        sd.set_onset_stage(stage, sampling_rate=50)
    assert rep.replicas[0].get("pool_live_bytes") == before
    sd.close()
    rep.close()


@pytest.mark.parametrize("cfg", [{"tie_rule": 1}, {"screen": 1}], ids=["tie_rule", "screen"])
def test_near_ties_with_tie_rule_and_screen(lib, oracle, cfg):
    from quakemigrate_amd.stream import StreamingDetector

    g = load_golden("ties_twins")
    tt, fsmp, lsmp, avail = g["traveltimes"], int(g["fsmp"]), int(g["lsmp"]), int(g["available"])
    base = oracle.log_onsets(g["onsets"])
    wins = [np.ascontiguousarray(np.roll(base, s, axis=1)) if s % 2 else base for s in range(7)]
    eng = lib.Engine(0, **cfg)
    eng.load_lut(tt)
    want = [eng.detect(w, fsmp, lsmp, avail) for w in wins]
    sd = StreamingDetector(eng, len(base), base.shape[1], fsmp, lsmp, avail, depth=2, steps_per_launch=2)
    streamed = sd.run(wins)
    sd.close()
    eng.close()
    _same(streamed, want)
    rep = lib.EngineReplicas([0, 0], **cfg)
    rep.load_lut(tt)
    assert rep.get(next(iter(cfg))) == 1
    sd = StreamingDetector(rep, len(base), base.shape[1], fsmp, lsmp, avail, depth=2, steps_per_launch=2)
    _same(_drive(sd, wins, [3, 1]), streamed)
    sd.close()
    rep.close()


# ------------------------------------------------------------------------------ front end
def _continuous_glue(lib, device_serving):
    import datetime as dt

    from quakemigrate_amd import scan

    grid, rows, rate, n_steps = (20, 18, 12), 8, 50, 7
    case = synth.make_case("C3", step=1, grid=grid, rows=rows, n_samples=300)
    keys = [f"ST{i}_{'P' if i < 4 else 'S'}" for i in range(rows)]
    full = dict.fromkeys(keys, 1)
    less = {**full, "ST2_P": 0}
    avail_of = [full, full, None, full, less, less, full]
    onsets_of = [synth.make_case("C3", step=s, grid=grid, rows=rows, n_samples=300, table=False).onsets
                 for s in range(n_steps)]
    timestep, pre, post = 300 / rate, case.fsmp / rate, case.lsmp / rate
    t0 = dt.datetime(2024, 5, 17, 10, 0, 0)

    class Data:
        def __init__(self, i, w_beg):
            self.i, self.starttime = i, w_beg

    class OnsetData:
        sampling_rate = rate

        def __init__(self, availability):
            self.availability = availability

    class Onset:
        def calculate_onsets(self, data):
            a = avail_of[data.i]
            return onsets_of[data.i][[j for j, k in enumerate(keys) if a[k] == 1]], OnsetData(dict(a))

    class Lut:
        unit_conversion_factor = 1000.0
        traveltimes = {}
        for j, k in enumerate(keys):
            st, ph = k.split("_")
            traveltimes.setdefault(st, {})[ph] = case.traveltimes[..., j] / rate

        def serve_traveltimes(self, sampling_rate, availability):
            return np.ascontiguousarray(case.traveltimes[..., [j for j, k in enumerate(keys) if availability[k]]])

        def index2coord(self, idx, unravel=True):
            return np.stack(np.unravel_index(idx, grid), axis=-1) * 0.5

    class Sink:
        written = False

        def __init__(self):
            self.appended, self.empties = [], []

        def append(self, time, a, b, coord, ucf):
            self.appended.append((time, np.array(a), np.array(b), np.array(coord)))

        def empty(self, starttime, timestep, i, msg, ucf):
            self.empties.append(i)

        def write(self):
            self.written = True

    out = {}
    for name, eng in (("engine", lib.Engine(0)), ("replicas", lib.EngineReplicas([0, 0]))):
        seen = []

        class Archive:
            def read_waveform_data(self, w_beg, w_end):
                i = len(seen)
                seen.append(i)
                if avail_of[i] is None:
                    raise scan.DataGapException(f"no data in step {i}")
                return Data(i, w_beg)

        sink = Sink()
        s = scan.MigrationScan(Lut(), Onset(), pre, post, engine=eng, device_serving=device_serving)
        rows_out = s.continuous_compute(Archive(), t0, n_steps, timestep, rate, sink, steps_per_launch=2, depth=2)
        out[name] = (rows_out, sink)
        eng.close()
    return out, n_steps


@pytest.mark.parametrize("device_serving", [False, True], ids=["host-served", "device-served"])
def test_continuous_compute_with_replicas(lib, device_serving):
    """A short run with one data gap and one change of availability: the replicas' pipeline puts the same
    times, series, coordinates and availability rows into the sink as the single engine's."""
    out, n_steps = _continuous_glue(lib, device_serving)
    (rows0, s0), (rows1, s1) = out["engine"], out["replicas"]
    assert rows1 == rows0 and s1.empties == s0.empties == [2] and s1.written
    assert len(s1.appended) == len(s0.appended) == n_steps - 1
    for (t1, a1, b1, c1), (t0_, a0, b0, c0) in zip(s1.appended, s0.appended):
        assert t1 == t0_ and np.array_equal(a1, a0) and np.array_equal(b1, b0) and np.array_equal(c1, c0)


def test_compute_and_locate_with_replicas(lib, oracle):
    from quakemigrate_amd import scan

    g = load_golden("compute_glue")
    keys = [str(k) for k in g["grid_keys"]]
    availability = {str(k): int(v) for k, v in zip(g["availability_keys"], g["availability_values"])}
    shape = g["grids"].shape[1:]
    rate = int(g["sampling_rate"])

    class Lut:
        node_spacing = g["node_spacing"]
        traveltimes = {}
        for k, grid in zip(keys, g["grids"]):
            st, ph = k.split("_")
            traveltimes.setdefault(st, {})[ph] = grid

        def serve_traveltimes(self, sr, avail):
            picked = [self.traveltimes[k.split("_")[0]][k.split("_")[1]] for k, v in avail.items() if v == 1]
            return oracle.np_serve_traveltimes(picked, sr)

        def index2coord(self, idx, unravel=True):
            return g["ll_corner"] + np.column_stack(np.unravel_index(idx, shape)) * g["node_spacing"]

    class OnsetData:
        sampling_rate = rate

    OnsetData.availability = availability

    class Onset:
        def calculate_onsets(self, data):
            return g["onsets"], OnsetData()

    class Data:
        starttime = float(g["starttime"])

    class Event:
        def mw_times(self, scan_rate):
            return np.arange(len(g["max_coa"])) / scan_rate

    class Archive:
        def read_waveform_data(self, w_beg, w_end):
            return Data()

    n = len(g["max_coa"])
    mw = (n - 1) / 4 / rate                              # the window holds 4 mw rate + 1 samples
    out = {}
    for name, eng in (("engine", lib.Engine(0)), ("replicas", lib.EngineReplicas([0, 0]))):
        pre, post = float(g["pre_pad"]), float(g["post_pad"])
        det = scan.MigrationScan(Lut(), Onset(), pre, post, engine=eng)
        loc = scan.MigrationScan(Lut(), Onset(), pre, post, stage="locate", scan_rate=rate, engine=eng)
        coa_map, fits = loc.calculate_location(Data(), 3, n - 3)[:2]
        located = loc.locate_compute(Archive(), [("ev", Data.starttime)], mw)
        out[name] = (det._compute(Data()), loc._compute(Data(), Event()), coa_map, located)
        eng.close()
    (d0, l0, c0, r0), (d1, l1, c1, r1) = out["engine"], out["replicas"]
    assert d1[0] == d0[0] and all(np.array_equal(x, y) for x, y in zip(d1[1:4], d0[1:4]))
    assert all(np.array_equal(x, y) for x, y in zip(l1[:5], l0[:5]))
    assert np.array_equal(c1, c0)
    assert len(r1) == len(r0)
    for e1, e0 in zip(r1, r0):
        assert e1["otime"] == e0["otime"] and (e1["first_sample"], e1["last_sample"]) == (e0["first_sample"],
                                                                                         e0["last_sample"])
        assert np.array_equal(e1["max_coa"], e0["max_coa"]) and np.array_equal(e1["coord"], e0["coord"])
        assert np.array_equal(e1["coa_map"], e0["coa_map"])


def test_full_size_c3_two_replicas_on_the_copy_path(lib, oracle):
    """The full C3 grid, 30 rows: four timesteps, one per launch, through [0, 0] against the Engine stream."""
    from quakemigrate_amd.stream import StreamingDetector

    cases = [synth.make_case("C3", step=s, table=(s == 0)) for s in range(4)]
    c0 = cases[0]
    wins = [oracle.log_onsets(c.onsets) for c in cases]
    assert wins[0].nbytes > (1 << 20)                    # slots above 1 MB: the copy path
    args = (c0.traveltimes.shape[-1], wins[0].shape[1], c0.fsmp, c0.lsmp, c0.available)
    eng = lib.Engine(0)
    eng.load_lut(c0.traveltimes)
    sd = StreamingDetector(eng, *args, depth=2)
    want = sd.run(wins)
    sd.close()
    eng.close()
    rep = lib.EngineReplicas([0, 0])
    rep.load_lut(c0.traveltimes)
    sd = StreamingDetector(rep, *args, depth=2)
    got = _drive(sd, wins, [3, 1])
    _same(got, want)
    sd.close()
    rep.close()
