# -*- coding: utf-8 -*-
"""
Three older stages on the GPU at their edges, against the restatements of tests/stage_edges_ref.py (pinned on the CPU by
tests/test_stage_edges_host.py): the STA/LTA onset stage (stalta_sums_kernel, onset_rows_kernel), on-device table
serving (serve_table_kernel<256 | 64>) and the scan of a materialised volume (scan_volume_kernel + combine_kernel in
mode 2).  Every input comes from a seeded NumPy generator.

The bounds, none of them a measurement:

* **Onset rows: 4 ulp** (``rtol = 4 * 2^-52``; the logged rows the same plus ``atol = 2^-52`` around log(1) = 0).  The
  running sums are additions in the restatement's order, so they carry the same bits.  What follows per sample is one
  division, one product with nlta / nsta, one square, the sum of a row's squares, one division by the count and one
  square root, each correctly rounded, the square and the sum with contraction off in the kernel: nothing is left to
  differ, the 4 ulp are the allowance for a division or a root that is faithfully instead of correctly rounded
  (1 ulp each, the root halving what comes before it).  The device's log is within 1 ulp, glibc's within 1.
  Observed on an MI355X: the raw rows of all 68 calls of this file carry the restatement's bits (0 ulp), the logged
  rows are within 1.0 ulp.
* **max_norm_coa: 2 N 2^-53 relative** to ``max * N / fsum``.  The volumes are positive, so a sum of N terms in any
  order, that of the kernel's sets and wavefronts included, is within (N - 1) 2^-53 of the exact one; the product and
  the division round once more each, the restatement's fsum, product and division three times: (N + 4) 2^-53 <= 2 N
  2^-53 from N = 4 on, and below that (N = 1 here) both sides are exact.  Observed, as a fraction of the bound and
  the same on all three paths: 0 (N = 1), 0.14 (7), 7.8e-3 (513), 4.5e-3 (1000), 1.2e-4 (17000).
* Indices, copied maxima and served tables are equal, with no tolerance.

Which path a shape takes is shown by the launch arithmetic restated in stage_edges_ref (``serve_plan``,
``onset_in_lds``, ``scan_plan``, the latter on the engine's own ``n_cu``), asserted beside each case.
"""

import numpy as np
import pytest

import stage_edges_ref as ref

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    if _lib.qmlib.qm_device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


@pytest.fixture(scope="module")
def engine(lib):
    eng = lib.Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def small_chunks(lib):
    eng = lib.Engine(0, chunk_bytes=1 << 20)
    yield eng
    eng.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ulps(got, want):
    """Largest |got - want| in units of 2^-52 |want| over the finite, non-zero entries."""
    both = np.isfinite(got) & np.isfinite(want) & (want != 0)
    if not both.any():
        return 0.0
    return float(np.max(np.abs(got[both] - want[both]) / (np.abs(want[both]) * ULP)))


# =====================================================================================================================
# 1. the onset stage
# =====================================================================================================================
def check_onsets(eng, signals, trace_row, nsta, nlta, **kw):
    """One call on the engine and on the strict restatement, at 4 ulp.  Returns (raw, strict raw)."""
    signals = np.ascontiguousarray(signals, dtype=np.float64)
    raw, logged = eng.onsets(signals, trace_row, nsta, nlta, **kw)
    want_raw, want_log = ref.onset_stage_strict(signals, trace_row, nsta, nlta, **kw)
    print(f"onsets T={signals.shape[1]} {kw}: raw {ulps(raw, want_raw):.2f} ulp, "
          f"logged {ulps(logged, want_log):.2f} ulp, bits equal: {np.array_equal(bits(raw), bits(want_raw))}")
    np.testing.assert_allclose(raw, want_raw, rtol=4 * ULP, atol=0, equal_nan=True)
    np.testing.assert_allclose(logged, want_log, rtol=4 * ULP, atol=ULP, equal_nan=True)
    return raw, want_raw


def single_rows(n):
    """n traces, each a row of its own."""
    return np.arange(n, dtype=np.int32)


@pytest.mark.parametrize("transform", ["energy", "abs"])
@pytest.mark.parametrize("position", ["classic", "centred"])
def test_onset_loop_remainders(engine, position, transform):
    """The four-way unrolled loops run (T - nlta) // 4 (classic) or (T - nsta - nlta) // 4 (centred) times and leave
    the rest to the scalar loop: every residue mod 4."""
    ns, nl = 3, 17
    lengths = range(81, 85) if position == "classic" else range(84, 88)
    left = lambda t: (t - nl) if position == "classic" else (t - ns - nl)          # noqa: E731
    assert sorted(left(t) % 4 for t in lengths) == [0, 1, 2, 3]
    rng = np.random.default_rng(101)
    for t in lengths:
        x = rng.standard_normal((3, t))
        raw, _ = check_onsets(engine, x, single_rows(3), [ns] * 3, [nl] * 3, transform=transform, position=position,
                              taper_pad=-1, min_onset_value=0.01)
        assert (raw[:, nl - 1:left(t) + nl] != 1.0).all()            # every sample the loops own was written


def test_onset_window_edges(engine):
    """T = 64.  nlta == T and nlta > T, nsta == nlta, nsta == 1, nsta > nlta; centred with nsta + nlta == T (only sample
    nlta - 1 carries a ratio) and > T (all ones); recursive with and without the nulled start."""
    t = 64
    windows = [(1, 1), (1, 2), (5, 5), (3, 64), (3, 61), (3, 62), (3, 65), (6, 5)]
    ns, nl = [w[0] for w in windows], [w[1] for w in windows]
    x = np.random.default_rng(102).standard_normal((len(windows), t))
    ones = np.ones(t)
    for transform in ("energy", "abs"):
        kw = dict(transform=transform, taper_pad=-1, min_onset_value=0.01)
        raw, _ = check_onsets(engine, x, single_rows(len(windows)), ns, nl, position="classic", **kw)
        # (classic with nsta == nlta: both sums are the same chain, the ratio is 1.0 exactly)
        flat = [(1, 1), (5, 5), (3, 65), (6, 5)]
        for k, w in enumerate(windows):
            assert np.array_equal(raw[k], ones) == (w in flat), w
            if w not in flat:
                assert np.array_equal(raw[k][:w[1] - 1], ones[:w[1] - 1]) and (raw[k][w[1] - 1:] != 1.0).all(), w
        raw, _ = check_onsets(engine, x, single_rows(len(windows)), ns, nl, position="centred", **kw)
        for k, w in enumerate(windows):
            assert np.array_equal(raw[k], ones) == (w in [(3, 64), (3, 62), (3, 65), (6, 5)]), w
        k = windows.index((3, 61))
        assert raw[k][60] != 1.0 and np.array_equal(np.delete(raw[k], 60), np.ones(t - 1))
        rec = [(3, 64), (3, 70), (3, 10)]
        raw, _ = check_onsets(engine, x[:3], single_rows(3), [3, 3, 3], [w[1] for w in rec], position="recursive",
                              transform=transform, taper_pad=-1, min_onset_value=0.0)
        assert raw[0][0] == 0.0 and raw[1][0] == 0.0 and (raw[:2, 1:] != 1.0).all()      # no nulling: nlta >= T
        assert np.array_equal(raw[2][:10], np.ones(10)) and (raw[2][10:] != 1.0).all()


@pytest.mark.parametrize("position", ["classic", "centred", "recursive"])
def test_onset_taper_and_floor(engine, position):
    """taper_pad < 0 (off), 0, 5, and two that cover the whole row from either side; a floor below and above 1.0."""
    t, ns, nl = 200, 7, 40
    x = np.random.default_rng(103).standard_normal((3, t))
    rows = [0, 1, 0]
    for pad in (-1, 0, 5, 80, 200):
        for floor in (0.4, 1.5):
            raw, _ = check_onsets(engine, x, rows, [ns, ns], [nl, nl], transform="energy", position=position,
                                  taper_pad=pad, min_onset_value=floor)
            assert raw.min() >= floor
            if pad >= 0:
                covered = np.zeros(t, dtype=bool)
                covered[:pad + nl - 1] = True
                covered[max(t - (ns + pad), 0):] = True
                assert covered.all() == (pad >= 80)
                assert (raw[:, covered] == max(1.0, floor)).all()
                if floor < 1.0 and position != "recursive":     # (recursive: sample nlta - 1 is nulled to 1.0)
                    assert (raw[:, ~covered] != 1.0).all()


@pytest.mark.parametrize("position", ["classic", "centred", "recursive"])
def test_onset_row_assembly(engine, position):
    """Four rows of 1, 2, 3 and 1 components, the traces interleaved, each row with windows of its own."""
    trace_row = [2, 0, 1, 2, 3, 1, 2]
    assert np.bincount(trace_row).tolist() == [1, 2, 3, 1]
    x = np.random.default_rng(104).standard_normal((7, 150))
    for transform in ("energy", "abs"):
        check_onsets(engine, x, trace_row, [3, 5, 7, 4], [20, 31, 50, 64], transform=transform, position=position,
                     taper_pad=3, min_onset_value=0.4)


@pytest.mark.parametrize("transform", ["energy", "abs"])
def test_onset_order_of_the_sliding_sums(engine, transform):
    """Behind a burst at x 1000 a 200-sample gap of zeros: the exact window sums there are 0, the running sums hold the
    residue of the burst's roundings, ~1e-8 (x * x) or ~1e-12 (|x|) with either sign, and the classic ratio and the
    centred ``lta > 0`` guard are decided by it -- by the ORDER of the additions.  A kernel that updated the sums in
    another order leaves another residue: ratios of another size and sign, far outside 4 ulp."""
    x = ref.stress_traces()
    n, ns, nl = x.shape[1], 7, 60
    k = len(x)
    kw = dict(transform=transform, taper_pad=-1, min_onset_value=0.01)
    for position in ("classic", "centred", "recursive"):
        raw, want = check_onsets(engine, x, single_rows(k), [ns] * k, [nl] * k, position=position, **kw)
        if position != "centred":
            continue
        guarded = 0
        for i in range(k):
            f = x[i] * x[i] if transform == "energy" else np.abs(x[i])
            _, L, _ = ref.stalta_strict(f, ns, nl, "centred")
            at = np.flatnonzero(L[nl:n - ns] <= 0.0) + nl
            guarded += len(at)
            assert (raw[i][at] == 1.0).all()
            gap = np.arange(1300, 1390)                     # long window wholly inside the zeros
            assert (L[gap] != 0.0).all() and ((raw[i][gap] == 1.0) == (L[gap] <= 0.0)).all()
        assert guarded > 100


@pytest.mark.parametrize("position", ["classic", "centred"])
@pytest.mark.parametrize("t", [20480, 20481])
def test_onset_lds_boundary(lib, engine, oracle, t, position):
    """T = 20 480: the trace fills the 160 KB of dynamic LDS exactly; T = 20 481: it does not fit and the recurrence
    reads global memory, transforming on the fly.  The beyond-LDS centred rows also stay on the device and feed a small
    detect."""
    assert ref.onset_in_lds(t) == (t == 20480)
    x = np.random.default_rng(105).standard_normal((2, t))
    kw = dict(transform="energy", position=position, taper_pad=-1, min_onset_value=0.4)
    _, want_raw = check_onsets(engine, x, single_rows(2), [11, 11], [51, 51], **kw)
    if not (t == 20481 and position == "centred"):
        return
    import torch

    rng = np.random.default_rng(106)
    grid, lsmp, fsmp = (5, 4, 3), 160, 120
    tt = rng.integers(0, lsmp + 1, size=grid + (2,), dtype=np.int32)
    d_log = torch.empty((2, t), dtype=torch.float64, device="cuda")
    engine.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        engine.onsets(x, single_rows(2), [11, 11], [51, 51], log_out=d_log, **kw)
        engine.load_lut(tt)
        got = engine.detect(d_log, fsmp, lsmp, 2)
    finally:
        engine.synchronize()
        engine.set_stream(None)
    want = oracle.detect(want_raw, tt, fsmp, lsmp, 2, threads=2)
    assert np.array_equal(got[2], want[2])
    np.testing.assert_allclose(got[0], want[0], rtol=1e-11)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-11)


# =====================================================================================================================
# 2. table serving
# =====================================================================================================================
GRID = (9, 7, 37)               # 2331 nodes: nine 256-node blocks + 27, thirty-six 64-node blocks + 27


def smooth_grids(shape, count, seed):
    """Travel times in seconds from ``count`` random sources at 0.31 .. 0.47 s per node."""
    rng = np.random.default_rng(seed)
    ix = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    out = []
    for _ in range(count):
        src = rng.uniform(-3.0, np.array(shape) + 3.0)
        out.append(np.sqrt(((ix - src) ** 2).sum(axis=-1)) * rng.uniform(0.31, 0.47))
    return out


@pytest.fixture(scope="module")
def served(engine):
    grids = smooth_grids(GRID, 5, 201)
    assert int(np.prod(GRID)) == 2331 == 9 * 256 + 27 == 36 * 64 + 27
    engine.set_traveltime_grids(grids)
    return grids


def check_serve(eng, grids, rows, rate, decimate=(1, 1, 1)):
    eng.serve(rate, rows, decimate=decimate)
    want = ref.serve_expected(grids, rows, rate, decimate)
    got = eng.download_lut()
    assert got.shape == want.shape and eng.grid == want.shape[:3]
    assert np.array_equal(got, want), (len(rows), rate, decimate)
    return got


@pytest.mark.parametrize("n_rows", [1, 7, 8, 9, 13, 62, 63, 64, 65, 254])
def test_serve_row_counts(lib, engine, served, n_rows):
    """One pass of the eight-wide load loop with and without a clamped remainder, a second pass with one (13), the last
    row count of the 256-node kernel (62), the first of the 64-node kernel (63) and its last (254); 255 is refused
    before anything is launched and leaves the resident table alone."""
    npb = ref.serve_plan(n_rows)[0]
    assert npb == (256 if n_rows <= 62 else 64)
    rows = np.random.default_rng(n_rows).integers(0, 5, n_rows)
    got = check_serve(engine, served, rows, 62.5)
    assert got.shape == GRID + (n_rows,) and got.min() >= 0 and got.max() > 300
    if n_rows == 254:
        assert ref.serve_plan(255)[0] == 0
        with pytest.raises(lib.QMHipError, match="too many rows"):
            engine.serve(62.5, np.zeros(255, dtype=np.int32))
        assert engine.n_rows == 254 and np.array_equal(engine.download_lut(), got)


@pytest.mark.parametrize("n_rows", [13, 63])
def test_serve_decimations(engine, served, n_rows):
    """None, the recorded fixture's factors, factors equal to the axes (one node, the middle one) and beyond them."""
    rows = np.random.default_rng(300 + n_rows).integers(0, 5, n_rows)
    shapes = {(1, 1, 1): (9, 7, 37), (2, 3, 4): (5, 3, 10), (9, 7, 37): (1, 1, 1), (20, 1, 50): (1, 7, 1)}
    for decimate, shape in shapes.items():
        got = check_serve(engine, served, rows, 62.5, decimate)
        assert got.shape == shape + (n_rows,)
    # a factor from the axis length on leaves the axis' middle node: (9 - 1) // 2, (7 - 1) // 2, (37 - 1) // 2
    mid = ref.serve_expected(served, rows, 62.5)[4, 3, 18]
    assert np.array_equal(got[0, 3, 0], mid)                # (the (20, 1, 50) table)
    assert np.array_equal(check_serve(engine, served, rows, 62.5, (9, 7, 37))[0, 0, 0], mid)


@pytest.mark.parametrize("shape", [(1, 1, 300), (300, 1, 1)])
def test_serve_one_node_axes(lib, shape):
    """Grids that are a line along the fastest or the slowest axis, whole and every seventh node."""
    eng = lib.Engine(0)
    grids = smooth_grids(shape, 3, 202)
    eng.set_traveltime_grids(grids)
    for n_rows in (6, 70):
        rows = np.random.default_rng(n_rows).integers(0, 3, n_rows)
        for f in (1, 7):
            got = check_serve(eng, grids, rows, 62.5, (f, f, f))
            assert got.size == (300 if f == 1 else 43) * n_rows
    eng.close()


SPECIALS = [0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 1000000.5, 1000001.5, -0.0, 5e-324, 2147483647.0, 2147483647.5,
            2147483648.0, -2147483648.0, -2147483648.5, -2147483649.0, 1e300, np.inf, -np.inf, np.nan]


@pytest.mark.parametrize("n_rows", [13, 63])
def test_serve_values_at_the_int32_edges(lib, n_rows):
    """Halves of either parity and sign, signed zero, the smallest subnormal, both ends of int32 and the halves and
    units just beyond them, a huge value, the infinities and NaN, planted in every grid at rate 1.0; the same grids at
    62.5 and 1e-3, where the edges fall elsewhere."""
    rng = np.random.default_rng(203)
    grids = smooth_grids(GRID, 5, 203)
    where = []
    for g in grids:
        flat = rng.permutation(g.size)[:len(SPECIALS)]
        g.reshape(-1)[flat] = SPECIALS
        where.append(flat)
    eng = lib.Engine(0)
    eng.set_traveltime_grids(grids)
    rows = np.concatenate([np.arange(5), rng.integers(0, 5, n_rows - 5)])
    lo = ref.INT32_MIN
    at_one = [0, 2, 2, 4, 0, -2, -2, -4, 1000000, 1000002, 0, 0, 2147483647, lo, lo, lo, lo, lo, lo, lo, lo, lo]
    for rate in (1.0, 62.5, 1e-3):
        got = check_serve(eng, grids, rows, rate).reshape(-1, n_rows)
        if rate == 1.0:
            for s in range(5):
                assert got[where[s], s].tolist() == at_one
        # per row: at 1.0 the nine specials from 2147483647.5 on; at 62.5 also 2147483647.0; at 1e-3 the last four
        assert (got == lo).sum() == {1.0: 9, 62.5: 10, 1e-3: 4}[rate] * n_rows
    eng.close()


# =====================================================================================================================
# 3. the volume scan
# =====================================================================================================================
SCAN_SHAPES = {
    (1, 1): dict(tiles=1, xgroups=1, waves=1, sets=1, per=1, last=1),
    (7, 65): dict(tiles=2, xgroups=1, waves=2, sets=1, per=7, last=7),                    # the remainder loop only
    (513, 300): dict(tiles=5, xgroups=1, waves=5, sets=2, per=257, last=256),
    (1000, 1025): dict(tiles=17, xgroups=2, waves=9, sets=3, per=334, last=332),          # wavefront 18 of 18 past the end
    (17000, 70): dict(tiles=2, xgroups=1, waves=2, sets=66, per=258, last=230),           # the combine's second pass
}


def planted_volume(shape, plan, seed):
    """Lognormal [nodes][samples] with, in samples of their own where the shape has room: the maximum at node 0, at the
    last node, equal maxima either side of every set boundary worth it (first / second set; sets 63 / 64, the
    combine's passes), equal maxima in the last slot of one 8-load group and the first of the next, and one sample
    where every node holds the same value.  Returns (volume, {sample: expected index})."""
    n, t = shape
    vol = np.random.default_rng(seed).lognormal(0.0, 1.0, size=shape)
    per, sets = plan["per"], plan["sets"]
    plants = [[0], [n - 1]]
    if sets >= 2:
        plants.append([per - 1, per])
    if sets >= 65:
        plants.append([64 * per - 1, 64 * per])
        plants.append([(sets - 1) * per - 1, n - 1])
    if per >= 17:
        n0 = (sets - 1) * per
        plants.append([n0 + 15, n0 + 16])
    samples = [int(s) for s in np.unique(np.linspace(0, t - 1, len(plants) + 1).round().astype(int))]
    expected = {}
    if n > 1 and len(samples) == len(plants) + 1:
        for s, nodes in zip(samples, plants):
            vol[nodes, s] = 2.0 * vol[:, s].max()
            expected[s] = nodes[0]
        vol[:, samples[-1]] = 1.75
        expected[samples[-1]] = 0
    return vol, expected


@pytest.fixture(scope="module")
def scan_cases():
    """Volume, planted indices and the restatement's answer per shape, computed once and shared by the three paths."""
    cases = {}
    for k, (shape, plan) in enumerate(SCAN_SHAPES.items()):
        vol, expected = planted_volume(shape, plan, 400 + k)
        want = ref.scan_expected(vol)
        for s, node in expected.items():
            assert want[2][s] == node
        cases[shape] = (vol, expected, want)
    return cases


def scan_on(path, engine, small_chunks, vol):
    n, t = vol.shape
    if path == "host":
        return engine.find_max_coa(vol, t, n)
    if path == "host-1MiB":
        assert small_chunks.get("chunk_bytes") == 1 << 20
        return small_chunks.find_max_coa(vol, t, n)
    import torch

    d_vol = torch.from_numpy(vol).cuda()
    out = engine.find_max_coa(d_vol, t, n)
    engine.synchronize()
    return out


@pytest.mark.parametrize("path", ["host", "host-1MiB", "device"])
@pytest.mark.parametrize("shape", list(SCAN_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_scan_volume_shapes(engine, small_chunks, scan_cases, shape, path):
    n, t = shape
    plan = ref.scan_plan(t, n, engine.get("n_cu"))
    assert plan == SCAN_SHAPES[shape]
    if shape == (1000, 1025):                               # two time workgroups of 9 wavefronts for 17 tiles
        assert plan["xgroups"] * plan["waves"] == plan["tiles"] + 1
    if shape == (17000, 70):
        assert plan["sets"] > 64 and (1 << 20) // (8 * n) == 7
    vol, expected, want = scan_cases[shape]
    assert len(expected) >= (0 if n == 1 else 3)
    got = scan_on(path, engine, small_chunks, vol)
    assert np.array_equal(got[2], want[2])
    for s, node in expected.items():
        assert got[2][s] == node
    assert np.array_equal(bits(got[0]), bits(want[0]))
    ratio = float(np.max(np.abs(got[1] / want[1] - 1.0))) / (2 * n * U)
    print(f"scan {shape} {path}: |max_norm_coa / expected - 1| / (2 N 2^-53) = {ratio:.2e}")
    np.testing.assert_allclose(got[1], want[1], rtol=2 * n * U, atol=0)


@pytest.mark.parametrize("path", ["host", "host-1MiB", "device"])
def test_scan_volume_non_finite_entries(engine, small_chunks, scan_cases, path):
    """A NaN never wins and turns its sample's sum -- hence max_norm_coa -- to NaN; +inf wins and does the same
    (inf / inf); every other sample keeps its bits.  A column of NaN: nothing compares greater than the -inf the scan
    starts from, so index 0, max_coa -inf and a NaN max_norm_coa (not the detect path's 0, which is
    exp(-inf), a value the volume holds; a column of zeros gives that 0 here as well)."""
    clean_vol, _, _ = scan_cases[(513, 300)]
    n, t = clean_vol.shape
    clean = scan_on(path, engine, small_chunks, clean_vol)
    vol = clean_vol.copy()
    top = int(np.argmax(vol[:, 5]))
    vol[top, 5] = np.nan                                    # the winner itself: the best FINITE entry takes over
    vol[300, 9] = np.inf                                    # (second set)
    vol[:, 20] = np.nan
    vol[:, 30] = 0.0
    want = ref.scan_expected(vol)
    got = scan_on(path, engine, small_chunks, vol)
    assert want[2][5] != top and want[0][5] == np.nanmax(vol[:, 5])
    assert got[2][5] == want[2][5] and got[0][5] == want[0][5] and np.isnan(got[1][5])
    assert got[2][9] == 300 and got[0][9] == np.inf and np.isnan(got[1][9])
    assert got[2][20] == 0 and got[0][20] == -np.inf and np.isnan(got[1][20])
    assert got[2][30] == 0 and got[0][30] == 0.0 and np.isnan(got[1][30])
    assert np.array_equal(got[2], want[2]) and np.array_equal(bits(got[0]), bits(want[0]))
    rest = np.setdiff1d(np.arange(t), [5, 9, 20, 30])
    for k in range(3):
        assert np.array_equal(np.asarray(got[k])[rest].view(np.uint64), np.asarray(clean[k])[rest].view(np.uint64)), k
