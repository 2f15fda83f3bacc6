# -*- coding: utf-8 -*-
"""
CPU-side checks (no GPU) of the restatements the edge tests of the onset stage, table serving and the volume scan
compare against (tests/stage_edges_ref.py): each is pinned to what the repository already trusts -- the fixtures
recorded from the reference's own classes, the C oracle on input where it is defined, exact window sums -- and the
launch arithmetic they restate gives the splits the GPU tests rely on.
"""

import numpy as np

import stage_edges_ref as ref
from conftest import load_golden

U = 2.0 ** -53                  # unit round-off of float64


# -- table serving -----------------------------------------------------------------------------------------------------
def test_serve_expected_equals_the_recorded_tables():
    """The explicit cast rule (in range: the value; otherwise INT32_MIN) against both tables recorded from the
    reference's LUT class, the non-finite one included."""
    g = load_golden("serve_traveltimes")
    index = {k: i for i, k in enumerate(g["keys"])}
    rows = [index[k] for k, v in zip(g["availability_keys"], g["availability_values"]) if v == 1]
    assert np.array_equal(ref.serve_expected(g["grids"], rows, 50), g["served_50"])
    dec = tuple(int(v) for v in g["decimate"])
    assert np.array_equal(ref.serve_expected(g["grids"], rows, 250, dec), g["served_dec_250"])
    nf = load_golden("serve_nonfinite")
    want = ref.serve_expected(nf["grids"], [0, 1, 2], 50)
    assert want.dtype == np.int32 and np.array_equal(want, nf["served_50"])
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.stack(list(nf["grids"]), axis=-1) * 50.0)
    outside = ~(np.isfinite(r) & (r >= -2.0 ** 31) & (r <= 2.0 ** 31 - 1))
    print("serve_nonfinite: entries outside int32:", int(outside.sum()))
    assert outside.sum() == 27 and (want[outside] == ref.INT32_MIN).all()


def test_serve_expected_at_the_int32_edges():
    """The edges themselves, written as literals: half-to-even, then the range test on the ROUNDED value."""
    vals = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, -0.0, 5e-324, 2147483647.0, 2147483647.5, 2147483648.0,
                     -2147483648.0, -2147483648.5, -2147483649.0, 1e300, np.inf, -np.inf, np.nan])
    lo = ref.INT32_MIN
    want = [0, 2, 2, 0, -2, -2, 0, 0, 2147483647, lo, lo, lo, lo, lo, lo, lo, lo, lo]
    got = ref.serve_expected([vals.reshape(1, 1, -1)], [0], 1.0)
    assert got.shape == (1, 1, len(vals), 1) and got.ravel().tolist() == want
    # -2147483648.5 rounds to -2^31, which IS in range (and is INT32_MIN); -2147483649.0 is not, and gives the same
    assert np.rint(-2147483648.5) == -2.0 ** 31


def test_serving_launch_arithmetic():
    """qm_engine_serve: 256 nodes per workgroup up to 62 rows (pitch 63 words), the 64-node kernel from 63 rows
    (pitch 65: 256 x 65 x 4 = 66 560 bytes do not fit 64 KB) up to 254 (pitch 255), refused from 255."""
    assert ref.serve_plan(62) == (256, 63, 64512)
    assert ref.serve_plan(63) == (64, 65, 16640)
    assert ref.serve_plan(64) == (64, 65, 16640)
    assert ref.serve_plan(254) == (64, 255, 65280)
    assert ref.serve_plan(255)[0] == 0
    assert all(ref.serve_plan(s)[0] == 256 for s in range(1, 63))
    assert all(ref.serve_plan(s)[0] == 64 for s in range(63, 255))
    assert all(ref.serve_plan(s)[1] % 2 == 1 and ref.serve_plan(s)[1] - s in (1, 2) for s in range(1, 255))


# -- onset stage -------------------------------------------------------------------------------------------------------
def test_onset_stage_strict_agrees_with_the_recorded_onsets():
    """Fixture onset_stage (the reference's STALTAOnset._onset on its own C STA/LTA): both positions, the two transforms
    the stage applies itself, taper and no taper, at the tolerance the GPU test of the stage uses for it."""
    g = load_golden("onset_stage")
    args = (g["signals"], g["trace_row"], g["nsta"], g["nlta"])
    worst = 0.0
    for pos in ("classic", "centred"):
        for tf in ("energy", "abs"):
            raw, logged = ref.onset_stage_strict(*args, transform=tf, position=pos, taper_pad=int(g["taper_pad"]),
                                                 min_onset_value=float(g["min_onset_value"]))
            worst = max(worst, float(np.max(np.abs(raw / g[f"raw_{pos}_{tf}"] - 1))))
            np.testing.assert_allclose(raw, g[f"raw_{pos}_{tf}"], rtol=1e-12)
            np.testing.assert_allclose(logged, g[f"log_{pos}_{tf}"], rtol=1e-12, atol=1e-14)
    raw, _ = ref.onset_stage_strict(*args, taper_pad=-1, min_onset_value=0.01)
    np.testing.assert_allclose(raw, g["raw_classic_energy_notaper"], rtol=1e-12)
    print(f"onset_stage fixture: largest relative deviation of the strict rows {worst:.2e}")


def test_stalta_strict_agrees_with_the_recorded_vectors(oracle):
    """Fixture stalta (the reference's three C functions, the toy case of its tests and a random trace); the recursive
    one at the GPU test's 1e-15, the windowed ones at the 1e-12 the onset stage is held to.  Then the C oracle at the
    window edges where the reference is defined."""
    g = load_golden("stalta")
    for sig, ns, nl, pre in ((g["toy"], 2, 3, "toy_"), (g["signal"], int(g["nsta"]), int(g["nlta"]), "")):
        for pos, kind in zip(ref.POSITIONS, ("overlapping", "centred", "recursive")):
            got = ref.stalta_strict(sig, ns, nl, pos)[2]
            np.testing.assert_allclose(got, g[pre + kind], rtol=1e-15 if pos == "recursive" else 1e-12, atol=0)
    assert (g["signal"] >= 0).all()
    raw, _ = ref.onset_stage_strict(g["signal"][None, :], [0], [int(g["nsta"])], [int(g["nlta"])], transform="abs",
                                    position="recursive", taper_pad=-1, min_onset_value=0.0)
    np.testing.assert_allclose(raw[0], g["recursive"], rtol=1e-15, atol=0)
    x = np.random.default_rng(21).standard_normal(64) ** 2
    for pos, fn, windows in (("classic", oracle.c_overlapping_sta_lta, [(1, 1), (1, 2), (5, 5), (3, 61), (3, 64)]),
                             ("centred", oracle.c_centred_sta_lta, [(1, 1), (1, 2), (5, 5), (3, 61)]),
                             ("recursive", oracle.c_recursive_sta_lta, [(3, 10), (3, 64), (3, 70)])):
        for ns, nl in windows:
            np.testing.assert_allclose(ref.stalta_strict(x, ns, nl, pos)[2], fn(x, ns, nl), rtol=1e-12, atol=0,
                                       err_msg=f"{pos} {ns} {nl}")


def test_stalta_strict_rules_where_the_reference_has_none():
    x = np.random.default_rng(22).standard_normal(64) ** 2
    ones = np.ones(64)
    for pos in ("classic", "centred"):
        for ns, nl in ((3, 65), (6, 5), (0, 5)):
            assert np.array_equal(ref.stalta_strict(x, ns, nl, pos)[2], ones), (pos, ns, nl)
    assert np.array_equal(ref.stalta_strict(x, 3, 62, "centred")[2], ones)
    assert not np.array_equal(ref.stalta_strict(x, 3, 62, "classic")[2], ones)
    # nsta + nlta == n: the centred loop is empty, only sample nlta - 1 carries a ratio
    o = ref.stalta_strict(x, 3, 61, "centred")[2]
    assert o[60] != 1.0 and np.array_equal(np.delete(o, 60), np.ones(63))
    # recursive: sample 0 is never written; the first nlta samples are nulled only when nlta < n
    for nl, nulled in ((10, True), (63, True), (64, False), (70, False)):
        o = ref.stalta_strict(x, 3, nl, "recursive")[2]
        assert (o[0] == 1.0) == nulled and (o[0] == 0.0) != nulled
        assert np.array_equal(o[:nl] == 1.0, np.full(min(nl, 64), nulled))


def test_strict_sums_stay_within_the_rounding_bound_on_the_stress_trace():
    """
    Each update ``s = s + (in - out)`` rounds twice: the difference (|in - out| <= max f <= M, every sample lying in
    some window and f >= 0) and the sum (|s| <= M (1 + small)), M the largest exact sum of a window of that length.  So
    after at most T updates the running sum is within 2 T 2^-53 M (1 + small) <= 3 T 2^-53 M of the exact window sum.
    Observed here: 9.4e-4 of that bound at the most (the errors do not line up) -- while in the gap of zeros behind
    the burst the residue, ~1e-9, is everything the sum holds.
    """
    xs = ref.stress_traces()
    n, ns, nl = xs.shape[1], 7, 60
    worst, signs = 0.0, set()
    for tf in ("energy", "abs"):
        for x in xs:
            f = x * x if tf == "energy" else np.abs(x)
            exact_s, exact_l = ref.window_sums_exact(f, ns), ref.window_sums_exact(f, nl)
            bound_s, bound_l = 3 * n * U * np.nanmax(exact_s), 3 * n * U * np.nanmax(exact_l)
            S, L, _ = ref.stalta_strict(f, ns, nl, "classic")
            v = np.arange(nl - 1, n)                        # S[i], L[i]: the windows ENDING at i
            r_cs = float(np.max(np.abs(S[v] - exact_s[v]))) / bound_s
            r_cl = float(np.max(np.abs(L[v] - exact_l[v]))) / bound_l
            S2, L2, o2 = ref.stalta_strict(f, ns, nl, "centred")
            v2 = np.arange(nl - 1, n - ns)                  # centred: the short window STARTS behind i
            r_ns = float(np.max(np.abs(S2[v2] - exact_s[v2 + ns]))) / bound_s
            r_nl = float(np.max(np.abs(L2[v2] - exact_l[v2]))) / bound_l
            print(f"stress trace, {tf}: |strict - exact| / (3 T 2^-53 max window sum): classic S {r_cs:.2e} "
                  f"L {r_cl:.2e}, centred S {r_ns:.2e} L {r_nl:.2e}; L in the gap {L2[1300]:.2e}")
            worst = max(worst, r_cs, r_cl, r_ns, r_nl)
            # the point of the traces: where the exact long sum is 0 the running one is not, with either sign, and
            # the centred guard follows that sign
            dead = np.flatnonzero(exact_l == 0.0)
            assert len(dead) > 100 and dead[0] > nl and dead[-1] < n - ns
            assert np.all(L[dead] != 0.0) and np.array_equal(L[dead], L2[dead])
            assert np.array_equal(o2[dead] == 1.0, L2[dead] <= 0.0)
            signs.add((tf, bool(L2[1300] > 0.0)))
    print(f"stress traces: worst ratio {worst:.2e}")
    assert worst <= 1.0
    assert len(signs) == 4


# -- volume scan -------------------------------------------------------------------------------------------------------
def test_scan_expected_equals_the_numpy_oracle_without_nans(oracle):
    rng = np.random.default_rng(3)
    vol = rng.lognormal(0, 1, size=(321, 77))
    vol[300, 5] = vol[17, 5] = vol[:, 5].max() + 1.0       # a tie: the first one
    vol[:, 9] = 2.5                                         # all equal: index 0
    a, b, c = ref.scan_expected(vol)
    wa, wb, wc = oracle.np_find_max_coa(vol)
    assert np.array_equal(c, wc) and c[5] == 17 and c[9] == 0
    assert np.array_equal(a, wa)
    # positive values: the oracle's sequential sum is within (N - 1) 2^-53 of fsum's
    np.testing.assert_allclose(b, wb, rtol=2 * 321 * U, atol=0)
    vol[4, 11] = np.nan
    vol[:, 13] = np.nan
    a, b, c = ref.scan_expected(vol)
    assert c[11] == wc[11] and a[11] == wa[11] and np.isnan(b[11])
    assert c[13] == 0 and a[13] == -np.inf and np.isnan(b[13])


def test_scan_launch_arithmetic_at_256_compute_units():
    """scan_fold's split of the shapes the GPU test scans, at the MI355X's 256 CUs and the default 32 wavefronts per
    CU: the remainder loop only, two sets, a second time workgroup whose last wavefront lies past the end, and 66
    sets -- more than the 64 the combine's 16 wavefronts x 4 loads take in one pass."""
    assert ref.scan_plan(1, 1, 256) == dict(tiles=1, xgroups=1, waves=1, sets=1, per=1, last=1)
    assert ref.scan_plan(65, 7, 256) == dict(tiles=2, xgroups=1, waves=2, sets=1, per=7, last=7)
    assert ref.scan_plan(300, 513, 256) == dict(tiles=5, xgroups=1, waves=5, sets=2, per=257, last=256)
    assert ref.scan_plan(1025, 1000, 256) == dict(tiles=17, xgroups=2, waves=9, sets=3, per=334, last=332)
    assert ref.scan_plan(70, 17000, 256) == dict(tiles=2, xgroups=1, waves=2, sets=66, per=258, last=230)
    assert ref.scan_plan(7, 17000, 256)["sets"] == 66 and (1 << 20) // (8 * 17000) == 7     # the 1 MiB chunks


def test_onset_lds_boundary():
    assert ref.onset_in_lds(20480) and not ref.onset_in_lds(20481)
