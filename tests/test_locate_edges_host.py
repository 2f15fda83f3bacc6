# -*- coding: utf-8 -*-
"""
CPU-side checks (no GPU) of tests/locate_edges_ref.py: the instrument -- the longdouble direct convolution and moments
against the float64 restatements the repository already trusts (oracle.np_gaufilt3d, oracle.np_covfit3d,
locate._cubic_rbf_on_grid) -- and the conditions every case of tests/test_locate_edges_gpu.py relies on, asserted on
the reference alone: which pass, block and thread of the reduction grids a maximum falls into, that the fits are well
conditioned there, that the thresholds select what the case says.  A change of the constants in qm_locate.hpp or of a
recipe fails here instead of silently turning a case into a one-pass case.
"""

import numpy as np
import pytest

import locate_edges_ref as ref
from oracle import qm_oracle as oracle
from quakemigrate_amd import locate


def absdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - np.asarray(b, dtype=np.longdouble))))


# -- the constants and the choice of the main shape --------------------------------------------------------------------
def test_constants_come_from_the_header():
    text = ref.HEADER.read_text()
    assert ref.header_constant("kFitBlock", text) == ref.K_FIT_BLOCK
    edited = text.replace(f"kFitBlocks = {ref.K_FIT_BLOCKS};", f"kFitBlocks = {4 * ref.K_FIT_BLOCKS};")
    assert edited != text and ref.header_constant("kFitBlocks", edited) == 4 * ref.K_FIT_BLOCKS
    with pytest.raises(LookupError):
        ref.header_constant("kNoSuchConstant", text)
    assert ref.SWEEP == ref.K_FIT_BLOCK * ref.K_FIT_BLOCKS
    f = 2 * ref.SWEEP + 5 * ref.K_FIT_BLOCK + 7
    assert (ref.pass_of(f), ref.block_of(f), ref.thread_of(f)) == (2, 5, 7)
    assert ref.n_passes(ref.SWEEP) == 1 and ref.n_passes(ref.SWEEP + 1) == 2


def last_inner_node(shape, half=2):
    """The node of the largest flat index whose (2 half + 1)^3 window lies inside the grid."""
    return tuple(n - 1 - half for n in shape)


def test_main_shape_reaches_a_third_pass_with_room_for_a_window():
    n = int(np.prod(ref.MAIN))
    assert n > 2 * ref.SWEEP and ref.n_passes(n) == 3 and n % ref.SWEEP != 0
    assert {v % 2 for v in ref.MAIN} == {0, 1}                              # even and odd axes
    assert ref.pass_of(ref.flat_of(ref.MAIN, last_inner_node(ref.MAIN))) == 2
    # the shape one would try first: three passes, but no 5^3 window fits into the third
    assert ref.n_passes(np.prod(ref.REJECTED)) == 3
    assert ref.pass_of(ref.flat_of(ref.REJECTED, last_inner_node(ref.REJECTED))) == 1
    assert ref.n_passes(np.prod(ref.FLAT)) == 3 and ref.n_passes(np.prod(ref.SMALL)) == 1
    # the project's own grid
    assert ref.n_passes(201 * 201 * 101) == 16


# -- the instrument ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sgm", [(ref.REJECTED, 0.3), (ref.REJECTED, 0.8), (ref.REJECTED, 3.0), (ref.FLAT, 0.8)])
def test_direct_convolution_agrees_with_the_fft_and_with_the_kernels_arithmetic(shape, sgm):
    """longdouble without a cut-off, the FFT restatement, and float64 with the kernel's cut-off: the first two within
    the project's 1e-14, the third within 8e-16 of both."""
    if shape == ref.FLAT:
        norm, exact = ref.reference("flat", sgm)["norm"], ref.reference("flat", sgm)["smoothed"]
    else:
        m = ref.bump_map(shape, (40.3, 41.2, 36.9), 3.0, 0.05, seed=int(sgm * 10))
        norm = m / m.max()
        exact = ref.direct_gaufilt3d(norm, sgm)
    fft = oracle.np_gaufilt3d(norm, sgm)
    cut = ref.direct_gaufilt3d(norm, sgm, dtype=np.float64, reach=ref.tap_reach(sgm))
    assert exact.dtype == np.longdouble and cut.dtype == np.float64
    d = absdiff(exact, fft), absdiff(cut, exact), absdiff(cut, fft)
    print(f"{shape} sgm {sgm}: longdouble vs fft {d[0]:.2e}, float64 cut-off vs longdouble {d[1]:.2e}, vs fft {d[2]:.2e}")
    assert d[0] <= 1e-14 and d[1] <= 8e-16 and d[2] <= 8e-16


def test_axis_matrix_is_the_same_mode_convolution():
    """Against numpy.convolve on one axis, odd and even length; the mirrored pass is the transpose."""
    rng = np.random.default_rng(5)
    for n in (9, 10):
        x = rng.random(n)
        a = ref.axis_matrix(n, 1.3, np.float64)
        k = np.arange(n) - (n - 1) / 2
        flt = np.exp(-k * k / (2 * 1.3 * 1.3))
        full = np.convolve(x, flt)
        start = (n - 1) // 2
        np.testing.assert_allclose(a @ x, full[start:start + n], rtol=1e-14)
        np.testing.assert_allclose(a.T @ x, (a @ x[::-1])[::-1], rtol=1e-14)
    assert ref.tap_reach(0.8) == 9 and ref.tap_reach(3.0) == 30 and ref.tap_reach(3.3) == 33


def test_longdouble_moments_agree_with_covfit3d():
    norm = ref.reference("small", 0.8)["norm"]
    for spacing in ref.MOMENT_SPACINGS:
        for thresh in (0.0, 0.5, 0.9):
            total, mean, cov = ref.moments(norm, spacing, thresh)
            want_mean, want_cov = oracle.np_covfit3d(norm, spacing, thresh)
            assert total.dtype == np.longdouble
            np.testing.assert_allclose(float(total), norm[norm > thresh].sum(), rtol=1e-14)
            np.testing.assert_allclose(mean.astype(np.float64), want_mean, rtol=1e-12)
            scale = np.sqrt(np.outer(np.diag(want_cov), np.diag(want_cov)))
            assert np.all(np.abs(cov.astype(np.float64) - want_cov) <= 1e-12 * scale)


def test_rbf_dense_agrees_with_the_host_interpolant():
    """The weights alternate in sign, so the two orders of summation are compared on the scale of the terms: each sum
    of N = n^3 products is within (N + 2) 2^-53 of sum |w| r^3, whatever its order."""
    for n, upscale, centre, scale, seed in ref.RBF_CASES:
        sub = ref.rbf_window(n, centre, scale, seed)
        weights = locate._cubic_rbf_weights(sub)
        want = locate._cubic_rbf_on_grid(sub, upscale)
        got = ref.rbf_dense(weights, upscale)
        terms = ref.rbf_dense(np.abs(weights), upscale)
        assert np.all(np.abs(got - want) <= 2 * (n ** 3 + 2) * 2.0 ** -53 * terms)


# -- section 1: peak placement x sgm -----------------------------------------------------------------------------------
def window(a, centre, size):
    lo, hi = oracle.np_window_bounds(a.shape, centre, size)
    return a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], hi - lo


@pytest.mark.parametrize("name,sgm", ref.PEAK_CASES)
def test_peak_case_conditions(name, sgm):
    shape = ref.MAIN
    n = int(np.prod(shape))
    r = ref.reference(name, sgm)
    norm, smoothed = r["norm"], r["smoothed"]
    flat = ref.flat_of(shape, r["peak"])
    assert tuple(r["peak"]) == ref.placement_node(shape, name) and norm.ravel()[flat] == 1.0
    assert np.count_nonzero(norm == 1.0) == 1
    _, ext5 = window(norm, r["peak"], 5)
    if name == "pass0":
        assert ref.pass_of(flat) == 0 and tuple(ext5) == (5, 5, 5)
    elif name == "first_of_pass1":
        assert flat == ref.SWEEP and (ref.pass_of(flat), ref.block_of(flat), ref.thread_of(flat)) == (1, 0, 0)
        assert tuple(ext5) == (5, 5, 5)
    elif name == "last_pass":
        assert ref.pass_of(flat) == ref.n_passes(n) - 1 == 2 and tuple(ext5) == (5, 5, 5)
    else:
        assert flat == n - 1 and ref.pass_of(flat) == 2
        assert tuple(ext5) == (3, 3, 3) and tuple(window(smoothed, r["smoothed_peak"], 7)[1]) != (7, 7, 7)
    # the taps: within the limit, and sgm 3.0 fills 61 of them on every axis
    counts = [ref.tap_count(v, sgm, mirror) for v in shape for mirror in (False, True)]
    assert max(counts) <= ref.K_MAX_TAPS and (sgm != 3.0 or set(counts) == {61})
    check_fit_conditions(name, sgm)
    sub, ext = window(norm, r["peak"], 5)
    assert ext[0] == ext[1] == ext[2]
    if name == "last_node":
        # (a corner clips the window to a cube of 3^3: the interpolant is still used, and its peak stays inside)
        assert not np.array_equal(ref.spline_reference(name), r["peak"])


def check_fit_conditions(name, sgm):
    """What the comparison of the smoothed map, its peak, the Gaussian fit and the spline relies on."""
    r = ref.reference(name, sgm)
    norm, smoothed = r["norm"], r["smoothed"]
    # the instrument at this case: the project's bound for the smoothed map
    fft = oracle.np_gaufilt3d(norm, sgm)
    print(f"{name} sgm {sgm}: longdouble vs fft {absdiff(smoothed, fft):.2e}")
    assert absdiff(smoothed, fft) <= 1e-14

    # the smoothed peak is decided by far more than the bound
    top = np.sort(smoothed.ravel())[-2:]
    assert top[1] - top[0] > 1e-10
    # the Gaussian fit: a positive window (no clip to 1e-300), and well conditioned
    s64 = smoothed.astype(np.float64)
    win7, _ = window(s64, r["smoothed_peak"], 7)
    assert (win7 - float(r["smoothed_mean"])).min() > 1e-3
    loc, sigma, spline = ref.fit_reference(name, sgm)
    noise = 1e-14 * np.random.default_rng(7).uniform(-1, 1, s64.shape)
    loc2, sigma2, _ = oracle.np_gaufit3d(s64 + noise)
    moved = max(np.max(np.abs(loc2 - loc)), np.max(np.abs(sigma2 - sigma)))
    print(f"{name} sgm {sgm}: a 1e-14 perturbation moves the fit by {moved:.2e}")
    assert moved < 1e-10
    # the spline: the interpolant's two largest values are apart
    sub, ext = window(norm, r["peak"], 5)
    if ext[0] == ext[1] == ext[2]:
        dense = np.sort(locate._cubic_rbf_on_grid(sub, 10).ravel())
        assert (dense[-1] - dense[-2]) > 1e-10 * dense[-1]
    else:
        assert np.array_equal(spline, r["peak"])                    # no cube: the gridded maximum


@pytest.mark.parametrize("name,sgm", ref.OTHER_SMOOTH_CASES)
def test_other_smoothing_case_conditions(name, sgm):
    r = ref.reference(name, sgm)
    shape = r["norm"].shape
    check_fit_conditions(name, sgm)
    counts = [ref.tap_count(v, sgm, mirror) for v in shape for mirror in (False, True)]
    assert max(counts) <= ref.K_MAX_TAPS
    if name == "flat":
        assert shape[0] < ref.tap_reach(sgm) and ref.n_passes(np.prod(shape)) == 3
    if name == "short":
        assert max(shape) == ref.K_MAX_TAPS and max(counts) == ref.K_MAX_TAPS
        # ... and the same sgm is refused on every axis of the main shape, as on any of 65 nodes
        assert ref.tap_count(65, sgm) > ref.K_MAX_TAPS and ref.tap_count(65, 3.125) <= ref.K_MAX_TAPS
        assert all(ref.tap_count(v, sgm) > ref.K_MAX_TAPS for v in ref.MAIN)
    top = np.sort(r["smoothed"].ravel())[-2:]
    assert top[1] - top[0] > 1e-10


# -- section 2: the moments --------------------------------------------------------------------------------------------
def test_moment_case_conditions():
    norm = ref.named_map("moments") / ref.named_map("moments").max()
    n = norm.size
    low, mid, high = ref.MOMENT_THRESHOLDS
    assert low < norm.min()                                         # every node carries weight: all three passes
    assert ref.n_passes(n) == 3
    for thresh in (mid, high):
        idx = np.argwhere(norm > thresh)
        assert 4 <= len(idx) <= 1000                                # a handful
        assert all(len(np.unique(idx[:, a])) >= 2 for a in range(3))        # no moment is a bare zero
        assert {ref.pass_of(ref.flat_of(norm.shape, i)) for i in idx} == {1, 2}      # across a pass boundary
    for spacing in ref.MOMENT_SPACINGS:
        for thresh in ref.MOMENT_THRESHOLDS:
            total, mean, cov = ref.moments(norm, spacing, thresh)
            want_mean, want_cov = oracle.np_covfit3d(norm, spacing, thresh)
            np.testing.assert_allclose(mean.astype(np.float64), want_mean, rtol=1e-12)
            scale = np.sqrt(np.outer(np.diag(want_cov), np.diag(want_cov)))
            assert np.all(np.abs(cov.astype(np.float64) - want_cov) <= 1e-12 * scale)
            assert np.all(np.diag(cov) > 1e-3)


# -- section 3: equal maxima -------------------------------------------------------------------------------------------
def test_tie_pairs_sit_where_their_names_say():
    kb = ref.K_FIT_BLOCK
    pairs = ref.tie_pairs()
    where = {k: [(ref.pass_of(f), ref.block_of(f), ref.thread_of(f)) for f in v] for k, v in pairs.items()}
    for name, (first, second) in pairs.items():
        assert 0 <= first < second < np.prod(ref.MAIN)
        m = ref.tie_map((first, second))
        assert np.flatnonzero(m.ravel() == m.max()).tolist() == [first, second] and np.argmax(m) == first
    (p0, b0, _), (p1, b1, _) = where["high_block_first"]
    assert (p0, p1) == (0, 1) and b0 > b1
    assert abs(pairs["high_block_first"][0] - 200000) < kb and abs(pairs["high_block_first"][1] - 300000) < kb

    def tie_goes_to_second(t0, t1):
        """In the halving fold thread t takes from t + s: of two equal values the one on the thread with a zero
        in the lowest bit where the thread numbers differ is kept unless the index decides."""
        low = (t0 ^ t1) & -(t0 ^ t1)
        return (t1 & low) == 0

    (_, b0, _), (_, b1, _) = where["high_block_first_low_thread"]
    assert b0 > b1 and tie_goes_to_second(b0 % kb, b1 % kb)
    (_, b0, _), (_, b1, _) = where["same_fold_slot"]
    assert b0 % kb == b1 % kb and b1 < b0                           # one thread of the final fold meets b1 first
    (p0, b0, t0), (p1, b1, t1) = where["same_thread"]
    assert (p0 + 1, b0, t0) == (p1, b1, t1) and pairs["same_thread"][1] - pairs["same_thread"][0] == ref.SWEEP
    (p0, b0, t0), (p1, b1, t1) = where["same_block"]
    assert (p0, p1) == (0, 1) and b0 == b1 and tie_goes_to_second(t0, t1)
    (p0, b0, _), (p1, b1, _) = where["third_pass"]
    assert (p0, p1) == (0, 2) and b0 > b1


def test_rbf_tie_weights_give_equal_maxima_in_both_passes():
    u = ref.RBF_TIE_UPSCALE
    m = 2 * u + 1
    assert m ** 3 > ref.SWEEP
    w = ref.rbf_tie_weights()
    dense = ref.rbf_dense(w["centre"], u).ravel()
    best = np.flatnonzero(dense == dense.max())
    assert len(best) == 8 and best[0] == 0 and [ref.pass_of(f) for f in best] == [0] * 4 + [1] * 4
    dense = ref.rbf_dense(w["face"], u).ravel()
    best = np.flatnonzero(dense == dense.max())
    assert len(best) == 4 and all(ref.pass_of(f) == 1 for f in best)
    # the first two share a block, the later one on the thread that keeps a tie
    assert ref.block_of(best[0]) == ref.block_of(best[1])
    t0, t1 = ref.thread_of(best[0]), ref.thread_of(best[1])
    low = (t0 ^ t1) & -(t0 ^ t1)
    assert (t1 & low) == 0


# -- section 4: NaN ----------------------------------------------------------------------------------------------------
def test_nan_case_conditions():
    base = ref.named_map("last_pass")
    node = np.array(ref.PLACEMENTS["last_pass"]["node"])
    m = ref.nan_block_map()
    holes = np.argwhere(np.isnan(m))
    assert len(holes) == 4 * 5 * 3 and np.nanmax(m) == base.max()
    assert np.abs(holes - node).max(axis=1).min() > ref.nan_reach(0.8) + 3          # far from both windows
    m = ref.nan_at_peak_map()
    assert np.argwhere(np.isnan(m)).tolist() == [node.tolist()] and np.nanmax(m) < base.max()
    peak = np.array(np.unravel_index(np.nanargmax(m), m.shape))
    assert np.abs(peak - node).max() == 1
    top = np.sort(m[~np.isnan(m)])[-2:]
    assert top[1] > top[0]


# -- section 7: the interpolant past one pass --------------------------------------------------------------------------
def test_rbf_case_conditions():
    seen = []
    for n, upscale, centre, scale, seed in ref.RBF_CASES:
        m = (n - 1) * upscale + 1
        dense = locate._cubic_rbf_on_grid(ref.rbf_window(n, centre, scale, seed), upscale).ravel()
        order = np.argsort(dense)
        gap = (dense[order[-1]] - dense[order[-2]]) / dense[order[-1]]
        print(f"n {n} upscale {upscale}: maximum at flat {order[-1]} of {m ** 3}, relative gap {gap:.1e}")
        assert gap > 1e-10
        seen.append((n, upscale, ref.pass_of(order[-1]), ref.n_passes(m ** 3)))
    assert seen == [(5, 16, 1, 2), (5, 16, 1, 2), (5, 16, 0, 2), (2, 8, 0, 1), (9, 3, 0, 1)]
