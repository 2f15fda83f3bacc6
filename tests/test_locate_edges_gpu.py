# -*- coding: utf-8 -*-
"""
The locate sweeps (csrc/qm_locate.hpp, qm_engine_locate_fits and qm_engine_rbf_peak) past one pass of their reduction
grids, against the high-precision restatements of tests/locate_edges_ref.py.  The arg-max, divide, sum and moment
kernels are grid-stride loops over kFitBlocks x kFitBlock = 262 144 threads; the maps here have 543 348 nodes (86 x 81
x 78: two full passes and a partly filled third) or 540 000 (3 x 400 x 450), the interpolant's fine grid 65^3 = 274 625
points.  tests/test_locate_edges_host.py asserts, on the reference alone, what each case relies on: where its maximum
falls, that its fits are well conditioned, what its threshold selects.  Every input comes from a seeded generator.

The bounds are the project's own for these quantities (tests/test_gpu_parity.py), none of them a measurement:

* the normalised map, ``map_max``, every index and the spline location: equal;
* the smoothed map: 1e-14 absolute, against the longdouble direct convolution (no FFT, no tap cut-off);
* the smoothed mean, the total weight, the expectation and the diagonal of the covariance: 1e-12 relative, against
  longdouble sums;
* the off-diagonal covariance: ``1e-12 sqrt(cov_aa cov_bb)`` absolute.  The kernel adds at most 3 terms serially per
  thread and folds them through two trees of 8 and 10 levels, so its sum is within about 21 x 2^-53 of ``sum |terms|``,
  and by Cauchy-Schwarz ``sum w |dx| |dy| <= sqrt(sum w dx^2 sum w dy^2)``; a relative bound would be wrong, the terms
  cancel;
* the Gaussian location 1e-8, its sigma 1e-7 relative, against ``np_gaufit3d`` of the reference's smoothed map;
* the interpolant's maximum: 1e-12 relative, its index equal.

NaN: the kernels give ``nanmax`` / ``nanargmax`` / ``nansum``; the direct convolution spreads a NaN only as far as its
taps reach (the reference's FFT spreads it over the whole map), so of the smoothed map only finiteness beyond
``2 (ceil(9.6 sgm) + 1)`` nodes of a NaN is asserted.

Each case prints its worst differences before it asserts; profiles/locate_edges_gpu.txt is the output of one such run
on an MI355X.  Observed there: smoothed map at most 8.6e-16 from the longdouble one (sgm 3.3 on 64 x 63 x 40; 2.3e-16 to
7.4e-16 on the large maps), its mean within 2.6e-16, the Gaussian location the reference's to the last bit in all but
one case (1.8e-16), sigma within 9.7e-16; weight, expectation and diagonal covariance within 2.9e-16, the off-diagonal
terms within 3.9e-17 of sqrt(cov_aa cov_bb); the interpolant's maximum within 3.3e-14 (n = 9, whose weights cancel).

Hand mutations of the kernels that this file notices and the tests of test_gpu_parity.py on their maps of at most
7 056 nodes do not: the arg-max fold without its lower-index rule (three of the six placements of two equal maxima and
the interpolant's "face" case; the other placements are the ones such a fold gets right by the order of its threads),
the sum or a moment sweep striding by one node less than the grid, the sum launched on half the blocks with all the
partials folded.  The same short stride in the arg-max or the divide sweep changes no result on any map of up to
three trips -- every node is still visited, some twice, and neither a maximum nor a quotient minds -- so nothing here or
anywhere can notice it; a stride one node too long skips the first node of the second trip, which is where
"first_of_pass1" puts its maximum.
"""

import numpy as np
import pytest

import locate_edges_ref as ref

pytestmark = pytest.mark.gpu

ONES = (1.0, 1.0, 1.0)
FIELDS = ("map_max", "peak", "smoothed_mean", "smoothed_peak", "weight", "expectation", "covariance", "pass_maxima",
          "gaussian_window", "spline_window")


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in FIELDS)


def absdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - np.asarray(b, dtype=np.longdouble))))


def relerr(got, want):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def fits_on_host(eng, m, spacing=ONES, sgm=0.8, cov_thresh=0.90):
    """One call, host arrays in and out: (the engine's dict, normalised map, smoothed map)."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    norm, smoothed = np.zeros_like(m), np.zeros_like(m)
    dev = eng.locate_fits(m, spacing, sgm=sgm, cov_thresh=cov_thresh, norm_out=norm, smoothed_out=smoothed)
    return dev, norm, smoothed


def check_maxima(dev, norm, m):
    """``map_max``, ``peak`` and the normalised map against the nanmax restatement, NaN staying NaN."""
    with np.errstate(invalid="ignore"):
        want = m / np.nanmax(m)
    assert dev["map_max"] == np.nanmax(m)
    assert np.array_equal(dev["peak"], np.unravel_index(np.nanargmax(want), want.shape))
    assert np.array_equal(bits(norm), bits(want))
    return want


def check_moments(dev, norm, spacing, thresh, what):
    total, mean, cov = ref.moments(norm, spacing, thresh)
    scale = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    off = ~np.eye(3, dtype=bool)
    d_w, d_e = relerr(dev["weight"], total), relerr(dev["expectation"], mean)
    d_c = relerr(np.diag(dev["covariance"]), np.diag(cov))
    d_o = float(np.max((np.abs(dev["covariance"] - cov) / scale)[off]))
    print(f"{what} thresh {thresh} spacing {tuple(spacing)}: weight {d_w:.1e}, expectation {d_e:.1e}, "
          f"cov diagonal {d_c:.1e} (relative), off-diagonal {d_o:.1e} of sqrt(cov_aa cov_bb)")
    assert d_w <= 1e-12 and d_e <= 1e-12 and d_c <= 1e-12 and d_o <= 1e-12
    assert np.array_equal(dev["covariance"], dev["covariance"].T)


def check_against_reference(eng, name, sgm):
    """Everything section 1 of the file asserts, for ``ref.named_map(name)`` at ``sgm``."""
    from quakemigrate_amd import locate

    m = ref.named_map(name)
    r = ref.reference(name, sgm)
    want_loc, want_sigma, want_spline = ref.fit_reference(name, sgm)
    dev, norm, smoothed = fits_on_host(eng, m, sgm=sgm)
    gaussian, sigma, _ = locate.gaussian_from_window(dev["gaussian_window"], dev["smoothed_mean"],
                                                     dev["smoothed_peak"], m.shape)
    spline = locate.spline_from_window(dev["spline_window"], dev["peak"], m.shape, engine=eng)
    print(f"{name} {m.shape} sgm {sgm}: smoothed {absdiff(smoothed, r['smoothed']):.2e} absolute, mean "
          f"{relerr(dev['smoothed_mean'], r['smoothed_mean']):.1e}, gaussian {relerr(gaussian, want_loc):.1e}, "
          f"sigma {relerr(sigma, want_sigma):.1e} relative; peak {dev['peak'].tolist()} "
          f"(pass {ref.pass_of(ref.flat_of(m.shape, dev['peak']))}), smoothed peak {dev['smoothed_peak'].tolist()}, "
          f"spline {spline.tolist()}")
    assert dev["map_max"] == r["map_max"]
    assert np.array_equal(dev["peak"], r["peak"])
    assert np.array_equal(bits(norm), bits(r["norm"]))
    assert absdiff(smoothed, r["smoothed"]) <= 1e-14
    assert relerr(dev["smoothed_mean"], r["smoothed_mean"]) <= 1e-12
    assert np.array_equal(dev["smoothed_peak"], r["smoothed_peak"])
    np.testing.assert_allclose(gaussian, want_loc, rtol=1e-8)
    np.testing.assert_allclose(sigma, want_sigma, rtol=1e-7)
    assert np.array_equal(spline, want_spline)
    return dev


# =====================================================================================================================
# 1. where the maximum lies x sgm
# =====================================================================================================================
@pytest.mark.parametrize("name,sgm", ref.PEAK_CASES)
def test_peak_in_every_pass(engine, name, sgm):
    """The maximum in the first pass, on the first node of the second, in the third with its 5^3 window inside the grid
    and on the last node (both windows clipped, a 3^3 cube left to the spline), at sgm 0.8 and 2.0; sgm 3.0 (61 taps
    on every axis) and 0.3 once."""
    dev = check_against_reference(engine, name, sgm)
    if name == "last_node":
        assert np.isnan(dev["spline_window"]).sum() == 125 - 27 and np.isnan(dev["gaussian_window"]).any()
    else:
        assert np.isfinite(dev["spline_window"]).all()


def test_flat_grid_with_an_axis_shorter_than_the_taps(engine):
    """3 x 400 x 450: the x axis holds 3 of the 19 taps, the other two all of them; three passes."""
    check_against_reference(engine, "flat", 0.8)


# =====================================================================================================================
# 2. the moments over all passes
# =====================================================================================================================
@pytest.mark.parametrize("spacing", ref.MOMENT_SPACINGS)
def test_moments_span_all_passes(engine, spacing):
    """A threshold below the floor gives every one of the 543 348 nodes weight; 0.90 and 0.99 leave a handful, which
    straddle the boundary between the second and the third pass."""
    m = ref.named_map("moments")
    for thresh in ref.MOMENT_THRESHOLDS:
        dev, norm, _ = fits_on_host(engine, m, spacing=spacing, cov_thresh=thresh)
        want = check_maxima(dev, norm, m)
        check_moments(dev, want, spacing, thresh, "moments")


# =====================================================================================================================
# 3. the first index among equal maxima
# =====================================================================================================================
@pytest.mark.parametrize("name", sorted(ref.tie_pairs()))
def test_first_of_two_equal_maxima(engine, name):
    """Two nodes with exactly the largest value: the lower flat index is the peak, whichever block, thread or trip
    finds it (the placements: ref.tie_pairs, asserted in the host file)."""
    first, second = ref.tie_pairs()[name]
    m = ref.tie_map((first, second))
    dev, norm, _ = fits_on_host(engine, m)
    got = ref.flat_of(m.shape, dev["peak"])
    print(f"{name}: equal maxima at flat {first} and {second}, peak at {got}")
    assert got == first and dev["map_max"] == m.max()
    check_maxima(dev, norm, m)
    # the window is taken around that node
    assert dev["spline_window"][2, 2, 2] == 1.0


@pytest.mark.parametrize("name", ["centre", "face"])
def test_first_of_equal_maxima_of_the_interpolant(engine, name):
    """rbf_peak's arg-max on 65^3 points: one unit weight makes the interpolant r^3 about its centre, with every
    coordinate exact (the step is 1/32), so the farthest corners carry the same bits -- eight of them in both passes
    ("centre"), or four in the second pass, the first two in one block with the later one on the thread whose value a
    fold without the index rule would keep ("face").  No cube was found cheaply whose equal maxima put the LOWER index
    into a HIGHER block of another pass, as the map cases do: bit-equal values need a single weight (or two, mirrored),
    and the maxima of such an interpolant are corners of the fine grid, which lie in block order."""
    w = ref.rbf_tie_weights()[name]
    dense = ref.rbf_dense(w, ref.RBF_TIE_UPSCALE)
    best = np.flatnonzero(dense.ravel() == dense.max())
    value, got = engine.rbf_peak(w, ref.RBF_TIE_UPSCALE)
    print(f"interpolant '{name}': equal maxima at flat {best.tolist()}, peak at {np.ravel_multi_index(got, dense.shape)}")
    assert np.ravel_multi_index(got, dense.shape) == best[0]
    np.testing.assert_allclose(value, dense.max(), rtol=1e-12)


# =====================================================================================================================
# 4. NaN
# =====================================================================================================================
def far_from_nan(m, sgm):
    from scipy.ndimage import maximum_filter

    near = maximum_filter(np.isnan(m).astype(np.uint8), size=2 * ref.nan_reach(sgm) + 1, mode="constant", cval=0)
    assert (near == 0).sum() > m.size // 4
    return near == 0


def test_nan_block_away_from_the_peak(engine):
    from quakemigrate_amd import locate

    m = ref.nan_block_map()
    dev, norm, smoothed = fits_on_host(engine, m, cov_thresh=0.005)
    want = check_maxima(dev, norm, m)
    assert np.isnan(norm).sum() == np.isnan(m).sum() == 60
    check_moments(dev, want, ONES, 0.005, "NaN block")
    dev90, _, _ = fits_on_host(engine, m)
    check_moments(dev90, want, ONES, 0.90, "NaN block")
    spline = locate.spline_from_window(dev["spline_window"], dev["peak"], m.shape, engine=engine)
    assert np.array_equal(spline, ref.spline_reference("last_pass"))       # the NaNs are outside the window
    assert np.isfinite(smoothed[far_from_nan(m, 0.8)]).all() and np.isnan(smoothed).any()


def test_single_nan_where_the_maximum_would_be(engine):
    m = ref.nan_at_peak_map()
    dev, norm, smoothed = fits_on_host(engine, m, cov_thresh=0.005)
    want = check_maxima(dev, norm, m)
    assert dev["map_max"] < ref.named_map("last_pass").max() and np.isnan(norm).sum() == 1
    check_moments(dev, want, ONES, 0.005, "NaN at the top")
    dev90, _, _ = fits_on_host(engine, m)
    check_moments(dev90, want, ONES, 0.90, "NaN at the top")
    assert np.isnan(dev["spline_window"]).sum() == 1
    assert np.isfinite(smoothed[far_from_nan(m, 0.8)]).all()


@pytest.mark.parametrize("fill", [np.nan, 0.0])
def test_map_without_a_finite_value_is_refused(lib, engine, fill):
    """All NaN, and all zero (whose normalised map is 0 / 0)."""
    for shape in (ref.SMALL, ref.MAIN):
        with pytest.raises(lib.QMHipError, match="no finite value"):
            engine.locate_fits(np.full(shape, fill), ONES)
    # the engine is none the worse for it
    check_against_reference(engine, "pass0", 0.8)


# =====================================================================================================================
# 5. refusals and limits
# =====================================================================================================================
def test_tap_limit(lib, engine):
    """sgm 3.3 reaches 33 nodes either way: 65 or more taps on an axis of 65 or more nodes, refused; 64 on an axis of 64
    nodes, the most the kernel's table holds."""
    with pytest.raises(lib.QMHipError, match="taps"):
        engine.locate_fits(ref.named_map("pass0"), ONES, sgm=3.3)
    with pytest.raises(lib.QMHipError, match="taps"):
        engine.locate_fits(np.ones((65, 5, 5)), ONES, sgm=3.3)
    engine.locate_fits(ref.named_map("pass0"), ONES, sgm=3.125)
    check_against_reference(engine, "short", 3.3)


def test_rbf_peak_argument_bounds(lib, engine):
    for n, upscale in [(1, 10), (10, 10), (5, 0), (5, 65)]:
        with pytest.raises(lib.QMHipError, match="2 <= n <= 9"):
            engine.rbf_peak(np.ones((n, n, n)), upscale)
    # the bounds themselves are served
    rng = np.random.default_rng(61)
    for n, upscale in [(2, 1), (2, 64), (9, 1)]:
        w = rng.standard_normal((n, n, n))
        dense = ref.rbf_dense(w, upscale)
        order = np.argsort(dense.ravel())
        assert dense.ravel()[order[-1]] - dense.ravel()[order[-2]] > 1e-9 * np.abs(dense).max()
        value, got = engine.rbf_peak(w, upscale)
        assert np.ravel_multi_index(got, dense.shape) == order[-1]


# =====================================================================================================================
# 6. host and device paths, reuse, repeatability
# =====================================================================================================================
def test_host_and_device_paths_give_the_same_bits(engine):
    import torch

    m = np.array(ref.named_map("last_pass"))                            # (a writable copy, for torch)
    dev_h, norm_h, smooth_h = fits_on_host(engine, m, spacing=(0.5, 0.5, 0.25))
    again, norm_2, smooth_2 = fits_on_host(engine, m, spacing=(0.5, 0.5, 0.25))
    assert same_bits(dev_h, again) and np.array_equal(bits(norm_h), bits(norm_2))
    assert np.array_equal(bits(smooth_h), bits(smooth_2))
    dm = torch.from_numpy(m).cuda()
    dnorm, dsmooth = torch.full_like(dm, -1.0), torch.full_like(dm, -1.0)
    torch.cuda.synchronize()                                            # (the engine runs on a stream of its own)
    dev_d = engine.locate_fits(dm, (0.5, 0.5, 0.25), norm_out=dnorm, smoothed_out=dsmooth)
    torch.cuda.synchronize()
    assert same_bits(dev_h, dev_d)
    assert np.array_equal(bits(dnorm.cpu().numpy()), bits(norm_h))
    assert np.array_equal(bits(dsmooth.cpu().numpy()), bits(smooth_h))
    assert np.array_equal(dm.cpu().numpy(), m)                          # the input is left alone
    # without the maps, and with one of them
    bare = engine.locate_fits(m, (0.5, 0.5, 0.25))
    one = np.zeros_like(m)
    only_smoothed = engine.locate_fits(dm, (0.5, 0.5, 0.25), smoothed_out=one)
    assert same_bits(dev_h, bare) and same_bits(dev_h, only_smoothed) and np.array_equal(bits(one), bits(smooth_h))


def test_fit_buffers_reused_across_map_sizes(lib, engine):
    """Large, small, an interpolant (which shares the first map buffer and the partials), large again, on one engine:
    each gives the bits of a fresh engine."""
    from quakemigrate_amd import locate

    big, small = ref.named_map("first_of_pass1"), ref.named_map("small")
    n, upscale, centre, scale, seed = ref.RBF_CASES[0]
    weights = locate._cubic_rbf_weights(ref.rbf_window(n, centre, scale, seed))
    fresh = {}
    for key, m in (("big", big), ("small", small)):
        eng = lib.Engine(0)
        fresh[key] = fits_on_host(eng, m, sgm=2.0)
        eng.close()
    eng = lib.Engine(0)
    fresh_peak = eng.rbf_peak(weights, upscale)
    eng.close()
    for key in ("big", "small", "rbf", "big", "rbf", "small", "big"):
        if key == "rbf":
            assert engine.rbf_peak(weights, upscale) == fresh_peak
            continue
        dev, norm, smoothed = fits_on_host(engine, big if key == "big" else small, sgm=2.0)
        want, want_norm, want_smoothed = fresh[key]
        assert same_bits(dev, want), key
        assert np.array_equal(bits(norm), bits(want_norm)) and np.array_equal(bits(smoothed), bits(want_smoothed)), key


# =====================================================================================================================
# 7. the interpolant past one pass
# =====================================================================================================================
@pytest.mark.parametrize("case", ref.RBF_CASES, ids=lambda c: f"n{c[0]}-up{c[1]}-seed{c[4]}")
def test_rbf_peak_past_one_pass(engine, case):
    """n = 5, upscale = 16: 65^3 = 274 625 points, 12 481 of them on the second trip; maxima in either pass.  n = 2 and
    n = 9, the bounds, at a small refinement."""
    from quakemigrate_amd import locate

    n, upscale, centre, scale, seed = case
    sub = ref.rbf_window(n, centre, scale, seed)
    dense = locate._cubic_rbf_on_grid(sub, upscale)
    want = int(np.nanargmax(dense))
    value, got = engine.rbf_peak(locate._cubic_rbf_weights(sub), upscale)
    got = int(np.ravel_multi_index(got, dense.shape))
    print(f"n {n} upscale {upscale}: maximum at flat {got} (pass {ref.pass_of(got)}, block {ref.block_of(got)}), "
          f"value off by {relerr(value, dense.ravel()[want]):.1e} relative")
    assert got == want
    np.testing.assert_allclose(value, dense.ravel()[want], rtol=1e-12)
