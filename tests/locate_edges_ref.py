# -*- coding: utf-8 -*-
"""
High-precision restatements and inputs for the locate sweeps past one pass of their reduction grids
(tests/test_locate_edges_gpu.py), pinned on the CPU by tests/test_locate_edges_host.py.

The sweeps of csrc/qm_locate.hpp (arg-max, divide, sum, the two moment kernels) are grid-stride loops over a fixed grid
of ``kFitBlocks x kFitBlock`` threads: node ``flat`` is visited on trip ``flat // SWEEP`` of thread ``flat % kFitBlock``
of block ``(flat % SWEEP) // kFitBlock``.  The constants are read from the header, so that a change there moves the
cases' conditions (asserted in the host test) with it.

* ``direct_gaufilt3d``: ``QuakeScan._gaufilt3d`` (scan.py:1008-1043) as a separable linear convolution per axis in
  ``np.longdouble``, with no tap cut-off -- what fftconvolve(mode="same") computes, without the FFT's round-off.
  ``reach`` (the kernel's cut-off, ``tap_reach``) and ``dtype=np.float64`` give the kernel's own arithmetic.
* ``moments``: ``_covfit3d``'s thresholded weight, expectation and central second moments in ``np.longdouble``.
* ``rbf_dense``: the cubic radial-basis interpolant of given weights on the fine grid, the centres summed one after
  the other as rbf_dense_kernel does.
* ``bump_map`` and the tables of cases: the inputs of the GPU file, every one from a seeded generator.
* ``reference`` / ``fit_reference``: what the engine must return for a named map, computed once per process.
"""

import functools
import math
import pathlib
import re

import numpy as np

HEADER = pathlib.Path(__file__).resolve().parent.parent / "quakemigrate_amd" / "csrc" / "qm_locate.hpp"


def header_constant(name, text=None):
    """``constexpr int <name> = <value>;`` of qm_locate.hpp."""
    text = HEADER.read_text() if text is None else text
    found = re.search(r"constexpr\s+int\s+" + re.escape(name) + r"\s*=\s*(\d+)\s*;", text)
    if not found:
        raise LookupError(f"{name} not found in {HEADER.name}")
    return int(found.group(1))


K_FIT_BLOCK = header_constant("kFitBlock")
K_FIT_BLOCKS = header_constant("kFitBlocks")
K_MAX_TAPS = header_constant("kMaxTaps")
SWEEP = K_FIT_BLOCK * K_FIT_BLOCKS            # nodes one pass of a reduction grid covers


def pass_of(flat):
    return int(flat) // SWEEP


def block_of(flat):
    return (int(flat) % SWEEP) // K_FIT_BLOCK


def thread_of(flat):
    return int(flat) % K_FIT_BLOCK


def n_passes(n):
    return -(-int(n) // SWEEP)


def flat_of(shape, ijk):
    return int(np.ravel_multi_index(tuple(int(v) for v in ijk), shape))


# -- the smoothing ----------------------------------------------------------------------------------------------------
def tap_reach(sgm):
    """Offsets |d| the host code keeps (axis_taps, qm_widen.hip): exp(-9.6^2 / 2) = 1e-20 of the peak."""
    return int(math.ceil(sgm * 9.6)) + 1


def tap_count(n, sgm, mirror=False):
    """Number of taps axis_taps builds for an axis of ``n`` nodes (refused above kMaxTaps)."""
    c, r = (n - 1) // 2, tap_reach(sgm)
    return sum(1 for d in range(-r, r + 1) if 0 <= (-d if mirror else d) + c <= n - 1)


def axis_matrix(n, sgm, dtype=np.longdouble, reach=None):
    """
    ``A[i, j] = flt[i - j + (n - 1) // 2]`` with ``flt[k] = exp(-x^2 / (2 sgm^2))`` at ``x = k - (n - 1) / 2``, zero
    where the index leaves the filter: one axis of fftconvolve(map, gaussian_3d, "same").  Its transpose is the
    mirrored pass.  ``reach`` drops the offsets ``|i - j| > reach``.
    """
    dtype = np.dtype(dtype).type
    k = np.arange(n).astype(dtype)
    x = k - dtype(n - 1) / dtype(2)
    flt = np.exp(-(x * x) / (dtype(2) * dtype(sgm) * dtype(sgm)))
    i, j = np.indices((n, n))
    idx = i - j + (n - 1) // 2
    ok = (idx >= 0) & (idx <= n - 1)
    if reach is not None:
        ok &= np.abs(i - j) <= reach
    a = np.zeros((n, n), dtype=dtype)
    a[ok] = flt[idx[ok]]
    return a


def direct_gaufilt3d(map3d, sgm, dtype=np.longdouble, reach=None):
    """Filter along x, y, z; divide by the maximum; filter with the mirrored weights; divide again."""
    out = np.asarray(map3d).astype(dtype)
    mats = [axis_matrix(n, sgm, dtype, reach) for n in out.shape]
    for mirror in (False, True):
        ax, ay, az = [m.T if mirror else m for m in mats]
        out = np.einsum("ia,abc->ibc", ax, out)
        out = np.einsum("jb,ibc->ijc", ay, out)
        out = np.einsum("kc,ijc->ijk", az, out)
        out = out / np.nanmax(out)
    return out


# -- the moments ------------------------------------------------------------------------------------------------------
def moments(norm, spacing, thresh, dtype=np.longdouble):
    """(total weight, expectation [3], central second moments [3][3]) of the nodes with ``norm > thresh``."""
    norm = np.asarray(norm, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ix, iy, iz = np.nonzero(norm > thresh)                  # NaN carries no weight: nansum
    w = norm[ix, iy, iz].astype(dtype)
    pos = [i.astype(dtype) * np.float64(s).astype(dtype) for i, s in zip((ix, iy, iz), spacing)]
    total = w.sum()
    mean = [(w * p).sum() / total for p in pos]
    cov = np.zeros((3, 3), dtype=dtype)
    for a in range(3):
        for b in range(3):
            cov[a, b] = (w * (pos[a] - mean[a]) * (pos[b] - mean[b])).sum() / total
    return total, np.array(mean), cov


# -- the interpolant --------------------------------------------------------------------------------------------------
def rbf_dense(weights, upscale):
    """``dense[i, j, k] = sum_abc w[a, b, c] r^3``, ``r^2 = ((x_j - b)^2 + (y_i - a)^2) + (z_k - c)^2``, the centres
    added in the order a, b, c -- rbf_dense_kernel in NumPy float64 (locate._cubic_rbf_on_grid uses a BLAS dot)."""
    weights = np.asarray(weights, dtype=np.float64)
    n = weights.shape[0]
    f = np.linspace(0, n - 1, (n - 1) * int(upscale) + 1)
    d2 = (f[:, None] - np.arange(n, dtype=np.float64)[None, :]) ** 2
    m = len(f)
    acc = np.zeros((m, m, m))
    for a in range(n):
        for b in range(n):
            dxy2 = d2[:, b][None, :, None] + d2[:, a][:, None, None]
            for c in range(n):
                r2 = dxy2 + d2[:, c][None, None, :]
                acc = acc + weights[a, b, c] * (r2 * np.sqrt(r2))
    return acc


# -- inputs -----------------------------------------------------------------------------------------------------------
def floor_map(shape, floor, seed):
    """A strictly positive random floor in [0.2, 1.0) x ``floor``."""
    return floor * (0.2 + 0.8 * np.random.default_rng(seed).random(shape))


def bump_map(shape, centre, width, floor, seed):
    """A Gaussian bump of height 1 and standard deviation ``width`` nodes at the fractional ``centre`` on the floor."""
    g = np.indices(shape).astype(np.float64)
    r2 = sum((g[a] - float(centre[a])) ** 2 for a in range(3))
    return floor_map(shape, floor, seed) + np.exp(-r2 / (2.0 * width * width))


MAIN = (86, 81, 78)             # 543 348 nodes: two full passes and a third one a thirteenth full
REJECTED = (84, 81, 78)         # only the last x-plane reaches the third pass: no 5^3 window fits there
FLAT = (3, 400, 450)            # an axis shorter than the tap reach
SMALL = (13, 12, 11)
SHORT = (64, 63, 40)            # every axis within kMaxTaps nodes

# where the maximum is put: the node, the offset of the bump's centre from it, the bump's width, the floor
PLACEMENTS = {
    "pass0": dict(node=(20, 33, 41), offset=(0.21, -0.17, 0.12), width=3.0, floor=0.05),
    "first_of_pass1": dict(node=None, offset=(0.12, 0.23, -0.19), width=3.0, floor=0.05),      # flat == SWEEP
    "last_pass": dict(node=(83, 40, 37), offset=(-0.22, 0.14, 0.18), width=3.0, floor=0.05),
    "last_node": dict(node=None, offset=(0.3, 0.2, 0.25), width=3.0, floor=0.002),              # flat == n - 1
}


def placement_node(shape, name):
    if name == "first_of_pass1":
        return tuple(int(v) for v in np.unravel_index(SWEEP, shape))
    if name == "last_node":
        return tuple(n - 1 for n in shape)
    return PLACEMENTS[name]["node"]


@functools.lru_cache(maxsize=None)
def placed_map(name, shape=MAIN):
    p = PLACEMENTS[name]
    node = placement_node(shape, name)
    m = bump_map(shape, np.array(node) + np.array(p["offset"]), p["width"], p["floor"], seed=sum(map(ord, name)))
    m.setflags(write=False)
    return m


# (placement, sgm) of section 1, all at MAIN
PEAK_CASES = [(name, sgm) for sgm in (0.8, 2.0) for name in PLACEMENTS] + [("last_pass", 3.0), ("pass0", 0.3)]


# section 2: a wide bump in the last pass, so that a handful of nodes lie above 0.90 and 0.99
MOMENT_FLOOR = 0.05
MOMENT_THRESHOLDS = (0.005, 0.90, 0.99)         # the first lies below the floor: every node carries weight
MOMENT_SPACINGS = ((1.0, 1.0, 1.0), (0.5, 0.5, 0.25))

OTHER_MAPS = {
    "flat": lambda: bump_map(FLAT, (1.1, 210.2, 300.3), 2.5, 0.05, seed=77),
    "short": lambda: bump_map(SHORT, (40.2, 30.1, 21.3), 4.0, 0.05, seed=78),
    "small": lambda: bump_map(SMALL, (6.2, 5.1, 4.3), 2.0, 0.05, seed=79),
    "moments": lambda: bump_map(MAIN, (83.1, 40.2, 37.15), 12.0, MOMENT_FLOOR, seed=80),
}
# (map, sgm) of the cases beside section 1 whose smoothed map is compared
OTHER_SMOOTH_CASES = [("flat", 0.8), ("short", 3.3)]


@functools.lru_cache(maxsize=None)
def named_map(name):
    """A map of PLACEMENTS (at MAIN) or OTHER_MAPS, read-only and built once."""
    if name in PLACEMENTS:
        return placed_map(name)
    m = OTHER_MAPS[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def reference(name, sgm):
    """What the engine must return for ``named_map(name)`` at ``sgm``, computed once: the normalised map, its peak,
    the longdouble smoothed map with its mean and peak.  Read-only."""
    m = named_map(name)
    norm = m / np.nanmax(m)
    smoothed = direct_gaufilt3d(norm, sgm)
    for a in (norm, smoothed):
        a.setflags(write=False)
    return {"map_max": float(np.nanmax(m)), "norm": norm,
            "peak": np.array(np.unravel_index(np.nanargmax(norm), norm.shape)),
            "smoothed": smoothed, "smoothed_mean": smoothed.mean(),
            "smoothed_peak": np.array(np.unravel_index(np.argmax(smoothed), smoothed.shape))}


@functools.lru_cache(maxsize=None)
def fit_reference(name, sgm):
    """(Gaussian location, sigma) of ``np_gaufit3d`` on the reference's smoothed map and ``np_splineloc`` of the
    normalised one."""
    from oracle import qm_oracle

    r = reference(name, sgm)
    loc, sigma, _ = qm_oracle.np_gaufit3d(r["smoothed"].astype(np.float64))
    return loc, sigma, spline_reference(name)


@functools.lru_cache(maxsize=None)
def spline_reference(name):
    from oracle import qm_oracle

    m = named_map(name)
    return qm_oracle.np_splineloc(m / np.nanmax(m))


# section 3: pairs (lower flat index, higher flat index) of nodes given exactly the same largest value
def tie_pairs():
    kb, sw = K_FIT_BLOCK, SWEEP
    return {
        # found early by a high block / found late by a low block
        "high_block_first": (781 * kb + 64, sw + 147 * kb + 224),
        # ... whose partials meet in the final fold with the late one on the lower thread
        "high_block_first_low_thread": (781 * kb + 64, sw + 146 * kb + 224),
        # the same block slot (13 = 781 % 256) of the final fold
        "same_fold_slot": (781 * kb + 64, sw + 13 * kb + 5),
        # the same thread, one trip apart
        "same_thread": (300 * kb + 17, sw + 300 * kb + 17),
        # the same block, the late one on the lower thread
        "same_block": (500 * kb + 201, sw + 500 * kb + 10),
        # first and third pass
        "third_pass": (900 * kb + 33, 2 * sw + 20 * kb + 32),
    }


def tie_map(pair, shape=MAIN):
    m = floor_map(shape, 0.05, seed=81).ravel().copy()
    m[list(pair)] = 1.75
    return m.reshape(shape)


# section 4
def nan_block_map():
    m = placed_map("last_pass").copy()
    m[10:14, 20:25, 30:33] = np.nan
    return m


def nan_at_peak_map():
    """A single NaN on the bump's top node, where the largest value would be: the runner-up beside it is the peak, and
    the NaN lies inside both fit windows."""
    m = placed_map("last_pass").copy()
    m[PLACEMENTS["last_pass"]["node"]] = np.nan
    return m


def nan_reach(sgm):
    """Chebyshev distance from a NaN beyond which the smoothed map must be finite: two passes of ``tap_reach``."""
    return 2 * tap_reach(sgm)


# section 7: (n, upscale, centre of the bump, width^2 x 2, seed)
RBF_CASES = [
    (5, 16, (3.9, 2.2, 1.7), 3.0, 91),          # maximum in pass 1
    (5, 16, (3.85, 2.3, 1.6), 2.5, 92),         # maximum in pass 1
    (5, 16, (1.4, 2.2, 2.6), 3.0, 93),          # maximum in pass 0
    (2, 8, (0.4, 0.7, 0.3), 2.0, 94),
    (9, 3, (4.4, 3.7, 5.2), 6.0, 95),
]


def rbf_window(n, centre, scale, seed):
    g = np.indices((n, n, n)).astype(np.float64)
    sub = np.exp(-sum((g[a] - centre[a]) ** 2 for a in range(3)) / scale)
    return sub + 0.02 * np.random.default_rng(seed).random(sub.shape)


def rbf_tie_weights():
    """n = 3, upscale = 32 (65^3 points, 12 481 of them in the second pass): one unit weight makes the interpolant
    r^3 about that centre, every coordinate difference exact, so equal distances give equal bits."""
    centre = np.zeros((3, 3, 3))
    centre[1, 1, 1] = 1.0           # eight equal maxima, the corners: four in each pass
    face = np.zeros((3, 3, 3))
    face[0, 1, 1] = 1.0             # four equal maxima, all in the second pass, two of them in one block
    return {"centre": centre, "face": face}


RBF_TIE_UPSCALE = 32
