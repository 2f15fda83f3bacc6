# -*- coding: utf-8 -*-
"""
The grid eikonal solver on the host: the NumPy restatement (tests/traveltimes3d_ref.py) in its two forms against each
other and against closed forms, the host pieces of quakemigrate_amd/traveltimes.py that feed it, the C ABI's new
symbol.

The figures of the scheme -- its error against the closed form of a constant-gradient medium at two spacings, the
error of the sections + sweep path on the same model, and how far the two solvers are apart -- are measured HERE, on
the restatements, and kept in profiles/traveltimes3d_accuracy.txt (``python tests/test_traveltimes3d_host.py``
rewrites it); DESIGN.md row f9 quotes them and ``test_profile_holds_the_measured_figures`` holds the file to what this
module measures.
"""

import ctypes
import fnmatch
import functools
import re
import sys

import numpy as np
import pytest

import traveltimes3d_ref as t3
import traveltimes_ref as tr
from conftest import ROOT

PROFILE = ROOT / "profiles" / "traveltimes3d_accuracy.txt"
NEW_SYMBOL = "qm_engine_tt_eikonal3d"

# Roundings between a node's three neighbours and its T in the three-sided update (csrc/qm_traveltimes.hpp): the three
# offsets from the source 3 each (index * spacing, + ll, - source); rho 6 (three products, two sums, the root) and T0 1;
# its three derivatives 2 each; alpha 2 and beta 2 per axis; qa 5, qb 5, qc 7 (s s and the difference with it), the
# discriminant 3; root, sum and quotient 3; T = T0 tau 1.
OPS3 = 9 + 6 + 1 + 6 + 12 + 5 + 5 + 7 + 3 + 3 + 1

# the bit-for-bit case: small, anisotropic spacing, a source off the nodes, random slowness
SMALL = dict(ll=(-1.0, 0.5, 0.2), spacing=(0.5, 0.4, 0.3), count=(7, 6, 5), source=(0.13, 1.71, 0.83))


def small_case():
    """7 x 6 x 5, spacings 0.5 / 0.4 / 0.3, slowness uniform in [1/4, 1/3]: (ll, spacing, count, sources, s0, slowness,
    row_model)."""
    rng = np.random.default_rng(20261021)
    slowness = rng.uniform(0.25, 1.0 / 3.0, size=(1,) + SMALL["count"])
    return SMALL["ll"], SMALL["spacing"], SMALL["count"], [SMALL["source"]], [0.29], slowness, [0]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# -- the two forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [0.0, t3.TOL])
def test_plane_sweeps_are_the_serial_sweeps(tol):
    """Every plane i' + j' + k' = d at once gives the serial x-outer / z-inner loop's values, bit for bit; and the
    smallest kept candidate of the stacked form is what the scalar form's running ``t < best`` ends with."""
    case = small_case()
    a = t3.solve(*case, tol=tol)
    b = t3.solve_serial(*case, tol=tol)
    assert same_bits(a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and not a[2].any()
    assert np.all(np.isfinite(a[0])) and a[0].min() >= 0.0


def test_orderings_are_the_product_of_the_signs():
    assert t3.ORDERS[0] == (1, 1, 1) and t3.ORDERS[1] == (1, 1, -1) and t3.ORDERS[-1] == (-1, -1, -1)
    assert len(set(t3.ORDERS)) == 8
    n = (4, 3, 5)
    for order in t3.ORDERS:
        seen = np.zeros(n, dtype=int)
        sizes = []
        for i, j, k in t3.planes(n, order):
            seen[i, j, k] += 1
            sizes.append(len(i))
        assert np.all(seen == 1) and len(sizes) == sum(n) - 2 and sizes[0] == sizes[-1] == 1


# -- closed forms ------------------------------------------------------------------------------------------------------
HOM = dict(ll=(0.0, 0.0, 0.0), spacing=(0.5, 0.4, 0.3), count=(21, 19, 17), source=(3.13, 2.71, 1.23), v=4.0)


@functools.lru_cache(maxsize=None)
def homogeneous_error(tol):
    n = HOM["count"]
    T, rounds, status = t3.solve(HOM["ll"], HOM["spacing"], n, [HOM["source"]], [1.0 / HOM["v"]],
                                 np.full((1,) + n, 1.0 / HOM["v"]), [0], tol=tol)
    assert status[0] == 0
    exact = tr.homogeneous(HOM["ll"], HOM["spacing"], n, HOM["source"], HOM["v"])
    return float(np.abs(T[0] - exact).max()), float(T.max()), int(rounds[0])


def test_homogeneous_medium_to_rounding():
    """tau = 1 solves the factored scheme exactly in a homogeneous medium -- sum (a - b)^2 = sum (dT0/dd)^2 = s0^2 --:
    what is left is rounding.  A node's value carries the OPS3 roundings of its own update, 2^-53 relative each, on top
    of its neighbours' errors, along a chain of at most nx + ny + nz nodes from the source: the strict iteration's
    bound.  With the acceptance tolerance a node may also keep a value up to tol (relative) above what its neighbours
    would give it now, once per node of the chain."""
    chain = sum(HOM["count"])
    err, tmax, _ = homogeneous_error(0.0)
    assert err <= OPS3 * chain * 2.0 ** -53 * tmax, (err, OPS3 * chain * 2.0 ** -53 * tmax)
    err, tmax, _ = homogeneous_error(t3.TOL)
    assert err <= (OPS3 * 2.0 ** -53 + t3.TOL) * chain * tmax, err


# v = v0 + g z on a 6.0 x 5.6 x 4.8 box, the source off the nodes at either spacing
BOX, SOURCE = (6.0, 5.6, 4.8), (2.13, 1.71, 1.23)
V0, GRADIENT = 3.0, 0.6


def _gradient_grid(h):
    count = tuple(int(round(b / h)) + 1 for b in BOX)
    return (0.0, 0.0, 0.0), (h, h, h), count


def _closed_form(ll, spacing, count):
    gx, gy, gz = tr.grid_xyz(ll, spacing, count)
    r2 = (gx - SOURCE[0]) ** 2 + (gy - SOURCE[1]) ** 2 + (gz - SOURCE[2]) ** 2
    vs, vr = V0 + GRADIENT * SOURCE[2], V0 + GRADIENT * gz
    return np.arccosh(1.0 + GRADIENT * GRADIENT * r2 / (2.0 * vs * vr)) / GRADIENT


@functools.lru_cache(maxsize=None)
def gradient_solution(h):
    """The grid solver on v = v0 + g z at spacing h: (T, rounds)."""
    ll, spacing, count = _gradient_grid(h)
    z = np.arange(count[2]) * h
    slowness = np.broadcast_to(1.0 / (V0 + GRADIENT * z), (1,) + count)
    T, rounds, status = t3.solve(ll, spacing, count, [SOURCE], [1.0 / (V0 + GRADIENT * SOURCE[2])], slowness, [0])
    assert status[0] == 0
    return T[0], int(rounds[0])


# The sections' spacings of the comparison.  0.2, the grid's own: every depth of the grid is a multiple of it up to
# rounding, where the reference's interpolation rule takes the cell from a quotient and the fraction from a remainder
# (quakemigrate_amd/traveltimes.py, plan_sections) -- at some depths the two part by one cell, and the sections path is
# then off by a cell's travel time.  0.13: no depth of the grid near a multiple, the rule at its best.
SECTION_DX = (0.2, 0.13)


@functools.lru_cache(maxsize=None)
def sections_solution(h, dx):
    """The sections + sweep restatement (tests/traveltimes_ref.py) of the same model on the same grid, the sections
    at spacing dx."""
    from quakemigrate_amd import traveltimes as tt

    ll, spacing, count = _gradient_grid(h)
    plan = tt.plan_sections(ll, spacing, count, [SOURCE], dx)
    depth = plan["z0"][0] + np.arange(plan["nz"]) * dx
    sections, _, status = tr.solve_sections(1.0 / (V0 + GRADIENT * depth), plan["source_depth"],
                                            [1.0 / (V0 + GRADIENT * SOURCE[2])], plan["nr"], dx)
    assert status[0] == 0
    return tr.sweep(ll, spacing, count, SOURCE[:2], sections[0], 0.0, plan["z0"][0], dx)


def gradient_error(h):
    return float(np.abs(gradient_solution(h)[0] - _closed_form(*_gradient_grid(h))).max())


def test_gradient_error_falls_with_the_spacing():
    """Against acosh(1 + g^2 r^2 / (2 v_s v_r)) / g: first order, so the error at h is below the one at 2 h.  No fixed
    bound: the figures are the scheme's, kept in the profile."""
    assert gradient_error(0.2) < gradient_error(0.4), (gradient_error(0.2), gradient_error(0.4))


def test_sections_path_on_the_same_model():
    """The other route to the same table solves the same equation against the same closed form; the two solvers
    differ by no more than the sum of their errors.  The errors themselves are figures, kept in the profile."""
    h = 0.2
    exact = _closed_form(*_gradient_grid(h))
    grid_err = gradient_error(h)
    for dx in SECTION_DX:
        sec_err = float(np.abs(sections_solution(h, dx) - exact).max())
        assert np.isfinite(sec_err) and np.isfinite(grid_err)
        assert float(np.abs(sections_solution(h, dx) - gradient_solution(h)[0]).max()) <= sec_err + grid_err


def figures():
    h = 0.2
    exact = _closed_form(*_gradient_grid(h))
    strict, default = homogeneous_error(0.0), homogeneous_error(t3.TOL)
    return {
        "grid_error_h0.4_s": gradient_error(0.4), "grid_error_h0.2_s": gradient_error(0.2),
        "sections_error_dx0.2_s": float(np.abs(sections_solution(h, 0.2) - exact).max()),
        "sections_error_dx0.13_s": float(np.abs(sections_solution(h, 0.13) - exact).max()),
        "solvers_largest_difference_dx0.2_s": float(np.abs(sections_solution(h, 0.2) - gradient_solution(h)[0]).max()),
        "solvers_largest_difference_dx0.13_s": float(np.abs(sections_solution(h, 0.13) - gradient_solution(h)[0]).max()),
        "gradient_tmax_s": float(exact.max()),
        "grid_rounds_h0.4": gradient_solution(0.4)[1], "grid_rounds_h0.2": gradient_solution(0.2)[1],
        "homogeneous_error_strict_s": strict[0], "homogeneous_error_default_tol_s": default[0],
        "homogeneous_error_strict_ulps_of_tmax": strict[0] / (2.0 ** -53 * strict[1]),
        "homogeneous_tmax_s": default[1], "homogeneous_rounds_strict": strict[2],
    }


def profile_text(f):
    lines = [
        "The grid eikonal solver: the scheme's figures, measured on the NumPy restatement (tests/traveltimes3d_ref.py)",
        "by tests/test_traveltimes3d_host.py -- not on the kernel, which has the restatement's bits.",
        f"Box {BOX[0]} x {BOX[1]} x {BOX[2]}, source at {SOURCE}; v = {V0} + {GRADIENT} z against the acosh closed form at",
        "h = 0.4 and 0.2 (grid_error); sections_error: the sections + sweep restatement (tests/traveltimes_ref.py) of",
        "the same model on the h = 0.2 grid, sections at spacing dx; solvers_largest_difference: between the two.",
        "dx = 0.2 makes every depth of the grid a multiple of dx up to rounding: the reference's interpolation rule",
        "(cell from a quotient, fraction from a remainder) then parts by one cell at some depths, and the sections",
        "path is off by a cell's travel time there.  dx = 0.13: no depth near a multiple.",
        f"homogeneous: v = {HOM['v']} on {HOM['count']} nodes of {HOM['spacing']}, source at {HOM['source']}, against",
        "rho / v, strict (tol = 0) and at the default tol = 2^-40.  No figure from scikit-fmm (1dfmm): not compared.",
        "",
    ]
    lines += [f"{k} = {v:.6e}" if isinstance(v, float) else f"{k} = {v}" for k, v in f.items()]
    return "\n".join(lines) + "\n"


def test_profile_holds_the_measured_figures():
    stored = dict(re.findall(r"^(\w[\w.]*) = (\S+)$", PROFILE.read_text(), flags=re.M))
    for key, value in figures().items():
        assert key in stored, key
        if isinstance(value, int):
            assert int(stored[key]) == value, key
        else:                                   # (acosh and the printed digits: six figures)
            assert float(stored[key]) == pytest.approx(value, rel=1e-3), key


# -- the host pieces of compute_traveltimes ----------------------------------------------------------------------------
LL, SPACING, COUNT = (-3.0, 1.5, -1.0), (0.5, 0.4, 0.25), (9, 8, 7)
UR = tuple(l + (n - 1) * s for l, s, n in zip(LL, SPACING, COUNT))


def test_trilinear_slowness_at_the_station():
    from quakemigrate_amd import traveltimes as tt

    gx, gy, gz = tr.grid_xyz(LL, SPACING, COUNT)
    linear = 3.0 + 0.2 * gx - 0.1 * gy + 0.6 * gz          # trilinear interpolation reproduces it to rounding
    points = np.array([[-1.13, 2.71, -0.33], [0.99, 4.29, 0.49], LL, UR, [-2.0, 2.3, 0.0]])
    got = tt.trilinear(linear, LL, SPACING, COUNT, points)
    want = 3.0 + 0.2 * points[:, 0] - 0.1 * points[:, 1] + 0.6 * points[:, 2]
    assert np.max(np.abs(got - want)) <= 32 * 2.0 ** -53 * linear.max()
    rng = np.random.default_rng(3)
    rough = rng.uniform(2.0, 6.0, size=COUNT)
    # at a node whose offset from ll is a whole number of spacings in floats too, the node's value exactly (x and z
    # here: 0.5 and 0.25 are powers of two; along y only index 0); at any node, to rounding
    nodes = np.array([[2, 0, 4], [0, 0, 0], [7, 0, 5], [8, 0, 3]])
    at_nodes = np.array(LL) + nodes * np.array(SPACING)
    assert np.array_equal(tt.trilinear(rough, LL, SPACING, COUNT, at_nodes), rough[tuple(nodes.T)])
    nodes = np.array([[2, 3, 4], [8, 7, 6], [1, 5, 0]])
    at_nodes = np.array(LL) + nodes * np.array(SPACING)
    # (two roundings in an offset of at most 8 spacings: a fraction within 2^-49 of whole; three axes, values 4 apart)
    assert np.max(np.abs(tt.trilinear(rough, LL, SPACING, COUNT, at_nodes) - rough[tuple(nodes.T)])) <= 12 * 2.0 ** -49
    # the stated expression, by hand, in one cell
    p = np.array([-1.13, 2.71, -0.33])
    q = (p - np.array(LL)) / np.array(SPACING)
    c0 = np.floor(q).astype(int)
    fx, fy, fz = q - c0
    c = rough[c0[0]:c0[0] + 2, c0[1]:c0[1] + 2, c0[2]:c0[2] + 2]
    by_hand = (((c[0, 0, 0] * (1 - fz) + c[0, 0, 1] * fz) * (1 - fy) + (c[0, 1, 0] * (1 - fz) + c[0, 1, 1] * fz) * fy)
               * (1 - fx)
               + ((c[1, 0, 0] * (1 - fz) + c[1, 0, 1] * fz) * (1 - fy) + (c[1, 1, 0] * (1 - fz) + c[1, 1, 1] * fz) * fy)
               * fx)
    assert tt.trilinear(rough, LL, SPACING, COUNT, [p])[0] == by_hand
    with pytest.raises(ValueError, match="shape"):
        tt.trilinear(rough[:-1], LL, SPACING, COUNT, [p])


def test_snap_to_node_picks_the_references_node():
    from quakemigrate_amd import traveltimes as tt

    gx, gy, gz = tr.grid_xyz(LL, SPACING, COUNT)
    points = np.array([[-1.13, 2.71, -0.33], [-1.25, 2.7, -0.375],      # the second: midway along x and z, a tie
                       LL, UR, [0.99, 4.29, 0.49]])
    idx, xyz = tt.nearest_node(LL, SPACING, COUNT, points)
    for p, i, node in zip(points, idx, xyz):
        # create_lut.py:379-384, evaluated directly
        flat = np.argmin(abs(gx - p[0]) + abs(gy - p[1]) + abs(gz - p[2]))
        assert tuple(i) == np.unravel_index(flat, COUNT)
        assert tuple(node) == (gx[tuple(i)], gy[tuple(i)], gz[tuple(i)])
    assert tuple(idx[2]) == (0, 0, 0) and tuple(idx[3]) == tuple(n - 1 for n in COUNT)


def test_refusals_that_need_no_engine():
    from quakemigrate_amd import traveltimes as tt

    v = np.full(COUNT, 4.0)
    inside, outside = {"A": (-1.0, 2.0, 0.0)}, {"A": (-1.0, 2.0, 0.0), "B": (-3.5, 2.0, 0.0)}
    vmod = {"Depth": [-1.0, 0.5], "Vp": [3.0, 5.0], "Vs": [1.7, 2.9]}
    with pytest.raises(ValueError, match="station B .* outside the grid"):
        tt.compute_traveltimes(None, LL, SPACING, COUNT, outside, "3d", velocity={"P": v, "S": v})
    with pytest.raises(ValueError, match="solver='grid'.*station B .* outside the grid"):
        tt.compute_traveltimes(None, LL, SPACING, COUNT, outside, "1d", vmod=vmod, solver="grid")
    with pytest.raises(ValueError, match=r"velocity\['S'\]"):
        tt.compute_traveltimes(None, LL, SPACING, COUNT, inside, "3d", velocity={"P": v})
    with pytest.raises(ValueError, match="shape"):
        tt.compute_traveltimes(None, LL, SPACING, COUNT, inside, "3d", velocity={"P": v, "S": v[:-1]})
    with pytest.raises(ValueError, match="not a solver"):
        tt.compute_traveltimes(None, LL, SPACING, COUNT, inside, "1d", vmod=vmod, solver="fmm")
    with pytest.raises(ValueError, match="needs vmod"):
        tt.compute_traveltimes(None, LL, SPACING, COUNT, inside, "1d", solver="grid")
    with pytest.raises(ValueError, match="'3d'.*'1dfmm'"):
        tt.compute_traveltimes(None, LL, SPACING, COUNT, inside, "1dfmm")
    # the restatement's own refusals
    case = list(small_case())
    for k, broken, text in ((3, [(9.0, 1.0, 0.5)], "outside"), (6, [1], "row_model"),
                            (5, np.where(np.arange(210).reshape(1, 7, 6, 5) == 77, 0.0, case[5]), "slowness")):
        args = list(case)
        args[k] = broken
        with pytest.raises(ValueError, match=text):
            t3.solve(*args)
    with pytest.raises(ValueError, match="shorter than 2"):
        t3.solve(SMALL["ll"], SMALL["spacing"], (7, 1, 5), [(0.13, 0.5, 0.83)], [0.29], np.full((1, 7, 1, 5), 0.3), [0])


# -- the C ABI and the Python layer ------------------------------------------------------------------------------------
def test_header_map_and_library_agree_on_the_new_symbol():
    import __graft_entry__ as g

    g.build_engine()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qmhip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+" + NEW_SYMBOL + r"\s*\(", text), f"include/qmhip.h does not declare {NEW_SYMBOL}"
    version_script = re.sub(r"/\*.*?\*/", "", (ROOT / "quakemigrate_amd" / "csrc" / "qmhip.map").read_text(), flags=re.S)
    exported = re.search(r"global:(.*?)local:", version_script, flags=re.S).group(1).replace(";", " ").split()
    assert any(fnmatch.fnmatchcase(NEW_SYMBOL, pattern) for pattern in exported), "csrc/qmhip.map keeps it local"
    lib = ctypes.CDLL(str(ROOT / "quakemigrate_amd" / "csrc" / "libqmhip.so"))
    assert hasattr(lib, NEW_SYMBOL), f"libqmhip.so does not export {NEW_SYMBOL}"


def test_python_layer_is_bound():
    from quakemigrate_amd import traveltimes as tt
    from quakemigrate_amd.core import lib

    assert len(getattr(lib.qmlib, NEW_SYMBOL).argtypes) == 16
    assert callable(lib.Engine.traveltimes_eikonal3d)
    assert callable(tt.trilinear) and callable(tt.nearest_node)


if __name__ == "__main__":
    PROFILE.write_text(profile_text(figures()))
    sys.stdout.write(PROFILE.read_text())
