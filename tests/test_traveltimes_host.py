# -*- coding: utf-8 -*-
"""
The travel-time stage on the host: the NumPy restatement (tests/traveltimes_ref.py) against closed forms and SciPy,
the section planner of quakemigrate_amd/traveltimes.py against the reference's expressions, the C ABI's new symbols.

The figures of the scheme -- its error against the closed form of a constant-gradient medium at two spacings, and
how much the result depends on the sequence of the four sweep orderings -- are measured HERE, on the restatement, and
kept in profiles/traveltimes_accuracy.txt (``python tests/test_traveltimes_host.py`` rewrites it); DESIGN.md row f8
quotes them and ``test_profile_holds_the_measured_figures`` holds the file to what this module measures.
"""

import ctypes
import re
import sys

import numpy as np
import pytest

import traveltimes_ref as tr
from conftest import ROOT

PROFILE = ROOT / "profiles" / "traveltimes_accuracy.txt"
NEW_SYMBOLS = ("qm_engine_tt_homogeneous", "qm_engine_tt_sections", "qm_engine_tt_sweep")

# The section of the closed-form checks: 9.8 x 6.2 km, source at 1.23 km depth, between two rows at either spacing
EXTENT_R, EXTENT_Z, SOURCE_Z = 9.8, 6.2, 1.23
V0, GRADIENT = 3.0, 0.6

# Roundings between a node's two neighbours and its T in the two-sided update (csrc/qm_traveltimes.hpp): rho 4 and
# T0 1; T0x, T0z 2 each; alpha 2 and beta 2 per axis; qa 3, qb 3, qc 5, the discriminant 3, root, sum and quotient 3;
# T = T0 tau 1.
OPS = 5 + 4 + 8 + 3 + 3 + 5 + 3 + 3 + 1


def _shape(h):
    return int(round(EXTENT_R / h)) + 1, int(round(EXTENT_Z / h)) + 1


def _closed_form_error(h, gradient, tol=tr.TOL):
    nr, nz = _shape(h)
    z = np.arange(nz) * h
    v = V0 + gradient * z
    vs = V0 + gradient * SOURCE_Z
    T, rounds, status = tr.solve_sections(1.0 / v, [SOURCE_Z], [1.0 / vs], nr, h, tol=tol)
    assert status[0] == 0
    r2 = (np.arange(nr) * h)[:, None] ** 2 + (z[None, :] - SOURCE_Z) ** 2
    if gradient == 0.0:
        exact = np.sqrt(r2) / V0
    else:
        exact = np.arccosh(1.0 + gradient * gradient * r2 / (2.0 * vs * v[None, :])) / gradient
    return float(np.abs(T[0] - exact).max()), float(T.max()), int(rounds[0]), (nr, nz)


# -- the restatement against closed forms ------------------------------------------------------------------------------
def test_homogeneous_section_to_rounding():
    """tau = 1 solves the factored scheme exactly in a homogeneous medium: what is left is rounding.  A node's value
    carries the OPS roundings of its own update, 2^-53 relative each, on top of its neighbours' errors, along a chain of
    at most nr + nz nodes from the source: |T - rho / v| <= OPS (nr + nz) 2^-53 Tmax.  That is the strict iteration's
    bound (tol = 0).  With the acceptance tolerance a node may also keep a value up to tol (relative) above what its
    neighbours would give it now, once per node of the chain: the bound gains tol (nr + nz) Tmax, and at the default
    2^-40 that term is the larger one."""
    err, tmax, _, (nr, nz) = _closed_form_error(0.1, 0.0, tol=0.0)
    assert err <= OPS * (nr + nz) * 2.0 ** -53 * tmax, (err, OPS * (nr + nz) * 2.0 ** -53 * tmax)
    err, tmax, _, _ = _closed_form_error(0.1, 0.0)
    assert err <= (OPS * 2.0 ** -53 + tr.TOL) * (nr + nz) * tmax, err


def gradient_errors():
    return {h: _closed_form_error(h, GRADIENT) for h in (0.2, 0.1)}


def test_gradient_error_falls_with_the_spacing():
    """v = v0 + g z against acosh(1 + g^2 (r^2 + dz^2) / (2 v_s v_r)) / g: first order, so the error at h is below the
    one at 2 h.  No fixed bound: the figures are the scheme's, kept in the profile."""
    e = gradient_errors()
    assert e[0.1][0] < e[0.2][0], e


def test_diagonal_sweeps_are_the_serial_sweeps():
    """Every anti-diagonal at once gives the serial i-outer / k-inner loop's values, bit for bit."""
    h, nz = 0.1, 13
    z = np.arange(nz) * h
    slowness = np.array([1.0 / (3.0 + 0.6 * z), 1.0 / np.where(z < 0.4, 4.0, np.where(z < 0.8, 2.0, 5.0))])
    zs, s0 = [0.37, 0.6], [1.0 / (3.0 + 0.6 * 0.37), 0.5]
    a = tr.solve_sections(slowness, zs, s0, 11, h)
    b = tr.solve_sections_serial(slowness, zs, s0, 11, h)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and not a[2].any()


# -- order independence ------------------------------------------------------------------------------------------------
OTHER_ORDERS = ((-1, -1), (+1, -1), (+1, +1), (-1, +1))


def order_dependence():
    """The largest difference, relative to Tmax, between the four orderings run in two sequences, over four model
    families at two source depths."""
    h, nr, nz = 0.1, 67, 45
    z = np.arange(nz) * h
    top = z[-1]
    families = [np.full(nz, 4.0), 3.0 + 0.6 * z, np.where(z < 0.3 * top, 3.0, np.where(z < 0.6 * top, 5.0, 6.5)),
                np.where(z < 0.3 * top, 4.0, np.where(z < 0.5 * top, 2.0, 5.0))]
    slowness, zs, s0 = [], [], []
    for v in families:
        for d in (0.7, 0.74):
            slowness.append(1.0 / v)
            zs.append(d)
            s0.append(1.0 / np.interp(d, z, v))
    a = tr.solve_sections(np.array(slowness), zs, s0, nr, h)
    b = tr.solve_sections(np.array(slowness), zs, s0, nr, h, orders=OTHER_ORDERS)
    assert not a[2].any() and not b[2].any()
    return float(np.max(np.abs(a[0] - b[0]) / a[0].max(axis=(1, 2), keepdims=True)))


def test_sequence_of_the_orderings_moves_the_last_digits_only():
    """Another sequence of the same four orderings is another valid iteration; its fixed point differs by what the
    acceptance tolerance leaves open per node, accumulated along a chain: far below a sample at any scan rate.  The
    figure itself goes to the profile; x 10 it is the only float tolerance a GPU test may use for a different but
    valid order (none does: the kernels keep the restatement's order)."""
    assert order_dependence() <= tr.TOL * (67 + 45)


def figures():
    e = gradient_errors()
    hom_strict, hom_default = _closed_form_error(0.1, 0.0, tol=0.0), _closed_form_error(0.1, 0.0)
    return {
        "gradient_error_h0.2_s": e[0.2][0], "gradient_error_h0.1_s": e[0.1][0], "gradient_tmax_s": e[0.1][1],
        "gradient_rounds_h0.1": e[0.1][2],
        "homogeneous_error_strict_s": hom_strict[0], "homogeneous_error_default_tol_s": hom_default[0],
        "homogeneous_tmax_s": hom_default[1],
        "order_dependence_rel": order_dependence(),
    }


def profile_text(f):
    lines = [
        "Travel-time sections: the scheme's figures, measured on the NumPy restatement (tests/traveltimes_ref.py)",
        "by tests/test_traveltimes_host.py -- not on the kernel, which has the restatement's bits.",
        f"Section {EXTENT_R} x {EXTENT_Z} km, source at {SOURCE_Z} km depth; v = {V0} + {GRADIENT} z against the closed form;",
        "homogeneous: v = 3.0 against rho / v, strict (tol = 0) and at the default tol = 2^-40.",
        "order_dependence_rel: the four sweep orderings in two sequences, largest |T1 - T2| / Tmax over four model",
        "families (homogeneous, gradient, three blocks, low-velocity layer) on 67 x 45 nodes; x 10 is the tolerance",
        "for 'a different but valid order'.",
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


# -- the planner -------------------------------------------------------------------------------------------------------
LL, SPACING, COUNT = (-3.0, 1.5, -1.0), (0.5, 0.4, 0.25), (23, 19, 17)
STATIONS = np.array([[-1.0, 3.5, 0.0], [0.77, 4.13, 0.33], [-5.2, 2.0, 0.1], [2.0, 6.0, -2.3], [-3.0, 1.5, -1.0],
                     [1.0, 2.0, 4.4]])


@pytest.mark.parametrize("dx", [0.125, 0.1, 0.07])
def test_planner_against_the_references_expressions(dx):
    from quakemigrate_amd import traveltimes as tt

    plan = tt.plan_sections(LL, SPACING, COUNT, STATIONS, dx)
    z_axis = tr.grid_xyz(LL, SPACING, COUNT)[2][0, 0, :]
    for i, station in enumerate(STATIONS):
        # what the reference takes from the grid (create_lut.py:471-474, 479-482), evaluated directly over all nodes:
        # the farthest node's horizontal distance, and the depths of grid and station together
        dist, depth = tr.distances_depths(LL, SPACING, COUNT, station[:2])
        farthest = dist.max()
        shallowest, deepest = min(z_axis[0], station[2]), max(z_axis[-1], station[2])
        assert plan["max_dist"][i] == farthest
        assert tuple(plan["depth_span"][i]) == (shallowest, deepest)
        assert plan["nr_each"][i] == int(np.ceil(farthest / dx)) + 5            # the margin of :864-865
        assert plan["nz_each"][i] == int(np.ceil((deepest - plan["z0"][i]) / dx)) + 5
        # z0: a multiple of dx, at least two nodes above the span
        m = np.rint(plan["z0"][i] / dx)                 # (the product m dx, rounded once: what "multiple" means in floats)
        assert plan["z0"][i] == m * dx and abs(plan["z0"][i] / dx - m) < 1e-9
        assert plan["z0"][i] <= shallowest - 2 * dx + 1e-12
        assert plan["source_depth"][i] == station[2] - plan["z0"][i]
        # every node's four corners are inside the station's own section, and so inside the padded one
        assert len(tr.outside(dist, depth, 0.0, plan["z0"][i], dx, plan["nr_each"][i], plan["nz_each"][i])) == 0
        # ... and the source box is inside its rows
        assert 0 <= np.floor(plan["source_depth"][i] / dx) <= plan["nz_each"][i] - 2
    assert plan["nr"] == plan["nr_each"].max() and plan["nz"] == plan["nz_each"].max()


def test_model_velocity():
    from quakemigrate_amd import traveltimes as tt

    vmod = {"Depth": [0.0, 1.0, 3.0], "Vp": [3.0, 5.0, 6.0], "Vs": [1.7, 2.9, 3.4]}
    depths = np.array([-1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 9.0])
    assert np.array_equal(tt.model_velocity(vmod, "P", depths), np.interp(depths, vmod["Depth"], vmod["Vp"]))
    assert np.array_equal(tt.model_velocity(vmod, "S", depths, block_model=True), [1.7, 1.7, 1.7, 2.9, 2.9, 3.4, 3.4])
    plain = (vmod["Depth"], vmod["Vp"], vmod["Vs"])
    assert np.array_equal(tt.model_velocity(plain, "S", depths), np.interp(depths, vmod["Depth"], vmod["Vs"]))
    with pytest.raises(KeyError):
        tt.model_velocity({"Depth": [0.0], "Vp": [3.0]}, "S", depths)
    with pytest.raises(KeyError):
        tt.model_velocity(plain[:2], "S", depths)
    with pytest.raises(ValueError):
        tt.compute_traveltimes(None, LL, SPACING, COUNT, {"A": (0, 0, 0)}, "1dfmm")


# -- the sweep's rule --------------------------------------------------------------------------------------------------
def test_bilinear_rule_against_scipy():
    """On a section whose origin is a multiple of the spacing the reference's rule IS linear interpolation on the
    regular grid: agreement with SciPy to rounding (a few operations of 2^-53 each on values below the maximum)."""
    from scipy.interpolate import RegularGridInterpolator

    rng = np.random.default_rng(7)
    h, nr, nz = 0.125, 60, 40
    x0, z0 = 0.0, -16 * h
    section = rng.uniform(0.0, 9.0, size=(nr, nz))
    xz = np.c_[rng.uniform(0.0, (nr - 1) * h, 4000), rng.uniform(z0, z0 + (nz - 1) * h, 4000)]
    xz[:50, 0] = np.arange(50) * h                  # on nodes as well
    xz[50:80, 1] = z0 + np.arange(30) * h
    xz = xz[(xz[:, 0] < (nr - 1) * h) & (xz[:, 1] < z0 + (nz - 1) * h)]
    got = tr.bilinear(xz[:, 0], xz[:, 1], x0, z0, h, section)
    want = RegularGridInterpolator((x0 + np.arange(nr) * h, z0 + np.arange(nz) * h), section, method="linear")(xz)
    assert np.max(np.abs(got - want)) <= 16 * 2.0 ** -53 * section.max()


def test_sweep_refuses_a_node_outside():
    section = np.ones((10, 10))
    with pytest.raises(IndexError):
        tr.sweep(LL, SPACING, COUNT, STATIONS[0, :2], section, 0.0, -2.0, 0.125)


def test_homogeneous_restatement_is_the_direct_expression():
    got = tr.homogeneous(LL, SPACING, COUNT, STATIONS[1], 2.9)
    ix, iy, iz = 7, 11, 13
    x, y, z = (LL[j] + i * SPACING[j] for j, i in enumerate((ix, iy, iz)))
    sx, sy, sz = STATIONS[1]
    assert got[ix, iy, iz] == np.sqrt((x - sx) * (x - sx) + (y - sy) * (y - sy) + (z - sz) * (z - sz)) / 2.9


# -- the C ABI and the Python layer ------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_symbols():
    import __graft_entry__ as g

    g.build_engine()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qmhip.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(ROOT / "quakemigrate_amd" / "csrc" / "libqmhip.so"))
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"include/qmhip.h does not declare {name}"
        assert hasattr(lib, name), f"libqmhip.so does not export {name}"


def test_python_layer_is_bound():
    from quakemigrate_amd import traveltimes as tt
    from quakemigrate_amd.core import lib

    for name in NEW_SYMBOLS:
        assert getattr(lib.qmlib, name).argtypes is not None
    for method in ("traveltimes_homogeneous", "traveltime_sections", "sweep_sections"):
        assert callable(getattr(lib.Engine, method))
    assert callable(tt.compute_traveltimes) and callable(tt.plan_sections)


if __name__ == "__main__":
    PROFILE.write_text(profile_text(figures()))
    sys.stdout.write(PROFILE.read_text())
