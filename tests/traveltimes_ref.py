# -*- coding: utf-8 -*-
"""
NumPy restatement of the travel-time stage (include/qmhip.h: qm_engine_tt_homogeneous, qm_engine_tt_sections,
qm_engine_tt_sweep; kernels: csrc/qm_traveltimes.hpp) -- the specification the GPU tests compare against, bit for bit.

* ``homogeneous``: the reference's ``_compute_homogeneous`` (quakemigrate/lut/create_lut.py:241-265) on the node
  coordinates of ``Grid3D.grid_xyz`` (lut/lut.py: ``ll_corner + index * node_spacing``);
* ``solve_sections``: the multiplicatively factored first-order upwind eikonal solver on (distance, depth) sections,
  Gauss-Seidel sweeps in four orderings, every anti-diagonal of a sweep at once and all sections side by side.  Only
  elementwise float64 operations, one rounding each, in the kernel's order: the values are the kernel's bits.  A
  diagonal reads the previous diagonal as the sweep left it and the next one as the sweep found it -- what the serial
  ``i``-outer / ``k``-inner loop reads (``solve_sections_serial`` is that loop, for the host tests);
* ``bilinear``: the rule of the reference's ``_bilinear_interpolate`` (create_lut.py:746-762) restated, and ``sweep``
  around it: distances and depths of a 3-D grid's nodes as create_lut.py:471-473 forms them.

tests/test_traveltimes_host.py pins the solver to closed forms and the transcription to SciPy.
"""

import numpy as np

TOL = 2.0 ** -40
MAX_ITERS = 64
ORDERS = ((+1, +1), (-1, +1), (-1, -1), (+1, -1))           # (direction of i, direction of k) of the four sweeps


# -- a. homogeneous ----------------------------------------------------------------------------------------------------
def grid_xyz(ll_corner, node_spacing, node_count):
    """``Grid3D.grid_xyz``: three (nx, ny, nz) arrays, ``ll_corner + index * node_spacing`` per axis."""
    ll = np.asarray(ll_corner, dtype=np.float64)
    sp = np.asarray(node_spacing, dtype=np.float64)
    axes = [ll[j] + (np.arange(int(node_count[j])) * sp[j]) for j in range(3)]
    return np.meshgrid(*axes, indexing="ij")


def homogeneous(ll_corner, node_spacing, node_count, station_xyz, velocity):
    """One row (what create_lut.py:262-265 computes): straight-line distance over velocity, the three squares
    single products, their sum taken left to right."""
    gx, gy, gz = grid_xyz(ll_corner, node_spacing, node_count)
    ox, oy, oz = gx - float(station_xyz[0]), gy - float(station_xyz[1]), gz - float(station_xyz[2])
    return np.sqrt(ox * ox + oy * oy + oz * oz) / float(velocity)


# -- b. sections -------------------------------------------------------------------------------------------------------
def _prepare(slowness, zsrc, s0, nr, h):
    slowness = np.atleast_2d(np.asarray(slowness, dtype=np.float64))
    n_sec, nz = slowness.shape
    zsrc = np.asarray(zsrc, dtype=np.float64).reshape(n_sec)
    s0 = np.asarray(s0, dtype=np.float64).reshape(n_sec)
    h = float(h)
    x = (np.arange(nr, dtype=np.float64) * h)[None, :, None] + np.zeros((n_sec, 1, nz))
    z = (np.arange(nz, dtype=np.float64) * h)[None, None, :] - zsrc[:, None, None] + np.zeros((1, nr, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.sqrt(x * x + z * z)
        t0 = s0[:, None, None] * rho
        t0x = s0[:, None, None] * x / rho
        t0z = s0[:, None, None] * z / rho
    # the source box: columns 0 and 1 of the two rows that bracket the source
    k0 = np.floor(zsrc / h).astype(np.int64)
    if np.any(zsrc < 0) or np.any(k0 + 1 > nz - 1) or nr < 2:
        raise ValueError("source outside the section")
    tau = np.full((n_sec, nr + 2, nz + 2), np.inf)          # (a border of +inf: a neighbour outside is not available)
    frozen = np.zeros((n_sec, nr, nz), dtype=bool)
    for s in range(n_sec):
        for k in (k0[s], k0[s] + 1):
            for i in (0, 1):
                frozen[s, i, k] = True
                tau[s, i + 1, k + 1] = 1.0 if rho[s, i, k] == 0.0 else (s0[s] + slowness[s, k]) / (2.0 * s0[s])
    return slowness, s0, h, tau, frozen, t0, t0x, t0z


def _candidates(old, ta_m, ta_p, tb_m, tb_p, t0, t0x, t0z, sk, h, tol):
    """The node update: the smallest candidate over the available neighbours.  ta_m / ta_p: tau at (i - 1, k) and
    (i + 1, k); tb_m / tb_p: at (i, k - 1) and (i, k + 1).  Elementwise."""
    best = np.full_like(old, np.inf)
    sides = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t0d, nbrs in ((t0x, ((1.0, ta_m), (-1.0, ta_p))), (t0z, ((1.0, tb_m), (-1.0, tb_p)))):
            axis = []
            for sg, ta in nbrs:
                av = np.isfinite(ta)
                a = t0 * sg / h + t0d
                b = t0 * sg * ta / h
                t = (b + sg * sk) / a
                ok = av & (sg * a > 0.0) & (t > 0.0) & (t < best)
                best = np.where(ok, t, best)
                axis.append((sg, av, a, b))
            sides.append(axis)
        for sx, avx, ax, bx in sides[0]:
            for sz, avz, az, bz in sides[1]:
                qa = ax * ax + az * az
                qb = ax * bx + az * bz
                qc = bx * bx + bz * bz - sk * sk
                disc = qb * qb - qa * qc
                t = (qb + np.sqrt(disc)) / qa
                ok = (avx & avz & (disc >= 0.0) & (sx * (ax * t - bx) >= 0.0) & (sz * (az * t - bz) >= 0.0)
                      & (t < best))
                best = np.where(ok, t, best)
        accept = (best < old) & (np.isinf(old) | (old - best > tol * old))
    return best, accept


def _diagonals(nr, nz, di, dk):
    for d in range(nr + nz - 1):
        ip = np.arange(max(0, d - nz + 1), min(nr - 1, d) + 1)
        kp = d - ip
        yield (ip if di > 0 else nr - 1 - ip), (kp if dk > 0 else nz - 1 - kp)


def solve_sections(slowness, zsrc, s0, nr, h, tol=TOL, max_iters=MAX_ITERS, orders=ORDERS, want_tau=False):
    """``slowness`` (n_sections, nz): per depth row; ``zsrc``: the source's depth below row 0; ``s0``: the slowness at
    the source.  Returns ``(T (n_sections, nr, nz), rounds, status)``: ``rounds`` counts the rounds run, the last one
    (which accepted nothing) included; status 1: ``max_iters`` rounds did not settle the section."""
    slowness, s0, h, tau, frozen, t0, t0x, t0z = _prepare(slowness, zsrc, s0, nr, h)
    n_sec, nz = slowness.shape
    tol = float(tol)
    rounds = np.zeros(n_sec, dtype=np.int32)
    done = np.zeros(n_sec, dtype=bool)
    for _ in range(int(max_iters)):
        any_accept = np.zeros(n_sec, dtype=bool)
        for di, dk in orders:
            for i, k in _diagonals(nr, nz, di, dk):
                old = tau[:, i + 1, k + 1]
                best, accept = _candidates(old, tau[:, i, k + 1], tau[:, i + 2, k + 1], tau[:, i + 1, k],
                                           tau[:, i + 1, k + 2], t0[:, i, k], t0x[:, i, k], t0z[:, i, k],
                                           slowness[:, k], h, tol)
                accept &= ~frozen[:, i, k]
                tau[:, i + 1, k + 1] = np.where(accept, best, old)
                any_accept |= accept.any(axis=1)
        rounds[~done] += 1                                  # (a settled section's further rounds change nothing)
        done |= ~any_accept
        if done.all():
            break
    status = np.where(done, 0, 1).astype(np.int32)
    with np.errstate(invalid="ignore"):
        out = t0 * tau[:, 1:-1, 1:-1]
    out = np.where(t0 == 0.0, 0.0, out)                     # the node at the source: T = 0
    return (out, rounds, status, tau[:, 1:-1, 1:-1]) if want_tau else (out, rounds, status)


def solve_sections_serial(slowness, zsrc, s0, nr, h, tol=TOL, max_iters=MAX_ITERS, orders=ORDERS):
    """The same solver as the plain serial loop, ``i`` outer and ``k`` inner: what the diagonal form must equal."""
    slowness, s0, h, tau, frozen, t0, t0x, t0z = _prepare(slowness, zsrc, s0, nr, h)
    n_sec, nz = slowness.shape
    tol = float(tol)
    rounds = np.zeros(n_sec, dtype=np.int32)
    status = np.ones(n_sec, dtype=np.int32)
    one = lambda v: np.array([v], dtype=np.float64)         # noqa: E731
    for s in range(n_sec):
        for _ in range(int(max_iters)):
            any_accept = False
            for di, dk in orders:
                for i in (range(nr) if di > 0 else range(nr - 1, -1, -1)):
                    for k in (range(nz) if dk > 0 else range(nz - 1, -1, -1)):
                        if frozen[s, i, k]:
                            continue
                        old = one(tau[s, i + 1, k + 1])
                        best, accept = _candidates(old, one(tau[s, i, k + 1]), one(tau[s, i + 2, k + 1]),
                                                   one(tau[s, i + 1, k]), one(tau[s, i + 1, k + 2]), one(t0[s, i, k]),
                                                   one(t0x[s, i, k]), one(t0z[s, i, k]), one(slowness[s, k]), h, tol)
                        if accept[0]:
                            tau[s, i + 1, k + 1] = best[0]
                            any_accept = True
            rounds[s] += 1
            if not any_accept:
                status[s] = 0
                break
    with np.errstate(invalid="ignore"):
        out = t0 * tau[:, 1:-1, 1:-1]
    out = np.where(t0 == 0.0, 0.0, out)
    return out, rounds, status


# -- c. sweep ----------------------------------------------------------------------------------------------------------
def bilinear(dist, depth, x0, z0, h, section):
    """The reference's interpolation rule (create_lut.py:746-762), restated: the cell comes from the floor of the
    OFFSETS from the section's origin, the fractions from ``np.remainder`` of the COORDINATES themselves; the two
    columns of the cell are blended along the distance first (row k, then row k + 1), then the two results along
    the depth.  ``dist``, ``depth``: 1-D arrays; ``section`` (nr, nz) of spacing ``h`` from ``(x0, z0)``."""
    col = np.floor((dist - x0) / h).astype(int)
    row = np.floor((depth - z0) / h).astype(int)
    fx = np.remainder(dist, h) / h
    fz = np.remainder(depth, h) / h
    upper = section[col, row] * (1 - fx) + section[col + 1, row] * fx
    lower = section[col, row + 1] * (1 - fx) + section[col + 1, row + 1] * fx
    return upper * (1 - fz) + lower * fz


def distances_depths(ll_corner, node_spacing, node_count, station_xy):
    """Per node of the grid, flat in C order: horizontal distance from the station, and depth (what
    create_lut.py:471-473 forms)."""
    gx, gy, gz = grid_xyz(ll_corner, node_spacing, node_count)
    off_x, off_y = gx - float(station_xy[0]), gy - float(station_xy[1])
    return np.sqrt(off_x * off_x + off_y * off_y).ravel(), gz.ravel()


def outside(dist, depth, x0, z0, h, nr, nz):
    """Flat indices of the nodes whose four corners are not all inside an (nr, nz) section."""
    col, row = np.floor((dist - x0) / h), np.floor((depth - z0) / h)
    return np.flatnonzero(~((col >= 0) & (col <= nr - 2) & (row >= 0) & (row <= nz - 2)))


def sweep(ll_corner, node_spacing, node_count, station_xy, section, x0, z0, h):
    """One row of the table: the section swept round its station over the grid (create_lut.py:504-513)."""
    dist, depth = distances_depths(ll_corner, node_spacing, node_count, station_xy)
    bad = outside(dist, depth, x0, z0, h, *section.shape)
    if len(bad):
        raise IndexError(f"node {bad[0]} lies outside its section")
    return bilinear(dist, depth, float(x0), float(z0), float(h), section).reshape(tuple(int(n) for n in node_count))
