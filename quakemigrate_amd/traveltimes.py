# -*- coding: utf-8 -*-
"""
Travel-time tables computed on the GPU -- the reference's ``compute_traveltimes``
(``quakemigrate/lut/create_lut.py``) without an external program:

* ``"homogeneous"`` (create_lut.py:241-265);
* ``"3d"``: a 3-D velocity model given per phase on the grid's own nodes -- what the reference reaches only through
  NonLinLoc and ``read_nlloc``, its own ``"3dfmm"`` being ``NotImplementedError`` (create_lut.py:214-217) --, and
  ``"1d"`` with ``solver="grid"``: a 1-D model spread over the grid's depths, the reference's ``1dfmm`` path
  (create_lut.py:298-317) with the engine's solver in scikit-fmm's place.  Both solve ``|grad T| = s`` on the grid's
  nodes (``Engine.traveltimes_eikonal3d``), one solve per station and phase, stations inside the grid (the
  reference's own condition for ``1dfmm``, :306-313).  This is a FIRST-ORDER factored sweep, not scikit-fmm's
  second-order fast march: the two solve the same equation and their values differ by the schemes' discretisation
  errors (measured here against closed forms: profiles/traveltimes3d_accuracy.txt), and the source is the station's
  true position unless ``snap_to_node`` moves it to the node ``_eikonal_fmm`` picks.  There is no fixture from
  ``1dfmm``: scikit-fmm is not among this project's dependencies, so nothing here was compared with it;
* ``"1d"``: a 1-D velocity model, along the structure of the reference's ``1dnlloc`` path (create_lut.py:389-513): a
  2-D travel-time section per station and phase in (horizontal distance, depth), swept round the station over the
  3-D grid by ``_bilinear_interpolate`` (:746-762).  The section comes from the engine's eikonal solver
  (``Engine.traveltime_sections``) instead of NonLinLoc's ``Grid2Time``.  A 1-D model is axisymmetric about the
  station, so the section is the whole problem; the station need not sit on a node or inside the grid.

This module is the host side: the velocity model's rows, the planner of the sections, the slowness at a station of a
3-D model (:func:`trilinear`), the reference's nearest node (:func:`nearest_node`) -- all pure NumPy -- and
:func:`compute_traveltimes`, which returns ``{station: {phase: grid}}`` -- the shape of ``lut.traveltimes``.  With
``device=True`` the grids are torch tensors on the engine's GPU, which ``Engine.set_traveltime_grids`` and
``MigrationScan(device_serving=True)`` take without a host round trip.

Coordinates are grid coordinates in one unit of length (the reference converts to km for NonLinLoc; nothing here
depends on the unit), depths positive down, velocities in that unit per second.  Not here: projections and the LUT
pickle (pyproj), NonLinLoc files, bit parity with ``1dfmm`` (another scheme).
"""

import numpy as np

MARGIN = 5                      # the reference's extra nodes on both section axes (create_lut.py:864-865)
LIFT = 2                        # nodes between the section's first row and the depth span
PLAIN_COLUMNS = ("Depth", "Vp", "Vs")       # a model given as plain arrays: (depths, vp) or (depths, vp, vs)


def _column(vmod, name):
    if isinstance(vmod, (tuple, list)):
        vmod = dict(zip(PLAIN_COLUMNS, vmod))
    try:
        col = vmod[name]
    except (KeyError, IndexError, TypeError, ValueError) as err:
        raise KeyError(f"the velocity model has no column {name!r}") from err
    return np.asarray(getattr(col, "values", col), dtype=np.float64).reshape(-1)


def model_velocity(vmod, phase, depths, block_model=False):
    """The velocity of ``phase`` at ``depths``.  ``vmod``: anything indexable by ``"Depth"`` and ``"V<phase>"``
    (``"Vp"``, ``"Vs"``) like the reference's DataFrame -- a dict of arrays will do --, or the plain arrays themselves
    as a tuple ``(depths, vp)`` or ``(depths, vp, vs)``.  By default linear between the model's depths and constant
    outside them; ``block_model``: the velocity of the layer whose top is at or above the depth (the first layer's
    above the model)."""
    top = _column(vmod, "Depth")
    vel = _column(vmod, f"V{phase.lower()}")
    if len(top) != len(vel) or len(top) < 1:
        raise ValueError(f"{len(top)} depths, {len(vel)} velocities for phase {phase}")
    if np.any(np.diff(top) <= 0):
        raise ValueError("the model's depths must increase")
    depths = np.asarray(depths, dtype=np.float64)
    if block_model:
        return vel[np.clip(np.searchsorted(top, depths, side="right") - 1, 0, len(top) - 1)]
    return np.interp(depths, top, vel)


def plan_sections(ll_corner, node_spacing, node_count, stations_xyz, section_dx):
    """
    The sections of a call, one per station, padded to one ``nr x nz``.  Per station (create_lut.py:471-482, 864-865):

    * ``max_dist``: the largest horizontal distance of a node from the station;
    * ``depth_span``: ``[min(ll z, station z), max(ur z, station z)]``;
    * ``x0 = 0``; ``z0``: an integer multiple of ``section_dx``, at least ``LIFT`` nodes above the span;
    * ``nr = ceil(max_dist / dx) + 5``, ``nz = ceil((span end - z0) / dx) + 5``.

    ``z0`` is a multiple of the spacing because ``_bilinear_interpolate`` takes its fractions from the coordinates
    (``np.remainder(z, dx)``) and its cell from the offsets (``floor((z - z0) / dx)``): the two name the same cell
    only then.  They can still differ by one cell where a depth lies within rounding of a multiple of ``dx`` -- the
    quotient rounds to the next integer while the remainder stays just below ``dx``, or the reverse -- and the value
    is then the linear extension of the neighbouring cell; that edge is the reference's own, for any origin.

    Returns a dict: ``max_dist``, ``depth_span`` (n, 2), ``z0``, ``source_depth`` (station depth below ``z0``), ``nr``,
    ``nz`` (the padded shape), ``nr_each``, ``nz_each``.
    """
    ll = np.asarray(ll_corner, dtype=np.float64)
    sp = np.asarray(node_spacing, dtype=np.float64)
    nc = [int(n) for n in node_count]
    xyz = np.asarray(stations_xyz, dtype=np.float64).reshape(-1, 3)
    dx_ = float(section_dx)
    if not dx_ > 0:
        raise ValueError(f"section_dx must be positive, got {section_dx}")
    gx, gy = np.meshgrid(ll[0] + (np.arange(nc[0]) * sp[0]), ll[1] + (np.arange(nc[1]) * sp[1]), indexing="ij")
    ur_z = ll[2] + ((nc[2] - 1) * sp[2])
    max_dist, span, z0, nr, nz = [], [], [], [], []
    for sx, sy, sz in xyz:
        off_x, off_y = gx - sx, gy - sy
        far = float(np.sqrt(off_x * off_x + off_y * off_y).max())
        top, bottom = min(float(ll[2]), float(sz)), max(float(ur_z), float(sz))
        first_row = (np.floor(top / dx_) - LIFT) * dx_
        max_dist.append(far)
        span.append([top, bottom])
        z0.append(first_row)
        nr.append(int(np.ceil(far / dx_)) + MARGIN)
        nz.append(int(np.ceil((bottom - first_row) / dx_)) + MARGIN)
    z0 = np.array(z0)
    return dict(max_dist=np.array(max_dist), depth_span=np.array(span), z0=z0, source_depth=xyz[:, 2] - z0,
                nr=max(nr), nz=max(nz), nr_each=np.array(nr), nz_each=np.array(nz))


def _stations(stations):
    if hasattr(stations, "items"):
        names, xyz = list(stations.keys()), [stations[k] for k in stations]
    else:
        names, xyz = [s[0] for s in stations], [s[1:4] for s in stations]
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    if len(set(names)) != len(names):
        raise ValueError("station names must be unique")
    return names, xyz


def _grid(ll_corner, node_spacing, node_count):
    ll = np.asarray(ll_corner, dtype=np.float64).reshape(3)
    sp = np.asarray(node_spacing, dtype=np.float64).reshape(3)
    nc = np.asarray([int(n) for n in node_count], dtype=np.int64).reshape(3)
    return ll, sp, nc


def trilinear(volume, ll_corner, node_spacing, node_count, xyz):
    """``volume`` (nx, ny, nz), a NumPy array or a device tensor, at the points ``xyz`` (n, 3) inside the grid.  Per
    axis the cell is ``floor((p - ll) / h)`` clipped to ``[0, n - 2]`` and the fraction ``f = (p - ll) / h - cell``;
    with ``c`` the cell's eight corners the value is the one expression

        ((c000 (1 - fz) + c001 fz) (1 - fy) + (c010 (1 - fz) + c011 fz) fy) (1 - fx)
        + ((c100 (1 - fz) + c101 fz) (1 - fy) + (c110 (1 - fz) + c111 fz) fy) fx

    in float64 on the host; where a fraction comes out as 0 or 1 it is the corner's value exactly."""
    ll, sp, nc = _grid(ll_corner, node_spacing, node_count)
    if tuple(volume.shape) != tuple(nc):
        raise ValueError(f"a volume of shape {tuple(volume.shape)} on a grid of {tuple(nc)} nodes")
    out = []
    for p in np.asarray(xyz, dtype=np.float64).reshape(-1, 3):
        q = (p - ll) / sp
        cell = np.clip(np.floor(q), 0, nc - 2).astype(np.int64)
        fx, fy, fz = q - cell
        c = volume[cell[0]:cell[0] + 2, cell[1]:cell[1] + 2, cell[2]:cell[2] + 2]
        c = np.asarray(c.cpu() if hasattr(c, "cpu") else c, dtype=np.float64)
        out.append(((c[0, 0, 0] * (1 - fz) + c[0, 0, 1] * fz) * (1 - fy)
                    + (c[0, 1, 0] * (1 - fz) + c[0, 1, 1] * fz) * fy) * (1 - fx)
                   + ((c[1, 0, 0] * (1 - fz) + c[1, 0, 1] * fz) * (1 - fy)
                      + (c[1, 1, 0] * (1 - fz) + c[1, 1, 1] * fz) * fy) * fx)
    return np.array(out, dtype=np.float64)


def nearest_node(ll_corner, node_spacing, node_count, xyz):
    """The node the reference's ``_eikonal_fmm`` moves a station to (create_lut.py:379-384): the smallest
    ``|dx| + |dy| + |dz|``, the lowest flat index among equals.  Returns ``(indices (n, 3), coordinates (n, 3))``."""
    ll, sp, nc = _grid(ll_corner, node_spacing, node_count)
    gx, gy, gz = (ll[j] + (np.arange(nc[j]) * sp[j]) for j in range(3))
    idx = []
    for p in np.asarray(xyz, dtype=np.float64).reshape(-1, 3):
        far = np.abs(gx - p[0])[:, None, None] + np.abs(gy - p[1])[None, :, None] + np.abs(gz - p[2])[None, None, :]
        idx.append(np.unravel_index(np.argmin(far), far.shape))
    idx = np.array(idx, dtype=np.int64).reshape(-1, 3)
    return idx, np.column_stack([gx[idx[:, 0]], gy[idx[:, 1]], gz[idx[:, 2]]])


def _require_inside(ll_corner, node_spacing, node_count, names, xyz, what):
    """The grid solver's condition, the reference's own for ``1dfmm`` (create_lut.py:306-313)."""
    ll, sp, nc = _grid(ll_corner, node_spacing, node_count)
    ur = ll + ((nc - 1) * sp)
    for name, p in zip(names, xyz):
        if (p < ll).any() or (p > ur).any():
            raise ValueError(f"{what}: station {name} at {tuple(p)} lies outside the grid {tuple(ll)} .. {tuple(ur)}; "
                             "the solver on the grid's own nodes needs every station inside it (method '1d' with "
                             "solver='sections' does not)")


def _solve_on_grid(engine, ll_corner, node_spacing, node_count, xyz, n_ph, s0, slowness, tol, max_iters, device):
    """One row per source and phase, phase ``j``'s rows in model ``j`` of ``slowness``."""
    grids, _, _ = engine.traveltimes_eikonal3d(ll_corner, node_spacing, node_count, np.repeat(xyz, n_ph, axis=0), s0,
                                               slowness, np.tile(np.arange(n_ph), len(xyz)), tol=tol,
                                               max_iters=max_iters, device=device)
    return grids


def compute_traveltimes(engine, ll_corner, node_spacing, node_count, stations, method, phases=("P", "S"), vp=None,
                        vs=None, vmod=None, section_dx=0.1, block_model=False, device=True, tol=2.0 ** -40,
                        max_iters=64, velocity=None, solver="sections", snap_to_node=False):
    """
    Travel-time grids for every station and phase, computed on ``engine``'s GPU.

    ``stations``: ``{name: (x, y, z)}`` or a sequence of ``(name, x, y, z)``, in grid coordinates.  ``method``:

    * ``"homogeneous"`` (``vp`` / ``vs``);
    * ``"1d"`` (``vmod``: see :func:`model_velocity`; ``block_model``) with ``solver="sections"`` (the default;
      ``section_dx``: the sections' spacing, the reference's ``nlloc_dx``) or ``solver="grid"``: the model spread over
      the grid's depths by :func:`model_velocity` and solved on the grid's own nodes, stations inside the grid;
    * ``"3d"`` (``velocity``: ``{"P": array, "S": array}`` of shape ``node_count``, NumPy arrays or tensors on the
      engine's GPU): solved on the grid's own nodes, stations inside the grid; the slowness at a station is ``1 /``
      :func:`trilinear` of the velocity there.

    ``snap_to_node`` (the two grid solves): move each station to the node the reference's ``_eikonal_fmm`` picks
    (:func:`nearest_node`) before solving; by default the source is the station's true position.  Returns
    ``{station: {phase: grid}}`` with grids of shape ``node_count`` in seconds -- torch tensors on the engine's GPU
    (views of one tensor) with ``device``, else NumPy arrays.
    """
    names, xyz = _stations(stations)
    phases = list(phases)
    if not names or not phases:
        raise ValueError("no stations or no phases")
    n_ph = len(phases)
    if method == "1d" and solver not in ("sections", "grid"):
        raise ValueError(f"'{solver}' is not a solver of method '1d': 'sections' or 'grid'")
    if method == "3d":
        velocity = velocity or {}
        shape = tuple(int(n) for n in node_count)
        for ph in phases:
            if velocity.get(ph) is None:
                raise ValueError(f"method '3d' needs velocity[{ph!r}] for phase {ph}")
            if tuple(velocity[ph].shape) != shape:
                raise ValueError(f"velocity[{ph!r}] has shape {tuple(velocity[ph].shape)}, the grid {shape}")
        _require_inside(ll_corner, node_spacing, node_count, names, xyz, "method '3d'")
        at = nearest_node(ll_corner, node_spacing, node_count, xyz)[1] if snap_to_node else xyz
        s0 = 1.0 / np.column_stack([trilinear(velocity[ph], ll_corner, node_spacing, node_count, at) for ph in phases])
        if all(hasattr(velocity[ph], "data_ptr") for ph in phases):
            import torch

            slowness = torch.stack([1.0 / velocity[ph].to(torch.float64) for ph in phases]).contiguous()
        else:
            slowness = np.stack([1.0 / np.asarray(velocity[ph].cpu() if hasattr(velocity[ph], "cpu") else velocity[ph],
                                                  dtype=np.float64) for ph in phases])
        grids = _solve_on_grid(engine, ll_corner, node_spacing, node_count, at, n_ph, s0.reshape(-1), slowness, tol,
                               max_iters, device)
    elif method == "1d" and solver == "grid":
        if vmod is None:
            raise ValueError("method '1d' needs vmod")
        _require_inside(ll_corner, node_spacing, node_count, names, xyz, "method '1d' with solver='grid'")
        ll, sp, nc = _grid(ll_corner, node_spacing, node_count)
        depths = ll[2] + (np.arange(nc[2]) * sp[2])
        at = nearest_node(ll_corner, node_spacing, node_count, xyz)[1] if snap_to_node else xyz
        s0 = np.column_stack([1.0 / model_velocity(vmod, ph, at[:, 2], block_model) for ph in phases])
        slowness = np.stack([np.broadcast_to(1.0 / model_velocity(vmod, ph, depths, block_model), tuple(nc))
                             for ph in phases])
        grids = _solve_on_grid(engine, ll_corner, node_spacing, node_count, at, n_ph, s0.reshape(-1), slowness, tol,
                               max_iters, device)
    elif method == "homogeneous":
        velocity = {"P": vp, "S": vs}
        for ph in phases:
            if velocity.get(ph) is None:
                raise ValueError(f"method 'homogeneous' needs v{ph.lower()} for phase {ph}")
        grids = engine.traveltimes_homogeneous(ll_corner, node_spacing, node_count, np.repeat(xyz, n_ph, axis=0),
                                               np.tile([float(velocity[ph]) for ph in phases], len(names)),
                                               device=device)
    elif method == "1d":
        if vmod is None:
            raise ValueError("method '1d' needs vmod")
        plan = plan_sections(ll_corner, node_spacing, node_count, xyz, section_dx)
        rows_k = np.arange(plan["nz"]) * float(section_dx)
        slowness, s0 = [], []
        for i in range(len(names)):
            for ph in phases:
                slowness.append(1.0 / model_velocity(vmod, ph, plan["z0"][i] + rows_k, block_model))
                s0.append(1.0 / model_velocity(vmod, ph, xyz[i, 2], block_model))
        sections, _, _ = engine.traveltime_sections(np.array(slowness), np.repeat(plan["source_depth"], n_ph),
                                                    plan["nr"], section_dx, source_slowness=np.array(s0), tol=tol,
                                                    max_iters=max_iters, device=True)
        origins = np.column_stack([np.zeros(len(names)), plan["z0"]])
        grids = engine.sweep_sections(sections, ll_corner, node_spacing, node_count, np.repeat(xyz[:, :2], n_ph, axis=0),
                                      np.arange(len(names) * n_ph), np.repeat(origins, n_ph, axis=0), section_dx,
                                      device=device)
    else:
        raise ValueError(f"'{method}' is not a valid method here: 'homogeneous', '1d' (solver='sections' or 'grid') or "
                         "'3d' ('1dfmm' and '1dnlloc' stay with the reference's create_lut)")
    return {name: {ph: grids[i * n_ph + j] for j, ph in enumerate(phases)} for i, name in enumerate(names)}
