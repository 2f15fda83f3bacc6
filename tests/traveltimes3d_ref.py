# -*- coding: utf-8 -*-
"""
NumPy restatement of the grid eikonal solver (include/qmhip.h: qm_engine_tt_eikonal3d; kernels:
csrc/qm_traveltimes.hpp) -- the specification the GPU tests compare against, bit for bit.

|grad T| = s(x, y, z) on the node grid ``ll_corner + index * node_spacing``, one solve per row: the section solver's
multiplicatively factored first-order upwind scheme (tests/traveltimes_ref.py) with one axis more.  T = T0 tau,
T0 = s0 rho from the row's source, which lies anywhere inside the grid; the eight nodes of the source's cell are
frozen; a node takes the smallest of its 6 one-sided, 12 two-sided and 8 three-sided candidates; Gauss-Seidel sweeps
in the eight orderings ``ORDERS`` make a round, rounds repeat until one accepts nothing in the row.

* ``solve``: every plane ``i' + j' + k' = d`` of a sweep at once (indices after the ordering's reflection), all rows
  side by side.  Only elementwise float64 operations, one rounding each, in the kernel's order; the candidates of a
  kind are stacked along a leading axis and the smallest kept one is taken -- the value the kernel's running
  ``t < best`` ends with, whatever the sequence.
* ``solve_serial``: the plain triple loop, x outer and z inner, scalar by scalar in the kernel's literal sequence.  A
  node's six neighbours lie in the planes d - 1 and d + 1, never in its own: the plane form reads what this loop reads.

tests/test_traveltimes3d_host.py pins both to each other and to closed forms.
"""

import itertools

import numpy as np

TOL = 2.0 ** -40
MAX_ITERS = 64
ORDERS = tuple(itertools.product((+1, -1), repeat=3))       # directions of (x, y, z) of the eight sweeps
PAIRS = ((0, 1), (0, 2), (1, 2))                            # the axes of the two-sided candidates, in this order
SIGNS = (1.0, -1.0)                                         # side 0: the neighbour at index - 1; side 1: at index + 1


def source_cell(ll_corner, node_spacing, node_count, source):
    """Per axis ``floor((src - ll) / h)``, clipped to ``n - 2``: the cell whose eight nodes are frozen."""
    ll, sp = np.asarray(ll_corner, dtype=np.float64), np.asarray(node_spacing, dtype=np.float64)
    cell = np.floor((np.asarray(source, dtype=np.float64) - ll) / sp).astype(np.int64)
    return np.minimum(cell, np.asarray(node_count, dtype=np.int64) - 2)


def _prepare(ll_corner, node_spacing, node_count, sources, s0, slowness, row_model):
    ll, sp = np.asarray(ll_corner, dtype=np.float64), np.asarray(node_spacing, dtype=np.float64)
    n = tuple(int(v) for v in node_count)
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 3)
    rows = len(src)
    s0 = np.asarray(s0, dtype=np.float64).reshape(rows)
    slowness = np.asarray(slowness, dtype=np.float64).reshape((-1,) + n)
    row_model = np.asarray(row_model, dtype=np.int64).reshape(rows)
    if min(n) < 2:
        raise ValueError("an axis shorter than 2 nodes")
    ur = ll + (np.array(n) - 1) * sp
    if np.any(src < ll) or np.any(src > ur):
        raise ValueError("source outside the grid")
    if row_model.min() < 0 or row_model.max() >= len(slowness):
        raise ValueError("row_model out of range")
    if not np.all(np.isfinite(slowness) & (slowness > 0.0)):
        raise ValueError("slowness not finite and positive")
    axes = [ll[j] + (np.arange(n[j]) * sp[j]) for j in range(3)]
    gx, gy, gz = np.meshgrid(*axes, indexing="ij")
    off = [g[None] - src[:, j, None, None, None] for j, g in enumerate((gx, gy, gz))]
    s0_ = s0[:, None, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.sqrt(off[0] * off[0] + off[1] * off[1] + off[2] * off[2])
        t0 = s0_ * rho
        t0d = [s0_ * o / rho for o in off]
    slow = slowness[row_model]                                  # (rows, nx, ny, nz)
    tau = np.full((rows, n[0] + 2, n[1] + 2, n[2] + 2), np.inf)     # (a border of +inf: no neighbour there)
    frozen = np.zeros((rows,) + n, dtype=bool)
    for r in range(rows):
        c = source_cell(ll, sp, n, src[r])
        for i, j, k in itertools.product((c[0], c[0] + 1), (c[1], c[1] + 1), (c[2], c[2] + 1)):
            frozen[r, i, j, k] = True
            tau[r, i + 1, j + 1, k + 1] = 1.0 if t0[r, i, j, k] == 0.0 else (s0[r] + slow[r, i, j, k]) / (2.0 * s0[r])
    return n, sp, s0, slow, tau, frozen, t0, t0d


def _finish(t0, tau):
    with np.errstate(invalid="ignore"):
        out = t0 * tau[:, 1:-1, 1:-1, 1:-1]
    return np.where(t0 == 0.0, 0.0, out)                       # the node at the source: T = 0


def _candidates(old, nb, t0, t0d, sk, sp, tol):
    """The node update, elementwise over arrays of one shape.  ``nb[d][side]``: tau of the neighbour along axis d at
    index - 1 (side 0) and index + 1 (side 1); ``t0d[d]``: the derivative of T0 along axis d."""
    inf = np.inf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sg = np.array(SIGNS).reshape((1, 2) + (1,) * old.ndim)
        h = np.asarray(sp, dtype=np.float64).reshape((3, 1) + (1,) * old.ndim)
        ta = np.array([[nb[d][0], nb[d][1]] for d in range(3)])
        av = np.isfinite(ta)
        a = t0[None, None] * sg / h + np.array(t0d)[:, None]
        b = t0[None, None] * sg * ta / h
        t = (b + sg * sk[None, None]) / a
        ok = av & (sg * a > 0.0) & (t > 0.0)
        best = np.where(ok, t, inf).min(axis=(0, 1))
        # two-sided: axes (x, y), (x, z), (y, z); sides (p, q)
        pick = [(d, p, e, q) for d, e in PAIRS for p in (0, 1) for q in (0, 1)]
        d1, p1, d2, p2 = (np.array(v) for v in zip(*pick))
        a1, b1, a2, b2 = a[d1, p1], b[d1, p1], a[d2, p2], b[d2, p2]
        s1, s2 = sg[0, p1], sg[0, p2]
        qa = a1 * a1 + a2 * a2
        qb = a1 * b1 + a2 * b2
        qc = b1 * b1 + b2 * b2 - sk * sk
        disc = qb * qb - qa * qc
        t = (qb + np.sqrt(disc)) / qa
        ok = av[d1, p1] & av[d2, p2] & (disc >= 0.0) & (s1 * (a1 * t - b1) >= 0.0) & (s2 * (a2 * t - b2) >= 0.0)
        best = np.minimum(best, np.where(ok, t, inf).min(axis=0))
        # three-sided: sides (p, q, r) of (x, y, z)
        p1, p2, p3 = (np.array(v) for v in zip(*itertools.product((0, 1), repeat=3)))
        a1, b1, a2, b2, a3, b3 = a[0, p1], b[0, p1], a[1, p2], b[1, p2], a[2, p3], b[2, p3]
        s1, s2, s3 = sg[0, p1], sg[0, p2], sg[0, p3]
        qa = a1 * a1 + a2 * a2 + a3 * a3
        qb = a1 * b1 + a2 * b2 + a3 * b3
        qc = b1 * b1 + b2 * b2 + b3 * b3 - sk * sk
        disc = qb * qb - qa * qc
        t = (qb + np.sqrt(disc)) / qa
        ok = (av[0, p1] & av[1, p2] & av[2, p3] & (disc >= 0.0) & (s1 * (a1 * t - b1) >= 0.0)
              & (s2 * (a2 * t - b2) >= 0.0) & (s3 * (a3 * t - b3) >= 0.0))
        best = np.minimum(best, np.where(ok, t, inf).min(axis=0))
        accept = (best < old) & (np.isinf(old) | (old - best > tol * old))
    return best, accept


def planes(n, order):
    """The planes of one sweep: per d = 0 .. nx + ny + nz - 3 the index arrays (i, j, k) of the nodes with
    i' + j' + k' = d, the primed indices counted from the end of an axis the ordering runs backwards."""
    ip, jp, kp = np.meshgrid(*(np.arange(m) for m in n), indexing="ij")
    d = (ip + jp + kp).ravel()
    idx = [(v if sgn > 0 else m - 1 - v).ravel() for v, sgn, m in zip((ip, jp, kp), order, n)]
    by_plane = np.argsort(d, kind="stable")
    starts = np.searchsorted(d[by_plane], np.arange(sum(n) - 1))
    for lo, hi in zip(starts[:-1], starts[1:]):
        sel = by_plane[lo:hi]
        yield idx[0][sel], idx[1][sel], idx[2][sel]


def solve(ll_corner, node_spacing, node_count, sources, s0, slowness, row_model, tol=TOL, max_iters=MAX_ITERS,
          orders=ORDERS):
    """``sources`` (rows, 3), ``s0`` (rows,): the slowness at the source; ``slowness`` (n_models, nx, ny, nz);
    ``row_model`` (rows,).  Returns ``(T (rows, nx, ny, nz), rounds, status)``: ``rounds`` counts a row's rounds, the
    last one (which accepted nothing) included; status 1: ``max_iters`` rounds did not settle the row."""
    n, sp, s0, slow, tau, frozen, t0, t0d = _prepare(ll_corner, node_spacing, node_count, sources, s0, slowness,
                                                     row_model)
    rows = len(s0)
    tol = float(tol)
    rounds = np.zeros(rows, dtype=np.int32)
    done = np.zeros(rows, dtype=bool)
    sweeps = [list(planes(n, order)) for order in orders]
    for _ in range(int(max_iters)):
        any_accept = np.zeros(rows, dtype=bool)
        for sweep in sweeps:
            for i, j, k in sweep:
                old = tau[:, i + 1, j + 1, k + 1]
                nb = ((tau[:, i, j + 1, k + 1], tau[:, i + 2, j + 1, k + 1]),
                      (tau[:, i + 1, j, k + 1], tau[:, i + 1, j + 2, k + 1]),
                      (tau[:, i + 1, j + 1, k], tau[:, i + 1, j + 1, k + 2]))
                best, accept = _candidates(old, nb, t0[:, i, j, k], [t[:, i, j, k] for t in t0d], slow[:, i, j, k], sp,
                                           tol)
                accept &= ~frozen[:, i, j, k]
                tau[:, i + 1, j + 1, k + 1] = np.where(accept, best, old)
                any_accept |= accept.any(axis=1)
        rounds[~done] += 1                                  # (a settled row's further rounds change nothing)
        done |= ~any_accept
        if done.all():
            break
    return _finish(t0, tau), rounds, np.where(done, 0, 1).astype(np.int32)


def _update_scalar(old, nb, t0, t0d, sk, sp, tol):
    """One node, float64 scalars, in the kernel's literal sequence: the running ``t < best``."""
    inf = np.float64(np.inf)
    best = inf
    a, b, av = [[None, None] for _ in range(3)], [[None, None] for _ in range(3)], [[None, None] for _ in range(3)]
    for d in range(3):
        for p, sg in enumerate(SIGNS):
            ta = nb[d][p]
            av[d][p] = ta < inf
            a[d][p] = t0 * sg / sp[d] + t0d[d]
            b[d][p] = t0 * sg * ta / sp[d]
            t = (b[d][p] + sg * sk) / a[d][p]
            if av[d][p] and sg * a[d][p] > 0.0 and t > 0.0 and t < best:
                best = t
    for d, e in PAIRS:
        for p in (0, 1):
            for q in (0, 1):
                a1, b1, a2, b2 = a[d][p], b[d][p], a[e][q], b[e][q]
                qa = a1 * a1 + a2 * a2
                qb = a1 * b1 + a2 * b2
                qc = b1 * b1 + b2 * b2 - sk * sk
                disc = qb * qb - qa * qc
                t = (qb + np.sqrt(disc)) / qa
                if (av[d][p] and av[e][q] and disc >= 0.0 and SIGNS[p] * (a1 * t - b1) >= 0.0
                        and SIGNS[q] * (a2 * t - b2) >= 0.0 and t < best):
                    best = t
    for p, q, r in itertools.product((0, 1), repeat=3):
        a1, b1, a2, b2, a3, b3 = a[0][p], b[0][p], a[1][q], b[1][q], a[2][r], b[2][r]
        qa = a1 * a1 + a2 * a2 + a3 * a3
        qb = a1 * b1 + a2 * b2 + a3 * b3
        qc = b1 * b1 + b2 * b2 + b3 * b3 - sk * sk
        disc = qb * qb - qa * qc
        t = (qb + np.sqrt(disc)) / qa
        if (av[0][p] and av[1][q] and av[2][r] and disc >= 0.0 and SIGNS[p] * (a1 * t - b1) >= 0.0
                and SIGNS[q] * (a2 * t - b2) >= 0.0 and SIGNS[r] * (a3 * t - b3) >= 0.0 and t < best):
            best = t
    return best, bool(best < old and (old == inf or old - best > tol * old))


def solve_serial(ll_corner, node_spacing, node_count, sources, s0, slowness, row_model, tol=TOL, max_iters=MAX_ITERS,
                 orders=ORDERS):
    """The same solver as the plain serial loop, x outer, y, z inner: what the plane form must equal."""
    n, sp, s0, slow, tau, frozen, t0, t0d = _prepare(ll_corner, node_spacing, node_count, sources, s0, slowness,
                                                     row_model)
    rows = len(s0)
    tol = np.float64(tol)
    rounds = np.zeros(rows, dtype=np.int32)
    status = np.ones(rows, dtype=np.int32)
    run = lambda m, sgn: range(m) if sgn > 0 else range(m - 1, -1, -1)      # noqa: E731
    with np.errstate(all="ignore"):
        for r in range(rows):
            tr_ = tau[r]
            for _ in range(int(max_iters)):
                any_accept = False
                for order in orders:
                    for i, j, k in itertools.product(*(run(m, sgn) for m, sgn in zip(n, order))):
                        if frozen[r, i, j, k]:
                            continue
                        nb = ((tr_[i, j + 1, k + 1], tr_[i + 2, j + 1, k + 1]),
                              (tr_[i + 1, j, k + 1], tr_[i + 1, j + 2, k + 1]),
                              (tr_[i + 1, j + 1, k], tr_[i + 1, j + 1, k + 2]))
                        best, accept = _update_scalar(tr_[i + 1, j + 1, k + 1], nb, t0[r, i, j, k],
                                                      [t[r, i, j, k] for t in t0d], slow[r, i, j, k], sp, tol)
                        if accept:
                            tr_[i + 1, j + 1, k + 1] = best
                            any_accept = True
                rounds[r] += 1
                if not any_accept:
                    status[r] = 0
                    break
    return _finish(t0, tau), rounds, status
