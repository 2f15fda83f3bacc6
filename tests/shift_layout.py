# -*- coding: utf-8 -*-
"""
The schedule arithmetic of the shift-reuse kernels, restated in NumPy, and travel-time tables DESIGNED to drive
the generated loops (csrc/gen_shift_asm.py) over the whole domain of that schedule (tests/test_shift_layout.py
checks on the CPU that the tables do what they are designed for; tests/test_shift_windows.py runs them on the GPU).

What the device builds per table (csrc/qm_shift.hpp: shift_group_delays, shift_window, shift_need_kernel): every
2x2x2 group of nodes reads, per table row, ONE window of consecutive samples per lane.  With d the eight nodes'
delays relative to the row's minimum over the brick (negative delays count as 0; a node outside the grid copies
node 0 of its group):

    e0  = min(d) rounded down to a multiple of 4 (wide tiles, six samples per lane: of 2)
    nq  = max(2, ceil((max(d) - e0 + samples per lane) / 4))       quads of four doubles; more than NQMAX: overflow
    node g adds window registers [2 (d_g - e0), ...): the OFFSET d_g - e0 is what the register index encodes

    need(brick, row) = the furthest 16-byte slot pair a lane may touch = max over the brick's groups of
                       (e0 + step * 63 + 4 * max(nq, NQMIN) + 3) // 4         (step = samples per lane: 4 or 6)
    run(brick)       = sum of need over the rows (row blocks: over the block's rows)
    fit              = no group overflows and (run + zero row) * 16 <= plane_bytes
                       (zero row: the all-zero window that the padding row of an ODD row count reads)

Here the same quantities come from whole-array operations over (group, node, row); nothing follows the kernels'
loops.  The constants are read from csrc/qm_shift_asm.inc when they are asked for.
"""

import collections
import pathlib
import re

import numpy as np

INC = pathlib.Path(__file__).resolve().parent.parent / "quakemigrate_amd" / "csrc" / "qm_shift_asm.inc"
WAVE = 64                       # lanes of a wavefront (qm_kernels.hpp: kWave)
INT32_MIN = -2 ** 31


def constants():
    """The generated header's integer constants by name (kShiftPlane, kShiftNqMax, ...)."""
    text = INC.read_text()
    out = {k: int(v) for k, v in re.findall(r"^constexpr int (\w+) = (-?\d+);", text, flags=re.M)}
    for name in ("kShiftNqMax", "kShiftNqMin", "kShiftNqMinWide", "kShiftPlane", "kShiftPlane3", "kShiftPlane8",
                 "kShiftWideSpl"):
        assert name in out, f"{name} not found in {INC.name}"
    return out


def plane_bytes(kind):
    """What shift_need_kernel is given as plane_bytes (qm_tables.hip: build_shift_tables) for each workgroup shape:
    '4' / '8' / '12' waves with all rows of a brick in LDS; 'wide': the wide tiles' ONE contiguous region (half of
    the 8-wave workgroup's LDS, kShiftLdsBytes8 / 2 with kShiftLdsBytes8 = 2 kShiftPlane8, qm_shift.hpp);
    'rows8': row blocks staged through registers; 'rows2' / 'rows4' / 'wide_rows': row blocks in one 80 KB half."""
    c = constants()
    return {"4": c["kShiftPlane"], "8": c["kShiftPlane8"], "12": c["kShiftPlane3"],
            "wide": (2 * c["kShiftPlane8"]) // 2, "rows8": c["kShiftPlane8"], "rows2": c["kShiftPlane"],
            "rows4": c["kShiftPlane"], "wide_rows": c["kShiftPlane"]}[kind]


# rows per block and brick shape of the row-block forms (build_shift_tables: block_rows, kShapesBlocks)
BLOCK_FORMS = {"rows8": (64, (4, 4, 4)), "rows2": (34, (4, 4, 4)), "rows4": (34, (4, 4, 2)),
               "wide_rows": (20, (4, 4, 4))}


def effective_brick(grid, brick):
    """A brick holds whole 2x2x2 groups and is no larger than the grid rounded up to even."""
    even = lambda v: v + (v & 1)
    return tuple(min(even(b), even(n)) for n, b in zip(grid, brick))


def row_blocks(S, block_rows):
    """(first row, rows) of every block: all rows at once (block_rows = 0), or nblk blocks of an even sb rows."""
    if not block_rows:
        return [(0, S)]
    nblk = -(-S // block_rows)
    sb = (-(-S // nblk) + 1) // 2 * 2
    return [(k * sb, min(sb, S - k * sb)) for k in range(nblk)]


class Layout:
    """Everything the restatement knows about (table, brick shape, tile kind, row blocks).

    Per (group, row) -- groups in lexicographic order of their first node over the WHOLE grid:
        dmin, e0, nq [G, S]; off [G, 8, S] (node n = 4 dx + 2 dy + dz); valid [G, 8]; brick_of_group [G]; first_node [G]
    per (brick, row): lo (the minimum delay), need, over (a group overflows); per (brick, block): run, zero, overflow
    totals: quads (fetched, with the unconditional ones), pairs ((group, row) pairs)."""

    def __init__(self, tt, brick, wide=False, block_rows=0):
        c = constants()
        tt = np.asarray(tt)
        nx, ny, nz, S = tt.shape
        self.grid, self.S, self.wide = (nx, ny, nz), S, bool(wide)
        self.step = c["kShiftWideSpl"] if wide else 4
        self.nq_min = c["kShiftNqMinWide"] if wide else c["kShiftNqMin"]
        self.nq_max = c["kShiftNqMax"]
        self.brick = effective_brick(self.grid, brick)
        d = np.maximum(tt.astype(np.int64), 0)                          # negative delays count as 0
        nb = [-(-n // b) for n, b in zip(self.grid, self.brick)]
        self.nbricks = int(np.prod(nb))
        bi = [np.arange(n) // b for n, b in zip(self.grid, self.brick)]
        brick_of_node = (bi[0][:, None, None] * nb[1] + bi[1][None, :, None]) * nb[2] + bi[2][None, None, :]
        self.lo = np.full((self.nbricks, S), np.iinfo(np.int64).max)
        np.minimum.at(self.lo, brick_of_node.ravel(), d.reshape(-1, S))
        hi = np.zeros((self.nbricks, S), dtype=np.int64)
        np.maximum.at(hi, brick_of_node.ravel(), d.reshape(-1, S))
        self.span = hi - self.lo
        # the 2x2x2 groups (bricks are even-sized: a group never straddles two bricks)
        g0 = np.stack(np.meshgrid(*(np.arange(0, n, 2) for n in self.grid), indexing="ij"), axis=-1).reshape(-1, 3)
        G = len(g0)
        delays = np.empty((G, 8, S), dtype=np.int64)
        self.valid = np.empty((G, 8), dtype=bool)
        self.node = np.empty((G, 8), dtype=np.int64)                    # flat node index (of valid nodes)
        for n in range(8):
            p = g0 + np.array([n >> 2, (n >> 1) & 1, n & 1])
            ok = (p < np.array(self.grid)).all(axis=1)
            q = np.where(ok[:, None], p, g0)                            # outside the grid: node 0's delays
            delays[:, n, :] = d[q[:, 0], q[:, 1], q[:, 2], :]
            self.valid[:, n] = ok
            self.node[:, n] = (q[:, 0] * ny + q[:, 1]) * nz + q[:, 2]
        self.first_node = self.node[:, 0]
        self.brick_of_group = brick_of_node[g0[:, 0], g0[:, 1], g0[:, 2]]
        rel = delays - self.lo[self.brick_of_group][:, None, :]
        dmin, dmax = rel.min(axis=1), rel.max(axis=1)
        self.dmin = dmin
        self.e0 = dmin - dmin % (2 if wide else 4)
        self.nq = np.maximum(2, (dmax - self.e0 + self.step + 3) // 4)
        self.off = rel - self.e0[:, None, :]
        fetched = np.maximum(self.nq, self.nq_min)
        touched = (self.e0 + self.step * (WAVE - 1) + 4 * fetched + 3) // 4
        self.need = np.zeros((self.nbricks, S), dtype=np.int64)
        np.maximum.at(self.need, self.brick_of_group, touched)
        self.over = np.zeros((self.nbricks, S), dtype=bool)
        np.logical_or.at(self.over, self.brick_of_group, self.nq > self.nq_max)
        self.quads, self.pairs = int(fetched.sum()), G * S
        self.blocks = row_blocks(S, block_rows)
        self.zero_slots = ((self.step * (WAVE - 1) + 4 * self.nq_min + 3) // 4 if wide else WAVE + self.nq_min)
        self.run = np.stack([self.need[:, r0:r0 + n].sum(axis=1) for r0, n in self.blocks], axis=1)
        self.zero = np.array([self.zero_slots if n & 1 else 0 for _, n in self.blocks])[None, :] + 0 * self.run
        self.overflow = np.stack([self.over[:, r0:r0 + n].any(axis=1) for r0, n in self.blocks], axis=1)

    def fits(self, plane):
        """per brick: every block of its rows fits `plane` bytes and no group overflows"""
        return (~self.overflow & ((self.run + self.zero) * 16 <= plane)).all(axis=1)

    def operands_x1000(self):
        """8-byte LDS operands fetched per add, x 1000, in the integer arithmetic of qm_engine_get"""
        return (self.quads * 4 * 1000) // (self.pairs * (8 * self.step))

    def top_offset(self):
        """the largest offset an add of a VALID node consumes"""
        return int((self.off * self.valid[:, :, None]).max())


def engine_layouts(tt, kind, brick=(8, 8, 8)):
    """What an engine builds for `tt` on workgroup shape `kind` (plane_bytes): (narrow layout or None, wide layout or
    None, direct bricks).  `brick` is the shape fixed with brick_x/_y/_z; the row-block forms have their own."""
    rows, shape = BLOCK_FORMS.get(kind, (0, brick))
    narrow = None if kind == "wide_rows" else Layout(tt, shape, False, rows)
    wide = Layout(tt, shape, True, rows) if kind in ("wide", "wide_rows") else None
    fit = np.ones((narrow or wide).nbricks, dtype=bool)
    if narrow is not None:                                   # (under the wide tiles: the 8-wave workgroup's planes)
        fit &= narrow.fits(plane_bytes("8" if kind == "wide" else kind))
    if wide is not None:
        fit &= wide.fits(plane_bytes(kind))
    return narrow, wide, int((~fit).sum())


# ------------------------------------------------------------------------------------------- the table designers
M_NARROW, M_WIDE = 20, 18       # the largest noise whose windows hold NQMAX quads: (20 + 4 + 3) // 4 = (18 + 6 + 3) // 4 = 6


def row_noise(rows, m):
    """m_r: two rows in three carry the full noise m (so that the top offset meets both row parities and every
    transition between large quad counts), the third cycles over 0..m in steps of 5 (low quad counts; 5 is coprime
    to m + 1 = 21 and 19)."""
    return np.array([m if r % 3 < 2 else (5 * (r // 3)) % (m + 1) for r in range(rows)])


def noise_table(grid, rows, m, seed, negatives=False, m_r=None):
    """tt[..., r] = c_r + U{0..m_r}, independently per node.  negatives: every fifth row has c_r = 0 and a few of its
    entries are -3 or INT32_MIN (they count as 0: inside the row's range, no brick is pushed to the direct kernel)."""
    rng = np.random.default_rng(seed)
    m_r = row_noise(rows, m) if m_r is None else np.asarray(m_r)
    c_r = rng.integers(0, 50, size=rows)
    if negatives:
        c_r[::5] = 0
    tt = (c_r + rng.integers(0, m_r + 1, size=tuple(grid) + (rows,))).astype(np.int32)
    if negatives:
        for r in range(0, rows, 5):
            pick = rng.integers(0, grid, size=(6, 3))
            tt[pick[:3, 0], pick[:3, 1], pick[:3, 2], r] = -3
            tt[pick[3:, 0], pick[3:, 1], pick[3:, 2], r] = INT32_MIN
    return tt


TableSpec = collections.namedtuple("TableSpec", "grid rows m seed negatives")
# name -> the bounded-noise tables of the GPU tests (all grids have odd dimensions: groups cut by the edge)
TABLES = collections.OrderedDict([
    ("n30", TableSpec((17, 15, 19), 30, M_NARROW, 4101, False)),     # <= 32 rows: two 4-wave workgroups per CU
    ("n29", TableSpec((15, 17, 13), 29, M_NARROW, 4102, False)),     # ... an odd row count (padding row)
    ("n41", TableSpec((15, 17, 19), 41, M_NARROW, 4103, False)),     # 33-64 rows: the 8-wave shape (far plane)
    ("n70", TableSpec((13, 11, 14), 70, M_NARROW, 4104, False)),     # > 64 rows: row blocks
    ("w30", TableSpec((17, 15, 19), 30, M_WIDE, 4105, False)),       # wide tiles
    ("w41", TableSpec((13, 11, 14), 41, M_WIDE, 4106, False)),       # wide tiles on row blocks
    ("neg29", TableSpec((17, 15, 13), 29, M_WIDE, 4107, True)),      # entries of -3 and INT32_MIN
])
# (table, workgroup shape) pairs the GPU tests launch: every one is held to the coverage conditions on the CPU
CASES = [("n30", "4"), ("n29", "4"), ("n30", "12"), ("n41", "8"), ("n29", "8"), ("n70", "rows8"), ("n70", "rows2"),
         ("n70", "rows4"), ("w30", "wide"), ("w41", "wide_rows"), ("neg29", "4"), ("neg29", "wide")]
BRICKS = {"12": (8, 8, 12), "wide": (8, 8, 16)}     # the brick shape the GPU tests fix (others: 8 x 8 x 8)


def table(name):
    s = TABLES[name]
    return noise_table(s.grid, s.rows, s.m, s.seed, s.negatives)


def case_layouts(name, kind):
    return engine_layouts(table(name), kind, BRICKS.get(kind, (8, 8, 8)))


def witness_targets(layout, tops, parities=(0, 1)):
    """One (flat node, row, node position, offset) per node position 0..7, offset of `tops` and row parity: a VALID
    node whose add in that row consumes the window register at that offset, in a group that fetches NQMAX quads;
    distinct nodes.  An event that arrives at such a node makes a sample whose maximum depends on that operand.
    (parities = None: one target per (position, offset), the parities alternating -- for tiles too short to hold 32
    events apart)"""
    out, used = [], set()
    for pos in range(8):
        for k, top in enumerate(tops):
            for parity in (parities if parities is not None else ((pos + k) % 2,)):
                hit = (layout.off[:, pos, :] == top) & layout.valid[:, pos, None] & (layout.nq == layout.nq_max)
                hit &= (np.arange(layout.S) % 2 == parity)[None, :]
                for g, r in np.argwhere(hit):
                    if int(layout.node[g, pos]) not in used:
                        used.add(int(layout.node[g, pos]))
                        out.append((int(layout.node[g, pos]), int(r), pos, top))
                        break
                else:
                    raise AssertionError(f"no cell at node position {pos}, offset {top}, row parity {parity}")
    return out


def witness_onsets(tt, targets, fsmp, lsmp, ns, t_lo, t_hi, seed):
    """Raw onsets (synth.synthetic_onsets) with one narrow event per target: target k's node sees all its rows
    arrive at sample t_k, the t_k spread evenly over [t_lo, t_hi).  Returns (onsets, [t_k])."""
    from quakemigrate_amd import synth

    S = tt.shape[-1]
    flat = np.maximum(tt.reshape(-1, S).astype(np.int64), 0)
    t_k = [t_lo + ((2 * k + 1) * (t_hi - t_lo)) // (2 * len(targets)) for k in range(len(targets))]
    arrivals = [fsmp + t + flat[node] for (node, _, _, _), t in zip(targets, t_k)]
    on = synth.synthetic_onsets(np.random.default_rng(seed), S, fsmp + ns + lsmp, arrivals, amplitude=8.0, sigma=0.8)
    return on, t_k


# ---- the boundary designer ---------------------------------------------------------------------------------------
def boundary_table(grid, brick, rows, kind, targets, seed, n_trim=20, m=8, k_max=60):
    """A table whose bricks' run + zero row hit requested slot totals on workgroup shape `kind` ('4', '8', 'wide').

    rows - n_trim rows carry noise U{0..m}; the last n_trim rows are flat (every node at c_r) and are then edited,
    per brick b of `targets` = {brick: (total, special)}:
      * special = 'nq7' / 'nq6': in the brick's first trim row ONE node of the brick's second group is raised to the
        offset that needs NQMAX + 1 / exactly NQMAX quads (one past the register window / its last register);
      * the brick's FIRST group is lifted by 4 k samples in the other trim rows -- its window then starts k slots
        later, the row needs k slots more -- until run + zero row = total.
    Bricks that are not named keep what the noise gives them (far below every limit).  The result is verified with
    the restatement before it is returned."""
    rng = np.random.default_rng(seed)
    m_r = np.array([m] * (rows - n_trim) + [0] * n_trim)
    tt = noise_table(grid, rows, m, rng.integers(1 << 30), m_r=m_r).astype(np.int64)
    wide = kind == "wide"
    c = constants()
    step = c["kShiftWideSpl"] if wide else 4
    probe = Layout(tt, brick, wide)
    bx, by, bz = probe.brick
    nby, nbz = -(-grid[1] // by), -(-grid[2] // bz)
    trim = list(range(rows - n_trim, rows))
    for b, (total, special) in targets.items():
        x0, y0, z0 = (b // (nby * nbz)) * bx, ((b // nbz) % nby) * by, (b % nbz) * bz
        if special:
            # nq = (offset + step + 3) // 4: the largest offset that NQMAX quads hold, or one more
            top = 4 * c["kShiftNqMax"] - step
            tt[x0, y0, z0 + 2, trim[0]] += top + (1 if special == "nq7" else 0)
    now = Layout(tt, brick, wide)
    for b, (total, special) in targets.items():
        x0, y0, z0 = (b // (nby * nbz)) * bx, ((b // nbz) % nby) * by, (b % nbz) * bz
        extra = total - int(now.run[b, 0] + now.zero[b, 0])
        assert 0 <= extra <= k_max * (n_trim - 1), (b, total, extra)
        for r in trim[1:]:
            k = min(extra, k_max)
            tt[x0:x0 + 2, y0:y0 + 2, z0:z0 + 2, r] += 4 * k
            extra -= k
    tt = tt.astype(np.int32)
    done = Layout(tt, brick, wide)
    for b, (total, special) in targets.items():
        assert int(done.run[b, 0] + done.zero[b, 0]) == total, (b, total, int(done.run[b, 0] + done.zero[b, 0]))
    return tt


BoundarySpec = collections.namedtuple("BoundarySpec", "grid brick rows kind seed")
# four bricks in a row along z (brick b = z / brick_z) -- even row counts: exact fit | one slot over | a group at
# NQMAX + 1 quads (far below the limit) | a group at exactly NQMAX.  Odd row counts: run alone fits and the padding
# row's zero window makes it an exact fit | ... pushes it one slot over | nq7 | nq6.
BOUNDARIES = collections.OrderedDict([
    ("b4", BoundarySpec((8, 8, 32), (8, 8, 8), 30, "4", 4201)),
    ("b4odd", BoundarySpec((8, 8, 32), (8, 8, 8), 31, "4", 4202)),
    ("b8", BoundarySpec((8, 8, 32), (8, 8, 8), 62, "8", 4203)),
    ("b8odd", BoundarySpec((8, 8, 32), (8, 8, 8), 63, "8", 4204)),
    ("bwide", BoundarySpec((8, 8, 64), (8, 8, 16), 46, "wide", 4205)),
    ("bwideodd", BoundarySpec((8, 8, 64), (8, 8, 16), 47, "wide", 4206)),
])
BOUNDARY_FIT = [True, False, False, True]           # per brick, every boundary table


def boundary(name):
    """(table, the slot limit of its workgroup shape)"""
    s = BOUNDARIES[name]
    limit = plane_bytes(s.kind) // 16
    targets = {0: (limit, None), 1: (limit + 1, None), 2: (limit - 100, "nq7"), 3: (limit - 100, "nq6")}
    return boundary_table(s.grid, s.brick, s.rows, s.kind, targets, s.seed), limit
