# -*- coding: utf-8 -*-
"""
Seeded call sequences for ONE long-lived engine (tests/test_call_sequences.py walks them on the GPU;
tests/test_sequence_plan.py checks on the CPU that they cover what they are meant to cover).

Pure Python: a roster of small tables, a fixed roster of *requests* per table (one call with all of its
arguments), a model of the engine's table parking (qm_engine_table_select / qm_engine_load_lut, csrc/qm_tables.hip)
and a generator that turns ``(flavour, seed, steps)`` into a list of operations.  The generator is a random walk
that is steered towards what has not occurred yet -- an ordered pair of launch kinds, a table that was not yet
brought back from parking -- so that a plan of a hundred-odd steps meets the coverage conditions with margin; the
conditions themselves are computed from the finished plan alone (:func:`coverage`).
"""

import collections
import copy
import random

import numpy as np

from quakemigrate_amd import synth

# ---------------------------------------------------------------------------------------------- the roster
KINDS = ("detect", "detect_batch", "detect_partial", "migrate_host", "migrate_device", "marginal_map",
         "find_max_coa")
GROUP_KINDS = ("detect", "migrate_host", "marginal_map", "find_max_coa")      # what an EngineGroup has

# every tile boundary of the engine: 64-sample wavefront rows, the 192-sample tail tiles, 256-sample tiles,
# 384-sample wide tiles (4 x 384 = 1536: where the automatic choice takes them) and five wide tiles
SCAN_LENGTHS = (1, 63, 192, 193, 256, 257, 401, 625, 777, 1536, 1537, 1920)
LONGEST = max(SCAN_LENGTHS)
FSMP_OFFSETS = (0, 41)              # added to the recipe's pre-pad (the post-pad keeps >= 59 samples of slack)
BATCH_SHIFT = 7                     # step k of a detect_batch: the onsets rolled by 7 k samples

TableSpec = collections.namedtuple("TableSpec", "recipe grid rows step mirror_of lengths volume_lengths")

# name -> recipe of synth.make_case, grid, rows, onset step, the table it mirrors (same shape, other delays), the
# scan lengths its series requests use, the lengths of its volume-writing requests (ascending)
TABLES = collections.OrderedDict([
    # coherent, <= 32 rows: shift-reuse, two 4-wave workgroups per CU
    ("c3_30", TableSpec("C3", (24, 22, 18), 30, 1, None, (1, 193, 256, 625, 1536, 1920), (1, 193, 257, 401))),
    # coherent, 33-64 rows: shift-reuse, one 8-wave workgroup per CU
    ("c3_44", TableSpec("C3", (20, 21, 22), 44, 2, None, (1, 63, 257, 401, 1537, 1920), (1, 192, 257, 401))),
    # coherent, > 64 rows: shift-reuse on row blocks
    ("c3_70", TableSpec("C3", (16, 16, 12), 70, 2, None, (1, 192, 257, 777, 1920), (1, 193, 256, 777))),
    # incoherent (delays of hundreds of samples across a brick): the exact-row-count kernels and, for volumes of
    # scans that fill whole 256-sample tiles (401, 777), the paired kernel
    ("c2_11", TableSpec("C2", (21, 18, 23), 11, 1, None, (1, 63, 193, 401, 777, 1537), (1, 63, 401, 777))),
    # the first table mirrored in x: the shape of an earlier entry, other delays
    ("c3_30m", TableSpec("C3", (24, 22, 18), 30, 3, "c3_30", (1, 256, 625, 1920), (1, 193, 257, 401))),
])
FMC_NODES = 2000                    # find_max_coa: host volumes of this many nodes ...
FMC_LENGTHS = (1, 63, 193, 257, 401, 625)      # ... and these sample counts (scan lengths of the rosters above)

# kind, table ("" for find_max_coa: it needs none), pre-pad offset, scanned samples, the kind's own arguments:
#   detect_batch (K,) | migrate_host (scan_out, several_chunks, accumulate) | migrate_device (scan_out,) |
#   marginal_map (first_sample, end_sample)
Request = collections.namedtuple("Request", "kind table fsmp_off ns args")
# op: "load" (table) | "select" (table, capacity, expect: is it resident?) | "launch" (table, request) |
#     "set_stream" ("torch" / "own") | "release"
Op = collections.namedtuple("Op", "op table arg expect")
Op.__new__.__defaults__ = (None, None, None)

FLAVOURS = collections.OrderedDict([
    # name -> (class, constructor arguments, configuration, steps of the walk)
    ("engine", ("Engine", 0, {}, 160)),
    ("tie_rule", ("Engine", 0, {"tie_rule": 1}, 160)),
    ("shift_wide", ("Engine", 0, {"shift_wide": 1}, 160)),
    ("screen", ("Engine", 0, {"screen": 1}, 160)),
    ("group_1", ("EngineGroup", [0], {}, 150)),
    ("group_3", ("EngineGroup", [0, 0, 0], {}, 150)),
])
SEEDS = {name: 20261016 for name in FLAVOURS}
POISON_STEPS = 50                   # the shorter plan of the poisoned-pool children
CAPACITIES = (0, 1, 4)


def is_group(flavour):
    return FLAVOURS[flavour][0] == "EngineGroup"


def kinds_of(flavour):
    return GROUP_KINDS if is_group(flavour) else KINDS


def roster(table):
    """The fixed list of requests on ``table``, by kind (the same for every flavour; a group draws its kinds)."""
    spec = TABLES[table]
    L, V = spec.lengths, spec.volume_lengths
    mid, mid2 = L[len(L) // 2], L[len(L) // 2 - 1]
    short_mid = [n for n in L if 1 < n <= 401][-1]
    out = collections.OrderedDict()
    out["detect"] = [Request("detect", table, 0, n, ()) for n in L] + [Request("detect", table, 41, mid, ())]
    out["detect_batch"] = [Request("detect_batch", table, 0, 1, (2,)),
                           Request("detect_batch", table, 0, mid2, (1,)),
                           Request("detect_batch", table, 41, mid, (2,)),
                           Request("detect_batch", table, 0, short_mid, (5,)),
                           Request("detect_batch", table, 0, L[-1], (2,))]
    out["detect_partial"] = [Request("detect_partial", table, 0, n, ()) for n in (1, mid, L[-1])]
    out["migrate_host"] = [Request("migrate_host", table, 0, V[0], (True, False, False)),
                           Request("migrate_host", table, 0, V[-1], (True, True, False)),
                           Request("migrate_host", table, 41, V[2], (False, False, False)),
                           Request("migrate_host", table, 0, V[-1], (False, True, True))]
    out["migrate_device"] = [Request("migrate_device", table, 0, V[0], (False,)),
                             Request("migrate_device", table, 0, V[1], (True,)),
                             Request("migrate_device", table, 41, V[2], (True,))]
    out["marginal_map"] = [Request("marginal_map", table, 0, 1, (0, 1)),
                           Request("marginal_map", table, 0, L[1], (0, L[1])),              # a single tile
                           Request("marginal_map", table, 41, mid, (10, mid // 2)),
                           Request("marginal_map", table, 0, L[-1], (3, L[-1] - 2))]        # many tiles
    out["find_max_coa"] = [Request("find_max_coa", "", 0, n, ()) for n in FMC_LENGTHS]
    return out


def single_tile_marginal(req):
    return req.kind == "marginal_map" and req.ns <= 256


def many_tile_marginal(req):
    return req.kind == "marginal_map" and req.ns >= 1536


# ---------------------------------------------------------------------------------------------- the inputs
_CASES = {}


def table_case(table):
    """(traveltimes, raw onsets (rows, T), fsmp0, T) of a roster table; the onsets hold the longest scan."""
    if table not in _CASES:
        spec = TABLES[table]
        case = synth.make_case(spec.recipe, step=spec.step, grid=spec.grid, rows=spec.rows, n_samples=LONGEST)
        tt = case.traveltimes
        if spec.mirror_of is not None:
            tt = np.ascontiguousarray(tt[::-1])
        _CASES[table] = (tt, np.ascontiguousarray(case.onsets), int(case.fsmp), int(case.onsets.shape[1]))
    return _CASES[table]


def pads(req):
    """(fsmp, lsmp) of a request on its table: lsmp = T - fsmp - ns."""
    _, _, fsmp0, t_samples = table_case(req.table)
    fsmp = fsmp0 + req.fsmp_off
    return fsmp, t_samples - fsmp - req.ns


def fmc_volume(n_samples):
    """The host volume (FMC_NODES, n_samples) of a find_max_coa request: positive, no two equal values."""
    rng = np.random.default_rng(977 + n_samples)
    return np.ascontiguousarray(rng.lognormal(0.0, 0.7, size=(FMC_NODES, n_samples)))


def accumulate_prefill(n_nodes, ns):
    """What an ``accumulate=True`` volume holds before the call (exact binary fractions)."""
    return np.ascontiguousarray(0.25 + 0.125 * (np.arange(n_nodes * ns, dtype=np.float64) % 7).reshape(n_nodes, ns))


# ---------------------------------------------------------------------------------------------- parking model
class ParkingModel:
    """What qm_engine_table_select / qm_engine_load_lut do to the resident and the parked tables (csrc/qm_tables.hip),
    with table NAMES for keys and contents.  ``lost_small``: tables whose state a select with capacity 0 or 1 threw
    away (evicted from their slot, or dropped because nothing may be parked)."""

    def __init__(self):
        self.have = False
        self.keyed = False
        self.key = None
        self.table = None
        self.slots = []                 # dicts(used, key, stamp, table)
        self.clock = 0
        self.loads = collections.Counter()
        self.returned = collections.Counter()       # brought back from parking
        self.rebuilt = collections.Counter()        # loaded again after lost_small
        self.lost_small = set()
        self.back_to_back = set()       # (a, b): b loaded on top of / right after a with no other table between
        self.last_loaded = None

    def _lose(self, table, capacity):
        if table is not None and capacity in (0, 1):
            self.lost_small.add(table)

    def select(self, key, capacity):
        if self.keyed and self.key == key and self.have:
            return True
        park = self.have and self.keyed and capacity > 0
        for sl in self.slots:
            if not sl["used"] or sl["key"] != key:
                continue
            incoming = sl["table"]
            if park:
                self.clock += 1
                sl.update(key=self.key, table=self.table, stamp=self.clock)
            else:
                if self.have:
                    self._lose(self.table, capacity)
                sl.update(used=False, table=None)
            self.table, self.have, self.key, self.keyed = incoming, True, key, True
            self.returned[incoming] += 1
            self.last_loaded = None     # (another table in between: the next load is not "back to back")
            return True
        if park:
            slot = next((sl for sl in self.slots if not sl["used"]), None)
            if slot is None and len(self.slots) < capacity:
                slot = {"used": False}
                self.slots.append(slot)
            if slot is None:
                slot = min(self.slots, key=lambda sl: sl["stamp"])
                self._lose(slot["table"], capacity)
            self.clock += 1
            slot.update(used=True, key=self.key, table=self.table, stamp=self.clock)
        elif self.have:
            self._lose(self.table, capacity)
        self.have, self.table, self.key, self.keyed = False, None, key, True
        return False

    def load(self, table):
        if self.have:
            self.keyed = False          # (a load on top of a resident table does not inherit its key)
        if self.last_loaded is not None and self.last_loaded != table:
            self.back_to_back.add((self.last_loaded, table))
        self.table, self.have = table, True
        self.loads[table] += 1
        if table in self.lost_small:
            self.lost_small.discard(table)
            self.rebuilt[table] += 1
        self.last_loaded = table

    def parked(self):
        return {sl["key"] for sl in self.slots if sl["used"]}


# ---------------------------------------------------------------------------------------------- the generator
def make_plan(flavour, seed=None, steps=None):
    """The list of :class:`Op` of one walk.  A "select" whose table is not resident is followed by its "load"."""
    seed = SEEDS[flavour] if seed is None else seed
    steps = FLAVOURS[flavour][3] if steps is None else steps
    rng = random.Random(f"{flavour}/{seed}")
    kinds = kinds_of(flavour)
    group = is_group(flavour)
    rosters = {t: roster(t) for t in TABLES}
    model = ParkingModel()
    plan = []
    pairs = set()
    state = {"prev": None, "drop": False, "marg": False, "fmc_equal": False, "stream": "own", "lengths": set()}

    def do_select(target, cap):
        resident = model.select(target, cap)
        plan.append(Op("select", target, cap, resident))
        if not resident:
            plan.append(Op("load", target))
            model.load(target)

    def apply(m, op):
        """One candidate table operation on a model: ("load", t) or ("select", t, capacity)."""
        if op[0] == "load":
            m.load(op[1])
            return None
        resident = m.select(op[1], op[2])
        if not resident:
            m.load(op[1])
        return resident

    def open_ends(m):
        """What a model still lacks of the table conditions, less half a point for every step towards one (a
        parked table that has yet to come back, a thrown-away table that has yet to be rebuilt)."""
        lack = sum(max(0, 3 - m.loads[t]) + (m.returned[t] == 0) + (m.rebuilt[t] == 0) for t in TABLES)
        lack += not (m.back_to_back & mirror_pairs())
        ahead = sum(m.returned[t] == 0 for t in m.parked()) + sum(m.rebuilt[t] == 0 for t in m.lost_small)
        return lack - 0.5 * ahead

    def switch_table():
        cands = []
        for t in TABLES:
            if t == model.table:
                continue
            cands.append(("load", t))
            cands += [("select", t, cap) for cap in CAPACITIES]
        if model.table is None:
            cands = [c for c in cands if c[0] == "select"]
        choice = None
        if open_ends(model) > 0:                                # the operation that closes most of what is open
            scored = []
            for c in cands:
                m = copy.deepcopy(model)
                apply(m, c)
                scored.append((open_ends(m), c))
            best = min(sc for sc, _ in scored)
            choice = rng.choice([c for sc, c in scored if sc == best])
        if choice is None:
            choice = rng.choice(cands)
        if choice[0] == "load":
            plan.append(Op("load", choice[1]))
            model.load(choice[1])
        else:
            do_select(choice[1], choice[2])

    def launch():
        prev = state["prev"]
        kind = None
        # towards what has not occurred: a missing pair from the previous kind, else the kind most pairs still start at
        open_from = {k: sum((k, b) not in pairs for b in kinds) for k in kinds}
        if prev is not None:
            missing = [k for k in kinds if (prev.kind, k) not in pairs]
            if missing and rng.random() < 0.9:
                most = max(open_from[k] for k in missing)
                kind = rng.choice([k for k in missing if open_from[k] == most])
        if kind is None and max(open_from.values()) > 0 and rng.random() < 0.8:
            kind = rng.choice([k for k in kinds if open_from[k] == max(open_from.values())])
        if kind is None:                # ... else a kind that has a scan length the walk has not seen
            unseen = [k for k in kinds if any(r.ns not in state["lengths"] for r in rosters[model.table][k])]
            kind = rng.choice(unseen if unseen and rng.random() < 0.7 else kinds)
        cands = rosters[model.table][kind]
        req = None
        if prev is not None:
            if prev.ns == LONGEST and not state["drop"]:
                req = next((r for r in cands if r.ns == 1), None)
            if req is None and many_tile_marginal(prev) and not state["marg"]:
                kind, cands = "marginal_map", rosters[model.table]["marginal_map"]
                req = next(r for r in cands if single_tile_marginal(r) and r.ns > 1)
            if req is None and kind == "find_max_coa" and prev.ns in FMC_LENGTHS and rng.random() < 0.7:
                req = next(r for r in cands if r.ns == prev.ns)
        if req is None and prev is not None and not state["drop"] and rng.random() < 0.3:
            longest = [r for r in cands if r.ns == LONGEST]         # (set the drop up)
            req = rng.choice(longest) if longest else None
        if req is None and kind == "marginal_map" and not state["marg"] and rng.random() < 0.5:
            req = next((r for r in cands if many_tile_marginal(r)), None)        # (... and this one)
        if req is None and rng.random() < 0.8:                 # a scan length the walk has not seen
            fresh = [r for r in cands if r.ns not in state["lengths"]]
            req = rng.choice(fresh) if fresh else None
        if req is None:
            req = rng.choice(cands)
        state["lengths"].add(req.ns)
        plan.append(Op("launch", model.table, req))
        if prev is not None:
            pairs.add((prev.kind, req.kind))
            state["drop"] |= prev.ns == LONGEST and req.ns == 1
            state["marg"] |= many_tile_marginal(prev) and single_tile_marginal(req)
        state["prev"] = req

    burst = 0
    while len(plan) < steps:
        u = rng.random()
        if model.table is None or burst <= 0:
            switch_table()
            state["prev"] = None        # (pairs count on one table)
            burst = rng.randint(2, 5)
        elif u < 0.05 and not group:
            state["stream"] = "torch" if state["stream"] == "own" else "own"
            plan.append(Op("set_stream", model.table, state["stream"]))
        elif u < 0.09:
            plan.append(Op("release", model.table))
        else:
            launch()
            burst -= 1
    return plan


# ---------------------------------------------------------------------------------------------- what a plan covers
def coverage(plan):
    """Counts over a finished plan (from the plan alone: the parking model is run again over its table operations).
    Two launches are "adjacent" when no table operation lies between them; a ``set_stream`` or a pool release may."""
    model = ParkingModel()
    cov = {"steps": len(plan), "launches": 0, "requests": set(), "pairs": collections.Counter(),
           "longer_then_shorter": 0, "shorter_then_longer": 0, "longest_to_one": 0, "marginal_many_to_single": 0,
           "fmc_equal_ns": 0, "kinds": collections.Counter(), "lengths": set(), "capacities": collections.Counter(),
           "set_stream": 0, "release": 0, "select_expectations_hold": True}
    prev = None
    for op in plan:
        if op.op == "load":
            model.load(op.table)
            prev = None
        elif op.op == "select":
            cov["capacities"][op.arg] += 1
            if model.select(op.table, op.arg) != op.expect:
                cov["select_expectations_hold"] = False
            prev = None
        elif op.op == "set_stream":
            cov["set_stream"] += 1
        elif op.op == "release":
            cov["release"] += 1
        else:
            req = op.arg
            assert op.table == model.table and req.table in ("", model.table), op
            cov["launches"] += 1
            cov["requests"].add(req)
            cov["kinds"][req.kind] += 1
            cov["lengths"].add(req.ns)
            if prev is not None:
                cov["pairs"][(prev.kind, req.kind)] += 1
                cov["longer_then_shorter"] += prev.ns > req.ns
                cov["shorter_then_longer"] += prev.ns < req.ns
                cov["longest_to_one"] += prev.ns == LONGEST and req.ns == 1
                cov["marginal_many_to_single"] += many_tile_marginal(prev) and single_tile_marginal(req)
                cov["fmc_equal_ns"] += req.kind == "find_max_coa" and prev.ns == req.ns
            prev = req
    cov["loads"] = dict(model.loads)
    cov["returned"] = dict(model.returned)
    cov["rebuilt"] = dict(model.rebuilt)
    cov["back_to_back"] = set(model.back_to_back)
    return cov


def describe(flavour, plan=None):
    """A short table of what a flavour's plan holds (printed by tests/test_sequence_plan.py -s and by
    ``python tests/sequence_plan.py``)."""
    plan = make_plan(flavour) if plan is None else plan
    cov = coverage(plan)
    kinds = kinds_of(flavour)
    lines = [f"{flavour}: {cov['steps']} steps, {cov['launches']} launches, {len(cov['requests'])} distinct requests, "
             f"{cov['set_stream']} set_stream, {cov['release']} release, select capacities {dict(cov['capacities'])}",
             "  adjacent pairs on one table (row: first, column: second)",
             "  " + " " * 15 + " ".join(f"{k[:7]:>7}" for k in kinds)]
    for a in kinds:
        lines.append(f"  {a:>15}" + " ".join(f"{cov['pairs'][(a, b)]:>7}" for b in kinds))
    lines.append("  table: loads / brought back from parking / rebuilt after a cache of 0 or 1 threw it away")
    for t in TABLES:
        lines.append(f"  {t:>15}: {cov['loads'].get(t, 0)} / {cov['returned'].get(t, 0)} / {cov['rebuilt'].get(t, 0)}")
    lines.append(f"  longer->shorter {cov['longer_then_shorter']}, shorter->longer {cov['shorter_then_longer']}, "
                 f"{LONGEST}->1 {cov['longest_to_one']}, marginal many->single tile {cov['marginal_many_to_single']}, "
                 f"find_max_coa at the previous ns {cov['fmc_equal_ns']}, same shape back to back "
                 f"{sorted(cov['back_to_back'] & mirror_pairs())}")
    return "\n".join(lines)


def mirror_pairs():
    out = set()
    for t, spec in TABLES.items():
        if spec.mirror_of:
            out |= {(spec.mirror_of, t), (t, spec.mirror_of)}
    return out


def format_ops(ops):
    """One line per operation, for a failure message: the prefix that replays it."""
    out = []
    for i, op in enumerate(ops):
        if op.op == "launch":
            r = op.arg
            out.append(f"{i}: {r.kind}(table={op.table}, fsmp+{r.fsmp_off}, ns={r.ns}, args={r.args})")
        elif op.op == "select":
            out.append(f"{i}: select_table({op.table}, capacity={op.arg}) -> resident={op.expect}")
        else:
            out.append(f"{i}: {op.op}({op.table if op.op == 'load' else op.arg})")
    return "\n".join(out)


if __name__ == "__main__":
    for name in FLAVOURS:
        print(describe(name))
