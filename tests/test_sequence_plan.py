# -*- coding: utf-8 -*-
"""
What the call-sequence plans of tests/sequence_plan.py cover -- conditions on the plans, checked without a GPU
(tests/test_call_sequences.py walks the same plans on one).  ``pytest -s`` prints a table per flavour.
"""

import itertools

import numpy as np
import pytest

import sequence_plan as sp

FLAVOURS = list(sp.FLAVOURS)
MARGIN = 0.85                       # the conditions also hold for the first 85 % of every plan


@pytest.fixture(scope="module")
def plans():
    return {f: sp.make_plan(f) for f in FLAVOURS}


def test_plans_are_functions_of_flavour_and_seed():
    for f in FLAVOURS:
        assert sp.make_plan(f) == sp.make_plan(f)
        assert sp.make_plan(f, seed=1) != sp.make_plan(f, seed=2)
        short = sp.make_plan(f, steps=sp.POISON_STEPS)
        assert short == sp.make_plan(f)[:len(short)]          # (a shorter plan is a prefix: it replays)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_plan_prints_its_summary(plans, flavour):
    text = sp.describe(flavour, plans[flavour])
    print("\n" + text)
    assert text.startswith(flavour)


@pytest.mark.parametrize("fraction", [1.0, MARGIN], ids=["whole", "first-85-percent"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_ordered_pair_of_launch_kinds_is_adjacent_on_one_table(plans, flavour, fraction):
    plan = plans[flavour]
    cov = sp.coverage(plan[:int(len(plan) * fraction)])
    kinds = sp.kinds_of(flavour)
    missing = [p for p in itertools.product(kinds, kinds) if cov["pairs"][p] < 1]
    assert not missing, missing
    assert set(cov["kinds"]) == set(kinds)


@pytest.mark.parametrize("fraction", [1.0, MARGIN], ids=["whole", "first-85-percent"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_scan_lengths_change_in_both_directions(plans, flavour, fraction):
    plan = plans[flavour]
    cov = sp.coverage(plan[:int(len(plan) * fraction)])
    assert cov["longer_then_shorter"] >= 5 and cov["shorter_then_longer"] >= 5
    assert cov["longest_to_one"] >= 1                     # from the longest scan to a single sample
    assert cov["marginal_many_to_single"] >= 1            # from a marginal map over many tiles to one over one
    if fraction == 1.0:                                   # (every tile boundary, in every flavour's walk)
        assert cov["lengths"] >= set(sp.SCAN_LENGTHS), sorted(set(sp.SCAN_LENGTHS) - cov["lengths"])


@pytest.mark.parametrize("fraction", [1.0, MARGIN], ids=["whole", "first-85-percent"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_table_is_loaded_parked_brought_back_evicted_and_rebuilt(plans, flavour, fraction):
    plan = plans[flavour]
    cov = sp.coverage(plan[:int(len(plan) * fraction)])
    assert cov["select_expectations_hold"]
    for t in sp.TABLES:
        assert cov["loads"].get(t, 0) >= 3, (t, cov["loads"])
        assert cov["returned"].get(t, 0) >= 1, (t, cov["returned"])
        assert cov["rebuilt"].get(t, 0) >= 1, (t, cov["rebuilt"])
    assert set(cov["capacities"]) == set(sp.CAPACITIES)
    # two tables of one shape and other delays, loaded back to back
    assert cov["back_to_back"] & sp.mirror_pairs()
    if not sp.is_group(flavour):
        assert cov["set_stream"] >= 2
    assert cov["release"] >= 1


def test_find_max_coa_at_the_previous_sample_count_in_the_tie_rule_flavour(plans):
    for f in FLAVOURS:
        assert sp.coverage(plans[f])["fmc_equal_ns"] >= 1, f
    assert sp.coverage(plans["tie_rule"][:int(len(plans["tie_rule"]) * MARGIN)])["fmc_equal_ns"] >= 2
    short = sp.make_plan("tie_rule", steps=sp.POISON_STEPS)
    assert sp.coverage(short)["fmc_equal_ns"] >= 1


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_flavour_draws_only_what_it_can_run(plans, flavour):
    """No request is skipped on the GPU: a group's plan holds a group's calls only, every launch is a roster entry
    of the table that is resident when it runs."""
    kinds = set(sp.kinds_of(flavour))
    for op in plans[flavour]:
        assert op.op in ("load", "select", "launch", "set_stream", "release")
        if sp.is_group(flavour):
            assert op.op != "set_stream"
        if op.op == "launch":
            assert op.arg.kind in kinds and op.arg in sp.roster(op.table)[op.arg.kind]
        if op.op == "select":
            assert op.arg in sp.CAPACITIES


def test_the_roster_respects_the_tables_and_the_scan_lengths():
    shapes = {}
    used = set()
    for t, spec in sp.TABLES.items():
        tt, onsets, fsmp0, t_samples = sp.table_case(t)
        assert tt.dtype == np.int32 and tt.flags["C_CONTIGUOUS"] and tt.shape == spec.grid + (spec.rows,)
        assert 2000 <= tt[..., 0].size <= 12000           # (small: the oracle costs seconds)
        assert onsets.shape == (spec.rows, t_samples)
        shapes[t] = tt
        for kind, reqs in sp.roster(t).items():
            assert len(set(reqs)) == len(reqs)
            for r in reqs:
                assert r.kind == kind and r.ns in sp.SCAN_LENGTHS and r.fsmp_off in sp.FSMP_OFFSETS
                used.add(r.ns)
                if kind == "find_max_coa":
                    continue
                fsmp, lsmp = sp.pads(r)
                assert fsmp + r.ns + lsmp == t_samples and lsmp >= int(tt.max()), (r, lsmp, int(tt.max()))
                if kind == "marginal_map":
                    assert 0 <= r.args[0] < r.args[1] <= r.ns
                if kind == "detect_batch":
                    assert r.args[0] in (1, 2, 5)
        if spec.mirror_of:
            assert tt.shape == shapes[spec.mirror_of].shape and not np.array_equal(tt, shapes[spec.mirror_of])
    assert used == set(sp.SCAN_LENGTHS)
    assert {r.args[0] for t in sp.TABLES for r in sp.roster(t)["detect_batch"]} == {1, 2, 5}
    assert sorted({spec.rows <= 32 for spec in sp.TABLES.values()}) == [False, True]
    assert any(32 < spec.rows <= 64 for spec in sp.TABLES.values()) and any(spec.rows > 64 for spec in sp.TABLES.values())


def test_parking_model_small_cases():
    m = sp.ParkingModel()
    assert m.select("a", 4) is False
    m.load("a")
    assert m.select("a", 4) is True and m.returned["a"] == 0          # (the resident table: nothing moves)
    assert m.select("b", 4) is False
    m.load("b")
    assert m.select("a", 4) is True and m.returned["a"] == 1 and m.parked() == {"b"}
    m.load("c")                                                         # a foreign load: no key
    assert m.select("b", 1) is True and m.table == "b" and m.parked() == set()    # (the un-keyed table is dropped)
    assert "c" in m.lost_small
    assert m.select("a", 0) is False and "b" in m.lost_small           # nothing may be parked
    m.load("a")
    assert m.select("b", 1) is False
    m.load("b")
    assert m.rebuilt["b"] == 1 and m.parked() == {"a"}
    assert m.select("c", 1) is False                                    # a cache of one: "a" is evicted
    m.load("c")
    assert m.parked() == {"b"} and "a" in m.lost_small and m.rebuilt["c"] == 1
