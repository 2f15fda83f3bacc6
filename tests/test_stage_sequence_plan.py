# -*- coding: utf-8 -*-
"""
What the stage-call plans of tests/stage_sequence_plan.py cover -- conditions on the plans, checked without a GPU
(tests/test_stage_sequences.py walks the same plans on one).  ``pytest -s`` prints a table per flavour.
"""

import itertools

import numpy as np
import pytest

import sequence_plan as sp
import stage_sequence_plan as ssp

FLAVOURS = list(ssp.FLAVOURS)
MARGIN = 0.85                       # the conditions also hold for the first 85 % of every plan


@pytest.fixture(scope="module")
def plans():
    return {f: ssp.make_plan(f) for f in FLAVOURS}


def test_plans_are_functions_of_flavour_seed_and_steps():
    for f in FLAVOURS:
        assert ssp.make_plan(f) == ssp.make_plan(f)
        assert len(ssp.make_plan(f)) == ssp.FLAVOURS[f][2]
        assert ssp.make_plan(f, seed=1, steps=120) != ssp.make_plan(f, seed=2, steps=120)
        short = ssp.make_plan(f, steps=ssp.POISON_STEPS)
        assert len(short) == ssp.POISON_STEPS
        assert short == ssp.make_plan(f)[:len(short)]         # (a shorter plan is a prefix: it replays)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_plan_prints_its_summary(plans, flavour):
    text = ssp.describe(flavour, plans[flavour])
    print("\n" + text)
    assert text.startswith(flavour) and text.endswith("unmet: nothing")


@pytest.mark.parametrize("fraction", [1.0, MARGIN], ids=["whole", "first-85-percent"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_condition_holds(plans, flavour, fraction):
    """``Tracker.unmet`` spelt out: the conditions one by one, on the counts of the finished plan."""
    plan = plans[flavour][:int(len(plans[flavour]) * fraction)]
    tracker = ssp.coverage(plan, flavour)
    c, kinds, reqs = tracker.c, list(ssp.KINDS), ssp.requests_of(flavour)
    assert tracker.unmet() == []
    # every request of every roster, every kind three times
    for k in kinds:
        assert all(c["requests"][r] >= 1 for r in reqs[k]), k
        assert c["kinds"][k] >= 3, k
    # every ordered pair of kinds adjacent
    missing = [p for p in itertools.product(kinds, kinds) if c["pairs"][p] < 1]
    assert not missing, missing
    # the buffer-sharing sets: every ordered pair three times, long in front of short and the other way round
    for p in ssp.sharing_pairs():
        assert c["pairs"][p] >= 3 and p in c["long_short"] and p in c["short_long"], p
    # both directions across every LDS limit, within the kind
    assert {(k, side) for k in ssp.LDS_KINDS for side in ("under", "over")} <= c["lds"]
    # refusals: a good call of the kind and one of another kind behind each, a release behind one
    refusals = ssp.refusals_of(flavour)
    assert len(refusals) == 8
    assert set(refusals) <= c["refusal_then_own"] and set(refusals) <= c["refusal_then_other"]
    assert c["refusal_then_release"]
    assert c["set_stream"] >= 6 and c["release"] >= 6
    assert {(k, s) for k in kinds for s in ("own", "torch")} <= c["on_stream"]
    if ssp.has_tables(flavour):
        m = tracker.model
        assert c["select_expectations_hold"]
        assert all(m.loads[t] >= 3 for t in ssp.TABLES), dict(m.loads)
        assert sum(m.returned.values()) >= 1 and sum(m.rebuilt.values()) >= 1
        assert c["load_between_stages"] >= 3
        assert c["pushes"] == 0
    else:
        assert c["pushes"] >= 8 and set(kinds) <= c["between_pushes"]
        assert not any(op.op in ("load", "select") for op in plan)


@pytest.mark.parametrize("flavour", ssp.POISON_FLAVOURS)
def test_the_poisoned_pool_plans_floor(flavour):
    """The shorter plan of the poisoned-pool children: every kind, every buffer-sharing pair, two refusals -- also
    in its first 85 %."""
    for fraction in (1.0, MARGIN):
        plan = ssp.make_plan(flavour, steps=int(ssp.POISON_STEPS * fraction))
        tracker = ssp.coverage(plan, flavour)
        assert tracker.unmet("poison") == []
        c = tracker.c
        assert all(c["kinds"][k] >= 1 for k in ssp.KINDS)
        assert all(c["pairs"][p] >= 1 for p in ssp.sharing_pairs())
        assert sum(c["refusals"].values()) >= 2


def test_the_conditions_can_fail():
    """``unmet`` names what a plan lacks: a plan cut short, and one with a kind's launches taken out."""
    plan = ssp.make_plan("engine")
    assert ssp.unmet(plan[:200], "engine")
    without = [op for op in plan if not (op.op == "launch" and op.arg.kind == "tt_sweep")]
    lacking = ssp.unmet(without, "engine")
    assert any("tt_sweep" in text for text in lacking) and all("tt_sweep" in text for text in lacking[:3])


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_flavour_draws_only_what_it_can_run(plans, flavour):
    """Every launch is a roster entry whose table, if it needs one, is resident when it runs; only with_stream pushes,
    and it has no table operations."""
    reqs = ssp.requests_of(flavour)
    model, table = sp.ParkingModel(), None if ssp.has_tables(flavour) else ssp.STREAM_TABLE
    pushes = []
    for op in plans[flavour]:
        assert op.op in ("load", "select", "launch", "set_stream", "release", "push")
        if op.op == "load":
            model.load(op.table)
            table = op.table
        elif op.op == "select":
            assert op.arg in ssp.CAPACITIES and model.select(op.table, op.arg) == op.expect
            table = op.table if op.expect else None
        elif op.op == "launch":
            assert op.arg in reqs[op.arg.kind] and op.arg.table in ("", table), op
        elif op.op == "push":
            pushes.append(op.arg)
    assert pushes == list(range(len(pushes))) and (len(pushes) > 0) == (flavour == "with_stream")
    if flavour == "with_stream":
        assert all(r.table in ("", ssp.STREAM_TABLE) for k in reqs for r in reqs[k])


def test_the_roster_has_what_each_family_offers():
    rosters = ssp.rosters()
    assert tuple(rosters) == ssp.KINDS and len(ssp.KINDS) == 17
    for kind, reqs in rosters.items():
        assert len({r.name for r in reqs}) == len(reqs) == len(set(reqs))
        good = [r for r in reqs if not r.refusal]
        short = [r.size for r in good if r.length == "short"]
        long_ = [r.size for r in good if r.length == "long"]
        assert short and long_ and min(long_) >= 2 * max(short), (kind, short, long_)
        for side in ("host_in", "host_out"):                    # both branches of stage_in / stage_host_out
            offered = {getattr(r, side) for r in good} - {None}
            assert offered in (set(), {True, False}) or kind in ssp.STACKING, (kind, side, offered)
    for kind in ssp.LDS_KINDS:
        assert {r.lds for r in rosters[kind]} >= {"under", "over"}, kind
    names = lambda kind: {r.name for r in rosters[kind]}        # noqa: E731
    assert {r.args[0] for r in rosters["onsets"]} == {"classic", "centred", "recursive"}
    assert {r.args[1:] for r in rosters["preprocess"]} >= {(True, 1), (False, 0)}
    assert {r.args[0] for r in rosters["pick_phases"]} == {0, 1}
    assert {r.args[0] for r in rosters["measure_amplitudes"]} == {"plain", "filter"}
    assert {r.args[0] for r in rosters["trigger_series"]} == {"static", "mad", "median_ratio"}
    assert {r.args[0] for r in rosters["scanmseed_encode"]} == {"int", "float"}
    assert {r.args[0] for r in rosters["scanmseed_decode"]} == {True, False}
    assert {r.host_in for r in rosters["tt_sweep"] if not r.refusal} == {True, False}
    assert {r.args[2] for r in rosters["tt_sections"]} == {True, False}
    assert names("exp_probe") == {"exp_correctly_rounded", "exp2f_max_error"}
    for kind in ssp.STACKING:
        assert {(r.table, r.args.ns) for r in rosters[kind]} == set(itertools.product(ssp.TABLES, ssp.SCAN_LENGTHS))
        assert all(r.args.kind == kind and r.args.table == r.table for r in rosters[kind])
    assert any(r.args.args[2] for r in rosters["migrate_host"])                 # an accumulate request
    refused = {(r.kind, r.name) for reqs in rosters.values() for r in reqs if r.refusal}
    assert refused == {("scanmseed_encode", "difference_of_2_29"), ("scanmseed_decode", "flipped_constant"),
                       ("tt_sections", "one_round"), ("tt_sweep", "node_outside_its_section"),
                       ("trigger_series", "too_many_events"), ("pick_phases", "window_outside_its_row"),
                       ("pick_phases", "over_the_limit"), ("measure_amplitudes", "window_outside_its_trace")}
    assert set(ssp.TABLES) <= set(sp.TABLES) and ssp.STREAM_TABLE in ssp.TABLES


def test_the_inputs_have_the_sizes_the_roster_states():
    """``build`` asserts that a request stages as many elements as its ``size`` says; the limits are the headers'."""
    lim = ssp.header_limits()
    assert lim["resample_lds_samples"] == 20480 and all(v > 4096 for v in lim.values())
    for kind, reqs in ssp.rosters().items():
        for r in reqs:
            d = ssp.build(r)
            assert d["elements"] == r.size
            if kind in ssp.STACKING:
                fsmp, lsmp = sp.pads(r.args)
                tt, _, _, t_samples = sp.table_case(r.table)
                assert fsmp + r.args.ns + lsmp == t_samples and lsmp >= int(tt.max())
    # the LDS limits' two sides
    by_name = {(r.kind, r.name): r for reqs in ssp.rosters().values() for r in reqs}
    assert by_name["resample", "dec_under"].size == lim["resample_lds_samples"] == by_name["resample", "dec_over"].size - 1
    d = ssp.build(by_name["measure_amplitudes", "windows_over"])
    assert d["recs"][1][2] - d["recs"][1][1] == lim["amp_lds_samples"] + 1
    d = ssp.build(by_name["measure_amplitudes", "windows_under"])
    assert d["recs"][1][2] - d["recs"][1][1] == lim["amp_lds_samples"]
    assert ssp.build(by_name["pick_phases", "at_the_limit"])["onsets"].shape[1] == lim["pick_lds_samples"]
    assert ssp.build(by_name["pick_phases", "over_the_limit"])["onsets"].shape[1] == lim["pick_lds_samples"] + 1
    under, over = by_name["tt_sections", "under"], by_name["tt_sections", "over"]
    assert under.args[0] * under.args[1] <= lim["tt_lds_nodes"] < over.args[0] * over.args[1]
    assert 67 * 45 <= lim["tt_lds_nodes"]                                       # (the forced request would fit)
    s = ssp.stream_setup()
    assert len(s["raws"]) == ssp.PUSH_STEPS >= 8 and s["rows"] == 11 and s["lsmp"] >= int(sp.table_case("c2_11")[0].max())
    assert np.bincount(ssp.STREAM_TRACE_ROW).min() >= 1 and len(ssp.STREAM_TRACE_ROW) == len(ssp.STREAM_RAW_RATE)
