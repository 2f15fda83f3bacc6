# -*- coding: utf-8 -*-
"""
The stacking launch's plan (``StackPlan``, csrc/qm_engine.hpp: plan_stack decides, issue_stack launches, ``e->last``
describes) against the launches of the commit before it existed.

tests/golden/stack_launches_parent.json was written by tools/record_stack_launches.py from that commit's library:
for every engine of a fixed matrix -- the five roster tables of tests/sequence_plan.py with their whole roster under
fourteen configurations, a table whose launches split between the LDS and the direct kernel, a three-part engine
group -- the read-outs after every request and a digest of everything the requests wrote.  The replay asserts
equality on every entry: the same kernel family, samples per lane, tiles, loop flavour and rows of maxima, and --
through the bits of the series, which the order of the sum over the node groups fixes -- the same group counts.

The automatic group counts follow the device's CU count; on a device with another count than the recorded one the
bits legitimately differ and the tests skip, saying so.
"""

import json
import sys

import pytest

from conftest import ROOT                          # (first: it puts the repository root on sys.path)

sys.path.insert(0, str(ROOT / "tools"))
import record_stack_launches as rec                 # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((ROOT / "tests" / "golden" / "stack_launches_parent.json").read_text())
TABLES = sorted({name.split("|")[0] + ("|group" if name.endswith("group_3") else "") for name in GOLDEN["entries"]})


@pytest.fixture(scope="module")
def lib():
    from quakemigrate_amd.core import lib as _lib

    assert _lib.qmlib.qm_device_count() >= 1, "no HIP device visible"
    cu = rec.n_cu(_lib)
    if cu != GOLDEN["n_cu"]:
        pytest.skip(f"recorded on a device of {GOLDEN['n_cu']} CUs, this one has {cu}: the automatic group counts, "
                    "and with them the bits of the sums over the nodes, differ")
    return _lib


def test_the_record_holds_the_whole_matrix():
    assert [name for name, _, _, _ in rec.matrix()] == list(GOLDEN["entries"])
    assert GOLDEN["readouts"][:-1] == list(rec.READOUTS)


@pytest.mark.parametrize("table", TABLES)
def test_launches_are_the_parents(lib, table):
    """Every engine of the matrix on ``table``: read-outs after every request and the digest of every kind's outputs
    equal the record's (the read-outs as the library gives them: ``last_launch_rule`` of the recorder is off)."""
    ran = 0
    for name, tab, cfg, group in rec.matrix():
        if tab + ("|group" if group else "") != table:
            continue
        got = json.loads(json.dumps(rec.walk(lib, tab, cfg, group)))
        want = GOLDEN["entries"][name]
        assert list(got) == list(want), name
        for kind in want:
            assert got[kind] == want[kind], f"{name}, {kind}:\n now      {got[kind]}\n recorded {want[kind]}"
        ran += 1
    assert ran >= 1
