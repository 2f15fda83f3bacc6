# -*- coding: utf-8 -*-
"""
Generate tests/golden/reference_binding.json from the REFERENCE itself (authoring container only).

What the reference's own binding, quakemigrate/core/lib.py, asks of the C library it loads: the
symbols it binds, the argtypes it sets on each (as data: ctypes scalar names, ndpointer dtypes
and flags) and, for the three STA/LTA wrappers, the header they pass and the value the output
buffer holds when the C function receives it.  Recorded by importing that file unmodified (the
stand-ins of make_golden.py for its package imports) against a library object that only records
what is set on it and what it is called with; nothing of the reference is executed on real data
and no reference source travels.  tests/test_host.py binds the drop-in library by this record.

Run:  python oracle/make_golden_binding.py       (writes tests/golden/reference_binding.json)
"""

import ctypes
import importlib.util
import json
import pathlib
import sys
import types

import numpy as np

from make_golden import REF  # where the reference lies, as for the other fixtures

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "reference_binding.json"
UNSET = object()


class RecordingSymbol:
    def __init__(self):
        self.argtypes = UNSET
        self.restype = UNSET
        self.calls = []

    def __call__(self, *args):
        self.calls.append([np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args])
        return 0


class RecordingLibrary:
    def __init__(self):
        self.symbols = {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self.symbols.setdefault(name, RecordingSymbol())


def describe_dtype(dt):
    if dt.names is None:
        return dt.str
    return {"names": list(dt.names), "formats": [dt.fields[n][0].str for n in dt.names],
            "offsets": [dt.fields[n][1] for n in dt.names], "itemsize": dt.itemsize}


def describe_type(t):
    if t is None:
        return None
    if isinstance(t, type) and issubclass(t, np.ctypeslib._ndptr):
        return {"ndpointer": {"dtype": describe_dtype(t._dtype_), "flags": int(t._flags_),
                              "ndim": t._ndim_, "shape": t._shape_}}
    assert isinstance(t, type) and issubclass(t, ctypes._SimpleCData), t
    return {"ctype": t.__name__, "size": ctypes.sizeof(t)}


def load_reference_binding(qmlib):
    qm = types.ModuleType("quakemigrate")
    qm.__path__ = []
    core = types.ModuleType("quakemigrate.core")
    core.__path__ = []
    util = types.ModuleType("quakemigrate.util")
    util.timeit = lambda *a, **k: (lambda f: f)
    ln = types.ModuleType("quakemigrate.core.libnames")
    ln._load_cdll = lambda name: qmlib
    qm.util = util
    sys.modules.update({"quakemigrate": qm, "quakemigrate.core": core, "quakemigrate.util": util,
                        "quakemigrate.core.libnames": ln})
    spec = importlib.util.spec_from_file_location(
        "quakemigrate.core.lib", REF / "quakemigrate" / "core" / "lib.py")
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    return lib


def main():
    qmlib = RecordingLibrary()
    lib = load_reference_binding(qmlib)
    record = {"generator": "oracle/make_golden_binding.py",
              "reference": "QuakeMigrate v1.2.1 core/lib.py", "symbols": {}, "stalta_calls": {}}
    for name, sym in sorted(qmlib.symbols.items()):
        entry = {"argtypes": None if sym.argtypes is UNSET else [describe_type(t) for t in sym.argtypes]}
        if sym.restype is not UNSET:
            entry["restype"] = describe_type(sym.restype)
        record["symbols"][name] = entry
    # the wrappers' calls: signal, header, output buffer as the C function receives them
    for kind in ("overlapping", "centred", "recursive"):
        sym = getattr(qmlib, f"{kind}_sta_lta")
        sym.calls.clear()
        getattr(lib, f"{kind}_sta_lta")(np.arange(6), 2, 3)
        (signal, head, onset), = sym.calls
        record["stalta_calls"][kind] = {
            "signal": {"dtype": signal.dtype.str, "values": signal.tolist()}, "nsta": 2, "nlta": 3,
            "header": {"dtype": describe_dtype(head.dtype), "values": [list(map(int, h)) for h in head.tolist()]},
            "output": {"dtype": onset.dtype.str, "length": len(onset), "initial_values": np.unique(onset).tolist()}}
    OUT.write_text(json.dumps(record, indent=1) + "\n")
    print(f"{OUT.name}: {len(record['symbols'])} symbols")


if __name__ == "__main__":
    main()
