# -*- coding: utf-8 -*-
"""
The engine's tunables as a caller sees them: one list, shared by the host check of the table
(tests/test_host.py, through tools/config_check.cpp) and the engine's own config / get
(tests/test_tunables_gpu.py).

CASES: key -> probes in the order they are made, each ``(value, outcome)``: the whole refusal text (str) or the
value ``get`` of the same key returns afterwards (int).  The probes of a key follow one rule:
  flag    0, 1, 7, -1                                   (never refused: any non-zero value is 1)
  range   one below, one above, the upper bound, the lower bound
  set     one below, one above, the top of the first gap, every member downwards
  open    one below the bound, the bound, a large value
and the keys are probed in this order on ONE engine (or one record), so a key's last probe is what the next key
finds: the brick keys end at 0, where none fills in the others.
"""

def FLAG():
    return [(0, 0), (1, 1), (7, 1), (-1, 1)]


def _range(lo, hi, text):
    return [(lo - 1, text), (hi + 1, text), (hi, hi), (lo, lo)]


def _set(members, gap, text):
    return [(min(members) - 1, text), (max(members) + 1, text), (gap, text)] + [(m, m) for m in reversed(members)]


_LDS = "lds_bytes must be in 1 KiB..160 KiB"

CASES = {
    "brick_x": _range(0, 64, "brick_x must be in 0..64 (0 = automatic)"),
    "brick_y": _range(0, 64, "brick_y must be in 0..64 (0 = automatic)"),
    "brick_z": _range(0, 64, "brick_z must be in 0..64 (0 = automatic)"),
    "samples_per_lane": _set([0, 1, 2, 4], 3, "samples_per_lane must be 0 (automatic), 1, 2 or 4"),
    "waves": _range(1, 16, "waves must be 1..16"),
    "groups": [(-1, "groups must be >= 0"), (0, 0), (100000, 100000)],
    "rounds": _range(1, 1024, "rounds must be in 1..1024"),
    # (rounded down to a multiple of 16)
    "lds_bytes": [(1023, _LDS), (163841, _LDS), (163840, 163840), (1039, 1024), (1024, 1024)],
    "force_direct": FLAG(),
    "generic": FLAG(),
    "exact": FLAG(),
    "scan_waves": _range(1, 4096, "scan_waves must be in 1..4096"),
    "chunk_bytes": [((1 << 20) - 1, "chunk_bytes must be >= 1 MiB"), (1 << 20, 1 << 20), (1 << 40, 1 << 40)],
    "pair": _range(0, 2, "pair must be 0 (off), 1 (automatic) or 2 (any scan length)"),
    "screen": FLAG(),
    "screen_pairs": _set([0, 1, 2, 4], 3, "screen_pairs must be 0, 1, 2 or 4"),
    "screen_brick16": FLAG(),
    "screen_big": _range(-1, 1, "screen_big must be -1 (automatic), 0 or 1"),
    "shift": _range(-1, 1, "shift must be -1 (automatic), 0 (off) or 1"),
    "shift_waves": _set([0, 4, 8, 12], 3, "shift_waves must be 0 (automatic), 4, 8 or 12"),
    "shift_lazy": _range(-1, 1, "shift_lazy must be -1 (automatic), 0 or 1"),
    "shift_tail": FLAG(),
    "shift_rows_direct": _range(0, 2, "shift_rows_direct must be 0, 1 or 2"),
    "shift_wide": _range(-1, 1, "shift_wide must be -1 (automatic), 0 (off) or 1"),
    "shift_wide_rows": _range(
        0, 2, "shift_wide_rows must be 0 (never), 1 (where all rows do not fit) or 2 (always)"),
    "stream_pull": _range(-1, 1, "stream_pull must be -1 (slots of <= 1 MB), 0 (never) or 1 (always)"),
    "stream_stamps": FLAG(),
    "preproc_skew": FLAG(),
    "tie_rule": _range(0, 1, "tie_rule must be 0 (largest sum) or 1 (the reference's exp rule)"),
    "tie_sets": FLAG(),
    "trigger_timing": FLAG(),
    "log_timing": FLAG(),
}

# What an ENGINE's get answers for these keys, whatever was set: the last launch's or plan's value
# (include/qmhip.h), 0 before any launch.  The record itself reads back as set.
ENGINE_READS_LAST_LAUNCH = {"shift_lazy": 0, "screen_pairs": 0, "screen_big": 0}

# The keys qm_engine_get refused with "unknown key" before the tunables became one record.
NEWLY_READABLE = ("generic", "exact", "rounds", "scan_waves", "pair", "shift_rows_direct", "screen_brick16",
                  "stream_stamps", "log_timing")

# A fresh record, key by key.
DEFAULTS = {
    "brick_x": 0, "brick_y": 0, "brick_z": 0, "samples_per_lane": 0, "waves": 8, "groups": 0, "rounds": 12,
    "lds_bytes": 80 * 1024, "force_direct": 0, "generic": 0, "exact": 1, "scan_waves": 32,
    "chunk_bytes": 4 << 30, "pair": 1, "screen": 0, "screen_pairs": 0, "screen_brick16": 0, "screen_big": -1,
    "shift": -1, "shift_waves": 0, "shift_lazy": -1, "shift_tail": 1, "shift_rows_direct": 1, "shift_wide": -1,
    "shift_wide_rows": 1, "stream_pull": -1, "stream_stamps": 0, "preproc_skew": 1, "tie_rule": 0, "tie_sets": 1,
    "trigger_timing": 0, "log_timing": 0,
}

# What a set key voids or marks besides storing its value, as the check program prints it.
EFFECTS = {
    "waves": "user_waves", "rounds": "user_rounds", "lds_bytes": "user_lds",
    "shift_waves": "void_sh", "shift_rows_direct": "void_sh", "shift_wide_rows": "void_shw",
    "screen_pairs": "void_screen", "screen_brick16": "void_screen", "screen_big": "void_screen",
    "log_timing": "reset_log",
}

# An explicit brick_x fills in the other two dimensions: steps on a fresh engine (or record), ("set", key, value)
# or ("get", key, expected); they end where they began.
BRICK_FILL_STEPS = [
    ("set", "brick_x", 4), ("get", "brick_y", 1), ("get", "brick_z", 1),
    ("set", "brick_z", 0), ("get", "brick_z", 1),      # (0 is accepted and filled in again)
    ("set", "brick_x", 0), ("set", "brick_y", 0), ("set", "brick_z", 0),
    ("get", "brick_x", 0), ("get", "brick_y", 0), ("get", "brick_z", 0),
]
