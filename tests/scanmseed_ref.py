# -*- coding: utf-8 -*-
"""
The STEIM2 packer of ``quakemigrate_amd/scanmseed.py`` restated on arrays, as the chain the kernels of
``csrc/qm_scanmseed.hpp`` are read against: widths -> count -> chain -> record cut -> words.

- The differences are global: ``d[0] = 0``, ``d[p] = x[p] - x[p - 1]`` (64-bit), across record boundaries too.
- ``count(p)``, the differences taken by the word that starts at ``p``, is the first of 7x4, 6x5, 5x6, 4x8, 3x10, 2x15,
  1x30 bits whose count is <= ``n - p`` (the end of the TRACE) and whose differences all fit.
- The words of a trace are the chain ``p -> p + count(p)`` from 0, cut into records every 943 words.

Also the series the codec's tests are run on (``designed_series``, ``switching_walk``, ``folded_switching_walk`` for
lengths beyond a Python loop's).
"""

import numpy as np

RECLEN, DATA_OFFSET, N_FRAMES = 4096, 64, 63
REC_WORDS = N_FRAMES * 15 - 2                                   # 943 data words per record
BITS = (4, 5, 6, 8, 10, 15, 30)                                 # width classes 0..6
# per count 1..7: (bits, code, dnib)
LAYOUT = {7: (4, 3, 2), 6: (5, 3, 1), 5: (6, 3, 0), 4: (8, 1, 0), 3: (10, 2, 3), 2: (15, 2, 2), 1: (30, 2, 1)}


def differences(x):
    x = np.asarray(x, dtype=np.int64)
    d = np.zeros(len(x), dtype=np.int64)
    d[1:] = x[1:] - x[:-1]
    return d


def width_class(d):
    """0..6 for the narrowest of 4, 5, 6, 8, 10, 15, 30 bits that holds d; 7: none does."""
    m = np.where(d < 0, ~d, d)                                  # d fits b bits iff m < 2^(b - 1)
    cls = np.zeros(len(d), dtype=np.int64)
    for b in BITS:
        cls += m >= (1 << (b - 1))
    return cls


def counts(cls):
    """count(p) for every position; OverflowError where a difference is outside 30 bits."""
    n = len(cls)
    if (cls > 6).any():
        raise OverflowError("difference does not fit 30 bits: not STEIM2-encodable")
    pad = np.concatenate([cls, np.zeros(6, dtype=cls.dtype)])
    left = n - np.arange(n)
    count = np.zeros(n, dtype=np.int64)
    run_max = [pad[:n]]
    for j in range(1, 7):
        run_max.append(np.maximum(run_max[-1], pad[j:n + j]))   # largest class of d[p .. p + j]
    for i in range(7):                                          # layout i: 7 - i differences of class <= i
        need = 7 - i
        ok = (count == 0) & (need <= left) & (run_max[need - 1] <= i)
        count[ok] = need
    return count


def chain(count):
    """The word starts: p -> p + count(p) from 0."""
    step, starts, p, n = count.tolist(), [], 0, len(count)     # (a list: the loop below runs millions of times)
    while p < n:
        starts.append(p)
        p += step[p]
    assert p == n
    return np.array(starts, dtype=np.int64)


def pack_words(d, starts, count):
    """(words uint32, codes) of the chain's words."""
    words = np.zeros(len(starts), dtype=np.uint64)
    codes = np.zeros(len(starts), dtype=np.uint64)
    for k, (bits, code, dnib) in LAYOUT.items():
        sel = np.nonzero(count[starts] == k)[0]
        w = np.zeros(len(sel), dtype=np.uint64)
        for i in range(k):
            w = (w << np.uint64(bits)) | (d[starts[sel] + i].astype(np.uint64) & np.uint64((1 << bits) - 1))
        words[sel] = w | np.uint64(dnib << 30)
        codes[sel] = code
    return words.astype(np.uint32), codes.astype(np.uint32)


def trace_chain(x):
    """``(d, count, starts)`` of one trace: its differences, count(p) of every position, the word starts."""
    d = differences(np.asarray(x, dtype=np.int32))
    count = counts(width_class(d))
    return d, count, chain(count)


def encode_trace(x, parts=None):
    """
    ``(records, rec_first, rec_count)`` of one trace: records uint8 (n_records, 4096) with the 64 header bytes zero and
    the payload complete, every record's first sample index and sample count.  ``parts``: ``trace_chain(x)``, where
    the caller has walked the chain already.
    """
    x = np.asarray(x, dtype=np.int32)
    n = len(x)
    d, count, starts = trace_chain(x) if parts is None else parts
    words, codes = pack_words(d, starts, count)
    n_rec = -(-len(starts) // REC_WORDS)
    payload = np.zeros((n_rec, N_FRAMES * 16), dtype=np.uint32)
    w = np.arange(len(starts))
    rec, slot = w // REC_WORDS, w % REC_WORDS + 2               # slots 0 and 1: the integration constants
    frame, k = slot // 15, slot % 15 + 1
    payload[rec, frame * 16 + k] = words
    np.bitwise_or.at(payload, (rec, frame * 16), (codes.astype(np.uint64) << (30 - 2 * k).astype(np.uint64)).astype(np.uint32))
    rec_first = starts[::REC_WORDS]
    rec_count = np.diff(np.append(rec_first, n))
    payload[:, 1] = x[rec_first].astype(np.uint32)
    payload[:, 2] = x[rec_first + rec_count - 1].astype(np.uint32)
    records = np.zeros((n_rec, RECLEN), dtype=np.uint8)
    records[:, DATA_OFFSET:] = payload.astype(">u4").view(np.uint8).reshape(n_rec, -1)
    return records, rec_first.astype(np.int32), rec_count.astype(np.int32)


def encode_channels(series, chains=None):
    """Five channels (5, n) -> what ``Engine.scanmseed_encode`` returns.  ``chains``: the rows' ``trace_chain``."""
    parts = [encode_trace(row, None if chains is None else chains[j]) for j, row in enumerate(series)]
    return {"n_records": np.array([len(p[0]) for p in parts], dtype=np.int64),
            "records": np.concatenate([p[0] for p in parts]),
            "rec_first": np.concatenate([p[1] for p in parts]),
            "rec_count": np.concatenate([p[2] for p in parts])}


# -- series ------------------------------------------------------------------------------------------------------------
CLASS_BOUNDS = tuple((-(1 << (b - 1)), (1 << (b - 1)) - 1) for b in BITS)


def from_differences(d, first=0):
    """The int32 series with these differences behind its first sample (the test keeps the walk inside int32)."""
    x = first + np.concatenate([[0], np.cumsum(np.asarray(d, dtype=np.int64))])
    assert x.min() >= -(1 << 31) and x.max() < (1 << 31)
    return x.astype(np.int32)


def boundary_differences():
    """
    For each width class: both boundary values, and the neighbour just outside the class, at each position of a word
    group of that class, the other positions holding a small difference; then a 4-bit difference at each offset behind
    runs of six and of seven others of every class.  Alternating signs keep the walk inside int32.
    """
    d = []
    for cls, (lo, hi) in enumerate(CLASS_BOUNDS):
        group = 7 - cls
        outside = [] if cls == 6 else [lo - 1, hi + 1]
        for value in [lo, hi] + outside:
            for at in range(group):
                block = [1, -1] * 4
                block = block[:group]
                block[at] = value
                d += block + [-(value // 2), -(value - value // 2)]      # two steps back: the walk stays bounded
                d += [0] * (at % 3)                              # ... and the groups drift against the word grid
    for cls, (lo, hi) in enumerate(CLASS_BOUNDS[1:], start=1):
        for run in (6, 7):
            for offset in range(7):
                d += [hi, lo] * (run // 2) + ([hi] if run % 2 else []) + [0] * offset + [7, -8]
                d += [-hi] if run % 2 else []
    return np.array(d, dtype=np.int64)


def switching_walk(rng, n, classes=(0, 1, 2, 3, 4, 5), max_run=40):
    """A walk whose differences switch width class in runs of random length (symmetric, so it stays bounded)."""
    d = np.zeros(n - 1, dtype=np.int64)
    at = 0
    while at < n - 1:
        run = int(rng.integers(1, max_run + 1))
        lo, hi = CLASS_BOUNDS[int(rng.choice(classes))]
        d[at:at + run] = rng.integers(lo, hi + 1, size=min(run, n - 1 - at))
        at += run
    # a step that would take the walk outside +-2^30 is mirrored (its width class stays, up to the asymmetric bound)
    x, bound = 0, 1 << 30
    for i, step in enumerate(d.tolist()):
        if abs(x + step) > bound:
            d[i] = step = -step - (1 if step < 0 else 0)
        x += step
    return from_differences(d)


def folded_switching_walk(rng, n, classes=(0, 1, 2, 3, 4, 5), max_run=40, bound=1 << 30):
    """
    ``switching_walk`` for series of millions of samples, without its Python loop: differences drawn from ``[-hi, hi]``
    of a width class that switches in runs of random length, their 64-bit running sum folded into ``[-bound, bound]``
    by reflection at both ends (a triangle wave of period ``4 bound``).  Between two reflections the series' differences
    are the drawn ones up to one sign, which keeps their class; the step across a reflection is shorter than the drawn
    one.
    """
    n_runs = 4 * n // (max_run + 1) + 64
    runs = rng.integers(1, max_run + 1, size=n_runs)
    assert int(runs.sum()) >= n - 1
    hi = np.array([b[1] for b in CLASS_BOUNDS], dtype=np.int64)[rng.choice(classes, size=n_runs)]
    hi = np.repeat(hi, runs)[:n - 1]
    walk = np.concatenate([[0], np.cumsum(rng.integers(-hi, hi + 1))])
    m = np.mod(walk + bound, 4 * bound)
    return np.where(m < 2 * bound, m - bound, 3 * bound - m).astype(np.int32)


def designed_series():
    """name -> int32 series: the width boundaries and the ends the issue lists."""
    out = {"boundaries": from_differences(boundary_differences())}
    big = (1 << 29) - 1
    for n in (1, 2, 7, 8, 10):                                  # (10: a trace ending inside frame 0)
        out[f"n{n}"] = from_differences([3, -2, 100, -100, 5, 1, -1, 40000, -40000][:n - 1], first=-5)
    for n in (943, 944, 1886, 1887):                            # all 30-bit: 943 samples per record
        d = np.where(np.arange(n - 1) % 2 == 0, big, -big)
        out[f"wide{n}"] = from_differences(d, first=-(1 << 28))
    for n in (6601, 6602, 13202):                               # all 4-bit: 6601 samples per record
        out[f"narrow{n}"] = from_differences(np.where(np.arange(n - 1) % 2 == 0, 7, -8))
    for tail in range(1, 7):                                    # the last word holds 1..6 differences: count <= left
        out[f"tail{tail}"] = from_differences(np.where(np.arange(7 * 5 + tail - 1) % 2 == 0, 3, -3))
    return out
