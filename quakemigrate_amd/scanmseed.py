# -*- coding: utf-8 -*-
"""
``.scanmseed`` without obspy: the wire format ``QuakeScan.detect()`` emits and ``Trigger`` reads
(quakemigrate/io/scanmseed.py:74-150, 222-240, 244-325).

The reference hands five int32 series -- COA*1e5, COA_N*1e5, X*1e6, Y*1e6, Z*1e3*ucf, the two
coalescence series clipped at 21474 first -- to obspy, which writes big-endian miniSEED 2 with
4096-byte records, blockette 1000, STEIM2 compression (encoding 11), one trace after the other,
station codes COA, COA_N, X, Y, Z, network NW.  This module quantises exactly like
``ScanmSEED._data2int`` and reads / writes that container directly, so the engine's detect
output can be compared with the reference's golden files
(``examples/benchmarks/*/2014_*.scanmseed``) and fed to the reference's ``Trigger`` unchanged.

STEIM2 (SEED manual, appendix B): 64-byte frames of 16 big-endian words; word 0 holds sixteen
2-bit codes; in the first frame words 1 and 2 are the forward and reverse integration constants
(first and last sample of the record).  Codes: 00 nothing, 01 four 8-bit differences, 10 and 11
select by the word's top two bits ("dnib") 1x30 / 2x15 / 3x10 and 5x6 / 6x5 / 7x4 differences.
The encoder packs greedily -- the widest count whose differences all fit -- as libmseed (the
library behind obspy's writer) does, which reproduces the reference's files byte for byte
(tests/test_scanmseed.py).
"""

from __future__ import annotations

import datetime as _dt
import logging
import struct
from dataclasses import dataclass

import numpy as np

RECLEN = 4096
DATA_OFFSET = 64
N_FRAMES = (RECLEN - DATA_OFFSET) // 64
CHANNELS = ("COA", "COA_N", "X", "Y", "Z")
COA_CLIP = 21474.0


def scale_factors(ucf=1.0):
    """Multipliers of the five channels (scanmseed.py:113-130)."""
    return {"COA": 1e5, "COA_N": 1e5, "X": 1e6, "Y": 1e6, "Z": 1e3 * ucf}


def data2int(data, factor):
    """``ScanmSEED._data2int`` (scanmseed.py:222-240): round half to even, int32."""
    return np.round(np.asarray(data, dtype=np.float64) * factor).astype(np.int32)


def quantise(max_coa, max_coa_n, coord, ucf=1.0):
    """The five int32 series of one ``append`` call (scanmseed.py:103-130)."""
    max_coa = np.minimum(np.asarray(max_coa, dtype=np.float64), COA_CLIP)
    max_coa_n = np.minimum(np.asarray(max_coa_n, dtype=np.float64), COA_CLIP)
    f = scale_factors(ucf)
    coord = np.asarray(coord, dtype=np.float64)
    return {"COA": data2int(max_coa, f["COA"]), "COA_N": data2int(max_coa_n, f["COA_N"]),
            "X": data2int(coord[:, 0], f["X"]), "Y": data2int(coord[:, 1], f["Y"]),
            "Z": data2int(coord[:, 2], f["Z"])}


# --------------------------------------------------------------------------------------
# STEIM2
# --------------------------------------------------------------------------------------
def _sign_extend(v, bits):
    return v - (1 << bits) if v & (1 << (bits - 1)) else v


def steim2_decode(payload: bytes, n_samples: int) -> np.ndarray:
    """Decode the data part of one record; checks the reverse integration constant."""
    words = struct.unpack(f">{len(payload) // 4}I", payload)
    x0 = _sign_extend(words[1], 32)
    xn = _sign_extend(words[2], 32)
    diffs = []
    for frame in range(len(words) // 16):
        w = words[frame * 16: frame * 16 + 16]
        for k in range(1, 16):
            if frame == 0 and k < 3:
                continue
            code = (w[0] >> (30 - 2 * k)) & 3
            v = w[k]
            if code == 0:
                continue
            if code == 1:
                layout = (4, 8)
            else:
                dnib = v >> 30
                layout = {(2, 1): (1, 30), (2, 2): (2, 15), (2, 3): (3, 10),
                          (3, 0): (5, 6), (3, 1): (6, 5), (3, 2): (7, 4)}.get((code, dnib))
                if layout is None:
                    raise ValueError(f"invalid STEIM2 code {code} / dnib {dnib}")
            n, bits = layout
            for i in range(n):
                shift = (n - 1 - i) * bits
                diffs.append(_sign_extend((v >> shift) & ((1 << bits) - 1), bits))
            if len(diffs) >= n_samples:
                break
        if len(diffs) >= n_samples:
            break
    if len(diffs) < n_samples:
        raise ValueError("record holds fewer differences than samples")
    out = np.empty(n_samples, dtype=np.int64)
    out[0] = x0
    if n_samples > 1:
        out[1:] = x0 + np.cumsum(np.array(diffs[1:n_samples], dtype=np.int64))
    if out[-1] != xn:
        raise ValueError("STEIM2 reverse integration constant mismatch")
    return out.astype(np.int32)


def _fits(v, bits):
    return -(1 << (bits - 1)) <= v <= (1 << (bits - 1)) - 1


_LAYOUTS = ((7, 4, 3, 2), (6, 5, 3, 1), (5, 6, 3, 0), (4, 8, 1, None),
            (3, 10, 2, 3), (2, 15, 2, 2), (1, 30, 2, 1))   # (count, bits, code, dnib)


def steim2_encode(samples: np.ndarray, prev: int, max_frames: int = N_FRAMES):
    """
    Pack as many of ``samples`` as fit into ``max_frames`` frames.  ``prev`` is the sample before
    the first one (difference 0 of the record).  Returns ``(payload bytes, n_packed)``.
    """
    # only what the frames can consume -- 15 words of at most 7 differences each, less the two constants -- plus the
    # look-ahead of a word is turned into Python ints (6601 + 7 samples for a record): the writer is linear in the
    # trace.  `left` below still counts to the true end of `samples`
    total = len(samples)
    x = [int(v) for v in samples[:(max_frames * 15 - 2) * 7 + 7]]
    diffs = [x[0] - int(prev)] + [x[i] - x[i - 1] for i in range(1, len(x))]
    frames = [[0] * 16 for _ in range(max_frames)]
    pos = 0                                            # next difference to pack
    for fi in range(max_frames):
        frame = frames[fi]
        for k in range(1, 16):
            if fi == 0 and k < 3:
                continue
            if pos >= total:
                break
            left = total - pos
            for count, bits, code, dnib in _LAYOUTS:
                if count <= left and all(_fits(d, bits) for d in diffs[pos:pos + count]):
                    break
            else:
                raise OverflowError("difference does not fit 30 bits: not STEIM2-encodable")
            word = 0
            for d in diffs[pos:pos + count]:
                word = (word << bits) | (d & ((1 << bits) - 1))
            if dnib is not None:
                word |= dnib << 30
            frame[k] = word
            frame[0] |= code << (30 - 2 * k)
            pos += count
        if pos >= total:
            break
    frames[0][1] = x[0] & 0xFFFFFFFF
    frames[0][2] = x[pos - 1] & 0xFFFFFFFF
    payload = b"".join(struct.pack(">16I", *f) for f in frames)
    return payload, pos


# --------------------------------------------------------------------------------------
# miniSEED 2 records
# --------------------------------------------------------------------------------------
@dataclass
class Trace:
    station: str
    network: str
    starttime: _dt.datetime           # UTC, first sample
    sampling_rate: float
    data: np.ndarray                  # int32

    @property
    def endtime(self):
        return self.starttime + _dt.timedelta(seconds=(len(self.data) - 1) / self.sampling_rate)


def _btime(t: _dt.datetime) -> bytes:
    frac = int(round(t.microsecond / 100.0))
    return struct.pack(">HHBBBBH", t.year, t.timetuple().tm_yday, t.hour, t.minute, t.second,
                       0, frac)


def _from_btime(raw: bytes) -> _dt.datetime:
    year, doy, hh, mm, ss, _, frac = struct.unpack(">HHBBBBH", raw)
    return (_dt.datetime(year, 1, 1) + _dt.timedelta(days=doy - 1, hours=hh, minutes=mm,
                                                      seconds=ss, microseconds=frac * 100))


def _rate_fields(rate: float):
    if rate >= 1 and float(rate).is_integer():
        return int(rate), 1
    raise ValueError("only integer sampling rates (samples per second) are supported")


def record_header(station, network, starttime, sampling_rate, seq, pos, n) -> bytes:
    """The 64 header bytes of the record that starts at sample ``pos`` of its trace and holds ``n`` samples: fixed
    header with BTIME from ``timedelta(seconds=pos / rate)``, sequence number ``seq``, blockette 1000."""
    factor, mult = _rate_fields(sampling_rate)
    start = starttime + _dt.timedelta(seconds=pos / sampling_rate)
    header = (f"{seq:06d}".encode() + b"D " + station.ljust(5).encode() + b"  "
              + b"   " + network.ljust(2).encode() + _btime(start)
              + struct.pack(">HhhBBBBiHH", n, factor, mult, 0, 0, 0, 1, 0, DATA_OFFSET, 48)
              + struct.pack(">HHBBBB", 1000, 0, 11, 1, 12, 0))
    return header.ljust(DATA_OFFSET, b"\x00")


def write_trace(trace: Trace) -> bytes:
    """All records of one trace (what obspy writes for one ``Trace`` with STEIM2, reclen 4096)."""
    out = []
    data = np.asarray(trace.data, dtype=np.int32)
    pos, seq = 0, 1
    _rate_fields(trace.sampling_rate)
    while pos < len(data):
        prev = int(data[pos - 1]) if pos else int(data[0])     # first record: difference 0 = 0
        payload, n = steim2_encode(data[pos:], prev)
        out.append(record_header(trace.station, trace.network, trace.starttime, trace.sampling_rate, seq, pos, n)
                   + payload)
        pos += n
        seq += 1
    return b"".join(out)


def fill_headers(records, n_records, rec_first, rec_count, starttime, sampling_rate, network="NW"):
    """
    The headers of records whose payloads are packed already: ``records`` (sum, 4096) uint8 with the channels'
    ``n_records`` records one after the other, ``rec_first`` / ``rec_count`` every record's first sample index and
    sample count (what ``Engine.scanmseed_encode`` and ``tests/scanmseed_ref.py`` return).  In place; returns the bytes.
    """
    _rate_fields(sampling_rate)
    r = 0
    for ch, count in zip(CHANNELS, n_records):
        for seq in range(1, int(count) + 1):
            head = record_header(ch, network, starttime, sampling_rate, seq, int(rec_first[r]), int(rec_count[r]))
            records[r, :DATA_OFFSET] = np.frombuffer(head, dtype=np.uint8)
            r += 1
    return records.tobytes()


def encode_scanmseed(starttime, sampling_rate, series, network="NW", engine=None):
    """The bytes of a ``.scanmseed`` file.  ``engine``: an ``Engine`` -- the payloads are packed on the GPU
    (``Engine.scanmseed_encode``), the headers filled here; None: the Python encoder."""
    if engine is None:
        return b"".join(write_trace(Trace(ch, network, starttime, sampling_rate, series[ch])) for ch in CHANNELS)
    rows = [np.asarray(series[ch], dtype=np.int32) for ch in CHANNELS]
    if any(r.ndim != 1 or len(r) != len(rows[0]) for r in rows):
        raise ValueError("the five channels must be one-dimensional and of one length")
    _rate_fields(sampling_rate)
    if len(rows[0]) == 0:
        return b""
    out = engine.scanmseed_encode(np.ascontiguousarray(np.stack(rows)))
    return fill_headers(out["records"], out["n_records"], out["rec_first"], out["rec_count"], starttime,
                        sampling_rate, network)


def write_scanmseed(path, starttime, sampling_rate, series, network="NW", engine=None):
    """``series``: dict channel -> int32 array (see :func:`quantise`), written in CHANNELS order.  ``engine``: see
    :func:`encode_scanmseed`; the file's bytes are the same either way."""
    blob = encode_scanmseed(starttime, sampling_rate, series, network, engine)
    with open(path, "wb") as f:
        f.write(blob)
    return len(blob)


def parse_header(rec: bytes):
    """``(station, network, starttime, sampling_rate, n_samples, data offset)`` of one record; refuses all but
    big-endian 4096-byte STEIM2 records."""
    station = rec[8:13].decode().strip()
    network = rec[18:20].decode().strip()
    start = _from_btime(rec[20:30])
    n, factor, mult, _, _, _, nblk, _, dstart, bstart = struct.unpack(">HhhBBBBiHH", rec[30:48])
    encoding = None
    b = bstart
    for _ in range(nblk):
        btype, nxt = struct.unpack(">HH", rec[b:b + 4])
        if btype == 1000:
            encoding, order, reclen_exp = rec[b + 4], rec[b + 5], rec[b + 6]
            if order != 1 or (1 << reclen_exp) != RECLEN:
                raise ValueError("only big-endian 4096-byte records are supported")
        b = nxt
    if encoding != 11:
        raise ValueError(f"encoding {encoding}: only STEIM2 (11) is supported")
    rate = float(factor) * (mult if mult > 0 else -1.0 / mult) if factor > 0 else -1.0 / factor
    return station, network, start, rate, n, dstart


def read_records(blob: bytes):
    """Yield ``(station, network, starttime, sampling_rate, int32 data)`` per record."""
    for off in range(0, len(blob), RECLEN):
        rec = blob[off:off + RECLEN]
        station, network, start, rate, n, dstart = parse_header(rec)
        yield station, network, start, rate, steim2_decode(rec[dstart:], n)


def _read_with_engine(blob, ucf, engine, device):
    """read_scanmseed's work with the payloads decoded on the GPU: headers parsed here, one decode call for the
    channels that come back to the host and -- ``device`` -- one for COA and COA_N that leaves them on the GPU."""
    if len(blob) % RECLEN:
        raise ValueError(f"{len(blob)} bytes: not a whole number of {RECLEN}-byte records")
    records = np.frombuffer(blob, dtype=np.uint8).reshape(-1, RECLEN)
    pieces, start, rate = {}, {}, None
    for r in range(len(records)):
        station, _, t0, sr, n, dstart = parse_header(blob[r * RECLEN:(r + 1) * RECLEN])
        if dstart != DATA_OFFSET:
            raise ValueError(f"record {r}: data at byte {dstart}, the engine reads payloads at byte {DATA_OFFSET}")
        pieces.setdefault(station, []).append((t0, r, n))
        rate = sr
        start[station] = min(start.get(station, t0), t0)
    lengths = {}
    for station, recs in pieces.items():
        recs.sort(key=lambda x: x[0])
        t = recs[0][0]
        for t0, _, n in recs:
            if abs((t0 - t).total_seconds()) > 0.5 / rate:
                raise ValueError(f"gap in {station} at {t0}")
            t = t0 + _dt.timedelta(seconds=n / rate)
        lengths[station] = sum(n for _, _, n in recs)
    f = scale_factors(ucf)

    def decode(channels, on_device):
        index, samples, offset, factor, at, base = [], [], [], [], 0, {}
        for ch in channels:
            base[ch] = at
            for _, r, n in pieces[ch]:
                index.append(r)
                samples.append(n)
                offset.append(at)
                factor.append(f[ch])
                at += n
        try:
            ints, vals = engine.scanmseed_decode(np.ascontiguousarray(records[index]), samples, offset, at,
                                                 rec_factor=factor, device=on_device)
        except RuntimeError as err:                 # (the message names the record by its index in this call)
            import re

            m = re.search(r"record (\d+)", str(err))
            which = f": record {index[int(m.group(1))]} of the file" if m and int(m.group(1)) < len(index) else ""
            raise ValueError(f"{err}{which}") from err
        return ({ch: ints[base[ch]:base[ch] + lengths[ch]] for ch in channels},
                {ch: vals[base[ch]:base[ch] + lengths[ch]] for ch in channels})

    if device:
        ints, cols = decode(CHANNELS[:2], True)
        host_ints, host_cols = decode(CHANNELS[2:], False)
        ints.update(host_ints)
        cols.update(host_cols)
    else:
        ints, cols = decode(CHANNELS, False)
    cols["int"] = ints
    return start[CHANNELS[0]], rate, cols


def read_scanmseed(path, ucf=1.0, engine=None, device=False):
    """
    Read one ``.scanmseed`` file: returns ``(starttime, sampling_rate, columns)`` with
    ``columns`` = dict of float64 arrays COA, COA_N, X, Y, Z, descaled as
    ``read_scanmseed`` does (scanmseed.py:300-305), plus the raw int32 series under ``"int"``.
    ``engine``: an ``Engine`` -- the payloads are decoded on the GPU (``Engine.scanmseed_decode``), the values are the
    same; with ``device=True`` COA and COA_N, descaled and int32, stay there as tensors (what
    ``Engine.trigger_series`` takes without a host round trip), X, Y, Z come back as arrays.
    """
    with open(path, "rb") as f:
        blob = f.read()
    if engine is not None:
        return _read_with_engine(blob, ucf, engine, device)
    if device:
        raise ValueError("device=True needs an engine")
    pieces = {}
    start, rate = {}, None
    for station, _, t0, sr, data in read_records(blob):
        pieces.setdefault(station, []).append((t0, data))
        rate = sr
        start[station] = min(start.get(station, t0), t0)
    ints = {}
    for station, recs in pieces.items():
        recs.sort(key=lambda r: r[0])
        # records of a trace must be contiguous in time
        t = recs[0][0]
        for t0, d in recs:
            if abs((t0 - t).total_seconds()) > 0.5 / rate:
                raise ValueError(f"gap in {station} at {t0}")
            t = t0 + _dt.timedelta(seconds=len(d) / rate)
        ints[station] = np.concatenate([d for _, d in recs])
    f = scale_factors(ucf)
    cols = {ch: ints[ch] / f[ch] for ch in CHANNELS}
    cols["int"] = ints
    return start[CHANNELS[0]], rate, cols


# --------------------------------------------------------------------------------------
# The detect loop's sink
# --------------------------------------------------------------------------------------
class CoalescenceSink:
    """
    The reference's ``ScanmSEED`` object (quakemigrate/io/scanmseed.py:27-220) without obspy, as far
    as the detect loop uses it (``QuakeScan._continuous_compute``, signal/scan.py:421-466):
    ``append`` clips, quantises and appends one timestep to the five int32 channels
    (scanmseed.py:74-131) and writes a day's file when the stream reaches the day line or crosses it
    (scanmseed.py:133-150: the part before midnight is written, the rest kept); ``empty`` appends an
    all-zero timestep (scanmseed.py:152-180); ``write`` writes what is held (one
    ``<year>_<julday>.scanmseed`` per day, scanmseed.py:182-220).  Times are ``datetime`` (UTC).
    """

    def __init__(self, directory, sampling_rate, continuous_write=False, engine=None):
        import pathlib

        self.engine = engine                # an Engine: the day files' payloads are packed on the GPU (same bytes)

        self.directory = pathlib.Path(directory)
        self.sampling_rate = float(sampling_rate)
        self.continuous_write = continuous_write
        self.written = False
        self.starttime = None
        self.series = {ch: np.zeros(0, dtype=np.int32) for ch in CHANNELS}
        self.files = []

    def _endtime(self):
        n = len(self.series["COA"])
        return self.starttime + _dt.timedelta(seconds=(n - 1) / self.sampling_rate)

    def append(self, starttime, max_coa, max_coa_n, coord, ucf):
        new = quantise(max_coa, max_coa_n, coord, ucf)
        if self.starttime is None or len(self.series["COA"]) == 0:
            self.starttime = starttime
        else:
            expect = self._endtime() + _dt.timedelta(seconds=1.0 / self.sampling_rate)
            if abs((starttime - expect).total_seconds()) > 0.5 / self.sampling_rate:
                raise ValueError(f"timestep starting {starttime} does not continue the stream ending "
                                 f"{self._endtime()}")
        for ch in CHANNELS:
            self.series[ch] = np.concatenate([self.series[ch], new[ch]])
        self.written = False
        delta = _dt.timedelta(seconds=1.0 / self.sampling_rate)
        start, end = self.starttime, self._endtime()
        midnight = _dt.datetime(start.year, start.month, start.day) + _dt.timedelta(days=1)
        if end == midnight - delta:                       # passed the day line: write, start afresh
            self.write()
            self.starttime = None
            self.series = {ch: np.zeros(0, dtype=np.int32) for ch in CHANNELS}
        elif end >= midnight:
            logging.debug("Timestep doesn't fall at midnight!")
            keep = int(round((midnight - start).total_seconds() * self.sampling_rate))
            rest = {ch: self.series[ch][keep:] for ch in CHANNELS}
            self.series = {ch: self.series[ch][:keep] for ch in CHANNELS}
            self.write()
            self.starttime, self.series = midnight, rest
            self.written = False                          # (residual data not yet in a file)
        if self.continuous_write and not self.written:
            self.write()

    def empty(self, starttime, timestep, i, msg, ucf):
        logging.info(msg)
        n = int(round(timestep * int(self.sampling_rate)))            # util.time2sample
        start = starttime + _dt.timedelta(seconds=timestep * i)
        self.append(start, np.zeros(n), np.zeros(n), np.zeros((n, 3)), ucf)

    def write(self, write_start=None, write_end=None):
        if self.starttime is None or len(self.series["COA"]) == 0:
            self.written = True
            return
        self.directory.mkdir(parents=True, exist_ok=True)
        t = self.starttime
        path = self.directory / f"{t.year}_{t.timetuple().tm_yday:03d}.scanmseed"
        write_scanmseed(path, t, self.sampling_rate, self.series, engine=self.engine)
        if path not in self.files:
            self.files.append(path)
        self.written = True
