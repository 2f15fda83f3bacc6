# -*- coding: utf-8 -*-
"""
Bindings for the MI355X coalescence-migration engine -- the host-side mirror of
the reference's ``quakemigrate/core/lib.py`` for the migrate / find_max_coa path.

Same function names, argument meaning, return values and error behaviour as the
reference (``lib.py:52-125`` ``migrate``, ``lib.py:131-170`` ``find_max_coa``,
``lib.py:176-285`` the three STA/LTA functions), so ``QuakeScan._compute``
(``quakemigrate/signal/scan.py:635-638``) can call them unchanged.  On top of that
``migrate_and_find_max`` is the fused call that never materialises the 4-D map
(what ``detect()`` wants, ``scan.py:641-642``).

Everything numeric below the clip/log pre-processing runs in the HIP library
(``include/qmhip.h``); NumPy is used only for the reference's own host-side
pre-processing (``np.clip`` + ``np.log``, ``lib.py:93-94``) and for allocating
the caller-owned result arrays.
"""

from __future__ import annotations

import ctypes
import logging
import weakref

import numpy as np
import numpy.ctypeslib as clib

from quakemigrate_amd.core.libnames import _load_cdll

qmlib = _load_cdll("qmlib")

c_int32 = ctypes.c_int32
c_int64 = ctypes.c_int64
c_dPt = clib.ndpointer(dtype=np.double, flags="C_CONTIGUOUS")
c_i32Pt = clib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
c_i64Pt = clib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")

stalta_header_t = np.dtype(
    [("n", c_int32), ("nsta", c_int32), ("nlta", c_int32)], align=True
)
stalta_header_pt = clib.ndpointer(stalta_header_t, flags="C_CONTIGUOUS")

# ---- reference-compatible symbols (qmlib.h:28-44) ---------------------------
qmlib.migrate.argtypes = [c_dPt, c_i32Pt, c_dPt, c_int32, c_int32, c_int32,
                          c_int32, c_int32, c_int64, c_int64]
qmlib.migrate.restype = None
qmlib.find_max_coa.argtypes = [c_dPt, c_dPt, c_dPt, c_i64Pt, c_int32, c_int64,
                               c_int64]
qmlib.find_max_coa.restype = None
for _f in (qmlib.overlapping_sta_lta, qmlib.centred_sta_lta,
           qmlib.recursive_sta_lta):
    _f.argtypes = [c_dPt, stalta_header_pt, c_dPt]
    _f.restype = None

# ---- handle API (include/qmhip.h part 2) ------------------------------------
_vp = ctypes.c_void_p
qmlib.qm_last_error.restype = ctypes.c_char_p
qmlib.qm_device_count.restype = ctypes.c_int
qmlib.qm_build_info.restype = ctypes.c_char_p
qmlib.qm_build_info.argtypes = []
qmlib.qm_compat_status.restype = ctypes.c_int
qmlib.qm_table_hash.restype = None
qmlib.qm_table_hash.argtypes = [ctypes.c_void_p, c_int64, ctypes.POINTER(ctypes.c_uint64),
                                ctypes.POINTER(ctypes.c_uint64)]
qmlib.qm_engine_create.argtypes = [ctypes.c_int, ctypes.POINTER(_vp)]
qmlib.qm_release_cached_memory.argtypes = []
qmlib.qm_release_cached_memory.restype = ctypes.c_int
qmlib.qm_engine_destroy.argtypes = [_vp]
qmlib.qm_engine_destroy.restype = None
qmlib.qm_engine_set_stream.argtypes = [_vp, _vp, ctypes.c_int]
qmlib.qm_engine_synchronize.argtypes = [_vp]
qmlib.qm_engine_config.argtypes = [_vp, ctypes.c_char_p, c_int64]
qmlib.qm_engine_get.argtypes = [_vp, ctypes.c_char_p, ctypes.POINTER(c_int64)]
qmlib.qm_engine_load_lut.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32,
                                     c_int32, c_int32, c_int64]
qmlib.qm_engine_table_select.argtypes = [_vp, ctypes.c_uint64, c_int32, ctypes.POINTER(c_int32)]
qmlib.qm_engine_lut_max.argtypes = [_vp, ctypes.POINTER(c_int32)]
qmlib.qm_engine_grids_begin.argtypes = [_vp, c_int32, c_int32, c_int32, c_int32]
qmlib.qm_engine_grids_set.argtypes = [_vp, c_int32, _vp, ctypes.c_int]
qmlib.qm_engine_serve.argtypes = [_vp, ctypes.c_double, c_i32Pt, c_int32, c_int32, c_int32,
                                  c_int32, c_int64]
qmlib.qm_engine_lut_download.argtypes = [_vp, c_i32Pt]
qmlib.qm_engine_table_digest.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint64)]
qmlib.qm_engine_detect.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32,
                                   c_int32, c_int32, c_int64, _vp, _vp, _vp,
                                   ctypes.c_int]
qmlib.qm_engine_detect_batch.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32, c_int32,
                                         c_int32, c_int32, c_int64, _vp, _vp, _vp,
                                         ctypes.c_int]
qmlib.qm_engine_detect_partial.argtypes = [_vp, _vp, ctypes.c_int, c_int32,
                                           c_int32, c_int32, c_int32, _vp, _vp,
                                           _vp]
qmlib.qm_engine_finalize.argtypes = [_vp, _vp, _vp, _vp, c_int32, c_int32,
                                     c_int64, _vp, _vp, _vp, ctypes.c_int]
qmlib.qm_engine_finalize_packed.argtypes = [_vp, _vp, c_int32, c_int32, c_int64, _vp, _vp,
                                            _vp, ctypes.c_int]
qmlib.qm_engine_tie_partial.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32, c_int32, c_int32, _vp,
                                        c_int32, _vp]
qmlib.qm_engine_tie_fold.argtypes = [_vp, _vp, c_int32, c_int32, _vp]
qmlib.qm_engine_migrate.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32,
                                    c_int32, c_int32, c_int64, _vp, ctypes.c_int,
                                    ctypes.c_int, _vp, _vp, _vp, ctypes.c_int]
qmlib.qm_engine_marginal.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32, c_int32,
                                     c_int32, c_int64, c_int32, c_int32, _vp, ctypes.c_int,
                                     _vp, _vp, _vp, ctypes.c_int]
qmlib.qm_engine_locate_fits.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32, c_int32,
                                        ctypes.c_double, ctypes.c_double,
                                        ctypes.POINTER(ctypes.c_double), _vp, _vp, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_double)]
qmlib.qm_engine_rbf_peak.argtypes = [_vp, ctypes.POINTER(ctypes.c_double), c_int32, c_int32,
                                     ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int64)]
qmlib.qm_engine_onsets.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32, c_i32Pt, c_int32,
                                   c_i32Pt, c_i32Pt, ctypes.c_int, ctypes.c_int, c_int32,
                                   ctypes.c_double, _vp, _vp, ctypes.c_int]
qmlib.qm_engine_preprocess.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32, c_i32Pt, c_dPt, c_int32, c_int32,
                                       ctypes.c_int, c_dPt, c_int32, c_dPt, c_int32, ctypes.c_int, _vp,
                                       ctypes.c_int]
qmlib.qm_engine_preprocess_segments.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32, c_i32Pt, c_dPt, c_int32,
                                                c_int32, ctypes.c_int, ctypes.c_int, c_i64Pt, c_int32, c_dPt, c_int64,
                                                ctypes.c_int, ctypes.c_double, _vp, ctypes.c_int]
qmlib.qm_engine_resample.argtypes = [_vp, _vp, ctypes.c_int, ctypes.c_int, c_int64, c_int32, c_i64Pt, c_dPt, c_int32,
                                     c_int32, ctypes.c_int, c_i32Pt, c_int32, c_dPt, c_int64, c_int32, _vp,
                                     ctypes.c_int]
qmlib.qm_engine_pick_phases.argtypes = [_vp, _vp, ctypes.c_int, c_int32, c_int32, _vp, _vp, ctypes.c_double, _vp,
                                        ctypes.c_int, ctypes.c_double, _vp, _vp, _vp]
qmlib.qm_engine_measure_amplitudes.argtypes = [_vp, _vp, ctypes.c_int, c_int64, c_int32, c_i64Pt, c_dPt, c_int32,
                                               c_int32, c_i32Pt, c_int32, c_dPt, c_int64, c_int32, c_i64Pt,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_double, _vp, _vp, _vp]
qmlib.qm_engine_tt_homogeneous.argtypes = [_vp, c_dPt, c_dPt, c_i32Pt, c_int32, c_dPt, _vp, ctypes.c_int]
qmlib.qm_engine_tt_sections.argtypes = [_vp, c_int32, c_int32, c_int32, ctypes.c_double, c_dPt, c_dPt, ctypes.c_double,
                                        c_int32, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int]
qmlib.qm_engine_tt_sweep.argtypes = [_vp, c_dPt, c_dPt, c_i32Pt, c_int32, c_dPt, c_i32Pt, _vp, ctypes.c_int, c_int32,
                                     c_int32, c_int32, ctypes.c_double, _vp, ctypes.c_int]
qmlib.qm_engine_tt_eikonal3d.argtypes = [_vp, c_dPt, c_dPt, c_i32Pt, c_int32, c_dPt, c_i32Pt, c_int32, _vp, ctypes.c_int,
                                         ctypes.c_double, c_int32, _vp, ctypes.c_int, c_i32Pt, c_i32Pt]


class TriggerParams(ctypes.Structure):
    """``qm_trigger_params`` (include/qmhip.h)."""
    _fields_ = [("trigger_on", c_int32), ("threshold_method", c_int32), ("threshold_value", ctypes.c_double),
                ("chunk_samples", c_int64), ("smooth_radius", c_int32), ("reserved", c_int32),
                ("smooth_weights", _vp), ("period_ns", c_int64), ("mw_ns", c_int64), ("mei_ns", c_int64)]


qmlib.qm_engine_trigger.argtypes = [_vp, _vp, _vp, c_int64, ctypes.POINTER(TriggerParams), c_int64,
                                    ctypes.POINTER(c_int64), ctypes.POINTER(c_int64), _vp, _vp, _vp, _vp, _vp,
                                    c_int64]
qmlib.qm_engine_trigger_resident.argtypes = qmlib.qm_engine_trigger.argtypes
qmlib.qm_engine_scanmseed_encode.argtypes = [_vp, _vp, ctypes.c_int, ctypes.c_int, c_int64, _vp, _vp, c_int64, _vp, _vp,
                                             _vp, _vp]
qmlib.qm_engine_scanmseed_decode.argtypes = [_vp, _vp, c_int64, _vp, _vp, _vp, c_int64, _vp, _vp, ctypes.c_int]
qmlib.qm_engine_find_max_coa.argtypes = [_vp, _vp, ctypes.c_int, c_int32,
                                         c_int64, _vp, _vp, _vp, ctypes.c_int]
qmlib.qm_exp2f_max_error.argtypes = [_vp, ctypes.c_float, ctypes.c_float,
                                     ctypes.POINTER(ctypes.c_double)]
qmlib.qm_exp_correctly_rounded.argtypes = [ctypes.c_double]
qmlib.qm_exp_correctly_rounded.restype = ctypes.c_double
qmlib.qm_engine_exp_correctly_rounded.argtypes = [_vp, c_dPt, c_int64, c_dPt]
qmlib.qm_stream_create.argtypes = [_vp, c_int32, c_int32, c_int32, c_int32, c_int64, c_int32, c_int32,
                                   ctypes.POINTER(_vp)]
qmlib.qm_stream_create_replicas.argtypes = [ctypes.POINTER(_vp), c_int32, c_int32, c_int32, c_int32, c_int32,
                                            c_int64, c_int32, c_int32, ctypes.POINTER(_vp)]
qmlib.qm_stream_destroy.argtypes = [_vp]
qmlib.qm_stream_destroy.restype = None
qmlib.qm_stream_push.argtypes = [_vp, _vp]
qmlib.qm_stream_push_signals.argtypes = [_vp, _vp]
qmlib.qm_stream_set_onset_stage.argtypes = [_vp, c_int32, c_i32Pt, c_i32Pt, c_dPt, c_int32, c_int32, ctypes.c_int,
                                            c_dPt, c_int32, c_dPt, c_int32, c_i32Pt, c_i32Pt, ctypes.c_int,
                                            ctypes.c_int, c_int32, ctypes.c_double]
qmlib.qm_stream_push_raw.argtypes = [_vp, _vp]
qmlib.qm_stream_set_resample_stage.argtypes = [_vp, c_int32, c_i64Pt, c_dPt, c_int32, c_int32, ctypes.c_int, c_i32Pt,
                                               c_int32, c_dPt, c_int64, c_int32, ctypes.c_int, c_int64]
qmlib.qm_stream_set_segment_feed.argtypes = [_vp, c_int32, c_int64, ctypes.c_int, ctypes.c_double]
qmlib.qm_stream_push_segments.argtypes = [_vp, _vp, c_i64Pt, c_int32, c_dPt, c_int64]
qmlib.qm_stream_flush.argtypes = [_vp]
qmlib.qm_stream_pop.argtypes = [_vp, c_int32, _vp, _vp, _vp]
qmlib.qm_stream_pending.argtypes = [_vp, ctypes.POINTER(c_int32), ctypes.POINTER(c_int32)]
qmlib.qm_engine_last_kernel_ms.argtypes = [_vp, ctypes.POINTER(ctypes.c_double)]
qmlib.qm_engine_kernel_log.argtypes = [_vp, ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(c_int32)]
# ---- engine groups (include/qmhip.h part 4) -----------------------------------
_i32p = ctypes.POINTER(c_int32)
qmlib.qm_group_plan.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, _i32p, _i32p]
qmlib.qm_group_create.argtypes = [_i32p, c_int32, ctypes.POINTER(_vp)]
qmlib.qm_group_destroy.argtypes = [_vp]
qmlib.qm_group_destroy.restype = None
qmlib.qm_group_config.argtypes = [_vp, ctypes.c_char_p, c_int64]
qmlib.qm_group_get.argtypes = [_vp, ctypes.c_char_p, ctypes.POINTER(c_int64)]
qmlib.qm_group_load_lut.argtypes = [_vp, _vp, c_int32, c_int32, c_int32, c_int32]
qmlib.qm_group_table_select.argtypes = [_vp, ctypes.c_uint64, c_int32, ctypes.POINTER(c_int32)]
qmlib.qm_group_detect.argtypes = [_vp, _vp, c_int32, c_int32, c_int32, c_int32, _vp, _vp, _vp]
qmlib.qm_group_marginal.argtypes = [_vp, _vp, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _vp, _vp,
                                    _vp, _vp]
qmlib.qm_group_migrate.argtypes = [_vp, _vp, c_int32, c_int32, c_int32, c_int32, _vp, ctypes.c_int, _vp, _vp, _vp]
qmlib.qm_group_find_max_coa.argtypes = [_vp, _vp, c_int32, c_int64, _vp, _vp, _vp]
qmlib.qm_group_synchronize.argtypes = [_vp]
qmlib.qm_group_n_parts.argtypes = [_vp, _i32p]
qmlib.qm_group_part_info.argtypes = [_vp, c_int32, _i32p, _i32p, _i32p, ctypes.POINTER(c_int64),
                                     ctypes.POINTER(ctypes.c_double)]


RAW_DTYPES = {np.dtype(np.int32): 0, np.dtype(np.float64): 1}       # qm_engine_resample's raw_dtype


def _sections(sos, name="sos", count="n_filters"):
    """``sos`` as the contiguous float64 (n, n_sections, 6) array the C ABI takes."""
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    if sos.ndim != 3 or sos.shape[2] != 6:
        raise ValueError(f"{name} of shape {sos.shape}: ({count}, n_sections, 6) expected")
    return sos


def _taper_arrays(table, weights):
    """A taper table (n_tapers, 2) int32 and its weights, float64 and flat; ``None``: none."""
    table = np.ascontiguousarray(np.zeros((0, 2)) if table is None else table, dtype=np.int32)
    weights = np.ascontiguousarray([] if weights is None else weights, dtype=np.float64).reshape(-1)
    if table.ndim != 2 or table.shape[1] != 2:
        raise ValueError(f"taper_table of shape {table.shape}: (n_tapers, 2) expected")
    return table, weights


def _pack_by_records(traces, offsets, lengths, total, dtype, refuse):
    """A list of traces as one packed array of ``total`` elements, trace i at ``offsets[i]``.  ``refuse(i, x, fits)``
    raises the caller's error for a trace it does not take; ``fits``: x is the 1-D array of ``lengths[i]`` samples that
    its record plans, inside the packed array."""
    packed = np.zeros(total, dtype=dtype)
    for i, (x, off, n) in enumerate(zip(traces, offsets, lengths)):
        x = np.asarray(x)
        refuse(i, x, x.ndim == 1 and len(x) == n and off >= 0 and off + n <= total)
        packed[off:off + n] = x
    return packed


def segment_arrays(records, taper_weights):
    """A timestep's segment records (n_segments, 8) int64 and taper weights, contiguous and flat, as the C ABI takes
    them (:func:`quakemigrate_amd.preprocess.plan_segments` makes them)."""
    records = np.ascontiguousarray(records, dtype=np.int64)
    if records.ndim != 2 or records.shape[1] != 8:
        raise ValueError(f"records of shape {records.shape}: (n_segments, 8) expected")
    weights = np.ascontiguousarray([] if taper_weights is None else taper_weights, dtype=np.float64).reshape(-1)
    return records, weights


def resample_arrays(stage, t_samples=None):
    """The checked, contiguous arrays of a resampling stage -- a :class:`quakemigrate_amd.preprocess.ResampleStage`
    (then ``t_samples`` is needed) or the dict its ``arrays(t_samples)`` returns -- in the order the C ABI takes them:
    ``(records, sos_lp, taper_table, taper_weights, detrend, t_samples, total_raw_samples)``."""
    if hasattr(stage, "arrays"):
        if t_samples is None:
            raise ValueError("a ResampleStage needs the t_samples of the windows")
        stage = stage.arrays(int(t_samples))
    a = stage
    records = np.ascontiguousarray(a["records"], dtype=np.int64)
    if records.ndim != 2 or records.shape[1] != 11:
        raise ValueError(f"records of shape {records.shape}: (n_traces, 11) expected")
    sos = _sections(a["sos_lp"], "sos_lp", "n_lowpass")
    table, weights = _taper_arrays(np.reshape(a["taper_table"], (-1, 2)), a["taper_weights"])
    if t_samples is not None and int(a["t_samples"]) != int(t_samples):
        raise ValueError(f"the stage was planned for windows of {a['t_samples']} samples, not {t_samples}")
    total = a.get("total_raw_samples")
    if total is None:
        total = int(np.max(records[:, 0] + records[:, 1])) if len(records) else 0
    return records, sos, table, weights, int(a.get("detrend", 1)), int(a["t_samples"]), int(total)


def pack_raw(raw, records, total, dtype=None):
    """A timestep's raw traces as one packed host array: ``raw`` is a list of 1-D arrays, one per trace (each goes to
    its record's raw offset), or the packed array itself.  int32 or float64 (``dtype``: the one asked for)."""
    if isinstance(raw, (list, tuple)):
        if len(raw) != len(records):
            raise ValueError(f"{len(raw)} raw traces, the stage plans {len(records)}")
        kind = np.dtype(dtype) if dtype is not None else np.result_type(*[np.asarray(x).dtype for x in raw])

        def refuse(i, x, fits):
            if not fits:
                n = int(records[i][1])
                raise ValueError(f"raw trace {i} of shape {x.shape}: the stage plans {n} samples for it")
            if x.dtype != kind:
                raise TypeError(f"raw trace {i}: expected {kind}, got {x.dtype}")

        raw = _pack_by_records(raw, [r[0] for r in records], [r[1] for r in records], total, kind, refuse)
    if isinstance(raw, np.ndarray):
        if dtype is not None and raw.dtype != np.dtype(dtype):
            raise TypeError(f"raw samples: expected {np.dtype(dtype)}, got {raw.dtype}")
        if raw.dtype not in RAW_DTYPES:
            raise TypeError(f"raw samples of type {raw.dtype}: int32 or float64")
        if raw.ndim != 1 or not raw.flags["C_CONTIGUOUS"] or raw.size < total:
            raise ValueError(f"packed raw samples of shape {raw.shape}: one contiguous axis of at least {total}")
    return raw


class QMHipError(RuntimeError):
    """A call into the HIP engine failed (message from ``qm_last_error``)."""


def _check(rc):
    if rc != 0:
        raise QMHipError(qmlib.qm_last_error().decode(errors="replace"))


def _host(a):
    return a.ctypes.data_as(_vp)


def build_info():
    """What the loaded library was built from (include/qmhip.h: qm_build_info): the generated shift-reuse
    loops' constants and generator digest, overlay and development defines ("none" in the product build)."""
    return qmlib.qm_build_info().decode()


class Engine:
    """
    One GPU's migration engine (thin object wrapper over the C handle API).

    Pointers may be NumPy arrays (host, synchronous) or integers / objects with
    ``data_ptr()`` (device memory on this engine's GPU, asynchronous on the
    engine's stream) -- see :func:`_ptr`.
    """

    def __init__(self, device=0, **config):
        h = _vp()
        _check(qmlib.qm_engine_create(int(device), ctypes.byref(h)))
        self._h = h
        self.device = int(device)
        self._finalizer = weakref.finalize(self, qmlib.qm_engine_destroy, h)
        self.grid = None
        self.n_rows = None
        self.node_offset = 0
        self.table_generation = 0       # bumped whenever the resident table is replaced
        self._current_key = None        # key of the resident table (select_table), if it has one
        self.grids_generation = 0       # bumped by set_traveltime_grids (the grids are shared by
                                        # every MigrationScan on this engine)
        for k, v in config.items():
            self.config(k, v)

    # -- plumbing -----------------------------------------------------------
    def close(self):
        self._finalizer()

    def config(self, key, value):
        _check(qmlib.qm_engine_config(self._h, key.encode(), int(value)))

    def get(self, key):
        v = c_int64()
        _check(qmlib.qm_engine_get(self._h, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def set_stream(self, stream_ptr):
        """
        Run on the given ``hipStream_t`` handle (an int; 0 is the device's default stream,
        i.e. ``torch.cuda.current_stream().cuda_stream`` outside a stream context), or on
        the engine's private stream with ``None``.
        """
        if stream_ptr is None:
            _check(qmlib.qm_engine_set_stream(self._h, _vp(None), 1))
        else:
            _check(qmlib.qm_engine_set_stream(self._h, _vp(int(stream_ptr) or None), 0))

    def synchronize(self):
        _check(qmlib.qm_engine_synchronize(self._h))

    def last_kernel_ms(self):
        ms = ctypes.c_double()
        _check(qmlib.qm_engine_last_kernel_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def exp2f_max_error(self, lo, hi):
        """Largest relative deviation of the GPU's ``v_exp_f32`` from the float64 ``exp2`` over
        every float32 in ``[lo, hi]`` (self-check behind the screened detect's error bound)."""
        out = ctypes.c_double()
        _check(qmlib.qm_exp2f_max_error(self._h, float(lo), float(hi), ctypes.byref(out)))
        return float(out.value)

    def exp_correctly_rounded(self, x):
        """``exp(x)`` rounded to nearest, evaluated on the GPU (csrc/qm_ties.hpp: what the opt-in
        ``tie_rule = 1`` compares near-tied nodes on)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        _check(qmlib.qm_engine_exp_correctly_rounded(self._h, x.reshape(-1), x.size, out.reshape(-1)))
        return out

    def kernel_log(self):
        """(total ms, launches) of the stacking kernels since the last call."""
        ms, n = ctypes.c_double(), c_int32()
        _check(qmlib.qm_engine_kernel_log(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    _TORCH_NAMES = {np.dtype(np.float64): "torch.float64", np.dtype(np.int64): "torch.int64",
                    np.dtype(np.int32): "torch.int32"}

    def _ptr(self, x, dtype=None, count=None):
        """
        (void*, on_device) for a NumPy array, a torch tensor or a raw int.  Arrays and tensors
        are checked: element type ``dtype``, contiguity, at least ``count`` elements, and -- for
        a device tensor -- that it lives on this engine's GPU (a wrong type or device would be
        reinterpreted silently by the C side).  A raw int is taken as a device address as is.
        """
        if isinstance(x, np.ndarray):
            if dtype is not None and x.dtype != dtype:
                raise TypeError(f"expected {np.dtype(dtype)}, got {x.dtype}")
            if not x.flags["C_CONTIGUOUS"]:
                raise ValueError("array must be C-contiguous")
            if count is not None and x.size < count:
                raise ValueError(f"array holds {x.size} elements, {count} needed")
            return _host(x), 0
        if hasattr(x, "data_ptr"):                  # torch tensor
            if not x.is_contiguous():
                raise ValueError("tensor must be contiguous")
            if dtype is not None and str(x.dtype) != self._TORCH_NAMES[np.dtype(dtype)]:
                raise TypeError(f"expected {self._TORCH_NAMES[np.dtype(dtype)]}, got {x.dtype}")
            if count is not None and x.numel() < count:
                raise ValueError(f"tensor holds {x.numel()} elements, {count} needed")
            if x.is_cuda and x.device.index != self.device:
                raise ValueError(f"tensor lives on cuda:{x.device.index}, this engine runs on "
                                 f"cuda:{self.device}")
            return _vp(x.data_ptr()), (1 if x.is_cuda else 0)
        return _vp(int(x)), 1

    def _series(self, out, n):
        """Pointers of a (float64, float64, int64) output triple of >= n elements each; the
        three must be all host or all device."""
        (pa, da), (pb, db), (pc, dc) = (self._ptr(out[0], np.float64, n),
                                        self._ptr(out[1], np.float64, n),
                                        self._ptr(out[2], np.int64, n))
        if not da == db == dc:
            raise ValueError("the three output series must be all host or all device")
        return pa, pb, pc, da

    # -- table --------------------------------------------------------------
    def load_lut(self, traveltimes, node_offset=0, shape=None):
        """
        Make the int32 travel-time table resident: shape (nx, ny, nz, n_rows), C
        order (what ``LUT.serve_traveltimes`` returns, lut.py:538).
        """
        if shape is None:
            shape = tuple(traveltimes.shape)
        if len(shape) != 4:
            raise ValueError("traveltimes must have shape (nx, ny, nz, n_rows)")
        p, dev = self._ptr(traveltimes, np.int32)
        nx, ny, nz, rows = (int(v) for v in shape)
        self._foreign_load()
        _check(qmlib.qm_engine_load_lut(self._h, p, dev, nx, ny, nz, rows,
                                        int(node_offset)))
        self.grid = (nx, ny, nz)
        self.n_rows = rows
        self.node_offset = int(node_offset)
        self.table_generation += 1

    def _foreign_load(self):
        """A load on top of a resident table (no ``select_table`` miss in between) replaces it and
        does not inherit its key -- the C side un-keys it the same way (qm_engine_load_lut)."""
        if self.grid is not None:
            self._current_key = None

    def select_table(self, key, capacity=4):
        """
        Work on the table known under ``key`` (any hashable): parks the current table's device
        state -- up to ``capacity`` tables, least recently used evicted -- and brings the one parked
        under ``key`` back (a pointer swap).  Returns True if that table is resident now; False if
        the caller has to load it (``load_lut`` / ``serve``: it is then known under ``key``).
        For the alternating station availabilities of a continuous run (lut.py:529-537).
        """
        import hashlib

        digest = hashlib.blake2b(repr(key).encode(), digest_size=8).digest()
        k64 = int.from_bytes(digest, "little")
        if not hasattr(self, "_tables"):
            self._tables = {}
        if self._current_key is not None:
            self._tables.pop(self._current_key, None)           # (most recent last)
            self._tables[self._current_key] = (self.grid, self.n_rows, self.node_offset)
            while len(self._tables) > 256:                      # shapes of long-evicted tables
                self._tables.pop(next(iter(self._tables)))
        resident = c_int32()
        _check(qmlib.qm_engine_table_select(self._h, k64, int(capacity), ctypes.byref(resident)))
        self._current_key = k64
        if resident.value and k64 in self._tables:
            self.grid, self.n_rows, self.node_offset = self._tables[k64]
        elif not resident.value:
            self.grid, self.n_rows = None, None
        self.table_generation += 1
        return bool(resident.value)

    # -- on-device serving (lut.py:502-538 / :102-140 moved to the GPU) ----------
    def set_traveltime_grids(self, grids):
        """
        Upload float64 travel-time grids in seconds, each (nx, ny, nz): one per
        station/phase, e.g. ``[lut[station][phase] for ...]``.  Done once per LUT.
        """
        grids = list(grids)
        nx, ny, nz = (int(v) for v in grids[0].shape)
        self.grids_generation += 1
        _check(qmlib.qm_engine_grids_begin(self._h, nx, ny, nz, len(grids)))
        for i, g in enumerate(grids):
            if tuple(g.shape) != (nx, ny, nz):
                raise ValueError("all travel-time grids must share one shape")
            if isinstance(g, np.ndarray):
                g = np.ascontiguousarray(g, dtype=np.float64)
            p, dev = self._ptr(g, np.float64)
            _check(qmlib.qm_engine_grids_set(self._h, i, p, dev))

    def serve(self, sampling_rate, rows, decimate=(1, 1, 1), node_offset=0):
        """
        Build and make resident the int32 table ``rint(grid[rows[s]] * sampling_rate)`` of
        the selected grids, decimated like ``Grid3D.decimate``.
        """
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        dfx, dfy, dfz = (int(v) for v in decimate)
        self._foreign_load()
        _check(qmlib.qm_engine_serve(self._h, float(sampling_rate), rows, len(rows), dfx, dfy,
                                     dfz, int(node_offset)))
        self.grid = (self.get("nx"), self.get("ny"), self.get("nz"))
        self.table_generation += 1
        self.n_rows = len(rows)
        self.node_offset = int(node_offset)

    def download_lut(self):
        out = np.empty(tuple(self.grid) + (self.n_rows,), dtype=np.int32)
        _check(qmlib.qm_engine_lut_download(self._h, out))
        return out

    def table_digest(self):
        """64-bit digest of the resident table and its shape, computed on the device once per table
        (``qm_engine_table_digest``)."""
        v = ctypes.c_uint64()
        _check(qmlib.qm_engine_table_digest(self._h, ctypes.byref(v)))
        return int(v.value)

    @property
    def lut_max(self):
        v = c_int32()
        _check(qmlib.qm_engine_lut_max(self._h, ctypes.byref(v)))
        return int(v.value)

    @property
    def n_nodes(self):
        return int(np.prod(self.grid))

    # -- steps --------------------------------------------------------------
    def detect(self, log_onsets, fsmp, lsmp, available, n_nodes_total=None,
               out=None):
        """Fused migrate + find_max_coa; ``log_onsets`` already log(clip(.))."""
        rows, t_samples = (int(v) for v in log_onsets.shape)
        self._check_rows(rows)
        n = t_samples - fsmp - lsmp
        if out is None:
            out = (np.zeros(max(n, 0)), np.zeros(max(n, 0)),
                   np.zeros(max(n, 0), dtype=np.int64))
        po, dev_on = self._ptr(log_onsets, np.float64)
        pa, pb, pc, da = self._series(out, max(n, 0))
        total = self.n_nodes if n_nodes_total is None else int(n_nodes_total)
        _check(qmlib.qm_engine_detect(self._h, po, dev_on, t_samples, int(fsmp),
                                      int(lsmp), int(available), total, pa, pb,
                                      pc, da))
        return out

    def detect_batch(self, log_onsets, fsmp, lsmp, available, n_nodes_total=None, out=None):
        """
        ``K`` consecutive timesteps of the detect sweep in one launch: ``log_onsets`` (K, rows, T),
        already ``log(clip(.))``; returns / fills three (K, n_samples) series.  Every step's result
        is what :meth:`detect` gives for it (``get("steps_per_launch")`` tells whether the kernels
        took the K steps in one launch or the call went step by step).
        """
        steps, rows, t_samples = (int(v) for v in log_onsets.shape)
        self._check_rows(rows)
        n = max(t_samples - int(fsmp) - int(lsmp), 0)
        if out is None:
            out = (np.zeros((steps, n)), np.zeros((steps, n)), np.zeros((steps, n), dtype=np.int64))
        po, dev_on = self._ptr(log_onsets, np.float64)
        pa, pb, pc, da = self._series(out, steps * n)
        total = self.n_nodes if n_nodes_total is None else int(n_nodes_total)
        _check(qmlib.qm_engine_detect_batch(self._h, po, dev_on, steps, t_samples, int(fsmp),
                                            int(lsmp), int(available), total, pa, pb, pc, da))
        return out

    def detect_partial(self, log_onsets, fsmp, lsmp, available, part):
        """``part`` = (max, idx, sum) device buffers of length n_samples."""
        rows, t_samples = (int(v) for v in log_onsets.shape)
        self._check_rows(rows)
        po, dev_on = self._ptr(log_onsets, np.float64)
        n = max(t_samples - int(fsmp) - int(lsmp), 0)
        (pm, dm), (pi, di), (ps, ds) = (self._ptr(part[0], np.float64, n),
                                        self._ptr(part[1], np.int64, n),
                                        self._ptr(part[2], np.float64, n))
        if not (dm and di and ds):
            raise ValueError("detect_partial writes device buffers: pass tensors on this GPU")
        _check(qmlib.qm_engine_detect_partial(
            self._h, po, dev_on, t_samples, int(fsmp), int(lsmp), int(available), pm, pi, ps))

    def finalize(self, part_max, part_idx, part_sum, n_sets, n_samples,
                 n_nodes_total, out=None):
        if out is None:
            out = (np.zeros(n_samples), np.zeros(n_samples),
                   np.zeros(n_samples, dtype=np.int64))
        pa, pb, pc, da = self._series(out, int(n_samples))
        need = int(n_sets) * int(n_samples)
        _check(qmlib.qm_engine_finalize(
            self._h, self._ptr(part_max, np.float64, need)[0],
            self._ptr(part_idx, np.int64, need)[0], self._ptr(part_sum, np.float64, need)[0],
            int(n_sets), int(n_samples), int(n_nodes_total), pa, pb, pc, da))
        return out

    def finalize_packed(self, packed, n_sets, n_samples, n_nodes_total, out=None):
        """``packed``: device float64 [n_sets][3][n_samples] (maxima, int64 index bits, sums) --
        the all-gathered partials of a sharded detect; returns the final series."""
        if out is None:
            out = (np.zeros(n_samples), np.zeros(n_samples),
                   np.zeros(n_samples, dtype=np.int64))
        pa, pb, pc, da = self._series(out, int(n_samples))
        pp, dev = self._ptr(packed, np.float64, 3 * int(n_sets) * int(n_samples))
        if not dev:
            raise ValueError("finalize_packed reads a device buffer")
        _check(qmlib.qm_engine_finalize_packed(self._h, pp, int(n_sets), int(n_samples),
                                               int(n_nodes_total), pa, pb, pc, da))
        return out

    def tie_partial(self, log_onsets, fsmp, lsmp, available, packed, n_sets, tie_packed):
        """``tie_rule = 1`` on a sharded detect: this engine's near-tie candidates of the step its last
        :meth:`detect_partial` computed, against the grid's maxima in ``packed`` (the gathered partials,
        device float64 [n_sets][3][n_samples]) -> ``tie_packed`` device float64 [2][n_samples] (bit
        patterns: largest correctly rounded exp, lowest global index reaching it)."""
        rows, t_samples = (int(v) for v in log_onsets.shape)
        self._check_rows(rows)
        po, dev_on = self._ptr(log_onsets, np.float64)
        n = max(t_samples - int(fsmp) - int(lsmp), 0)
        pp, dev = self._ptr(packed, np.float64, 3 * int(n_sets) * n)
        pt, dev_t = self._ptr(tie_packed, np.float64, 2 * n)
        if not (dev and dev_t):
            raise ValueError("tie_partial reads and writes device buffers")
        _check(qmlib.qm_engine_tie_partial(self._h, po, dev_on, t_samples, int(fsmp), int(lsmp),
                                           int(available), pp, int(n_sets), pt))

    def tie_fold(self, tie_gathered, n_sets, n_samples, idx):
        """The gathered ``[n_sets][2][n_samples]`` outcomes of :meth:`tie_partial` folded into the
        device index series ``idx`` (in place)."""
        pg, dev = self._ptr(tie_gathered, np.float64, 2 * int(n_sets) * int(n_samples))
        pi, dev_i = self._ptr(idx, np.int64, int(n_samples))
        if not (dev and dev_i):
            raise ValueError("tie_fold reads and writes device buffers")
        _check(qmlib.qm_engine_tie_fold(self._h, pg, int(n_sets), int(n_samples), pi))

    def migrate(self, log_onsets, fsmp, lsmp, available, map4d, scan_out=None,
                accumulate=False, n_nodes_total=None):
        rows, t_samples = (int(v) for v in log_onsets.shape)
        self._check_rows(rows)
        po, dev_on = self._ptr(log_onsets, np.float64)
        n = max(t_samples - int(fsmp) - int(lsmp), 0)
        pm, dev_map = self._ptr(map4d, np.float64, self.n_nodes * n)
        if scan_out is None:
            pa = pb = pc = _vp(None)
            da = 0
        else:
            pa, pb, pc, da = self._series(scan_out, n)
        total = self.n_nodes if n_nodes_total is None else int(n_nodes_total)
        _check(qmlib.qm_engine_migrate(
            self._h, po, dev_on, t_samples, int(fsmp), int(lsmp), int(available),
            total, pm, dev_map, 1 if accumulate else 0, pa, pb, pc, da))
        return map4d

    def marginal_map(self, log_onsets, fsmp, lsmp, available, first_sample, end_sample,
                     out=None, scan_out=None, n_nodes_total=None):
        """
        Sum over scanned samples ``[first_sample, end_sample)`` of every node's coalescence,
        shape ``grid`` -- ``np.sum(map4d[..., first:end], axis=-1)`` without the 4-D map.
        """
        rows, t_samples = (int(v) for v in log_onsets.shape)
        self._check_rows(rows)
        if out is None:
            out = np.zeros(self.grid, dtype=np.float64)
        po, dev_on = self._ptr(log_onsets, np.float64)
        pm, dev_map = self._ptr(out, np.float64, self.n_nodes)
        if scan_out is None:
            pa = pb = pc = _vp(None)
            da = 0
        else:
            pa, pb, pc, da = self._series(scan_out, max(t_samples - int(fsmp) - int(lsmp), 0))
        total = self.n_nodes if n_nodes_total is None else int(n_nodes_total)
        _check(qmlib.qm_engine_marginal(
            self._h, po, dev_on, t_samples, int(fsmp), int(lsmp), int(available), total,
            int(first_sample), int(end_sample), pm, dev_map, pa, pb, pc, da))
        return out

    def locate_fits(self, coa_map, node_spacing, sgm=0.8, cov_thresh=0.90, norm_out=None,
                    smoothed_out=None):
        """
        Device part of ``QuakeScan._calculate_location`` (scan.py:696-733) on a marginalised
        map ``coa_map`` (nx, ny, nz), host array or device tensor: normalisation, the two-pass
        Gaussian smoothing, the covariance moments and the two fit windows.  Returns a dict;
        ``norm_out`` / ``smoothed_out`` (both host or both device) receive the maps.
        """
        nx, ny, nz = (int(v) for v in coa_map.shape)
        pm, dev_map = self._ptr(coa_map, np.float64)
        outs = [o for o in (norm_out, smoothed_out) if o is not None]
        pn = ps = _vp(None)
        dev_out = 0
        if norm_out is not None:
            pn, dev_out = self._ptr(norm_out, np.float64)
        if smoothed_out is not None:
            ps, dev_s = self._ptr(smoothed_out, np.float64)
            if len(outs) == 2 and dev_s != dev_out:
                raise ValueError("norm_out and smoothed_out must both be host or both device")
            dev_out = dev_s
        spacing = (ctypes.c_double * 3)(*[float(v) for v in node_spacing])
        summary = (ctypes.c_double * 16)()
        gau = np.zeros((7, 7, 7))
        spl = np.zeros((5, 5, 5))
        dp = ctypes.POINTER(ctypes.c_double)
        _check(qmlib.qm_engine_locate_fits(
            self._h, pm, dev_map, nx, ny, nz, float(sgm), float(cov_thresh), spacing, pn, ps,
            dev_out, summary, gau.ctypes.data_as(dp), spl.ctypes.data_as(dp)))
        sm = np.array(summary[:])
        cov = np.array([[sm[8], sm[11], sm[12]], [sm[11], sm[9], sm[13]],
                        [sm[12], sm[13], sm[10]]])
        return {"map_max": sm[0],
                "peak": np.array(np.unravel_index(int(sm[1]), (nx, ny, nz))),
                "smoothed_mean": sm[2],
                "smoothed_peak": np.array(np.unravel_index(int(sm[3]), (nx, ny, nz))),
                "weight": sm[4], "expectation": sm[5:8].copy(), "covariance": cov,
                "pass_maxima": sm[14:16].copy(), "gaussian_window": gau,
                "spline_window": spl}

    def rbf_peak(self, weights, upscale=10):
        """
        First maximum of the cubic radial-basis interpolant with the given ``weights`` (n, n, n)
        on the ``upscale``-times finer grid (``_splineloc``'s refinement, scan.py:777-812),
        evaluated on the GPU.  Returns ``(value, (i, j, k))`` -- indices into the fine grid of
        ``(n - 1) * upscale + 1`` points per axis.
        """
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim != 3 or not (w.shape[0] == w.shape[1] == w.shape[2]):
            raise ValueError("weights must be a cube")
        n = int(w.shape[0])
        value, index = ctypes.c_double(), c_int64()
        _check(qmlib.qm_engine_rbf_peak(self._h, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        n, int(upscale), ctypes.byref(value), ctypes.byref(index)))
        m = (n - 1) * int(upscale) + 1
        return float(value.value), tuple(int(v) for v in np.unravel_index(int(index.value), (m, m, m)))

    def onsets(self, signals, trace_row, nsta, nlta, transform="energy", position="classic",
               taper_pad=-1, min_onset_value=0.4, raw_out=None, log_out=None):
        """
        Onset stage on the GPU (``STALTAOnset._onset`` + the clip/log of ``lib.migrate``): from
        pre-processed component waveforms ``signals`` (n_traces, T) to the raw onset rows and
        ``log(clip(onset, 0.01))`` rows, shape (n_rows, T).  Returns ``(raw, logged)``.

        ``transform``: the reference's four ``signal_transform`` values (stalta.py:515-521).
        ``"env"`` / ``"env_squared"`` take the envelope ``|hilbert(x)|`` first -- an upstream
        transform like the filters, done here with the reference's own ``scipy.signal.hilbert``
        call on host signals (pass the envelope yourself with ``"abs"`` / ``"energy"`` for
        device-resident signals) -- the STA/LTA and everything after it run on the GPU.
        ``position``: ``"classic"``, ``"centred"`` or ``"recursive"`` (onsetlib.c:126-148).
        """
        if transform in ("env", "env_squared"):
            if not isinstance(signals, np.ndarray):
                raise ValueError("env transforms of device-resident signals: pass the envelope "
                                 "|hilbert(x)| with transform='abs' / 'energy'")
            from scipy.signal import hilbert

            signals = np.ascontiguousarray(np.abs(hilbert(signals, axis=-1)))
            transform = "abs" if transform == "env" else "energy"
        n_traces, t_samples = (int(v) for v in signals.shape)
        trace_row = np.ascontiguousarray(trace_row, dtype=np.int32)
        nsta = np.ascontiguousarray(nsta, dtype=np.int32)
        nlta = np.ascontiguousarray(nlta, dtype=np.int32)
        n_rows = len(nsta)
        ps, dev_s = self._ptr(signals, np.float64)
        if log_out is None:
            log_out = np.zeros((n_rows, t_samples))
        if raw_out is None and isinstance(log_out, np.ndarray):
            raw_out = np.zeros((n_rows, t_samples))
        pl, dev_o = self._ptr(log_out, np.float64, n_rows * t_samples)
        pr = (self._ptr(raw_out, np.float64, n_rows * t_samples)[0] if raw_out is not None
              else _vp(None))
        _check(qmlib.qm_engine_onsets(
            self._h, ps, dev_s, n_traces, t_samples, trace_row, n_rows, nsta, nlta,
            {"energy": 0, "abs": 1}[transform],
            {"classic": 0, "centred": 1, "recursive": 2}[position],
            int(taper_pad), float(min_onset_value), pr, pl, dev_o))
        return raw_out, log_out

    def preprocess(self, signals, trace_filter, sos, taper=(None, None), detrend=True, zero_phase=True,
                   out=None):
        """
        Pre-processing on the GPU, the step before :meth:`onsets` (what ``STALTAOnset.calculate_onsets`` does to
        every gap-free, full-timespan component trace before the STA/LTA, stalta.py:137-211, :353-489): linear
        detrend and demean, taper, band-pass as a cascade of second-order sections -- forward, and with
        ``zero_phase`` backward as well.  The filter's bits are ``scipy.signal.sosfilt``'s.

        ``signals`` (n_traces, T), host or device like :meth:`onsets`; ``trace_filter`` (n_traces,) picks each
        trace's filter out of ``sos`` (n_filters, n_sections, 6), SciPy's layout with ``a0 == 1``
        (:func:`quakemigrate_amd.preprocess.butter_bandpass_sos`); ``taper = (left, right)``: the weights of
        the first and last samples (:func:`quakemigrate_amd.preprocess.cosine_taper_sides`), either may be
        ``None``.  Returns the filtered traces (``out``, host or device, or a new host array).
        """
        n_traces, t_samples = (int(v) for v in signals.shape)
        trace_filter = np.ascontiguousarray(trace_filter, dtype=np.int32)
        if trace_filter.shape != (n_traces,):
            raise ValueError(f"trace_filter of shape {trace_filter.shape} for {n_traces} traces")
        sos = _sections(sos)
        left, right = (np.ascontiguousarray([] if w is None else w, dtype=np.float64).reshape(-1) for w in taper)
        ps, dev_s = self._ptr(signals, np.float64)
        if out is None:
            out = np.zeros((n_traces, t_samples))
        po, dev_o = self._ptr(out, np.float64, n_traces * t_samples)
        _check(qmlib.qm_engine_preprocess(
            self._h, ps, dev_s, n_traces, t_samples, trace_filter, sos.reshape(-1), int(sos.shape[0]),
            int(sos.shape[1]), 1 if detrend else 0, left, len(left), right, len(right), 1 if zero_phase else 0,
            po, dev_o))
        return out

    def preprocess_segments(self, signals, trace_filter, sos, records, taper_weights, detrend=True, zero_phase=True,
                            second_taper=True, fill_value=None, out=None):
        """
        Pre-processing of gappy traces on the GPU (what ``STALTAOnset.calculate_onsets`` does with ``allow_gaps=True``
        or ``full_timespan=False``, stalta.py:137-211, :442-461; include/qmhip.h: ``qm_engine_preprocess_segments``):
        every segment detrended, tapered and filtered on its own, tapered again behind the filter (``second_taper``),
        gaps and the window's ends set to ``fill_value`` (``None``: the reference's ``sqrt(finfo(float).tiny)``).

        ``signals`` (n_traces, T) in window layout, host or device like :meth:`preprocess`; ``trace_filter`` and
        ``sos`` as there; ``records`` (n_segments, 8) int64 and ``taper_weights`` from
        :func:`quakemigrate_amd.preprocess.plan_segments`.  Returns the filtered traces (``out``, host or device -- it
        may be ``signals`` on the device --, or a new host array).
        """
        from quakemigrate_amd.preprocess import GAP_FILL_VALUE

        n_traces, t_samples = (int(v) for v in signals.shape)
        trace_filter = np.ascontiguousarray(trace_filter, dtype=np.int32)
        if trace_filter.shape != (n_traces,):
            raise ValueError(f"trace_filter of shape {trace_filter.shape} for {n_traces} traces")
        sos = _sections(sos)
        records, weights = segment_arrays(records, taper_weights)
        ps, dev_s = self._ptr(signals, np.float64)
        if out is None:
            out = np.zeros((n_traces, t_samples))
        po, dev_o = self._ptr(out, np.float64, n_traces * t_samples)
        _check(qmlib.qm_engine_preprocess_segments(
            self._h, ps, dev_s, n_traces, t_samples, trace_filter, sos.reshape(-1), int(sos.shape[0]),
            int(sos.shape[1]), 1 if detrend else 0, 1 if zero_phase else 0, records.reshape(-1), len(records), weights,
            len(weights), 1 if second_taper else 0, GAP_FILL_VALUE if fill_value is None else float(fill_value),
            po, dev_o))
        return out

    def resample(self, raw, stage, out=None, t_samples=None):
        """
        Resampling on the GPU, the step before :meth:`preprocess` (the reference's ``util.resample``, util.py:404-604;
        include/qmhip.h: ``qm_engine_resample``): raw component traces in, each at its own rate and length, the
        (n_traces, t_samples) float64 traces at the scan rate out.

        ``raw``: a list of 1-D arrays, one per trace, or the packed 1-D array the records' offsets point into -- a
        host array or a torch device tensor --, int32 or float64.  ``stage``: a
        :class:`quakemigrate_amd.preprocess.ResampleStage` (then ``t_samples`` or ``out`` says how long the windows
        are) or the dict its ``arrays(t_samples)`` returns.  Returns the traces (``out``, host or device, or a new
        host array).
        """
        if t_samples is None and out is not None and hasattr(stage, "arrays"):
            t_samples = int(out.shape[-1])
        records, sos, table, weights, detrend, t_samples, total = resample_arrays(stage, t_samples)
        n_traces = len(records)
        if hasattr(raw, "data_ptr"):
            names = {"torch.int32": 0, "torch.float64": 1}
            if str(raw.dtype) not in names:
                raise TypeError(f"raw samples of type {raw.dtype}: int32 or float64")
            code = names[str(raw.dtype)]
            pr, dev_r = self._ptr(raw, None, total)
        else:
            raw = pack_raw(raw, records, total)
            code = RAW_DTYPES[raw.dtype]
            pr, dev_r = _host(raw), 0
        if out is None:
            out = np.zeros((n_traces, t_samples))
        po, dev_o = self._ptr(out, np.float64, n_traces * t_samples)
        _check(qmlib.qm_engine_resample(
            self._h, pr, code, dev_r, total, n_traces, records.reshape(-1), sos.reshape(-1), int(sos.shape[0]),
            int(sos.shape[1]), detrend, table.reshape(-1), len(table), weights, len(weights), t_samples, po, dev_o))
        return out

    def pick_phases(self, onsets, windows, row_group, sampling_rate, halfwidth, threshold_mode=0,
                    mad_multiplier=8.0, thresholds=None):
        """
        Phase picks on the GPU, the step after the location (``GaussianPicker``'s threshold, peak and Gaussian fit
        per onset row, gaussian.py:319-560; include/qmhip.h: ``qm_engine_pick_phases``).  ``onsets`` (n_rows, T):
        the un-logged onset functions, host array or device tensor like :meth:`preprocess`; ``windows``
        (n_rows, 3) int32 ``[lo, arrival, hi]`` (:func:`quakemigrate_amd.picks.pick_windows`); ``row_group``
        (n_rows,): the rows of one station share a value; ``halfwidth`` (n_rows,) in samples.
        ``threshold_mode`` 0: median + ``mad_multiplier`` x MAD of the row outside its station's windows; 1: the
        given ``thresholds`` (n_rows,).  Returns ``(picks (n_rows, 8) float64, status (n_rows,) int32)``: columns
        threshold, a, b (s), |c| (s), c, f0, f1, iterations; status 0 is a pick.
        """
        n_rows, t_samples = (int(v) for v in onsets.shape)
        po, dev = self._ptr(onsets, np.float64, n_rows * t_samples)
        windows = np.ascontiguousarray(windows, dtype=np.int32)
        row_group = np.ascontiguousarray(row_group, dtype=np.int32)
        halfwidth = np.ascontiguousarray(halfwidth, dtype=np.float64)
        if windows.shape != (n_rows, 3):
            raise ValueError(f"windows of shape {windows.shape} for {n_rows} rows: (n_rows, 3) expected")
        for name, a in (("row_group", row_group), ("halfwidth", halfwidth)):
            if a.shape != (n_rows,):
                raise ValueError(f"{name} of shape {a.shape} for {n_rows} rows")
        pt = _vp(None)
        if thresholds is not None:
            thresholds = np.ascontiguousarray(thresholds, dtype=np.float64)
            if thresholds.shape != (n_rows,):
                raise ValueError(f"thresholds of shape {thresholds.shape} for {n_rows} rows")
            pt = _host(thresholds)
        picks, status = np.zeros((n_rows, 8)), np.zeros(n_rows, dtype=np.int32)
        _check(qmlib.qm_engine_pick_phases(
            self._h, po, dev, n_rows, t_samples, _host(windows), _host(row_group), float(sampling_rate),
            _host(halfwidth), int(threshold_mode), float(mad_multiplier), pt, _host(picks), _host(status)))
        return picks, status

    AVERAGE_METHODS = {"RMS": 0, "STD": 1}

    def measure_amplitudes(self, traces, trace_records, window_records, sos=None, taper_table=None,
                           taper_weights=None, detrend_windows=True, average_method="RMS", prominence_multiplier=0.0,
                           want_filtered=False):
        """
        Local-magnitude amplitudes on the GPU, the step after the picks (``Amplitude.get_amplitudes``' filter, window
        detrend, ``find_peaks``, peak/trough pairing and average per component trace, amplitude.py:174-371;
        include/qmhip.h: ``qm_engine_measure_amplitudes``).  ``traces``: the packed 1-D float64 samples of every
        trace, host array or device tensor like :meth:`pick_phases`, or a list of 1-D arrays that is packed here in
        the records' order; ``trace_records`` (n_traces, 4) int64 ``[offset, n, filter (-1: none), taper (-1:
        none)]`` -- a trace with a filter shares no sample with another trace --; ``window_records`` (n_windows, 4) int64 ``[trace, lo, hi, kind (0 noise, 1 signal)]``; ``sos``
        (n_filters, n_sections, 6), SciPy's layout with ``a0 == 1``; ``taper_table`` (n_tapers, 2) int32 and
        ``taper_weights`` as :meth:`resample` takes them.  Returns ``(values (n_windows, 4) float64, index
        (n_windows, 4) int32)`` -- values: full peak-to-trough, average, max|y|, 0; index: status, peak sample, trough
        sample, peaks kept -- and with ``want_filtered`` the packed traces as the windows were cut from them as a
        third entry.
        """
        trace_records = np.ascontiguousarray(trace_records, dtype=np.int64)
        window_records = np.ascontiguousarray(window_records, dtype=np.int64)
        if trace_records.ndim != 2 or trace_records.shape[1] != 4:
            raise ValueError(f"trace_records of shape {trace_records.shape}: (n_traces, 4) expected")
        if window_records.ndim != 2 or window_records.shape[1] != 4:
            raise ValueError(f"window_records of shape {window_records.shape}: (n_windows, 4) expected")
        if average_method not in self.AVERAGE_METHODS:
            raise ValueError(f"average_method must be 'RMS' or 'STD', got {average_method!r} (the envelope average "
                             "stays on the host: quakemigrate_amd.amplitudes)")
        if isinstance(traces, (list, tuple)):
            total = int(max((r[0] + r[1] for r in trace_records), default=0))

            def refuse(i, x, fits):
                if not fits:
                    raise ValueError(f"a trace of {len(x)} samples where its record says {trace_records[i][1]}")

            traces = _pack_by_records(traces, trace_records[:, 0], trace_records[:, 1], total, np.float64, refuse)
        total = int(traces.numel() if hasattr(traces, "numel") else traces.size)
        pt, dev = self._ptr(traces, np.float64)
        sos = _sections(np.zeros((0, 1, 6)) if sos is None else sos)
        table, weights = _taper_arrays(taper_table, taper_weights)
        n_windows = len(window_records)
        values, index = np.zeros((n_windows, 4)), np.zeros((n_windows, 4), dtype=np.int32)
        filtered = np.zeros(total) if want_filtered else None
        _check(qmlib.qm_engine_measure_amplitudes(
            self._h, pt, dev, total, len(trace_records), trace_records.reshape(-1), sos.reshape(-1), int(sos.shape[0]),
            int(sos.shape[1]), table.reshape(-1), len(table), weights, len(weights), n_windows,
            window_records.reshape(-1), 1 if detrend_windows else 0, self.AVERAGE_METHODS[average_method],
            float(prominence_multiplier), _host(values), _host(index),
            _host(filtered) if want_filtered else _vp(None)))
        return (values, index, filtered) if want_filtered else (values, index)

    # -- travel-time tables (create_lut.py's compute_traveltimes on the GPU) ----
    @staticmethod
    def _tt_grid(ll_corner, node_spacing, node_count):
        ll = np.ascontiguousarray(ll_corner, dtype=np.float64).reshape(-1)
        sp = np.ascontiguousarray(node_spacing, dtype=np.float64).reshape(-1)
        nc = np.ascontiguousarray(node_count, dtype=np.int32).reshape(-1)
        if not len(ll) == len(sp) == len(nc) == 3:
            raise ValueError("ll_corner, node_spacing and node_count have three entries each")
        return ll, sp, nc

    def _tt_out(self, shape, device, dtype=np.float64):
        """A new output array: a torch tensor on this engine's GPU (``device``) or a NumPy array."""
        if not device:
            return np.zeros(shape, dtype=dtype)
        import torch

        where = torch.device("cuda", self.device)
        out = torch.empty(shape, dtype=torch.float64 if dtype == np.float64 else torch.int32, device=where)
        torch.cuda.synchronize(where)                   # (the allocator's stream is not the engine's)
        return out

    def traveltimes_homogeneous(self, ll_corner, node_spacing, node_count, stations_xyz, velocities, device=False):
        """
        Travel-time grids of a homogeneous medium (``_compute_homogeneous``, create_lut.py:241-265; include/qmhip.h:
        ``qm_engine_tt_homogeneous``).  One row per entry of ``stations_xyz`` (n_rows, 3) and ``velocities``
        (n_rows,).  Returns (n_rows, nx, ny, nz) float64 seconds: a NumPy array, or with ``device`` a torch tensor on
        this engine's GPU.
        """
        ll, sp, nc = self._tt_grid(ll_corner, node_spacing, node_count)
        xyz = np.ascontiguousarray(stations_xyz, dtype=np.float64).reshape(-1, 3)
        vel = np.ascontiguousarray(velocities, dtype=np.float64).reshape(-1)
        if len(vel) != len(xyz):
            raise ValueError(f"{len(xyz)} stations, {len(vel)} velocities: one row each")
        rows = np.ascontiguousarray(np.column_stack([xyz, vel]))
        out = self._tt_out((len(rows),) + tuple(int(n) for n in nc), device)
        p, dev = self._ptr(out, np.float64)
        _check(qmlib.qm_engine_tt_homogeneous(self._h, ll, sp, nc, len(rows), rows.reshape(-1), p, dev))
        return out

    def traveltime_sections(self, slowness, source_depth, nr, h, source_slowness=None, tol=2.0 ** -40, max_iters=64,
                            force_scratch=False, device=False):
        """
        Eikonal travel-time sections of 1-D models (include/qmhip.h: ``qm_engine_tt_sections``).  ``slowness``
        (n_sections, nz): per depth row of spacing ``h``; ``source_depth`` (n_sections,): below the first row;
        ``source_slowness``: at the source, by default interpolated linearly between the rows.  Returns
        ``(T (n_sections, nr, nz), rounds, status)``, NumPy arrays or with ``device`` torch tensors on this
        engine's GPU.  A section that ``max_iters`` rounds do not settle raises.
        """
        slowness = np.ascontiguousarray(np.atleast_2d(slowness), dtype=np.float64)
        n_sec, nz = (int(v) for v in slowness.shape)
        zs = np.ascontiguousarray(source_depth, dtype=np.float64).reshape(-1)
        if len(zs) != n_sec:
            raise ValueError(f"{n_sec} sections, {len(zs)} source depths")
        if source_slowness is None:
            depth = np.arange(nz) * float(h)
            source_slowness = [np.interp(zs[s], depth, slowness[s]) for s in range(n_sec)]
        s0 = np.ascontiguousarray(source_slowness, dtype=np.float64).reshape(-1)
        if len(s0) != n_sec:
            raise ValueError(f"{n_sec} sections, {len(s0)} source slownesses")
        source = np.ascontiguousarray(np.column_stack([zs, s0]))
        T = self._tt_out((n_sec, int(nr), nz), device)
        rounds, status = self._tt_out(n_sec, device, np.int32), self._tt_out(n_sec, device, np.int32)
        (pt, dev), (pr, _), (ps, _) = self._ptr(T, np.float64), self._ptr(rounds, np.int32), self._ptr(status, np.int32)
        _check(qmlib.qm_engine_tt_sections(self._h, n_sec, int(nr), nz, float(h), slowness.reshape(-1),
                                           source.reshape(-1), float(tol), int(max_iters), 1 if force_scratch else 0,
                                           pt, pr, ps, dev))
        return T, rounds, status

    def sweep_sections(self, sections, ll_corner, node_spacing, node_count, stations_xy, row_section, origins, h,
                       device=False):
        """
        (distance, depth) sections swept round their stations over a 3-D grid by the reference's bilinear rule
        (create_lut.py:471-474, 504-513, 746-762; include/qmhip.h: ``qm_engine_tt_sweep``).  ``sections``
        (n_sections, nr, nz): a NumPy array -- a caller's own, NonLinLoc's for instance -- or a tensor on this engine's
        GPU (:meth:`traveltime_sections`'); per row ``stations_xy`` (n_rows, 2), ``row_section`` (n_rows,) and
        ``origins`` (n_rows, 2), the section's ``(x0, z0)``; ``h``: the sections' spacing.  Returns (n_rows, nx, ny, nz)
        like :meth:`traveltimes_homogeneous`.  A node outside its section raises.
        """
        ll, sp, nc = self._tt_grid(ll_corner, node_spacing, node_count)
        if not hasattr(sections, "data_ptr"):           # (anything but a tensor: an array, nested lists)
            sections = np.ascontiguousarray(sections, dtype=np.float64)
        if len(sections.shape) != 3:
            raise ValueError(f"sections of shape {tuple(sections.shape)}: (n_sections, nr, nz) expected")
        n_sec, nr, nz = (int(v) for v in sections.shape)
        psec, dev_sec = self._ptr(sections, np.float64)
        xy = np.ascontiguousarray(stations_xy, dtype=np.float64).reshape(-1, 2)
        org = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 2)
        row_section = np.ascontiguousarray(row_section, dtype=np.int32).reshape(-1)
        if not len(xy) == len(org) == len(row_section):
            raise ValueError(f"{len(xy)} stations, {len(org)} origins, {len(row_section)} section indices: one row each")
        rows = np.ascontiguousarray(np.column_stack([xy, org]))
        out = self._tt_out((len(rows),) + tuple(int(n) for n in nc), device)
        p, dev = self._ptr(out, np.float64)
        _check(qmlib.qm_engine_tt_sweep(self._h, ll, sp, nc, len(rows), rows.reshape(-1), row_section, psec, dev_sec,
                                        n_sec, nr, nz, float(h), p, dev))
        return out

    def traveltimes_eikonal3d(self, ll_corner, node_spacing, node_count, sources_xyz, source_slowness, slowness,
                              row_model, tol=2.0 ** -40, max_iters=64, device=True):
        """
        Eikonal travel-time grids of 3-D slowness volumes, solved on the grid's own nodes (include/qmhip.h:
        ``qm_engine_tt_eikonal3d``): a first-order factored sweep, one solve per row.  ``sources_xyz`` (n_rows, 3):
        anywhere inside the grid, not snapped to a node; ``source_slowness`` (n_rows,): at the source; ``slowness``
        (n_models, nx, ny, nz) -- a single (nx, ny, nz) volume will do --: a NumPy array or a tensor on this engine's
        GPU; ``row_model`` (n_rows,): the row's volume.  Returns ``(grids (n_rows, nx, ny, nz), rounds, status)``: the
        grids float64 seconds, with ``device`` a torch tensor on this engine's GPU, else a NumPy array; ``rounds`` and
        ``status`` NumPy int32 arrays.  A row that ``max_iters`` rounds do not settle raises.
        """
        ll, sp, nc = self._tt_grid(ll_corner, node_spacing, node_count)
        shape = tuple(int(n) for n in nc)
        if not hasattr(slowness, "data_ptr"):
            slowness = np.ascontiguousarray(slowness, dtype=np.float64)
        if tuple(slowness.shape) == shape:
            slowness = slowness.reshape((1,) + shape)
        if len(slowness.shape) != 4 or tuple(slowness.shape[1:]) != shape:
            raise ValueError(f"slowness of shape {tuple(slowness.shape)}: (n_models,) + {shape} expected")
        pslow, dev_slow = self._ptr(slowness, np.float64)
        if dev_slow and hasattr(slowness, "is_cuda"):
            import torch

            torch.cuda.synchronize(slowness.device)     # (whatever wrote the volumes ran on torch's stream, not the engine's)
        xyz = np.ascontiguousarray(sources_xyz, dtype=np.float64).reshape(-1, 3)
        s0 = np.ascontiguousarray(source_slowness, dtype=np.float64).reshape(-1)
        row_model = np.ascontiguousarray(row_model, dtype=np.int32).reshape(-1)
        if not len(xyz) == len(s0) == len(row_model):
            raise ValueError(f"{len(xyz)} sources, {len(s0)} source slownesses, {len(row_model)} model indices: one "
                             "row each")
        rows = np.ascontiguousarray(np.column_stack([xyz, s0]))
        out = self._tt_out((len(rows),) + shape, device)
        rounds, status = np.zeros(len(rows), dtype=np.int32), np.zeros(len(rows), dtype=np.int32)
        p, dev = self._ptr(out, np.float64)
        _check(qmlib.qm_engine_tt_eikonal3d(self._h, ll, sp, nc, len(rows), rows.reshape(-1), row_model,
                                            int(slowness.shape[0]), pslow, dev_slow, float(tol), int(max_iters), p, dev,
                                            rounds, status))
        return out, rounds, status

    TRIGGER_METHODS = {"static": 0, "mad": 1, "median_ratio": 2}

    def trigger_series(self, coa, coa_n, period_ns, mw_ns, mei_ns, trigger_on=0, method="static", value=1.5,
                       chunk_samples=1, weights=None, max_events=65536, want_candidates=False):
        """
        The trigger stage on the GPU, the step between detect and locate (``Trigger._trigger_batch``'s smoothing,
        threshold, candidates and merge, trigger.py:318-638; include/qmhip.h: ``qm_engine_trigger``).  ``coa``,
        ``coa_n`` (n,): float64 host arrays, contiguous, already cut to the batch and its pads -- or both tensors on this
        engine's GPU (``scanmseed_decode(..., device=True)``'s: ``qm_engine_trigger_resident``, no host copy); times in int64
        nanoseconds from the first sample.  ``trigger_on`` 0: COA, 1: COA_N; ``method`` "static" (``value``: the
        threshold), "mad" or "median_ratio" (``value``: the multiplier, per chunk of ``chunk_samples``); ``weights``
        (2 r + 1,): the Gaussian kernel of the smoothing, None: none.  Returns a dict: ``n_candidates``, ``n_events``,
        ``events_i`` (n_events, 4) int64 [peak index, MinTime, MaxTime, members], ``events_f`` (n_events, 3) [TRIG_COA,
        COA, COA_NORM], ``thresholds`` (chunks,), ``smoothed`` (2, n) or None and -- ``want_candidates`` --
        ``candidates`` (n_candidates, 5) int64 [f, l, p, MinTime, MaxTime].  More than ``max_events`` events: refused,
        the message names the number.
        """
        resident = all(hasattr(a, "data_ptr") and a.is_cuda for a in (coa, coa_n))
        for name, a in (("coa", coa), ("coa_n", coa_n)):
            if resident:
                # (device tensors, e.g. scanmseed_decode's with device=True: qm_engine_trigger_resident, no host copy)
                if a.dim() != 1:
                    raise ValueError(f"{name} must be one-dimensional and contiguous")
                self._ptr(a, np.float64)
                continue
            if not isinstance(a, np.ndarray):
                raise TypeError(f"{name}: a NumPy array expected, got {type(a).__name__}")
            if a.dtype != np.float64:
                raise TypeError(f"{name}: expected float64, got {a.dtype}")
            if a.ndim != 1 or not a.flags["C_CONTIGUOUS"]:
                raise ValueError(f"{name} must be one-dimensional and C-contiguous")
        if coa_n.shape != coa.shape:
            raise ValueError(f"coa_n of shape {coa_n.shape} for coa of shape {coa.shape}")
        if method not in self.TRIGGER_METHODS:
            raise ValueError(f"method must be one of {sorted(self.TRIGGER_METHODS)}, got {method!r}")
        n, code = int(coa.shape[0]), self.TRIGGER_METHODS[method]
        par = TriggerParams(int(trigger_on), code, float(value), int(chunk_samples), 0, 0, _vp(None), int(period_ns),
                            int(mw_ns), int(mei_ns))
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64)
            if weights.ndim != 1 or weights.size % 2 != 1:
                raise ValueError(f"weights of shape {weights.shape}: an odd number (2 r + 1) expected")
            par.smooth_radius, par.smooth_weights = weights.size // 2, _host(weights)
        # one threshold per chunk (a chunk longer than the series is the series); what the call refuses gets one slot
        chunks = -(-n // min(int(chunk_samples), n)) if code != 0 and chunk_samples >= 1 and n >= 1 else 1
        max_events = int(max_events)
        events_i = np.zeros((max(max_events, 0), 4), dtype=np.int64)
        events_f = np.zeros((max(max_events, 0), 3))
        thresholds = np.zeros(max(chunks, 1))
        smoothed = np.zeros((2, n)) if weights is not None else None
        room = (n + 1) // 2 if want_candidates else 0
        candidates = np.zeros((room, 5), dtype=np.int64) if want_candidates else None
        nc, ne = c_int64(0), c_int64(0)
        call = qmlib.qm_engine_trigger_resident if resident else qmlib.qm_engine_trigger
        p_coa, p_coa_n = (_vp(coa.data_ptr()), _vp(coa_n.data_ptr())) if resident else (_host(coa), _host(coa_n))
        _check(call(
            self._h, p_coa, p_coa_n, n, ctypes.byref(par), max_events, ctypes.byref(nc), ctypes.byref(ne),
            _host(events_i), _host(events_f), _host(thresholds), _host(smoothed) if smoothed is not None else _vp(None),
            _host(candidates) if want_candidates else _vp(None), room))
        out = {"n_candidates": int(nc.value), "n_events": int(ne.value), "events_i": events_i[:ne.value].copy(),
               "events_f": events_f[:ne.value].copy(), "thresholds": thresholds, "smoothed": smoothed}
        if want_candidates:
            out["candidates"] = candidates[:nc.value].copy()
        return out

    SCANMSEED_RECLEN = 4096
    SCANMSEED_RECORD_WORDS = 943            # data words of a record: a record holds at least that many samples

    def scanmseed_encode(self, series, factors=None, clips=None):
        """
        The STEIM2 records of a ``.scanmseed`` file's five channels on the GPU (include/qmhip.h:
        ``qm_engine_scanmseed_encode``).  ``series`` (5, n): COA, COA_N, X, Y, Z -- a NumPy array or a tensor on this
        engine's GPU; int32: already quantised; float64: quantised on the device as ``scanmseed.quantise`` does, with
        ``factors`` (5,) and ``clips`` (5,), ``inf`` or ``None`` where a channel has no clip.  Returns a dict:
        ``n_records`` (5,) int64; ``records`` (sum, 4096) uint8, channel after channel, the 64 header bytes zero;
        ``rec_first``, ``rec_count`` (sum,) int32: every record's first sample index and sample count.
        """
        on_device = hasattr(series, "data_ptr")
        if not on_device and not isinstance(series, np.ndarray):
            raise TypeError(f"series: a NumPy array or a device tensor expected, got {type(series).__name__}")
        shape = tuple(series.shape)
        if len(shape) != 2 or shape[0] != 5:
            raise ValueError(f"series of shape {shape}: (5, n) expected")
        kind = str(series.dtype).replace("torch.", "")
        if kind not in ("int32", "float64"):
            raise TypeError(f"series: expected int32 or float64, got {series.dtype}")
        is_float = kind == "float64"
        n = int(shape[1])
        if n < 1:
            raise ValueError("series holds no samples")
        ps, dev = self._ptr(series, np.float64 if is_float else np.int32)
        if on_device and not dev:
            raise ValueError("series: a tensor on this engine's GPU expected (pass host data as a NumPy array)")
        if on_device:
            import torch

            torch.cuda.synchronize(series.device)   # (what filled the tensor ran on a stream that is not the engine's)
        pf = pc = _vp(None)
        if is_float:
            if factors is None:
                raise ValueError("float64 series need factors")
            factors = np.ascontiguousarray(factors, dtype=np.float64)
            clips = np.ascontiguousarray([np.inf if c is None else c for c in (clips if clips is not None else [None] * 5)],
                                         dtype=np.float64)
            if factors.shape != (5,) or clips.shape != (5,):
                raise ValueError(f"factors of shape {factors.shape}, clips of shape {clips.shape}: (5,) expected")
            pf, pc = _host(factors), _host(clips)
        room = 5 * -(-n // self.SCANMSEED_RECORD_WORDS)
        records = np.empty((room, self.SCANMSEED_RECLEN), dtype=np.uint8)
        rec_first, rec_count = np.empty(room, dtype=np.int32), np.empty(room, dtype=np.int32)
        n_records = np.zeros(5, dtype=np.int64)
        _check(qmlib.qm_engine_scanmseed_encode(self._h, ps, 1 if is_float else 0, dev, n, pf, pc, room,
                                                _host(n_records), _host(records), _host(rec_first), _host(rec_count)))
        total = int(n_records.sum())
        return {"n_records": n_records, "records": records[:total], "rec_first": rec_first[:total],
                "rec_count": rec_count[:total]}

    def scanmseed_decode(self, records, rec_samples, rec_offset, n_total, rec_factor=None, device=False):
        """
        The samples of STEIM2 records on the GPU (include/qmhip.h: ``qm_engine_scanmseed_decode``).  ``records``
        (n_records, 4096) uint8: whole records, payload at byte 64; ``rec_samples`` (n_records,): their headers' sample
        counts; ``rec_offset`` (n_records,): where each record's samples go in the output of ``n_total`` samples;
        ``rec_factor`` (n_records,): if given, the descaled float64 ``sample / factor`` is returned as well.  Returns
        ``(int32, float64 or None)``: NumPy arrays, or -- ``device=True`` -- tensors on this engine's GPU.
        """
        if not isinstance(records, np.ndarray):
            raise TypeError(f"records: a NumPy array expected, got {type(records).__name__}")
        if records.dtype != np.uint8:
            raise TypeError(f"records: expected uint8, got {records.dtype}")
        if records.ndim != 2 or records.shape[1] != self.SCANMSEED_RECLEN or not records.flags["C_CONTIGUOUS"]:
            raise ValueError(f"records of shape {records.shape}: (n_records, {self.SCANMSEED_RECLEN}), C-contiguous, "
                             f"expected")
        nrec = int(records.shape[0])
        rec_samples = np.ascontiguousarray(rec_samples, dtype=np.int32)
        rec_offset = np.ascontiguousarray(rec_offset, dtype=np.int64)
        if rec_samples.shape != (nrec,) or rec_offset.shape != (nrec,):
            raise ValueError(f"rec_samples of shape {rec_samples.shape}, rec_offset of shape {rec_offset.shape}: "
                             f"({nrec},) expected")
        want_f = rec_factor is not None
        if want_f:
            rec_factor = np.ascontiguousarray(rec_factor, dtype=np.float64)
            if rec_factor.shape != (nrec,):
                raise ValueError(f"rec_factor of shape {rec_factor.shape}: ({nrec},) expected")
        n_total = int(n_total)
        if n_total < 1:
            raise ValueError(f"n_total must be positive, got {n_total}")
        if device:
            import torch

            where = torch.device("cuda", self.device)
            out = torch.empty(n_total, dtype=torch.int32, device=where)
            out_f = torch.empty(n_total, dtype=torch.float64, device=where) if want_f else None
            torch.cuda.synchronize(where)           # (the allocator's stream is not the engine's)
            po, pof = _vp(out.data_ptr()), _vp(out_f.data_ptr()) if want_f else _vp(None)
        else:
            out = np.empty(n_total, dtype=np.int32)
            out_f = np.empty(n_total, dtype=np.float64) if want_f else None
            po, pof = _host(out), _host(out_f) if want_f else _vp(None)
        _check(qmlib.qm_engine_scanmseed_decode(self._h, _host(records), nrec, _host(rec_samples), _host(rec_offset),
                                                _host(rec_factor) if want_f else _vp(None), n_total, po, pof,
                                                1 if device else 0))
        return out, out_f

    def find_max_coa(self, map4d, n_samples, n_nodes, out=None):
        if out is None:
            out = (np.zeros(n_samples), np.zeros(n_samples),
                   np.zeros(n_samples, dtype=np.int64))
        pm, dev_map = self._ptr(map4d, np.float64, int(n_samples) * int(n_nodes))
        pa, pb, pc, da = self._series(out, int(n_samples))
        _check(qmlib.qm_engine_find_max_coa(self._h, pm, dev_map, int(n_samples),
                                            int(n_nodes), pa, pb, pc, da))
        return out

    def _check_rows(self, rows):
        if self.n_rows is None:
            raise QMHipError("no travel-time table resident: call load_lut first")
        if rows != self.n_rows:
            raise ValueError(
                "Mismatch between number of stations for data and LUT, "
                f"{rows}:{self.n_rows}")


def group_plan(nx, ny, nz, n_parts, part):
    """Boxes ``(x0, x1, y0, y1, z0, z1)`` of part ``part`` of an engine group of ``n_parts`` over the grid
    (``qm_group_plan``: the column partition of ``distributed.column_boxes``, or balanced z-runs of a flat
    ``(1, 1, N)`` table).  Host code."""
    boxes = (c_int32 * 18)()
    n = c_int32()
    _check(qmlib.qm_group_plan(int(nx), int(ny), int(nz), int(n_parts), int(part), boxes, ctypes.byref(n)))
    return [tuple(int(v) for v in boxes[6 * k: 6 * k + 6]) for k in range(n.value)]


def _host_f64(x, what, count=None):
    if not isinstance(x, np.ndarray) or x.dtype != np.float64 or not x.flags["C_CONTIGUOUS"]:
        raise TypeError(f"{what}: an engine group takes C-contiguous float64 host arrays")
    if count is not None and x.size < count:
        raise ValueError(f"{what}: array holds {x.size} elements, {count} needed")
    return _host(x)


class EngineGroup:
    """
    One process driving a grid on several GPUs (``include/qmhip.h`` part 4): ``devices`` lists one part per
    entry, ids may repeat (``[0, 0]``: two parts on GPU 0); entry 0 is the lead device.  The surface of
    :class:`Engine` that :class:`quakemigrate_amd.scan.MigrationScan`, :func:`migrate` and :func:`find_max_coa`
    use, host arrays in and out.  ``locate_fits``, ``rbf_peak`` and ``onsets`` run on an :class:`Engine` of the
    lead device.  Not available: ``screen = 1``, on-device serving, ``detect_batch`` / the continuous pipeline.
    """

    def __init__(self, devices, **config):
        ids = [int(d) for d in devices]
        arr = (c_int32 * max(len(ids), 1))(*ids)
        h = _vp()
        _check(qmlib.qm_group_create(arr, len(ids), ctypes.byref(h)))
        self._h = h
        self.devices = ids
        self.device = ids[0]
        self._finalizer = weakref.finalize(self, qmlib.qm_group_destroy, h)
        self.lead = Engine(ids[0])
        self.grid = None
        self.n_rows = None
        self.node_offset = 0
        self.table_generation = 0
        self.grids_generation = 0
        for k, v in config.items():
            self.config(k, v)

    def close(self):
        self._finalizer()
        self.lead.close()

    def config(self, key, value):
        _check(qmlib.qm_group_config(self._h, key.encode(), int(value)))
        if key != "screen":                 # (the lead's own engine runs the locate rows only)
            self.lead.config(key, value)

    def get(self, key):
        v = c_int64()
        _check(qmlib.qm_group_get(self._h, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def synchronize(self):
        _check(qmlib.qm_group_synchronize(self._h))

    @property
    def n_parts(self):
        return len(self.devices)

    def part_info(self, part):
        """``dict(device, boxes, node_range, last_ms)`` of one part (``last_ms``: device time of its share of
        the last step, -1 if none)."""
        dev, n = c_int32(), c_int32()
        boxes = (c_int32 * 18)()
        rng = (c_int64 * 2)()
        ms = ctypes.c_double()
        _check(qmlib.qm_group_part_info(self._h, int(part), ctypes.byref(dev), boxes, ctypes.byref(n), rng,
                                        ctypes.byref(ms)))
        return {"device": int(dev.value),
                "boxes": [tuple(int(v) for v in boxes[6 * k: 6 * k + 6]) for k in range(n.value)],
                "node_range": (int(rng[0]), int(rng[1])), "last_ms": float(ms.value)}

    # -- table --------------------------------------------------------------
    def load_lut(self, traveltimes, node_offset=0, shape=None):
        if int(node_offset) != 0:
            raise ValueError("an engine group holds the whole grid (node_offset = 0)")
        if not isinstance(traveltimes, np.ndarray) or traveltimes.dtype != np.int32 \
                or not traveltimes.flags["C_CONTIGUOUS"]:
            raise TypeError("an engine group loads a C-contiguous int32 host table")
        shape = tuple(traveltimes.shape) if shape is None else tuple(shape)
        if len(shape) != 4:
            raise ValueError("traveltimes must have shape (nx, ny, nz, n_rows)")
        nx, ny, nz, rows = (int(v) for v in shape)
        _check(qmlib.qm_group_load_lut(self._h, _host(traveltimes), nx, ny, nz, rows))
        self.grid = (nx, ny, nz)
        self.n_rows = rows
        self.table_generation += 1

    def select_table(self, key, capacity=4):
        """As :meth:`Engine.select_table`, on every box engine of the group."""
        import hashlib

        k64 = int.from_bytes(hashlib.blake2b(repr(key).encode(), digest_size=8).digest(), "little")
        resident = c_int32()
        _check(qmlib.qm_group_table_select(self._h, k64, int(capacity), ctypes.byref(resident)))
        if resident.value:
            self.grid = (self.get("nx"), self.get("ny"), self.get("nz"))
            self.n_rows = self.get("n_rows")
        else:
            self.grid, self.n_rows = None, None
        self.table_generation += 1
        return bool(resident.value)

    def set_traveltime_grids(self, grids):
        raise ValueError("on-device table serving is not available on an engine group")

    def serve(self, *args, **kwargs):
        raise ValueError("on-device table serving is not available on an engine group")

    @property
    def lut_max(self):
        return self.get("lut_max")

    @property
    def n_nodes(self):
        return int(np.prod(self.grid))

    # -- steps --------------------------------------------------------------
    def _steps(self, log_onsets, fsmp, lsmp):
        rows, t_samples = (int(v) for v in log_onsets.shape)
        if self.n_rows is None:
            raise QMHipError("no travel-time table resident: call load_lut first")
        if rows != self.n_rows:
            raise ValueError("Mismatch between number of stations for data and LUT, "
                             f"{rows}:{self.n_rows}")
        return _host_f64(log_onsets, "log_onsets"), t_samples, max(t_samples - int(fsmp) - int(lsmp), 0)

    @staticmethod
    def _series_ptrs(out, n):
        if out is None:
            return _vp(None), _vp(None), _vp(None)
        a, b, c = out
        if not isinstance(c, np.ndarray) or c.dtype != np.int64 or not c.flags["C_CONTIGUOUS"] or c.size < n:
            raise TypeError("the index series must be a C-contiguous int64 host array")
        return _host_f64(a, "max_coa", n), _host_f64(b, "max_norm_coa", n), _host(c)

    def _total(self, n_nodes_total):
        if n_nodes_total is not None and int(n_nodes_total) != self.n_nodes:
            raise ValueError("an engine group normalises by its whole grid's node count")

    def detect(self, log_onsets, fsmp, lsmp, available, n_nodes_total=None, out=None):
        """Fused migrate + find_max_coa over the group (host arrays)."""
        self._total(n_nodes_total)
        po, t_samples, n = self._steps(log_onsets, fsmp, lsmp)
        if out is None:
            out = (np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64))
        pa, pb, pc = self._series_ptrs(out, n)
        _check(qmlib.qm_group_detect(self._h, po, t_samples, int(fsmp), int(lsmp), int(available), pa, pb, pc))
        return out

    def marginal_map(self, log_onsets, fsmp, lsmp, available, first_sample, end_sample, out=None,
                     scan_out=None, n_nodes_total=None):
        """As :meth:`Engine.marginal_map`: the whole grid's map, each part's flat range at its offset."""
        self._total(n_nodes_total)
        po, t_samples, n = self._steps(log_onsets, fsmp, lsmp)
        if out is None:
            out = np.zeros(self.grid, dtype=np.float64)
        pm = _host_f64(out, "out", self.n_nodes)
        pa, pb, pc = self._series_ptrs(scan_out, n)
        _check(qmlib.qm_group_marginal(self._h, po, t_samples, int(fsmp), int(lsmp), int(available),
                                       int(first_sample), int(end_sample), pm, pa, pb, pc))
        return out

    def migrate(self, log_onsets, fsmp, lsmp, available, map4d, scan_out=None, accumulate=False,
                n_nodes_total=None):
        self._total(n_nodes_total)
        po, t_samples, n = self._steps(log_onsets, fsmp, lsmp)
        pm = _host_f64(map4d, "map4d", self.n_nodes * n)
        pa, pb, pc = self._series_ptrs(scan_out, n)
        _check(qmlib.qm_group_migrate(self._h, po, t_samples, int(fsmp), int(lsmp), int(available), pm,
                                      1 if accumulate else 0, pa, pb, pc))
        return map4d

    def find_max_coa(self, map4d, n_samples, n_nodes, out=None):
        if out is None:
            out = (np.zeros(n_samples), np.zeros(n_samples), np.zeros(n_samples, dtype=np.int64))
        pm = _host_f64(map4d, "map4d", int(n_samples) * int(n_nodes))
        pa, pb, pc = self._series_ptrs(out, int(n_samples))
        _check(qmlib.qm_group_find_max_coa(self._h, pm, int(n_samples), int(n_nodes), pa, pb, pc))
        return out

    # -- the rows next to the path: the lead device's engine ---------------------
    def locate_fits(self, *args, **kwargs):
        return self.lead.locate_fits(*args, **kwargs)

    def rbf_peak(self, *args, **kwargs):
        return self.lead.rbf_peak(*args, **kwargs)

    def onsets(self, *args, **kwargs):
        return self.lead.onsets(*args, **kwargs)


class EngineReplicas:
    """
    One process driving a continuous stream on several GPUs by TIME: ``devices`` lists one
    :class:`Engine` per entry, ids may repeat (``[0, 0]``: two engines on GPU 0); entry 0 is the lead.  Every
    replica holds the whole table.  :class:`quakemigrate_amd.stream.StreamingDetector` runs one pipeline over all
    of them (``qm_stream_create_replicas``: launch j on replica j mod n, results in push order), which is what
    ``MigrationScan.continuous_compute`` uses; single calls (``detect``, ``migrate``, ``marginal_map``, the locate
    rows) run on the lead and are an :class:`Engine`'s bit for bit.  Table operations and ``config`` go to every
    replica.  For one large step over several GPUs use :class:`EngineGroup` instead.
    """

    def __init__(self, devices, **config):
        ids = [int(d) for d in devices]
        if not ids:
            raise ValueError("EngineReplicas needs at least one device")
        self.devices = ids
        self.replicas = []
        try:
            for d in ids:
                self.replicas.append(Engine(d))
            for k, v in config.items():
                self.config(k, v)
        except BaseException:
            self.close()
            raise
        self.table_generation = 0
        self.grids_generation = 0

    @property
    def lead(self):
        return self.replicas[0]

    def close(self):
        for r in self.replicas:
            r.close()

    def config(self, key, value):
        for r in self.replicas:
            r.config(key, value)

    def get(self, key):
        values = [r.get(key) for r in self.replicas]
        if any(v != values[0] for v in values):
            raise QMHipError(f"the replicas disagree on {key!r}: {values}")
        return values[0]

    def synchronize(self):
        for r in self.replicas:
            r.synchronize()

    # -- table: every replica ----------------------------------------------------
    def load_lut(self, traveltimes, node_offset=0, shape=None):
        for r in self.replicas:
            r.load_lut(traveltimes, node_offset=node_offset, shape=shape)
        self.table_generation += 1

    def select_table(self, key, capacity=4):
        """As :meth:`Engine.select_table` on every replica; True only if every one has the table resident (else
        the caller's ``load_lut`` / ``serve`` goes to all of them)."""
        resident = [r.select_table(key, capacity) for r in self.replicas]
        self.table_generation += 1
        return all(resident)

    def set_traveltime_grids(self, grids):
        grids = list(grids)
        for r in self.replicas:
            r.set_traveltime_grids(grids)
        self.grids_generation += 1
        self.table_generation += 1

    def serve(self, sampling_rate, rows, decimate=(1, 1, 1), node_offset=0):
        for r in self.replicas:
            r.serve(sampling_rate, rows, decimate=decimate, node_offset=node_offset)
        self.table_generation += 1

    def table_digest(self):
        """The replicas' common table digest (:meth:`Engine.table_digest`); raises if one holds another table."""
        digests = [r.table_digest() for r in self.replicas]
        for i, d in enumerate(digests):
            if d != digests[0]:
                raise QMHipError(f"replica {i} holds another table than replica 0")
        return digests[0]

    def download_lut(self):
        return self.lead.download_lut()

    @property
    def device(self):
        return self.lead.device

    @property
    def grid(self):
        return self.lead.grid

    @property
    def n_rows(self):
        return self.lead.n_rows

    @property
    def node_offset(self):
        return self.lead.node_offset

    @property
    def n_nodes(self):
        return self.lead.n_nodes

    @property
    def lut_max(self):
        return self.lead.lut_max

    # -- single calls: the lead ----------------------------------------------------
    def detect(self, *args, **kwargs):
        return self.lead.detect(*args, **kwargs)

    def migrate(self, *args, **kwargs):
        return self.lead.migrate(*args, **kwargs)

    def marginal_map(self, *args, **kwargs):
        return self.lead.marginal_map(*args, **kwargs)

    def find_max_coa(self, *args, **kwargs):
        return self.lead.find_max_coa(*args, **kwargs)

    def locate_fits(self, *args, **kwargs):
        return self.lead.locate_fits(*args, **kwargs)

    def rbf_peak(self, *args, **kwargs):
        return self.lead.rbf_peak(*args, **kwargs)

    def onsets(self, *args, **kwargs):
        return self.lead.onsets(*args, **kwargs)

    def preprocess(self, *args, **kwargs):
        return self.lead.preprocess(*args, **kwargs)

    def preprocess_segments(self, *args, **kwargs):
        return self.lead.preprocess_segments(*args, **kwargs)

    def resample(self, *args, **kwargs):
        return self.lead.resample(*args, **kwargs)

    def pick_phases(self, *args, **kwargs):
        return self.lead.pick_phases(*args, **kwargs)

    def measure_amplitudes(self, *args, **kwargs):
        return self.lead.measure_amplitudes(*args, **kwargs)

    def trigger_series(self, *args, **kwargs):
        return self.lead.trigger_series(*args, **kwargs)

    def scanmseed_encode(self, *args, **kwargs):
        return self.lead.scanmseed_encode(*args, **kwargs)

    def scanmseed_decode(self, *args, **kwargs):
        return self.lead.scanmseed_decode(*args, **kwargs)


def timeit(*args_, **kwargs_):
    """
    The reference's per-call wall-time log line (quakemigrate/util.py:651-669, applied at
    core/lib.py:52,131 and signal/scan.py:593): same message, ``timeit("info")`` logs at info
    level, ``timeit()`` at debug.  The wrapped functions here take host arrays and return host
    arrays, so the elapsed time includes the copies and the wait for the GPU.
    """
    import functools
    import time

    def inner_function(func):
        @functools.wraps(func)
        def wrapper(*args, **kwargs):
            ts = time.time()
            result = func(*args, **kwargs)
            msg = " " * 21 + f"Elapsed time: {time.time() - ts:6f} seconds."
            if args_ and args_[0] == "info":
                logging.info(msg)
            else:
                logging.debug(msg)
            return result

        return wrapper

    return inner_function


# --------------------------------------------------------------------------
# module-level engine for the reference-signature functions.  They receive the
# table on every call (lib.py:53-60); like the C symbols beside them
# (qm_compat.hip: migrate) they keep it resident and upload it again only when
# its shape or content -- two independent 64-bit hashes of every word,
# qm_table_hash -- changes (QM_HIP_COMPAT_REUPLOAD=1: on every call).  Callers
# that keep a table across timesteps use an Engine (or
# quakemigrate_amd.scan.MigrationScan) and never pay for the hash either.
# --------------------------------------------------------------------------
_default = {"engine": None, "table_key": None}


def release_cached_memory():
    """Return the device memory that destroyed engines / replaced tables left parked in the process
    (``qm_release_cached_memory``) to the driver."""
    qmlib.qm_release_cached_memory()


def _device_list():
    """``QM_HIP_DEVICES`` ("0,1,2,3") as a list of ids, or None when it is unset or empty."""
    import os

    text = os.environ.get("QM_HIP_DEVICES", "").strip()
    if not text:
        return None
    return [int(v) for v in text.replace(" ", "").split(",") if v != ""]


def default_engine():
    """The process-wide engine: an :class:`EngineGroup` when ``QM_HIP_DEVICES`` lists more than one id, else
    an :class:`Engine` on ``$QM_HIP_DEVICE`` (default 0)."""
    if _default["engine"] is None:
        import os

        ids = _device_list()
        if ids is not None and len(ids) > 1:
            _default["engine"] = EngineGroup(ids)
        else:
            _default["engine"] = Engine(int(os.environ.get("QM_HIP_DEVICE", "0")))
    return _default["engine"]


def _table_key(traveltimes):
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    qmlib.qm_table_hash(traveltimes.ctypes.data_as(ctypes.c_void_p), traveltimes.size,
                        ctypes.byref(a), ctypes.byref(b))
    return (tuple(traveltimes.shape), int(a.value), int(b.value))


def _resident(traveltimes):
    import os

    eng = default_engine()
    key = _table_key(traveltimes)
    if (os.environ.get("QM_HIP_COMPAT_REUPLOAD", "0") not in ("", "0")
            or _default["table_key"] != (key, eng.table_generation)):
        _default["table_key"] = None
        eng.load_lut(traveltimes)
        _default["table_key"] = (key, eng.table_generation)
    return eng


def _prepare(onsets, traveltimes, first_idx, last_idx):
    """Pre-processing and checks of lib.py:93-110, in the reference's order."""
    onsets = np.clip(onsets, 0.01, np.inf)
    onsets = np.ascontiguousarray(np.log(onsets), dtype=np.float64)
    *grid_dimensions, n_luts = traveltimes.shape
    n_onsets, t_samples = onsets.shape
    logging.debug(f"(n_onsets, t_samples) : ({n_onsets}, {t_samples})")
    n_samples = t_samples - first_idx - last_idx
    logging.debug(f"n_samples : {n_samples}")
    if not n_luts == n_onsets:
        raise ValueError(
            f"Mismatch between number of stations for data and LUT, {n_onsets}:{n_luts}"
        )
    if onsets.size < n_samples + first_idx:
        raise ValueError("Data array smaller than coalescence array.")
    if traveltimes.dtype != np.int32 or not traveltimes.flags["C_CONTIGUOUS"]:
        # the reference's ndpointer argtype raises ctypes.ArgumentError here
        raise ctypes.ArgumentError(
            "traveltimes must be a C-contiguous int32 array")
    return onsets, tuple(grid_dimensions), n_samples


@timeit()
def migrate(onsets, traveltimes, first_idx, last_idx, available, threads=1):
    """
    Computes 4-D coalescence map by migrating seismic phase onset functions.

    Same contract as the reference's ``migrate`` (lib.py:52-125); ``threads`` is
    accepted and ignored (the GPU engine has no thread knob).

    Returns
    -------
    map4d: 4-D coalescence map, shape(nx, ny, nz, nsamples).
    """
    onsets, grid, n_samples = _prepare(onsets, traveltimes, first_idx, last_idx)
    eng = _resident(traveltimes)
    map4d = np.zeros(grid + (n_samples,), dtype=np.double)
    logging.debug(f"map4d shape : {map4d.shape}")
    eng.migrate(onsets, first_idx, last_idx, available, map4d)
    return map4d


@timeit()
def find_max_coa(map4d, threads=1):
    """
    Finds time series of the maximum coalescence/normalised coalescence in the
    3-D volume, and the corresponding grid indices (reference lib.py:131-170).
    """
    *grid_dimensions, n_samples = map4d.shape
    n_nodes = int(np.prod(grid_dimensions))
    max_coa = np.zeros(n_samples, dtype=np.double)
    max_norm_coa = np.zeros(n_samples, dtype=np.double)
    max_coa_idx = np.zeros(n_samples, dtype=np.int64)
    default_engine().find_max_coa(
        np.ascontiguousarray(map4d, dtype=np.double), n_samples, n_nodes,
        (max_coa, max_norm_coa, max_coa_idx))
    return max_coa, max_norm_coa, max_coa_idx


@timeit()
def migrate_and_find_max(onsets, traveltimes, first_idx, last_idx, available,
                         threads=1, return_map=False):
    """
    Fused ``migrate`` + ``find_max_coa`` (what ``QuakeScan._compute`` does back to
    back, scan.py:635-638).  With ``return_map=False`` (detect) the 4-D map is
    never written anywhere.

    Returns ``(max_coa, max_norm_coa, max_coa_idx)`` or, with ``return_map``,
    ``(max_coa, max_norm_coa, max_coa_idx, map4d)``.
    """
    onsets, grid, n_samples = _prepare(onsets, traveltimes, first_idx, last_idx)
    eng = _resident(traveltimes)
    out = (np.zeros(n_samples), np.zeros(n_samples),
           np.zeros(n_samples, dtype=np.int64))
    if not return_map:
        eng.detect(onsets, first_idx, last_idx, available, out=out)
        return out
    map4d = np.zeros(grid + (n_samples,), dtype=np.double)
    eng.migrate(onsets, first_idx, last_idx, available, map4d, scan_out=out)
    return out + (map4d,)


def _stalta(fn, signal, nsta, nlta, fill):
    head = np.empty(1, dtype=stalta_header_t)
    head[:] = (len(signal), nsta, nlta)
    signal = np.ascontiguousarray(signal, dtype=np.double)
    onset = np.full(len(signal), fill, dtype=np.double)
    fn(signal, head, onset)
    return onset


def overlapping_sta_lta(signal, nsta, nlta):
    """Overlapping-window STA/LTA (reference lib.py:176-208)."""
    return _stalta(qmlib.overlapping_sta_lta, signal, nsta, nlta, 1.0)


def centred_sta_lta(signal, nsta, nlta):
    """Centred STA/LTA (reference lib.py:214-246)."""
    return _stalta(qmlib.centred_sta_lta, signal, nsta, nlta, 1.0)


def recursive_sta_lta(signal, nsta, nlta):
    """Recursive STA/LTA (reference lib.py:252-285)."""
    return _stalta(qmlib.recursive_sta_lta, signal, nsta, nlta, 0.0)
