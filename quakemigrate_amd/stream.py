# -*- coding: utf-8 -*-
"""
Continuous detect sweep with copies overlapped with compute (BASELINE.json configs[4]:
"continuous 24 h synthetic stream ... overlapped H2D copy + compute on HIP streams").

The reference's ``QuakeScan._continuous_compute`` (quakemigrate/signal/scan.py:407-470; the loop
:434-448) walks the timesteps serially: read -> onsets -> migrate -> find_max_coa -> append.  The
hot-path part of that loop is the library's native pipeline (``qm_stream_*``, include/qmhip.h part 3,
csrc/qm_stream.hip): a pinned ring of ``depth`` slots of ``steps_per_launch`` timesteps, H2D on a copy
stream, one fused-detect launch per slot, one packed D2H per launch, HIP events for the ordering.
This class is the thin caller: it pushes windows, pops results in order, and nothing else -- no
torch, no per-step staging in Python (round 4's Python loop cost the example-sized grids 30-40 % of
their kernel rate once the copies were inside the clock).
"""

from __future__ import annotations

import ctypes

import numpy as np

from quakemigrate_amd.core import lib as _lib

_qm = _lib.qmlib


class StreamingDetector:
    """
    Parameters
    ----------
    engine : quakemigrate_amd.core.Engine with the travel-time table resident, or a
        quakemigrate_amd.core.EngineReplicas whose replicas all hold it: then ONE pipeline runs over
        every replica (``qm_stream_create_replicas``: launch j on replica j mod n, results in push
        order, bit for bit an Engine's).
    n_rows, t_samples : shape of every onset window (rows x samples, float64, already
        ``log(clip(., 0.01))``).
    fsmp, lsmp, available : as in ``Engine.detect``.
    n_nodes_total : node count of the full grid (normalisation).
    depth : slots of the ring = launches that may be in flight or un-popped (>= 2); per replica.
    steps_per_launch : timesteps stacked by ONE launch (``qm_engine_detect_batch``).  Timesteps are
        independent given their onsets, so K of them can share a launch: on the grids the
        reference's examples use (1e4 - 3e5 nodes) one timestep is a few workgroup rounds and a
        fraction of a millisecond, and K steps per launch are what fills the GPU and amortises the
        launch, the combine and the copies' latencies.  Results are identical step for step.
    device : accepted for compatibility with round 4's signature; the engine's device is used.
    onset_stage : ``None`` -- the windows are log-onsets (``push``) -- or the stage that makes them on the device
        from resampled component traces (``push_signals``): a :class:`quakemigrate_amd.preprocess.OnsetStage`
        (then ``sampling_rate`` is needed) or the dict its ``arrays(t_samples, sampling_rate)`` returns.  A slot's
        launch is then pre-processing (detrend, taper, zero-phase band-pass) -> onsets -> fused detect, every
        timestep's bits those of ``Engine.detect(Engine.onsets(Engine.preprocess(x)))``.  A stream takes one kind
        of window, never both.
    resample_stage : ``None``, or -- on top of an onset stage -- the plan that makes those component traces on the
        device from a timestep's RAW traces, each at its own rate and length (``push_raw``): a
        :class:`quakemigrate_amd.preprocess.ResampleStage` or the dict its ``arrays(t_samples)`` returns;
        ``raw_dtype``: what the raw samples are, int32 (as miniSEED holds them) or float64.  A slot's launch then
        starts with the resampling kernel, every timestep's bits those of ``Engine.resample`` in front of the calls
        above.
    max_segments : with an onset stage whose ``fill_gaps`` is set (or whose dict holds ``second_taper`` /
        ``fill_value``), the stream takes GAPPY traces with their segment layout (``push_segments``): up to this many
        segments per timestep (``None``: 4 per trace).  A slot's launch is then the segment kernel -- every segment
        conditioned on its own, tapered twice, gaps filled -> onsets -> fused detect, every timestep's bits those of
        ``Engine.preprocess_segments`` in front of ``Engine.onsets`` and ``Engine.detect``.
    max_taper_weights : room for a timestep's taper weights; ``None``: ``ceil(2 * taper_percentage * n_traces *
        t_samples)``, which suffices for any layout, since sum 2 int(p n_s) <= 2 p n_traces T.
    """

    def __init__(self, engine, n_rows, t_samples, fsmp, lsmp, available, n_nodes_total=None,
                 depth=2, device=None, steps_per_launch=1, onset_stage=None, sampling_rate=None,
                 resample_stage=None, raw_dtype=np.int32, max_segments=None, max_taper_weights=None):
        if engine.n_rows is None:
            raise _lib.QMHipError("no travel-time table resident: call load_lut first")
        if int(n_rows) != engine.n_rows:
            raise ValueError("Mismatch between number of stations for data and LUT, "
                             f"{int(n_rows)}:{engine.n_rows}")
        self.engine = engine
        self.n_rows, self.t_samples = int(n_rows), int(t_samples)
        self.fsmp, self.lsmp, self.available = int(fsmp), int(lsmp), int(available)
        self.n_samples = self.t_samples - self.fsmp - self.lsmp
        self.depth = max(2, int(depth))
        self.k = max(1, int(steps_per_launch))
        total = engine.n_nodes if n_nodes_total is None else int(n_nodes_total)
        h = ctypes.c_void_p()
        if isinstance(engine, _lib.EngineReplicas):
            handles = (ctypes.c_void_p * len(engine.replicas))(*[r._h.value for r in engine.replicas])
            _lib._check(_qm.qm_stream_create_replicas(handles, len(engine.replicas), self.t_samples, self.fsmp,
                                                      self.lsmp, self.available, total, self.k, self.depth,
                                                      ctypes.byref(h)))
        else:
            _lib._check(_qm.qm_stream_create(engine._h, self.t_samples, self.fsmp, self.lsmp,
                                             self.available, total, self.k, self.depth, ctypes.byref(h)))
        self._h = h
        import weakref

        self._finalizer = weakref.finalize(self, _qm.qm_stream_destroy, h)
        self.feed = "log_onsets"            # the kind of timestep the stages call for: each set_* call names its own
        self.n_traces = None
        self.raw_dtype = self._raw_records = self.total_raw_samples = None
        self.max_segments = self.max_taper_weights = None
        self.taper_percentage = 0.05
        if onset_stage is not None:
            self.taper_percentage = float(getattr(onset_stage, "taper_percentage", 0.05))
            gaps = self.set_onset_stage(onset_stage, sampling_rate)
            if gaps is not None:
                self.set_segment_feed(max_segments, max_taper_weights, *gaps)
            elif max_segments is not None:
                raise ValueError("max_segments: the onset stage does not fill gaps (OnsetStage(fill_gaps=True))")
        elif max_segments is not None:
            raise ValueError("max_segments goes with an onset stage that fills gaps")
        if resample_stage is not None:
            self.set_resample_stage(resample_stage, raw_dtype)

    def set_onset_stage(self, onset_stage, sampling_rate=None):
        """Once, before the first push (``qm_stream_set_onset_stage``).  Returns ``(second_taper, fill_value)`` of a
        stage that fills gaps -- what :meth:`set_segment_feed` takes -- and ``None`` of any other."""
        if hasattr(onset_stage, "arrays"):
            if sampling_rate is None:
                raise ValueError("an OnsetStage needs the sampling_rate of the windows")
            onset_stage = onset_stage.arrays(self.t_samples, sampling_rate)
        a = onset_stage
        i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)     # noqa: E731
        f64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)   # noqa: E731
        trace_row, trace_filter = i32(a["trace_row"]), i32(a["trace_filter"])
        nsta, nlta = i32(a["nsta"]), i32(a["nlta"])
        left, right = f64(a["taper_left"]).reshape(-1), f64(a["taper_right"]).reshape(-1)
        sos = _lib._sections(a["sos"])
        if trace_filter.shape != trace_row.shape or trace_row.ndim != 1:
            raise ValueError("trace_row and trace_filter: one entry per trace each")
        if nsta.shape != (self.n_rows,) or nlta.shape != (self.n_rows,):
            raise ValueError(f"nsta / nlta: one entry per onset row ({self.n_rows}) each")
        _lib._check(_qm.qm_stream_set_onset_stage(
            self._h, len(trace_row), trace_row, trace_filter, sos.reshape(-1), int(sos.shape[0]), int(sos.shape[1]),
            int(a.get("detrend", 1)), left, len(left), right, len(right), nsta, nlta, int(a["transform"]),
            int(a["position"]), int(a["taper_pad"]), float(a["min_onset_value"])))
        self.n_traces, self.feed = len(trace_row), "signals"
        if "fill_value" in a or "second_taper" in a:
            from quakemigrate_amd.preprocess import GAP_FILL_VALUE

            return int(a.get("second_taper", 1)), float(a.get("fill_value", GAP_FILL_VALUE))
        return None

    def set_segment_feed(self, max_segments=None, max_taper_weights=None, second_taper=1, fill_value=None):
        """Once, after the onset stage and before the first push (``qm_stream_set_segment_feed``)."""
        from quakemigrate_amd.preprocess import GAP_FILL_VALUE

        if self.n_traces is None:                       # (the library's own refusal)
            raise _lib.QMHipError("qm_stream_set_segment_feed: the stream has no onset stage "
                                  "(qm_stream_set_onset_stage comes first)")
        if max_segments is None:
            max_segments = 4 * self.n_traces
        if max_taper_weights is None:
            max_taper_weights = int(np.ceil(2.0 * self.taper_percentage * self.n_traces * self.t_samples))
        _lib._check(_qm.qm_stream_set_segment_feed(
            self._h, int(max_segments), int(max_taper_weights), int(second_taper),
            GAP_FILL_VALUE if fill_value is None else float(fill_value)))
        self.max_segments, self.max_taper_weights, self.feed = int(max_segments), int(max_taper_weights), "segments"

    def set_resample_stage(self, resample_stage, raw_dtype=np.int32):
        """Once, after the onset stage and before the first push (``qm_stream_set_resample_stage``)."""
        kind = np.dtype(raw_dtype)
        if kind not in _lib.RAW_DTYPES:
            raise TypeError(f"raw samples of type {kind}: int32 or float64")
        records, sos, table, weights, detrend, t_samples, total = _lib.resample_arrays(resample_stage, self.t_samples)
        _lib._check(_qm.qm_stream_set_resample_stage(
            self._h, len(records), records.reshape(-1), sos.reshape(-1), int(sos.shape[0]), int(sos.shape[1]), detrend,
            table.reshape(-1), len(table), weights, len(weights), t_samples, _lib.RAW_DTYPES[kind], total))
        self.raw_dtype, self._raw_records, self.total_raw_samples, self.feed = kind, records, total, "raw"

    def close(self):
        self._finalizer()

    # -- the three calls --------------------------------------------------------------
    @staticmethod
    def _pushed(rc):
        """A push's return code: False for 2 (every slot holds un-popped results), the library's error otherwise."""
        if rc == 2:
            return False
        _lib._check(rc)
        return True

    def push_step(self, item):
        """One timestep of the kind the stream's stages call for (``feed``), as :meth:`run` documents it per kind;
        returns like :meth:`push`."""
        if self.feed == "segments":
            return self.push_segments(*item)
        return {"log_onsets": self.push, "signals": self.push_signals, "raw": self.push_raw}[self.feed](item)

    def push(self, window):
        """One timestep's log-onsets (n_rows, t_samples) into the pipeline.  False: every slot holds
        results that have not been popped (``pop`` first, then push again)."""
        w = np.ascontiguousarray(window, dtype=np.float64)
        if w.shape != (self.n_rows, self.t_samples):
            raise ValueError(f"window of shape {w.shape}, the stream takes {(self.n_rows, self.t_samples)}")
        return self._pushed(_qm.qm_stream_push(self._h, w.ctypes.data_as(ctypes.c_void_p)))

    def push_signals(self, window):
        """One timestep's resampled component traces (n_traces, t_samples) into a pipeline with an onset stage;
        returns like :meth:`push`."""
        w = np.ascontiguousarray(window, dtype=np.float64)
        if self.n_traces is not None and w.shape != (self.n_traces, self.t_samples):
            raise ValueError(f"window of shape {w.shape}, the stage takes {(self.n_traces, self.t_samples)}")
        return self._pushed(_qm.qm_stream_push_signals(self._h, w.ctypes.data_as(ctypes.c_void_p)))

    def push_raw(self, raw):
        """One timestep's raw traces -- a list of 1-D arrays, one per trace, or the packed array, of the stage's
        ``raw_dtype`` -- into a pipeline with a resampling stage; returns like :meth:`push`."""
        if self._raw_records is None:                   # (the library's own refusal, before any list is packed)
            raise _lib.QMHipError("qm_stream_push_raw: the stream has no resampling stage "
                                  "(qm_stream_set_resample_stage)")
        w = _lib.pack_raw(raw, self._raw_records, self.total_raw_samples, self.raw_dtype)
        return self._pushed(_qm.qm_stream_push_raw(self._h, w.ctypes.data_as(ctypes.c_void_p)))

    def push_segments(self, window, segments, taper_weights=None):
        """One timestep's gappy component traces (n_traces, t_samples) in window layout with their layout into a
        pipeline with the segment feed: ``segments`` is a list of ``(trace, first, n)``, planned here
        (:func:`quakemigrate_amd.preprocess.plan_segments` with the stage's taper percentage), or -- with
        ``taper_weights`` -- the (n_segments, 8) records themselves.  Returns like :meth:`push`."""
        w = np.ascontiguousarray(window, dtype=np.float64)
        if self.n_traces is not None and w.shape != (self.n_traces, self.t_samples):
            raise ValueError(f"window of shape {w.shape}, the stage takes {(self.n_traces, self.t_samples)}")
        if taper_weights is None:
            from quakemigrate_amd.preprocess import plan_segments

            segments, taper_weights = plan_segments(self.t_samples, w.shape[0], segments, self.taper_percentage)
        records, weights = _lib.segment_arrays(segments, taper_weights)
        return self._pushed(_qm.qm_stream_push_segments(self._h, w.ctypes.data_as(ctypes.c_void_p), records.reshape(-1),
                                                        len(records), weights, len(weights)))

    def flush(self):
        _lib._check(_qm.qm_stream_flush(self._h))

    def pending(self):
        """(timesteps launched and not yet popped, timesteps pushed into a launch that has not gone out)"""
        a, b = ctypes.c_int32(), ctypes.c_int32()
        _lib._check(_qm.qm_stream_pending(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def pop(self, n_steps=1):
        """The next ``n_steps`` timesteps' ``(max_coa, max_norm_coa, max_coa_idx)``, each
        ``(n_steps, n_samples)``; blocks until their launch has finished."""
        n, ns = int(n_steps), self.n_samples
        a, b = np.empty((n, ns)), np.empty((n, ns))
        c = np.empty((n, ns), dtype=np.int64)
        _lib._check(_qm.qm_stream_pop(self._h, n, a.ctypes.data_as(ctypes.c_void_p),
                                      b.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p)))
        return a, b, c

    # -- the loop -----------------------------------------------------------------------
    def run(self, windows, on_result=None):
        """
        ``windows``: iterable with one item per timestep, of the stream's kind (``feed``):

        ``"log_onsets"``  a float64 array (n_rows, t_samples), already logged
        ``"signals"``     (an onset stage) a float64 array (n_traces, t_samples) of resampled component traces
        ``"raw"``         (a resampling stage as well) the timestep's raw traces as :meth:`push_raw` takes them
        ``"segments"``    (the segment feed) a ``(traces, segments)`` pair -- or ``(traces, records, taper_weights)`` --
                          as :meth:`push_segments` takes them

        Returns a list of ``(max_coa, max_norm_coa, max_coa_idx)`` NumPy triples (or calls ``on_result(step, triple)``
        and returns the number of steps).
        """
        results = []
        step = 0

        def take(n):
            nonlocal step
            a, b, c = self.pop(n)
            for j in range(n):
                triple = (a[j], b[j], c[j])
                if on_result is None:
                    results.append(triple)
                else:
                    on_result(step, triple)
                step += 1

        for w in windows:
            while not self.push_step(w):
                take(min(self.k, self.pending()[0]))     # the oldest launch's timesteps
        self.flush()
        left = self.pending()[0]
        while left > 0:
            n = min(self.k, left)
            take(n)
            left -= n
        return results if on_result is None else step
