# -*- coding: utf-8 -*-
"""
Host-side counterpart of ``QuakeScan._compute`` for the migrate / find_max_coa path.

``MigrationScan.continuous_compute(...)`` is the loop around it (reference ``scan.py:407-470``).
``MigrationScan._compute(data, event=None)`` reproduces the glue of the reference's
``quakemigrate/signal/scan.py:593-647`` around the hot path -- onset plugin ->
served travel-time table -> ``fsmp`` / ``lsmp`` -> ``available`` -> migrate ->
find_max_coa -> ``index2coord`` -- with the same argument meaning, return tuples and
error behaviour, but:

* the table is made resident on the GPU once per ``(sampling_rate, availability)``
  (the reference rebuilds and re-passes it every timestep, ``lut.py:502-538``), and
* in the detect stage the fused kernel runs, so the 4-D map is never materialised
  (the reference allocates it only to reduce and delete it, ``scan.py:641-642``).

It is duck-typed against the reference's plugin API, so the reference's own objects
drop in unchanged:

* ``onset``  : ``calculate_onsets(data) -> (onsets[S, T] float64, onset_data)`` with
  ``onset_data.sampling_rate`` and ``onset_data.availability`` (dict "STATION_PHASE"
  -> 0/1), see ``quakemigrate/signal/onsets/base.py:24-130, 133-191``;
* ``lut``    : ``serve_traveltimes(sampling_rate, availability) -> int32
  (nx, ny, nz, S)`` and ``index2coord(idx, unravel=True)``
  (``quakemigrate/lut/lut.py:502-538, 211-243``).

obspy / pyproj are not needed here: whatever ``data.starttime`` and
``event.mw_times`` return is passed through.
"""

from __future__ import annotations

import itertools
import logging

import numpy as np

from quakemigrate_amd.core import lib


_LUT_TOKENS = itertools.count(1)


def _lut_token(lut):
    """A process-unique name for ``lut`` in the keys of parked tables (``id()`` would be reused by a
    later object at the same address and bring a dead LUT's table back): kept on the object where
    it takes attributes, else the caller gets a fresh one (no sharing between scans)."""
    token = getattr(lut, "_qm_hip_token", None)
    if token is None:
        token = next(_LUT_TOKENS)
        try:
            lut._qm_hip_token = token
        except (AttributeError, TypeError):
            pass
    return token


class LUTPhasesException(Exception):
    """Mirror of ``quakemigrate.util.LUTPhasesException`` (util.py)."""


class _NoDataException(Exception):
    def __init__(self, msg="no data"):
        super().__init__(msg)
        self.msg = msg


class ArchiveEmptyException(_NoDataException):
    """Mirror of ``quakemigrate.util.ArchiveEmptyException`` (carries ``.msg``)."""


class DataGapException(_NoDataException):
    """Mirror of ``quakemigrate.util.DataGapException``."""


class DataAvailabilityException(_NoDataException):
    """Mirror of ``quakemigrate.util.DataAvailabilityException``."""


# the reference's own exception objects (raised by ITS archive / onset classes when both packages are
# installed) are recognised by name: nothing of the reference is imported here
_NO_DATA = ("ArchiveEmptyException", "DataGapException", "DataAvailabilityException")


def _is_no_data(exc):
    """The reference catches util.ArchiveEmptyException / DataGapException / DataAvailabilityException AND their
    subclasses (scan.py:449-458); its exception objects are recognised by the names in the raised class's MRO
    (obspy-free: the reference's util module is not imported here)."""
    return any(cls.__name__ in _NO_DATA for cls in type(exc).__mro__)


def _shift(t, seconds):
    """``t + seconds`` for obspy ``UTCDateTime`` (adds floats) and ``datetime`` alike."""
    try:
        return t + seconds
    except TypeError:
        import datetime as _dt

        return t + _dt.timedelta(seconds=float(seconds))


def time2sample(time, sampling_rate):
    """Seconds -> whole samples, as ``quakemigrate/util.py:152-172``."""
    return int(round(time * int(sampling_rate)))


class MigrationScan:
    """
    Parameters
    ----------
    lut, onset : plugin objects (see module docstring).
    pre_pad, post_pad : float
        Seconds of onset data before / after the scanned window (what
        ``QuakeScan`` gets from ``onset.pad(timestep)``, scan.py:425).
    stage : {"detect", "locate"}
        ``run.stage`` of the reference (scan.py:641).
    scan_rate : int, optional
        Passed to ``event.mw_times`` in the locate stage (scan.py:646).
    engine : quakemigrate_amd.core.Engine, EngineGroup or EngineReplicas, optional
        Defaults to the process-wide engine (``lib.default_engine``: a group when ``$QM_HIP_DEVICES``
        lists several devices, else an engine on ``$QM_HIP_DEVICE``).  A group runs ``_compute``, the
        locate calls and ``continuous_compute`` (timestep by timestep, without the pipeline); it takes
        neither ``device_serving`` nor ``screen=True``.  Replicas run ``_compute`` and the locate calls
        on their lead and ``continuous_compute`` as one pipeline over all of them (timesteps split
        round-robin by launch); they take everything an Engine takes.
    threads : int
        Accepted for signature compatibility; the GPU engine ignores it.
    device_serving : bool
        Build the int32 table on the GPU from ``lut.traveltimes`` (see ``_ensure_table``).
    screen : bool, optional
        Detect precision, see ``INTEGRATION.md`` section 4b.
    table_cache : int
        Tables of other station availabilities kept parked on the device (``_ensure_table``);
        0 = one resident table, rebuilt at every change.
    """

    def __init__(self, lut, onset, pre_pad, post_pad, stage="detect", scan_rate=None,
                 engine=None, threads=1, device_serving=False, screen=None, table_cache=4):
        self.lut = lut
        self.onset = onset
        self.pre_pad = pre_pad
        self.post_pad = post_pad
        self.stage = stage
        self.scan_rate = scan_rate
        self.threads = threads
        self.engine = engine if engine is not None else lib.default_engine()
        # screen: None leaves the engine as configured (float64 throughout unless it was created
        # with screen=1); True / False select the opt-in screened detect (exact argmax and
        # max_coa, max_coa_n within 6.7e-7 by a deterministic bound) for THIS scan's steps only:
        # the setting is applied around each call and the engine's own restored afterwards (the
        # default engine is shared by every MigrationScan and by lib.migrate_and_find_max)
        self.screen = None if screen is None else bool(screen)
        self._lut_token = _lut_token(lut)
        self._resident_key = None
        self._resident_generation = -1
        self._grids_generation = -1
        self.table_cache = int(table_cache)
        # device_serving: the float64 grids of ``lut.traveltimes`` ({station: {phase: grid}},
        # quakemigrate/lut/lut.py) are uploaded once and the int32 table of the available
        # station/phase pairs is built on the GPU (rint(tt * sampling_rate), lut.py:536-538)
        # whenever the availability changes -- no per-timestep host stack / rint / upload.
        self.device_serving = bool(device_serving)
        self._grid_index = None
        if isinstance(self.engine, lib.EngineGroup):
            if self.device_serving:
                raise ValueError("device_serving is not available on an engine group")
            if self.screen:
                raise ValueError("screen=True is not available on an engine group (the screened detect has "
                                 "no partial form)")

    # -- table residency ------------------------------------------------------
    def _ensure_table(self, sampling_rate, availability):
        """
        Make the table of this ``(sampling_rate, availability)`` the engine's resident one.  The
        reference serves it anew every timestep (lut.py:502-538); here it is built the first time
        an availability is seen and PARKED on the device when another one takes over
        (``Engine.select_table``, up to ``table_cache`` tables, least recently used evicted), so
        stations dropping in and out alternate between resident tables at no cost.
        """
        key = (sampling_rate, tuple(availability.items()))
        eng = self.engine
        # (the engine may be shared -- the default one is -- so residency is the engine's word:
        # its table generation moves whenever anybody replaces or switches the table)
        if key == self._resident_key and eng.table_generation == self._resident_generation:
            return eng
        if eng.select_table((self._lut_token, key), capacity=self.table_cache):
            self._resident_key, self._resident_generation = key, eng.table_generation
            return eng
        if self.device_serving:
            if self._grid_index is None or self._grids_generation != getattr(eng, "grids_generation", 0):
                names, grids = [], []
                for station, phases in self.lut.traveltimes.items():
                    for phase, grid in phases.items():
                        names.append(f"{station}_{phase}")
                        grids.append(grid)
                eng.set_traveltime_grids(grids)
                self._grids_generation = eng.grids_generation
                self._grid_index = {n: i for i, n in enumerate(names)}
            rows = []
            for k, available in availability.items():
                if available != 1:
                    continue
                station, phase = k.split("_")
                if k in self._grid_index:
                    rows.append(self._grid_index[k])
                elif f"{station}_TIME_{phase}" in self._grid_index:      # lut.py:534-535
                    rows.append(self._grid_index[f"{station}_TIME_{phase}"])
                else:
                    phases = sorted({kk.split("_")[-1] for kk in availability})
                    raise LUTPhasesException(
                        f"Attempting to migrate phases {phases}; but traveltimes for "
                        f"'{phase}' not found in the LUT. Please create a new lookup table "
                        f"with phases={phases}")
            eng.serve(sampling_rate, rows)
        else:
            try:
                traveltimes = self.lut.serve_traveltimes(sampling_rate, availability)
            except KeyError as e:
                phases = sorted({k.split("_")[-1] for k in availability})
                raise LUTPhasesException(
                    f"Attempting to migrate phases {phases}; but traveltimes for {e} "
                    f"not found in the LUT. Please create a new lookup table with "
                    f"phases={phases}")
            traveltimes = np.ascontiguousarray(traveltimes, dtype=np.int32)
            eng.load_lut(traveltimes)
            logging.debug("travel-time table %s made resident", traveltimes.shape)
        self._resident_key, self._resident_generation = key, eng.table_generation
        return eng

    # -- the hot-path glue ------------------------------------------------------
    @lib.timeit("info")
    def _compute(self, data, event=None):
        """
        Compute 3-D coalescence between two time stamps (reference scan.py:593-647).

        Returns (detect) ``time, max_coa, max_coa_n, coord, onset_data`` or
        (locate) ``times, max_coa, max_coa_n, coord, map4d, onset_data``.
        """
        onsets, onset_data = self.onset.calculate_onsets(data)
        eng = self._ensure_table(onset_data.sampling_rate, onset_data.availability)
        fsmp = time2sample(self.pre_pad, onset_data.sampling_rate)
        lsmp = time2sample(self.post_pad, onset_data.sampling_rate)
        avail = int(np.sum([value for _, value in onset_data.availability.items()]))

        # lib.py:93-110 -- same pre-processing and checks, same order
        onsets = np.ascontiguousarray(np.log(np.clip(onsets, 0.01, np.inf)))
        n_onsets, t_samples = onsets.shape
        n_samples = t_samples - fsmp - lsmp
        if n_onsets != eng.n_rows:
            raise ValueError("Mismatch between number of stations for data and LUT, "
                             f"{n_onsets}:{eng.n_rows}")
        if onsets.size < n_samples + fsmp:
            raise ValueError("Data array smaller than coalescence array.")

        series = (np.zeros(n_samples), np.zeros(n_samples),
                  np.zeros(n_samples, dtype=np.int64))
        if self.stage == "detect":
            previous = eng.get("screen")
            if self.screen is not None:
                eng.config("screen", 1 if self.screen else 0)
            try:
                eng.detect(onsets, fsmp, lsmp, avail, out=series)
            finally:
                if self.screen is not None:
                    eng.config("screen", previous)
            map4d = None
        else:
            map4d = np.zeros(tuple(eng.grid) + (n_samples,), dtype=np.double)
            eng.migrate(onsets, fsmp, lsmp, avail, map4d, scan_out=series)
        max_coa, max_coa_n, max_idx = series
        coord = self.lut.index2coord(max_idx, unravel=True)

        if self.stage == "detect":
            time = data.starttime + self.pre_pad
            return time, max_coa, max_coa_n, coord, onset_data
        times = event.mw_times(self.scan_rate)
        return times, max_coa, max_coa_n, coord, map4d, onset_data


    # -- the loop around the path ------------------------------------------------------
    def continuous_compute(self, archive, starttime, n_steps, timestep, scan_rate, sink,
                           steps_per_launch=None, depth=3):
        """
        ``QuakeScan._continuous_compute`` (reference scan.py:407-470): coalescence between two
        timestamps in increments of ``timestep`` -- per timestep read the waveforms, compute the onsets,
        migrate, scan, hand ``(time, max_coa, max_coa_n, coord)`` to ``sink.append`` -- with the
        reference's behaviour around the path: a timestep whose data raise ``ArchiveEmptyException`` /
        ``DataGapException`` / ``DataAvailabilityException`` becomes an all-zero timestep
        (``sink.empty(starttime, timestep, i, e.msg, ucf)``, scan.py:449-458) with an all-zero
        availability row, and ``sink.write()`` closes the run if the last append did not.

        ``archive``: ``read_waveform_data(w_beg, w_end)`` (the reference's ``Archive``);
        ``sink``: the reference's ``ScanmSEED`` duck-typed (``append`` / ``empty`` / ``write`` /
        ``written``; ``quakemigrate_amd.scanmseed.CoalescenceSink`` is one without obspy).
        The window arithmetic is the reference's (``w_beg = starttime + timestep * i - pre_pad``,
        ``w_end = starttime + timestep * (i + 1) - 1 / scan_rate + post_pad``).

        What differs is only WHEN the GPU works: timesteps are independent given their onsets, so
        their log-onsets go through the native pipeline (``qm_stream_*``: H2D, one fused launch per
        ``steps_per_launch`` timesteps, D2H on their own streams) while the host reads and
        pre-processes the next timestep; results reach the sink in timestep order.  A change of
        station availability (another served table) or a data gap drains the pipeline first.

        Waveforms in: an onset plugin that offers ``device_stage(data) -> (signals, OnsetStage, onset_data)`` has
        its detrend, taper, zero-phase band-pass and STA/LTA run on the GPU inside the pipeline's launch
        (``StreamingDetector(..., onset_stage=...)``, ``qm_stream_push_signals``) instead of on the host per
        timestep: ``signals`` are the resampled, not yet filtered, full-timespan traces of the available rows in
        availability order, (n_traces, T) float64; the stage (``quakemigrate_amd.preprocess.OnsetStage``) names
        their filters, windows and row layout.  That 3-tuple is the reference's default, gap-free traces of the full
        timespan (``full_timespan=True, allow_gaps=False``).  Gappy traces (``allow_gaps=True`` /
        ``full_timespan=False``: every segment conditioned on its own, a second taper, tiny-float padding,
        stalta.py:442-461) run on the GPU as well: ``device_stage`` returns ``(signals, stage, onset_data, segments)``
        with ``stage.fill_gaps`` set, ``signals`` in window layout and ``segments`` the list of ``(trace, first, n)``
        that hold data (``quakemigrate_amd.preprocess.plan_segments``); the pipeline is then made on the segment feed
        (``qm_stream_push_segments``) with room for ``4 * n_traces`` segments, and a timestep with more than that
        drains the pipeline and goes through ``calculate_onsets``, as a ``None`` does.  Which channels pass
        ``check_availability`` -- the reference's flatline test on the filtered segments included -- stays the
        plugin's decision.  The ``env`` transforms and -- in this loop -- resampling (the
        device's resampling stage, ``StreamingDetector(resample_stage=...)``, takes a plan of the timestep's raw
        traces; which ones a timestep has, and at what times, is the plugin's ``Stream`` bookkeeping) stay on the host
        plugin path -- ``device_stage`` returns ``None`` for a timestep it cannot describe and ``calculate_onsets`` is
        called for it.  The new path is used on an ``Engine`` or ``EngineReplicas`` only; a group, and a plugin
        without ``device_stage``, run as before.  A changed stage (other windows, filters or layout) makes a new
        pipeline, as a changed table does.

        ``steps_per_launch``: None = 8 on grids of up to a million nodes (where one timestep is a
        fraction of a millisecond and a launch's fixed costs show: x1.04-1.09 of the resident step
        instead of x1.3-1.4), else 1; results do not depend on it.

        Returns the availability rows (list of dicts, one per timestep; scan.py:428, 448, 458).
        """
        from collections import deque

        if self.stage != "detect":
            raise ValueError("continuous_compute is the detect stage's loop")
        ucf = getattr(self.lut, "unit_conversion_factor", 1.0)
        rows = []
        pending = deque()                  # timesteps in the pipeline: (time, onset_data), oldest first
        state = {"stream": None, "key": None}

        def emit(n):
            a, b, c = state["stream"].pop(n)
            for j in range(n):
                time, onset_data = pending.popleft()
                coord = self.lut.index2coord(c[j], unravel=True)
                logging.debug(f"1-D con shape : {a[j].shape}")
                sink.append(time, a[j], b[j], coord, ucf)

        def drain():
            if state["stream"] is not None:
                state["stream"].flush()
                while pending:
                    emit(min(state["stream"].k, len(pending)))

        # (what the pipeline holds when anything else goes wrong mid-run is sunk before the error travels on: the
        # reference has appended every timestep it computed, scan.py:434-448)
        try:
            self._continuous_steps(archive, starttime, timestep, scan_rate, n_steps, sink, ucf, rows, pending,
                                   state, emit, drain, steps_per_launch, depth)
        except BaseException:
            try:
                drain()
            except Exception:  # noqa: BLE001  (the first error is the one to report)
                pass
            raise
        finally:
            if state["stream"] is not None:
                state["stream"].close()
            self._restore_screen(state.get("engine"), state.get("screen_before"))
        if not getattr(sink, "written", False):
            sink.write()
        columns = next((list(r) for r in rows if r is not None), [])
        return [r if r is not None else dict.fromkeys(columns, 0) for r in rows]

    def _apply_screen(self, eng):
        """MigrationScan.screen on the engine for the calls that follow (as _compute does per step); returns what
        to restore."""
        previous = eng.get("screen")
        if self.screen is not None:
            eng.config("screen", 1 if self.screen else 0)
        return previous

    def _restore_screen(self, eng, previous):
        if eng is not None and previous is not None and self.screen is not None:
            eng.config("screen", previous)

    def _continuous_steps(self, archive, starttime, timestep, scan_rate, n_steps, sink, ucf, rows, pending, state,
                          emit, drain, steps_per_launch, depth):
        from quakemigrate_amd.stream import StreamingDetector

        for i in range(n_steps):
            w_beg = _shift(_shift(starttime, timestep * i), -self.pre_pad)
            w_end = _shift(_shift(starttime, timestep * (i + 1) - 1 / scan_rate), self.post_pad)
            logging.debug(f" Processing : {w_beg}-{w_end} ".center(110, "~"))
            device_stage = getattr(self.onset, "device_stage", None)
            if not callable(device_stage) or not isinstance(self.engine, (lib.Engine, lib.EngineReplicas)):
                device_stage = None
            try:
                data = archive.read_waveform_data(w_beg, w_end)
                staged = device_stage(data) if device_stage is not None else None
                segments = None
                if staged is not None and len(staged) == 4:     # gappy waveforms in, where their segments fit the feed
                    segments = list(staged[3])
                    if not staged[1].fill_gaps:
                        raise ValueError("device_stage: segments go with a stage that fills gaps "
                                         "(OnsetStage(fill_gaps=True))")
                    if len(segments) > 4 * staged[1].n_traces:
                        staged = None
                    else:
                        staged = staged[:3]
                elif staged is not None and getattr(staged[1], "fill_gaps", False):
                    raise ValueError("device_stage: a stage that fills gaps needs the timestep's segments "
                                     "(signals, stage, onset_data, segments)")
                if staged is not None:                   # waveforms in: the onsets are made in the launch
                    signals, stage, onset_data = staged
                    onsets = None
                else:
                    stage = signals = None
                    onsets, onset_data = self.onset.calculate_onsets(data)
            except Exception as e:  # noqa: BLE001
                if not _is_no_data(e):
                    raise
                drain()
                sink.empty(starttime, timestep, i, getattr(e, "msg", str(e)), ucf)
                rows.append(None)
                continue
            # (another availability = another table: what is in the pipeline belongs to the one
            # that is resident NOW and has to go through before the engine switches)
            if (onset_data.sampling_rate, tuple(onset_data.availability.items())) != self._resident_key:
                drain()
            eng = self._ensure_table(onset_data.sampling_rate, onset_data.availability)
            if state.get("engine") is None:              # (the scan's `screen` holds for the whole run)
                state["engine"], state["screen_before"] = eng, self._apply_screen(eng)
            fsmp = time2sample(self.pre_pad, onset_data.sampling_rate)
            lsmp = time2sample(self.post_pad, onset_data.sampling_rate)
            avail = int(np.sum([value for _, value in onset_data.availability.items()]))
            if stage is not None:
                signals = np.ascontiguousarray(signals, dtype=np.float64)
                if signals.ndim != 2 or signals.shape[0] != stage.n_traces:
                    raise ValueError(f"device_stage: signals of shape {signals.shape} for a stage of "
                                     f"{stage.n_traces} traces")
                n_onsets, t_samples = stage.n_rows, signals.shape[1]
            else:
                onsets = np.ascontiguousarray(np.log(np.clip(onsets, 0.01, np.inf)))      # lib.py:93-94
                n_onsets, t_samples = onsets.shape
            if n_onsets != eng.n_rows:
                raise ValueError("Mismatch between number of stations for data and LUT, "
                                 f"{n_onsets}:{eng.n_rows}")
            if n_onsets * t_samples < t_samples - lsmp:
                raise ValueError("Data array smaller than coalescence array.")
            # (an Engine or EngineReplicas goes through the native pipeline below -- over every replica for the
            # latter; a group: one timestep after the other, no pipeline)
            if isinstance(eng, lib.EngineGroup):
                a, b, c = eng.detect(onsets, fsmp, lsmp, avail)
                sink.append(_shift(data.starttime, self.pre_pad), a, b, self.lut.index2coord(c, unravel=True), ucf)
                rows.append(dict(onset_data.availability))
                continue
            key = (self._resident_key, t_samples, fsmp, lsmp, avail, stage)
            if key != state["key"]:                      # another table, window shape or onset stage: a new pipeline
                drain()
                if state["stream"] is not None:
                    state["stream"].close()
                k = steps_per_launch if steps_per_launch else (8 if eng.n_nodes <= 1_000_000 else 1)
                state["stream"] = StreamingDetector(eng, n_onsets, t_samples, fsmp, lsmp, avail,
                                                    depth=depth, steps_per_launch=k, onset_stage=stage,
                                                    sampling_rate=onset_data.sampling_rate,
                                                    max_segments=(4 * stage.n_traces if stage is not None
                                                                  and stage.fill_gaps else None))
                state["key"] = key
            stream = state["stream"]
            item = {"log_onsets": onsets, "signals": signals, "segments": (signals, segments)}[stream.feed]
            while not stream.push_step(item):
                emit(min(stream.k, stream.pending()[0]))
            pending.append((_shift(data.starttime, self.pre_pad), onset_data))
            rows.append(dict(onset_data.availability))
        drain()

    def locate_compute(self, archive, triggers, marginal_window, sgm=0.8, cov_thresh=0.90, on_event=None,
                       picker=None, amplitudes=None):
        """
        ``QuakeScan._locate_events``' loop around the path (reference scan.py:472-545), up to and including
        ``_calculate_location``: per triggered event read ``trigger_time -/+ (2 * marginal_window + pad)``
        (scan.py:497-498), compute the onsets, migrate and scan the ``4 * marginal_window * rate + 1``
        samples of ``event.mw_times`` (event.py:398-420); the origin time is the FIRST maximum of the
        coalescence series (``idxmax``, event.py:239-240); an event whose trigger time is not strictly
        inside ``otime -/+ marginal_window`` is dropped (``in_marginal_window``, event.py:369-396), as is
        one whose data raise ``ArchiveEmptyException`` / ``DataGapException`` / ``DataAvailabilityException``
        (scan.py:513-519); the series are trimmed to ``otime - mw <= t <= otime + mw`` and the 4-D map to the
        same samples WITHOUT the last one (``trim2window`` slices ``index[0]:index[-1]``, event.py:430-435:
        the reference's marginal sum runs over one sample fewer than its trimmed series has rows); the
        marginalised map is normalised and fitted three ways (scan.py:719-733).

        What differs is that the 4-D map never exists: the first pass is the fused detect kernel over the
        event's window (series only), which fixes the origin time; the second sums the marginal window's
        samples inside the stacking kernel (``calculate_location``) -- two launches of a few milliseconds
        on a C3-sized grid instead of a 13 GB volume.

        ``triggers``: iterable of ``(uid, trigger_time)``; time stamps only need ``t + timedelta`` /
        ``t + seconds`` (``_shift``).  ``on_event(result)`` is called per located event (the reference writes
        and picks there).  Returns the list of results, each a dict: ``uid, trigger_time, otime, times0``
        (time stamp of the first trimmed sample), ``first_sample, last_sample`` (trimmed series, inclusive,
        in scanned samples), ``max_coa, max_coa_n, coord`` (trimmed), ``coa_map`` (normalised), ``fits``
        (:class:`locate.LocationFits`), ``onset_data``.

        ``picker`` (:class:`quakemigrate_amd.picks.DevicePicker`): the reference's next step, ``pick_phases``
        (pickers/gaussian.py:115-243), on the engine as well.  The onsets are computed again un-logged, with the
        taper windows set to 1 (``onset.calculate_onsets(data, timespan=4 * marginal_window)``, gaussian.py:142-144),
        the hypocentre is the spline location, the traveltimes are ``lut.traveltime_to(phase, ijk, station)`` per
        row, and the result gets ``"picks"`` (the picker's table) before ``on_event`` sees it.

        ``amplitudes`` (:class:`quakemigrate_amd.amplitudes.DeviceAmplitude`): the step after that, the amplitude
        measurements of ``LocalMag.calc_magnitude`` (local_mag/amplitude.py:174-371), on the engine as well.  The
        archive's ``read_wa_waveforms(otime - pre_pad, otime + post_pad)`` -- the pads of ``amplitudes.pad(
        marginal_window, lut.max_traveltime, lut.fraction_tt)`` -- returns the Wood-Anderson displacement traces
        (``id, station, component, starttime, sampling_rate, data``; response removal is the archive's); the
        hypocentre is the location named by ``amplitudes.loc_method``, the traveltimes are the lookup table's, the
        picks are ``result["picks"]`` where a picker ran and the modelled times otherwise, and the result gets
        ``"amplitudes"`` (the reference's table as a dict of columns) before ``on_event`` sees it.
        """
        from quakemigrate_amd import locate

        if self.stage != "locate":
            raise ValueError("locate_compute is the locate stage's loop")
        if amplitudes is not None and not hasattr(archive, "read_wa_waveforms"):
            raise ValueError("locate_compute(amplitudes=...): the archive has no read_wa_waveforms(starttime, endtime) "
                             "(the Wood-Anderson displacement traces of a window)")
        if amplitudes is not None and amplitudes.loc_method not in ("spline", "gaussian", "covariance"):
            raise ValueError(f"loc_method must be 'spline', 'gaussian' or 'covariance', got {amplitudes.loc_method!r}")
        mw = float(marginal_window)
        results = []
        triggers = list(triggers)
        for n, (uid, trigger_time) in enumerate(triggers):
            w_beg = _shift(trigger_time, -2 * mw - self.pre_pad)
            w_end = _shift(trigger_time, 2 * mw + self.post_pad)
            logging.info(f"\tEVENT - {n + 1} of {len(triggers)} - {uid}")
            try:
                data = archive.read_waveform_data(w_beg, w_end)
                onsets, onset_data = self.onset.calculate_onsets(data)
            except Exception as e:  # noqa: BLE001
                if not _is_no_data(e):
                    raise
                logging.info(getattr(e, "msg", str(e)))
                continue
            rate = onset_data.sampling_rate
            eng = self._ensure_table(rate, onset_data.availability)
            fsmp, lsmp = time2sample(self.pre_pad, rate), time2sample(self.post_pad, rate)
            avail = int(np.sum([value for _, value in onset_data.availability.items()]))
            onsets = np.ascontiguousarray(np.log(np.clip(onsets, 0.01, np.inf)))      # lib.py:93-94
            n_onsets, t_samples = onsets.shape
            n_samples = t_samples - fsmp - lsmp
            if n_onsets != eng.n_rows:
                raise ValueError("Mismatch between number of stations for data and LUT, "
                                 f"{n_onsets}:{eng.n_rows}")
            if onsets.size < n_samples + fsmp:
                raise ValueError("Data array smaller than coalescence array.")
            # times[i] below takes the first scanned sample for trigger - 2 mw (event.py:412-420): the window read
            # must hold exactly 4 mw rate + 1 samples (the reference fails on the DataFrame's length otherwise)
            if n_samples != int(round(4 * mw * rate)) + 1:
                raise ValueError(f"Event {uid}: {n_samples} scanned samples where 4 * marginal_window * rate + 1 = "
                                 f"{int(round(4 * mw * rate)) + 1} are expected (pre_pad / post_pad / the archive's "
                                 "window do not match the marginal window)")
            series = (np.zeros(n_samples), np.zeros(n_samples), np.zeros(n_samples, dtype=np.int64))
            screen_before = self._apply_screen(eng)
            try:
                eng.detect(onsets, fsmp, lsmp, avail, out=series)                      # pass 1: the origin time
            finally:
                self._restore_screen(eng, screen_before)
            i_max = int(np.nanargmax(series[0]))                                       # idxmax: the first maximum
            # times[i] = trigger_time - 2 mw + i / rate (event.py:412-420)
            offset = i_max / rate - 2 * mw                                             # otime - trigger_time
            if not (-mw < offset < mw):                                                # event.py:381-383
                logging.info(f"\tEvent {uid} is outside marginal window.")
                continue
            eps = 1e-6                                                                 # (time stamps are whole ns)
            first = max(0, int(np.ceil(i_max - mw * rate - eps)))
            last = min(n_samples - 1, int(np.floor(i_max + mw * rate + eps)))
            if last <= first:
                raise ValueError(f"Event {uid}: the marginal window holds no sample interval (marginal_window "
                                 f"{mw} s at {rate} Hz: samples {first}..{last})")
            marginal = eng.marginal_map(onsets, fsmp, lsmp, avail, first, last)        # pass 2: samples [first, last)
            coa_map = np.zeros_like(marginal)
            fits = locate.calculate_location(eng, marginal, self.lut.node_spacing, sgm=sgm,
                                             cov_thresh=cov_thresh, norm_out=coa_map)
            sel = slice(first, last + 1)
            result = {
                "uid": uid, "trigger_time": trigger_time,
                "otime": _shift(trigger_time, offset), "times0": _shift(trigger_time, first / rate - 2 * mw),
                "first_sample": first, "last_sample": last,
                "max_coa": series[0][sel], "max_coa_n": series[1][sel],
                "coord": self.lut.index2coord(series[2][sel], unravel=True),
                "coa_map": coa_map, "fits": fits, "onset_data": onset_data,
            }
            if picker is not None:
                result["picks"] = self._pick_phases(picker, eng, data, onset_data, result, mw)
            if amplitudes is not None:
                result["amplitudes"] = self._measure_amplitudes(amplitudes, eng, archive, onset_data, result, mw)
            results.append(result)
            if on_event is not None:
                on_event(result)
        return results

    def _pick_phases(self, picker, eng, data, onset_data, result, mw):
        """The located event's picks: one launch over its onset rows (``DevicePicker.pick``)."""
        raw_onsets, raw_data = self.onset.calculate_onsets(data, timespan=4 * mw)      # gaussian.py:142-144
        raw_onsets = np.ascontiguousarray(raw_onsets, dtype=np.float64)
        keys = [key for key, available in raw_data.availability.items() if available]
        ijk = np.asarray(result["fits"].spline, dtype=np.float64)
        traveltimes = []
        for key in keys:
            station, _, phase = key.rpartition("_")
            traveltimes.append(float(np.ravel(self.lut.traveltime_to(phase, ijk, station))[0]))
        return picker.pick(eng, raw_onsets, keys, getattr(raw_data, "starttime", data.starttime),
                           raw_data.sampling_rate, result["otime"], mw, traveltimes,
                           fraction_tt=getattr(self.lut, "fraction_tt", None))

    def _hypocentre_ijk(self, fits, loc_method):
        """The location estimate named by the reference's ``loc_method`` as fractional grid indices: the spline and
        Gaussian fits are that already; the covariance fit's is its expectation, xyz from the grid's lower-left corner
        (``LocationFits.expectation``), over the node spacing."""
        if loc_method in ("spline", "gaussian"):
            ijk = np.asarray(getattr(fits, loc_method), dtype=np.float64)
        elif loc_method == "covariance":
            ijk = np.asarray(fits.expectation, dtype=np.float64) / np.asarray(self.lut.node_spacing, dtype=np.float64)
        else:
            raise ValueError(f"loc_method must be 'spline', 'gaussian' or 'covariance', got {loc_method!r}")
        if ijk.shape != (3,):
            raise ValueError(f"the {loc_method} location has shape {ijk.shape}, (3,) expected")
        return ijk

    def _measure_amplitudes(self, amplitudes, eng, archive, onset_data, result, mw):
        """The located event's amplitude table: one call over its Wood-Anderson traces
        (``DeviceAmplitude.get_amplitudes``).  ``distance_fn``, where the measurer has one, is handed the hypocentre
        as fractional grid indices (``ev_loc``): the transform to geographic coordinates is the caller's, with its
        lookup table."""
        fraction_tt = self.lut.fraction_tt
        pre_pad, post_pad = amplitudes.pad(mw, self.lut.max_traveltime, fraction_tt)
        tr_start, tr_end = _shift(result["otime"], -float(pre_pad)), _shift(result["otime"], float(post_pad))
        wa_traces = archive.read_wa_waveforms(tr_start, tr_end)
        stations = list(dict.fromkeys(key.rpartition("_")[0] for key in onset_data.availability))
        ijk = self._hypocentre_ijk(result["fits"], amplitudes.loc_method)
        p_tt, s_tt = ([float(np.ravel(self.lut.traveltime_to(phase, ijk, station))[0]) for station in stations]
                      for phase in ("P", "S"))
        return amplitudes.get_amplitudes(eng, wa_traces, stations, result.get("picks"), result["otime"], mw, p_tt,
                                         s_tt, fraction_tt, ev_loc=ijk, tr_start=tr_start, tr_end=tr_end)

    def marginal_coalescence(self, data, first_sample, end_sample):
        """
        The marginalised 3-D coalescence map of one event window without the 4-D map: what
        ``event.trim2window()`` + ``np.sum(event.map4d, axis=-1)`` produce in the reference
        (quakemigrate/io/event.py:421-439, signal/scan.py:720), for the scanned samples
        ``[first_sample, end_sample)``.  Returns ``(coa_map (nx, ny, nz), max_coa, max_coa_n,
        max_idx, onset_data)``; the caller normalises by ``nanmax`` as the reference does.
        """
        onsets, onset_data = self.onset.calculate_onsets(data)
        eng = self._ensure_table(onset_data.sampling_rate, onset_data.availability)
        fsmp = time2sample(self.pre_pad, onset_data.sampling_rate)
        lsmp = time2sample(self.post_pad, onset_data.sampling_rate)
        avail = int(np.sum([value for _, value in onset_data.availability.items()]))
        onsets = np.ascontiguousarray(np.log(np.clip(onsets, 0.01, np.inf)))
        n_samples = onsets.shape[1] - fsmp - lsmp
        series = (np.zeros(n_samples), np.zeros(n_samples),
                  np.zeros(n_samples, dtype=np.int64))
        coa_map = eng.marginal_map(onsets, fsmp, lsmp, avail, first_sample, end_sample,
                                   scan_out=series)
        return (coa_map,) + series + (onset_data,)

    def calculate_location(self, data, first_sample, end_sample, sgm=0.8, cov_thresh=0.90):
        """
        ``QuakeScan._calculate_location`` (scan.py:696-733) for the marginal window
        ``[first_sample, end_sample)`` without the 4-D map ever existing: the marginalised map is
        summed inside the stacking kernel, normalised / smoothed / reduced on the GPU, and only
        the two fit windows come back for the Gaussian and spline algebra.

        Returns ``(coa_map, fits, max_coa, max_coa_n, max_idx, onset_data)``: ``coa_map`` is the
        normalised map the reference returns; ``fits`` a :class:`locate.LocationFits` (use
        ``fits.coordinates(self.lut)`` for the reference's lon / lat / depth triplets).
        """
        from quakemigrate_amd import locate

        marginal, max_coa, max_coa_n, max_idx, onset_data = self.marginal_coalescence(
            data, first_sample, end_sample)
        coa_map = np.zeros_like(marginal)
        fits = locate.calculate_location(self.engine, marginal, self.lut.node_spacing, sgm=sgm,
                                         cov_thresh=cov_thresh, norm_out=coa_map)
        return coa_map, fits, max_coa, max_coa_n, max_idx, onset_data
