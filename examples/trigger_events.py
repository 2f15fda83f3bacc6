# -*- coding: utf-8 -*-
"""
Detect, trigger, locate -- the reference's three stages on the GPU engine, each feeding the next.

``QuakeScan.detect()`` writes a day's coalescence series to ``.scanmseed``; ``Trigger.trigger()`` reads them back,
thresholds the series, merges what exceeds it into events and writes ``TriggeredEvents.csv``
(quakemigrate/signal/trigger.py:273-380); ``QuakeScan.locate()`` takes the events one by one.  Here
``MigrationScan.continuous_compute`` fills a ``CoalescenceSink`` (examples/continuous_detect.py),
``trigger.DeviceTrigger.trigger`` runs the trigger stage on the engine over the day files the sink wrote -- smoothing,
threshold, candidates and merge are kernels (include/qmhip.h: ``qm_engine_trigger``), the time window and the
``EventID`` host rules -- and ``MigrationScan.locate_compute`` locates what it returns
(examples/locate_events.py).  Everything is synthetic and obspy-free; the run crosses midnight, so two day files are
triggered as two batches.

Run:  python examples/trigger_events.py [out_dir]
"""

import datetime as dt
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from quakemigrate_amd import scan, scanmseed, synth, trigger  # noqa: E402


def run(out_dir, n_steps=12, grid=(36, 32, 20), rows=12, rate=50, n_samples=600, marginal_window=0.5,
        static_threshold=7.5):
    """One synthetic event per timestep of ``n_samples / rate`` seconds.  Returns ``(events, located, truth)``:
    the triggered events, ``locate_compute``'s results and, per timestep, ``(node, origin time)`` of its event."""
    mw, spacing, ucf = marginal_window, 0.5, 1000.0
    cases = [synth.make_case("C3", step=s, grid=grid, rows=rows, n_samples=n_samples, n_events=1, table=(s == 0))
             for s in range(n_steps)]
    c0 = cases[0]
    keys = [f"ST{i % (rows // 2)}_{'P' if i < rows // 2 else 'S'}" for i in range(rows)]
    timestep, pre, post = n_samples / rate, c0.fsmp / rate, c0.lsmp / rate
    t0 = dt.datetime(2024, 5, 17, 23, 58, 0)               # (the run crosses midnight: two files, two batches)
    step_start = [t0 + dt.timedelta(seconds=timestep * s) for s in range(n_steps)]
    truth = [(c.event_nodes[0][0], step_start[s] + dt.timedelta(seconds=c.event_nodes[0][1] / rate))
             for s, c in enumerate(cases)]

    class Data:
        def __init__(self, onsets, starttime):
            self.onsets, self.starttime = onsets, starttime

    class Archive:                                          # a window of ONE timestep's record
        def __init__(self, lead=0.0):
            self.lead = lead                                # seconds the scanned window starts before its subject

        def read_waveform_data(self, w_beg, w_end):
            since = (w_beg - t0).total_seconds() + pre      # the first scanned sample, from the start of the run
            s = int((since + self.lead + 1e-6) // timestep)
            n = int(round((w_end - w_beg).total_seconds() * rate)) + 1
            first = int(round((since - s * timestep) * rate)) if 0 <= s < n_steps else -1
            if first < 0 or first + n > cases[s].onsets.shape[1]:
                raise scan.DataGapException(f"no record covers {w_beg} to {w_end}")
            return Data(cases[s].onsets[:, first:first + n], w_beg)

    class OnsetData:
        sampling_rate = rate
        availability = dict.fromkeys(keys, 1)

        def __init__(self, starttime):
            self.starttime = starttime

    class Onset:
        def calculate_onsets(self, data, timespan=None):
            return data.onsets, OnsetData(data.starttime)

    class Lut:
        unit_conversion_factor = ucf
        node_spacing = np.array([spacing] * 3)
        fraction_tt = 0.1

        def serve_traveltimes(self, sampling_rate, availability):
            return c0.traveltimes

        def index2coord(self, idx, unravel=True):
            return np.stack(np.unravel_index(idx, grid), axis=-1) * spacing

    # detect: the coalescence series of the run, one .scanmseed per day
    detect = scan.MigrationScan(Lut(), Onset(), pre, post, stage="detect")
    sink = scanmseed.CoalescenceSink(out_dir, rate, engine=detect.engine)    # (the day files are packed on the GPU)
    detect.continuous_compute(Archive(), t0, n_steps, timestep, rate, sink)

    # trigger: the day files in, events out
    trig = trigger.DeviceTrigger(threshold_method="static", static_threshold=static_threshold, marginal_window=mw,
                                 min_event_interval=2 * mw, pad=10.0)
    end = t0 + dt.timedelta(seconds=timestep * n_steps)
    events = trig.trigger(sink.directory, t0, end, ucf, engine=detect.engine)
    trigger.write_triggered_events(sink.directory / "TriggeredEvents.csv", events)

    # locate: the triggered events, one by one (an event's window starts 2 mw before its trigger time: the record is
    # the one that holds the trigger)
    locate = scan.MigrationScan(Lut(), Onset(), pre, post, stage="locate", scan_rate=rate, engine=detect.engine)
    located = locate.locate_compute(Archive(lead=2 * mw), trigger.triggers(events), mw)
    return events, located, truth


if __name__ == "__main__":
    out = pathlib.Path(sys.argv[1] if len(sys.argv) > 1 else "trigger_events_out")
    events, located, truth = run(out)
    print(f"{len(events)} events triggered from {len(truth)} timesteps -> {out / 'TriggeredEvents.csv'}")
    by_uid = {r["uid"]: r for r in located}
    for ev in events:
        near = min(truth, key=lambda nt: abs((nt[1] - ev["CoaTime"]).total_seconds()))
        line = f"{ev['EventID']}: COA {ev['COA']:.2f} at {trigger.stamp(ev['CoaTime'])} (truth {trigger.stamp(near[1])})"
        r = by_uid.get(ev["EventID"])
        if r is not None:
            line += f", located at node {np.round(r['fits'].spline, 2)} (truth {near[0]})"
        print(line)
