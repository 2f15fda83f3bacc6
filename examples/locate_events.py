# -*- coding: utf-8 -*-
"""
The reference's locate loop on the GPU engine, up to and including the location fits.

``QuakeScan._locate_events`` (quakemigrate/signal/scan.py:472-545) reads ``trigger_time -/+ (2 *
marginal_window + pad)`` per triggered event, computes the onsets and the 4-D coalescence map, takes the
time of the maximum as the origin time, drops the event if its trigger time is not inside ``origin -/+
marginal_window``, trims the map to that window, marginalises it over time and fits three locations.
``MigrationScan(stage="locate").locate_compute`` is that loop with the same plugin objects and the same
rules -- without the 4-D map: one fused detect launch over the event's window fixes the origin time, one
marginal-map launch sums the window inside the stacking kernel.  With a ``picker`` the phase picks follow on the
engine too (``quakemigrate_amd.picks.DevicePicker`` for the reference's ``GaussianPicker``: one launch over the
event's onset rows).  With ``--amplitudes`` the amplitude measurements of ``LocalMag`` follow as well
(``quakemigrate_amd.amplitudes.DeviceAmplitude`` for the reference's ``Amplitude``, on synthetic Wood-Anderson traces).
The magnitude algebra and the event files remain the reference's (``on_event`` is where they would be called).
Everything here is synthetic and obspy-free.

Run:  python examples/locate_events.py [--amplitudes]
"""

import datetime as dt
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from quakemigrate_amd import picks, scan, synth  # noqa: E402


WA_RATE = 100.0                                             # Hz, the synthetic Wood-Anderson traces
WA_COMPONENTS = ("E", "N", "Z")


def wa_trace(record, station, component, starttime, npts, arrivals):
    """One synthetic Wood-Anderson displacement trace (metres): seeded noise with a decaying wavelet at each of the
    ``arrivals`` (seconds after ``starttime``), the S wavelet three times the P one."""
    rng = np.random.default_rng([record, station, WA_COMPONENTS.index(component)])
    t = np.arange(npts) / WA_RATE
    x = 2e-7 * rng.standard_normal(npts)
    for k, at in enumerate(arrivals):
        since = np.clip(t - at, 0.0, None)
        x += (1 + 2 * k) * 4e-6 * since * np.exp(-3.0 * since) * np.sin(2 * np.pi * (6.0 - 2 * k) * since) * 8
    return dict(id=f"XX.ST{station}..HH{component}", station=f"ST{station}", component=component,
                starttime=starttime, sampling_rate=WA_RATE, data=x)


def run(grid=(36, 32, 20), rows=12, rate=50, marginal_window=1.0, n_events=5, with_picker=True,
        on_event=None, amplitudes=None):
    """``n_events`` synthetic events, one per trigger, each somewhere inside a 12-s record; the trigger
    times are what a detect run would hand over: within a fraction of the marginal window of the truth.
    (The third record ends too early for its event's window: the archive raises, the event is dropped.)
    ``with_picker=False`` stops after the location fits; ``on_event`` is handed to ``locate_compute``, as is
    ``amplitudes`` (a ``quakemigrate_amd.amplitudes.DeviceAmplitude``: the amplitude table per event, measured on
    synthetic Wood-Anderson traces -- three components per station, half a second longer than the window asked for on
    either side)."""
    mw, spacing = marginal_window, 0.5
    n_win = int(4 * mw * rate) + 1
    cases = [synth.make_case("C3", step=10 + s, grid=grid, rows=rows, n_samples=600, n_events=1,
                             table=(s == 0)) for s in range(n_events)]
    c0 = cases[0]
    keys = [f"ST{i % (rows // 2)}_{'P' if i < rows // 2 else 'S'}" for i in range(rows)]
    pre, post = c0.fsmp / rate, c0.lsmp / rate
    day = dt.datetime(2024, 5, 17, 10, 0, 0)
    # the event of record s has its origin at scanned sample t0 of that record; the trigger is 0.2 s late
    truth = [(c.event_nodes[0][0], c.event_nodes[0][1]) for c in cases]
    record_start = [day + dt.timedelta(seconds=60 * s) for s in range(n_events)]
    triggers = [(f"event_{s}", record_start[s] + dt.timedelta(seconds=truth[s][1] / rate + 0.2))
                for s in range(n_events)]

    record_of = {t - dt.timedelta(seconds=2 * mw + pre): s for s, (_, t) in enumerate(triggers)}

    class Data:
        pass

    class Archive:                                          # what the reference's Archive does for a window
        def read_waveform_data(self, w_beg, w_end):
            s = record_of[w_beg]
            first = int(round(((w_beg - record_start[s]).total_seconds() + pre) * rate))   # scanned sample
            n = int(round((w_end - w_beg).total_seconds() * rate)) + 1
            if first < 0 or first + n > cases[s].onsets.shape[1]:
                raise scan.DataGapException(f"the record of {triggers[s][0]} does not cover its window")
            d = Data()
            d.onsets, d.starttime = cases[s].onsets[:, first:first + n], w_beg
            return d

        def read_wa_waveforms(self, w_beg, w_end):
            s = min(range(n_events), key=lambda k: abs((w_beg - record_start[k]).total_seconds()))
            start = w_beg - dt.timedelta(seconds=0.5)
            npts = int(round(((w_end - w_beg).total_seconds() + 1.0) * WA_RATE)) + 1
            origin = (record_start[s] - start).total_seconds() + truth[s][1] / rate
            xyz = np.asarray(truth[s][0], dtype=np.float64) * spacing
            traces = []
            for k in range(rows // 2):
                tt = [np.sqrt(((c0.stations[row] - xyz) ** 2).sum()) / c0.velocities[row] for row in (k, k + rows // 2)]
                traces += [wa_trace(s, k, comp, start, npts, [origin + v for v in tt]) for comp in WA_COMPONENTS]
            return traces

    class OnsetData:
        sampling_rate = rate
        availability = dict.fromkeys(keys, 1)

        def __init__(self, starttime):
            self.starttime = starttime

    class Onset:
        taper_pad = 10                                      # samples of either end a taper would have touched

        def calculate_onsets(self, data, timespan=None):
            onsets = data.onsets
            if timespan:                                    # the picker's call: un-logged, taper windows set to 1
                onsets = onsets.copy()
                onsets[:, :self.taper_pad] = 1.0
                onsets[:, onsets.shape[1] - self.taper_pad:] = 1.0
            return onsets, OnsetData(data.starttime)

        def gaussian_halfwidth(self, phase):                # samples (the reference: half a short-term window)
            return 5.0 if phase == "P" else 7.5

    class Lut:
        node_spacing = np.array([spacing] * 3)
        fraction_tt = 0.1
        max_traveltime = float(np.max(c0.traveltimes)) / rate

        def traveltime_to(self, phase, ijk, station):       # homogeneous velocities: no interpolation needed
            row = keys.index(f"{station}_{phase}")
            xyz = np.asarray(ijk, dtype=np.float64) * spacing
            return np.array([np.sqrt(((c0.stations[row] - xyz) ** 2).sum()) / c0.velocities[row]])

        def serve_traveltimes(self, sampling_rate, availability):
            return c0.traveltimes

        def index2coord(self, idx, unravel=True):
            return np.stack(np.unravel_index(idx, grid), axis=-1) * spacing

    s = scan.MigrationScan(Lut(), Onset(), pre, post, stage="locate", scan_rate=rate)
    located = s.locate_compute(Archive(), triggers, mw, on_event=on_event,
                               picker=picks.DevicePicker(s.onset) if with_picker else None, amplitudes=amplitudes)
    assert all(r["max_coa"].shape[0] <= n_win for r in located)
    return located, truth, record_start, rate


if __name__ == "__main__":
    measure = None
    if "--amplitudes" in sys.argv[1:]:                      # the step after the picks: the local-magnitude amplitudes
        from quakemigrate_amd.amplitudes import DeviceAmplitude

        measure = DeviceAmplitude({"signal_window": 1.0, "bandpass_filter": True, "bandpass_lowcut": 1.0,
                                   "bandpass_highcut": 20.0})
    located, truth, record_start, rate = run(amplitudes=measure)
    for r in located:
        k = int(r["uid"].split("_")[1])
        (node, t0), start = truth[k], record_start[k]
        origin = (r["otime"] - start).total_seconds() * rate
        print(f"{r['uid']}: origin sample {origin:.0f} (truth {t0}), spline node {np.round(r['fits'].spline, 2)}, "
              f"gaussian {np.round(r['fits'].gaussian, 2)} (truth {node}), "
              f"marginal window {r['last_sample'] - r['first_sample']} samples")
        p = r["picks"]
        for i in range(len(p["Station"])):
            made = (f"pick {(p['PickTime'][i] - start).total_seconds():.3f} s +/- {p['PickError'][i]:.3f} s, SNR "
                    f"{p['SNR'][i]:.1f}, residual {p['Residual'][i]:+.3f} s" if p["status"][i] == 0
                    else f"no pick (status {p['status'][i]})")
            print(f"    {p['Station'][i]} {p['Phase'][i]}: modelled "
                  f"{(p['ModelledTime'][i] - start).total_seconds():.3f} s, {made}")
        a = r.get("amplitudes")
        for i in range(len(a["id"]) if a else 0):
            print(f"    {a['id'][i]}: P {a['P_amp'][i]:.4g} mm at {a['P_freq'][i]:.3g} Hz, S {a['S_amp'][i]:.4g} mm at "
                  f"{a['S_freq'][i]:.3g} Hz, noise {a['Noise_amp'][i]:.3g} mm, picked {a['is_picked'][i]}")
