# -*- coding: utf-8 -*-
"""
NumPy restatement of the phase-pick stage (include/qmhip.h: qm_engine_pick_phases) -- the specification the GPU
tests compare against.  Three parts:

* the reference's rules, line for line (quakemigrate/signal/pickers/gaussian.py: ``_find_pick_threshold``,
  ``_find_peak``, the padding and starting point of ``_fit_gaussian``, ``_distinguish_windows``;
  util.py: ``calculate_mad``, ``gaussian_1d``) -- ``find_pick_threshold``, ``find_peak``, ``distinguish_windows``;
* the solver the kernel runs (``lm_fit``): Levenberg-Marquardt on the 3x3 normal equations with the analytic
  Jacobian, More's scaling, a gain-ratio test and Nielsen's damping update;
* the SciPy yardsticks (``scipy_tight``: ``curve_fit`` with the analytic Jacobian and ftol = xtol = gtol = 1e-15;
  ``scipy_default``: the reference's own call) and the seeded family of onset rows the tests run on.

``pick_rows`` is the C call restated: same arguments, same outputs.  tests/test_picks_host.py pins ``lm_fit`` to
``scipy_tight`` and the rules to the reference's expressions.
"""

import numpy as np

MAX_ITER = 200
STEP_TOL = 1e-13
GAIN_MIN = 1e-4
MAD_SCALE = 1.4826

PICKED, NOTHING_ABOVE, ONE_SAMPLE, LEAVES_TRACE, NOT_CONVERGED, MEAN_OUTSIDE, NON_FINITE = range(7)


class NoOnsetPeak(Exception):
    pass


# -- the reference's rules ---------------------------------------------------------------------------------------
def calculate_mad(x, scale=MAD_SCALE):
    """util.calculate_mad."""
    x = np.asarray(x)
    if not x.size:
        return np.nan
    if np.isnan(np.sum(x)):
        return np.nan
    med = np.apply_over_axes(np.median, x, 0)
    mad = np.median(np.abs(x - med), axis=0)
    return scale * mad


def find_pick_threshold(onset, windows, method="MAD", mad_pick_threshold=8.0, percentile_pick_threshold=1.0):
    """``GaussianPicker._find_pick_threshold``; ``windows``: the [lo, arrival, hi] of every phase of the station."""
    onset_noise = onset.copy()
    for window in windows:
        onset_noise[window[0]:window[2]] = -1
    onset_noise = onset_noise[onset_noise > 1]
    if method == "percentile":
        if not onset_noise.size:
            return np.nan
        return np.percentile(onset_noise, percentile_pick_threshold * 100)
    if not onset_noise.size:                    # (np.median of nothing is nan, with a warning)
        return np.nan
    med = np.median(onset_noise)
    mad = calculate_mad(onset_noise)
    return med + (mad * mad_pick_threshold)


def find_peak(windowed_onset, pick_threshold):
    """``GaussianPicker._find_peak``: [start, end) of the run above the threshold that holds the window's maximum."""
    exceedence = np.where(windowed_onset > pick_threshold)[0]
    if len(exceedence) == 0:
        raise NoOnsetPeak("nothing above the threshold")
    peaks = np.split(exceedence, np.where(np.diff(exceedence) != 1)[0] + 1)
    true_maximum = np.argmax(windowed_onset)
    for i, peak in enumerate(peaks):
        if np.any(peak == true_maximum):
            break
    if len(peaks[i]) < 2:
        raise NoOnsetPeak("a single sample above the threshold")
    return [peaks[i][0], peaks[i][-1] + 1]


def distinguish_windows(windows, samples):
    """``GaussianPicker._distinguish_windows`` on the list of a station's [lo, arrival, hi], in phase order."""
    windows = [list(w) for w in windows]
    first_idx = windows[0][0]
    windows[0][0] = 0 if first_idx < 0 else first_idx
    for w1, w2 in zip(windows[:-1], windows[1:]):
        mid_idx = int((w1[1] + w2[1]) / 2)
        w1[2] = min(mid_idx, w1[2])
        w2[0] = max(mid_idx, w2[0])
    last_idx = windows[-1][2]
    windows[-1][2] = samples if last_idx > samples else last_idx
    return windows


def gaussian_1d(x, a, b, c):
    return a * np.exp(-1.0 * ((x - b) ** 2) / (2 * (c**2)))


def gaussian_jac(x, a, b, c):
    d = x - b
    e = np.exp(-(d * d) / (2 * (c * c)))
    return np.stack([e, a * e * d / (c * c), a * e * d * d / (c * c * c)], axis=1)


# -- the kernel's solver -----------------------------------------------------------------------------------------
def _solve3(s, rhs):
    """Cholesky solve of the symmetric 3x3 ``s``; None where it is not positive definite."""
    l00 = s[0, 0]
    if not l00 > 0.0:
        return None
    l00 = np.sqrt(l00)
    l10, l20 = s[1, 0] / l00, s[2, 0] / l00
    l11 = s[1, 1] - l10 * l10
    if not l11 > 0.0:
        return None
    l11 = np.sqrt(l11)
    l21 = (s[2, 1] - l20 * l10) / l11
    l22 = s[2, 2] - l20 * l20 - l21 * l21
    if not l22 > 0.0:
        return None
    l22 = np.sqrt(l22)
    z0 = rhs[0] / l00
    z1 = (rhs[1] - l10 * z0) / l11
    z2 = (rhs[2] - l20 * z0 - l21 * z1) / l22
    q2 = z2 / l22
    q1 = (z1 - l21 * q2) / l11
    q0 = (z0 - l10 * q1 - l20 * q2) / l00
    return np.array([q0, q1, q2])


def lm_fit(x, y, p0, max_iter=MAX_ITER):
    """
    Least-squares fit of ``a exp(-(x - b)^2 / (2 c^2))`` from ``p0``.  Per iteration: J, A = J'J, g = J'r at p; D =
    running maximum of the column norms sqrt(A_ii); the step solves (A + mu D^2) dp = -g (in the scaled variables
    q = D dp); gain ratio rho = (f - f_new) / (q . (mu q - g / D)); rho > 1e-4 accepts the step and sets
    mu *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; otherwise mu *= nu, nu *= 2.  The iteration ends when every
    |dp_i| <= 1e-13 (|p_i| + 1e-13), whether the step was accepted or not.  Returns (p, iterations, converged).
    """
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    p = np.array(p0, dtype=np.float64)
    r = gaussian_1d(x, *p) - y
    f = float(r @ r)
    d_scale = np.zeros(3)
    mu, nu = 1e-3, 2.0
    with np.errstate(all="ignore"):
        for it in range(1, max_iter + 1):
            jac = gaussian_jac(x, *p)
            r = p[0] * jac[:, 0] - y
            a_mat, g = jac.T @ jac, jac.T @ r
            d_scale = np.fmax(d_scale, np.sqrt(np.diag(a_mat)))
            s = a_mat / np.outer(d_scale, d_scale) + mu * np.eye(3)
            rhs = -g / d_scale
            q = _solve3(s, rhs) if np.all(np.isfinite(s)) and np.all(np.isfinite(rhs)) else None
            rho, dp = -1.0, None
            if q is not None and np.all(np.isfinite(q)):
                dp = q / d_scale
                p_new = p + dp
                r_new = gaussian_1d(x, *p_new) - y
                f_new = float(r_new @ r_new)
                pred = float(q @ (mu * q + rhs))
                if np.isfinite(f_new) and pred > 0.0:
                    rho = (f - f_new) / pred
            small = dp is not None and bool(np.all(np.abs(dp) <= STEP_TOL * (np.abs(p) + STEP_TOL)))
            if rho > GAIN_MIN:
                p, f = p_new, f_new
                t = 2.0 * rho - 1.0
                mu *= max(1.0 / 3.0, 1.0 - t * t * t)
                nu = 2.0
            else:
                mu *= nu
                nu *= 2.0
            if small:
                return p, it, True
    return p, max_iter, False


# -- the C call, restated ----------------------------------------------------------------------------------------
def pick_row(onset, window, threshold, sampling_rate, halfwidth):
    """One row after its threshold: (status, [a, b, |c|, c, f0, f1, iterations]) as the C call writes them."""
    out = np.array([-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, 0.0])
    lo, hi = int(window[0]), int(window[2])
    try:
        peak = find_peak(onset[lo:hi], threshold)
    except NoOnsetPeak as e:
        return (NOTHING_ABOVE if "nothing" in str(e) else ONE_SAMPLE), out
    f0, f1 = lo + peak[0] - 1, lo + peak[1] + 1
    out[4], out[5] = f0, f1
    if f0 < 0 or f1 > len(onset):
        return LEAVES_TRACE, out
    x_data = np.arange(f0, f1) / sampling_rate
    y_data = onset[f0:f1]
    p0 = [max(y_data), (f0 + np.argmax(y_data)) / sampling_rate, halfwidth / sampling_rate]
    popt, iterations, converged = lm_fit(x_data, y_data, p0)
    out[6] = iterations
    if not converged:
        return NOT_CONVERGED, out
    if not lo < popt[1] * sampling_rate < hi:
        return MEAN_OUTSIDE, out
    out[:4] = popt[0], popt[1], abs(popt[2]), popt[2]
    return PICKED, out


def pick_rows(onsets, windows, row_group, sampling_rate, halfwidth, threshold_mode=0, mad_multiplier=8.0,
              thresholds_in=None):
    """``qm_engine_pick_phases``: (picks (n_rows, 8), status (n_rows,))."""
    onsets = np.asarray(onsets, dtype=np.float64)
    n_rows = onsets.shape[0]
    picks, status = np.full((n_rows, 8), -1.0), np.zeros(n_rows, dtype=np.int32)
    for r in range(n_rows):
        picks[r, 7] = 0.0
        if not np.all(np.isfinite(onsets[r])):
            picks[r, 0], status[r] = np.nan, NON_FINITE
            continue
        if threshold_mode == 0:
            group = [windows[k] for k in range(n_rows) if row_group[k] == row_group[r]]
            with np.errstate(all="ignore"):
                picks[r, 0] = find_pick_threshold(onsets[r], group, "MAD", mad_multiplier)
        else:
            picks[r, 0] = thresholds_in[r]
        status[r], picks[r, 1:] = pick_row(onsets[r], windows[r], picks[r, 0], sampling_rate, halfwidth[r])
    return picks, status


# -- yardsticks --------------------------------------------------------------------------------------------------
def fit_inputs(onset, f0, f1, sampling_rate, halfwidth):
    """x, y, p0 of ``_fit_gaussian`` for the fit range [f0, f1)."""
    x_data = np.arange(f0, f1) / sampling_rate
    y_data = onset[f0:f1]
    p0 = [max(y_data), (f0 + np.argmax(y_data)) / sampling_rate, halfwidth / sampling_rate]
    return x_data, y_data, p0


def scipy_tight(x, y, p0):
    """The minimum: ``curve_fit`` with the analytic Jacobian and every tolerance at 1e-15."""
    from scipy.optimize import curve_fit

    popt, _ = curve_fit(gaussian_1d, x, y, p0, jac=gaussian_jac, ftol=1e-15, xtol=1e-15, gtol=1e-15,
                        maxfev=20000)
    return popt


def scipy_default(x, y, p0):
    """The reference's own call (gaussian.py:438); raises what it raises there."""
    from scipy.optimize import curve_fit

    popt, _ = curve_fit(gaussian_1d, x, y, p0)
    return popt


def fit_distance(p, q, sampling_rate):
    """max(|da| / |a|, |db| rate, |d|c|| / |c|): amplitude and sigma relative, mean in samples (q: the yardstick)."""
    return max(abs(p[0] - q[0]) / abs(q[0]), abs(p[1] - q[1]) * sampling_rate,
               abs(abs(p[2]) - abs(q[2])) / abs(q[2]))


# -- the family --------------------------------------------------------------------------------------------------
def family(seed=7, n_stations=80, t_samples=451, sampling_rate=50.0, pads=(20, 15)):
    """
    Onset rows of ``n_stations`` stations, P rows first, then S rows: smoothed noise around 1.3, one asymmetric bump
    per row (amplitude 0.3-30, widths 1.5-12 samples, up to 25 samples off the modelled arrival), the first
    ``pads[0]`` and last ``pads[1]`` samples set to 1 (the taper pads).  Returns a dict: onsets, windows (n_rows, 3)
    after ``distinguish_windows``, row_group (the station), halfwidth (samples), sampling_rate.
    """
    rng = np.random.default_rng(seed)
    n_rows, t = 2 * n_stations, np.arange(t_samples, dtype=np.float64)
    white = rng.normal(0.0, 0.12, size=(n_rows, t_samples + 8))
    kernel = np.ones(9) / 9.0
    onsets = 1.3 + 3.0 * np.stack([np.convolve(w, kernel, mode="valid") for w in white])
    arrival_p = rng.integers(110, 200, size=n_stations)
    arrival_s = arrival_p + rng.integers(30, 150, size=n_stations)
    arrival = np.concatenate([arrival_p, arrival_s])
    half = np.concatenate([rng.integers(50, 61, size=n_stations), rng.integers(50, 71, size=n_stations)])
    amplitude = np.exp(rng.uniform(np.log(0.3), np.log(30.0), size=n_rows))
    left, right = rng.uniform(1.5, 12.0, size=n_rows), rng.uniform(1.5, 12.0, size=n_rows)
    centre = arrival + rng.uniform(-25.0, 25.0, size=n_rows)
    for r in range(n_rows):
        d = t - centre[r]
        onsets[r] += amplitude[r] * np.exp(-d * d / (2.0 * np.where(d < 0, left[r], right[r]) ** 2))
    onsets[:, :pads[0]] = 1.0
    onsets[:, t_samples - pads[1]:] = 1.0
    windows = np.zeros((n_rows, 3), dtype=np.int32)
    for s in range(n_stations):
        rows = (s, n_stations + s)
        raw = [[arrival[r] - half[r], arrival[r], arrival[r] + half[r]] for r in rows]
        for r, w in zip(rows, distinguish_windows(raw, t_samples)):
            windows[r] = w
    return dict(onsets=np.ascontiguousarray(onsets), windows=windows,
                row_group=np.concatenate([np.arange(n_stations), np.arange(n_stations)]).astype(np.int32),
                halfwidth=np.concatenate([np.full(n_stations, 5.0), np.full(n_stations, 10.0)]),
                sampling_rate=float(sampling_rate))


_cache = {}


def family_results(**kw):
    """The family, ``pick_rows`` on it and, per row with a fit range inside the trace, the two SciPy fits -- computed
    once per process and shared (``tight`` / ``default``: row -> popt, or the exception the call raised)."""
    key = tuple(sorted(kw.items()))
    if key not in _cache:
        import warnings

        fam = family(**kw)
        picks, status = pick_rows(fam["onsets"], fam["windows"], fam["row_group"], fam["sampling_rate"],
                                  fam["halfwidth"])
        tight, default = {}, {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for r in np.flatnonzero(np.isin(status, (PICKED, NOT_CONVERGED, MEAN_OUTSIDE))):
                x, y, p0 = fit_inputs(fam["onsets"][r], int(picks[r, 5]), int(picks[r, 6]), fam["sampling_rate"],
                                      fam["halfwidth"][r])
                for store, fit in ((tight, scipy_tight), (default, scipy_default)):
                    try:
                        store[r] = fit(x, y, p0)
                    except (ValueError, RuntimeError) as e:
                        store[r] = e
        _cache[key] = dict(fam, picks=picks, status=status, tight=tight, default=default)
    return _cache[key]


# -- designed rows -----------------------------------------------------------------------------------------------
def designed_rows(t_samples=700, sampling_rate=50.0):
    """
    One call's worth of rows, each the smallest case of its kind.  Returns a dict like ``family`` plus ``names``
    and ``expected`` (the status each row is built to give).  The noise is a fixed ripple of +/- 0.05 around 1.3
    (threshold near 1.9 with the default multiplier) unless the row says otherwise.
    """
    T = t_samples
    t = np.arange(T, dtype=np.float64)
    rng = np.random.default_rng(11)
    rows = []

    def base():
        return 1.3 + 0.05 * np.sin(0.7 * t) + 0.02 * rng.standard_normal(T)

    def bump(y, centre, amplitude, width):
        y += amplitude * np.exp(-((t - centre) ** 2) / (2.0 * width * width))
        return y

    def add(name, y, window, expected, group=None, halfwidth=5.0):
        rows.append(dict(name=name, y=y, window=list(window), expected=expected,
                         group=len(rows) + 1000 if group is None else group, halfwidth=halfwidth))

    y = base(); y[300], y[301] = 5.0, 4.0
    add("run of two samples", y, (250, 300, 350), PICKED)
    y = base(); y[300] = 5.0
    add("run of one sample", y, (250, 300, 350), ONE_SAMPLE)
    add("nothing above the threshold", base(), (250, 300, 350), NOTHING_ABOVE)
    add("two runs, the maximum in the second", bump(bump(base(), 270, 3.0, 3.0), 320, 6.0, 4.0), (230, 300, 370),
        PICKED)
    y = base(); y[288:293] = [3.0, 4.5, 6.0, 4.5, 3.0]; y[318:323] = [3.0, 4.5, 6.0, 4.5, 3.0]
    add("tied maximum in two runs", y, (230, 300, 370), PICKED)
    y = base(); y[298:304] = [3.0, 4.5, 6.0, 6.0, 4.5, 3.0]
    add("tied maximum in one run", y, (230, 300, 370), PICKED)
    add("fit range of more than 64 points", bump(base(), 330, 10.0, 20.0), (200, 320, 460), PICKED, halfwidth=10.0)
    add("fit range of more than 256 points", bump(base(), 375, 10.0, 80.0), (150, 370, 600), PICKED,
        halfwidth=40.0)
    add("noise set of none", bump(base(), 330, 6.0, 4.0), (0, 330, T), NOTHING_ABOVE)
    y = np.ones(T); y[40] = 1.5; bump(y, 330, 6.0, 4.0)
    add("noise set of one", y, (250, 330, 400), PICKED)
    y = np.ones(T); y[40], y[600] = 1.4, 1.6; bump(y, 330, 6.0, 4.0)
    add("noise set of two", y, (250, 330, 400), PICKED)
    y = np.ones(T); y[40], y[600], y[601] = 1.4, 1.6, 1.7; bump(y, 330, 6.0, 4.0)
    add("noise set of three", y, (250, 330, 400), PICKED)
    y = bump(base(), 330, 6.0, 4.0); y[0] = 1.0
    y[1] = 1.0 if np.count_nonzero(np.concatenate([y[:250], y[400:]]) > 1) % 2 == 0 else y[1]
    add("noise set of an odd number", y, (250, 330, 400), PICKED)
    y = np.full(T, 1.25); y[250:400] = 1.2; bump(y, 330, 6.0, 4.0)
    add("constant noise", y, (250, 330, 400), PICKED)
    add("window touching 0", bump(base(), 50, 6.0, 4.0), (0, 50, 100), PICKED)
    add("window touching T", bump(base(), T - 50, 6.0, 4.0), (T - 100, T - 50, T), PICKED)
    y = base(); y[0:4] = [5.0, 6.0, 5.0, 4.0]
    add("run touching sample 0", y, (0, 40, 100), LEAVES_TRACE)
    y = base(); y[T - 4:] = [4.0, 5.0, 6.0, 5.0]
    add("run touching the last sample", y, (T - 100, T - 40, T), LEAVES_TRACE)
    add("one-phase group", bump(base(), 310, 6.0, 4.0), (250, 300, 350), PICKED, group=1)
    three = distinguish_windows([[140, 200, 260], [190, 250, 310], [270, 330, 390]], T)
    for k, (w, c) in enumerate(zip(three, (205, 262, 335))):
        add(f"three-phase group, phase {k}", bump(base(), c, 6.0, 4.0), w, PICKED, group=2)
    y = bump(base(), 310, 6.0, 4.0); y[500] = np.nan
    add("NaN row", y, (250, 300, 350), NON_FINITE)
    y = bump(base(), 310, 6.0, 4.0); y[20] = np.inf
    add("infinite sample outside the window", y, (250, 300, 350), NON_FINITE)
    # a rising exponential up to the window's end: the least-squares Gaussian runs off to b, c -> infinity
    y = base(); y[260:301] = 2.0 * np.exp(0.08 * (t[260:301] - 260.0))
    add("no minimum: a rising exponential", y, (200, 280, 300), NOT_CONVERGED)
    return dict(onsets=np.ascontiguousarray(np.stack([r["y"] for r in rows])),
                windows=np.array([r["window"] for r in rows], dtype=np.int32),
                row_group=np.array([r["group"] for r in rows], dtype=np.int32),
                halfwidth=np.array([r["halfwidth"] for r in rows]), sampling_rate=float(sampling_rate),
                names=[r["name"] for r in rows], expected=np.array([r["expected"] for r in rows], dtype=np.int32))


# -- noise sets at the median's edges ------------------------------------------------------------------------------
NOISE_SIZES = (0, 1, 2, 3, 4, 255, 256, 257)
NOISE_KINDS = ("distinct", "all equal", "two middle values equal", "middle value across the even split",
               "last bit apart")


def noise_values(n, kind, rng):
    """``n`` values above 1, in sorted order, of one of ``NOISE_KINDS``."""
    v = np.sort(1.0 + 0.25 * (1 + np.arange(n)) / (n + 1) + 1e-3 * rng.random(n))
    if kind == "all equal":
        v[:] = 1.75
    elif kind == "two middle values equal" and n > 1:
        v[n // 2 - 1] = v[n // 2]
    elif kind == "middle value across the even split" and n > 1:
        v[n // 4:n - n // 4] = v[n // 2]
    elif kind == "last bit apart":
        v = 1.5 + np.arange(n) * np.spacing(1.5)
    return v


def noise_set_rows(t_samples=331, window=(40, 70, 100), sampling_rate=50.0, seed=5):
    """
    One row per (size, kind) of ``NOISE_SIZES`` x ``NOISE_KINDS``, each a station of its own: the noise set -- the
    samples above 1 outside the row's window -- has that size and those values at shuffled places, every other sample
    is 0.5 (nothing in the window exceeds any threshold: status 1 throughout).  Returns a dict like ``family`` plus
    ``names`` and ``noise`` (each row's values, sorted).
    """
    rng = np.random.default_rng(seed)
    outside = np.concatenate([np.arange(window[0]), np.arange(window[2], t_samples)])
    names, noise, rows = [], [], []
    for n in NOISE_SIZES:
        for kind in NOISE_KINDS:
            y = np.full(t_samples, 0.5)
            v = noise_values(n, kind, rng)
            y[rng.permutation(outside)[:n]] = rng.permutation(v)
            names.append(f"{n} {kind}")
            noise.append(v)
            rows.append(y)
    n_rows = len(rows)
    return dict(onsets=np.ascontiguousarray(np.stack(rows)),
                windows=np.tile(np.array(window, dtype=np.int32), (n_rows, 1)), row_group=np.arange(n_rows, dtype=np.int32), halfwidth=np.full(n_rows, 5.0),
                sampling_rate=float(sampling_rate), names=names, noise=noise)
