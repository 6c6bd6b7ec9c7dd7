"""An fp64 statement of STL (Cleveland et al. 1990, as netlib's stl.f computes it) in plain Python floats and scalar
loops, one series at a time, positions 1-based as in the Fortran.  It is the oracle of tests/test_cabi_stl.py and
tests/test_gpu_stl.py and shares no code with csrc/stl_core.h.  `STATS["not_ok"]` counts the `est` calls that found no
positive weight (the `ok = false` branch).  Also here: the series the two test files share and the tolerance they hold.

This is NOT statsmodels and nothing in it was checked against a run of statsmodels."""
import math

import numpy as np

STATS = {"not_ok": 0}
TOL = 1e-12                      # per element, times max|y| of the case: the bound of both test files


def est(y, n, length, deg, xs, nleft, nright, userw, rw):
    """one LOESS value at position xs (0 .. n + 1) from y[nleft .. nright]; y and rw are 1-based (index 0 unused)"""
    h = max(xs - nleft, nright - xs)
    if length > n:
        h += (length - n) // 2
    h = float(h)
    w = [0.0] * (n + 1)
    a = 0.0
    for j in range(nleft, nright + 1):
        r = float(abs(j - xs))
        if r <= 0.999 * h:
            if r <= 0.001 * h:
                w[j] = 1.0
            else:
                q = r / h
                u = 1.0 - q * q * q
                w[j] = u * u * u
            if userw:
                w[j] = w[j] * rw[j]
        a += w[j]
    if a <= 0.0:
        STATS["not_ok"] += 1
        return False, 0.0
    for j in range(nleft, nright + 1):
        w[j] = w[j] / a
    if h > 0.0 and deg > 0:
        a = 0.0
        for j in range(nleft, nright + 1):
            a += w[j] * float(j)
        b = float(xs) - a
        c = 0.0
        for j in range(nleft, nright + 1):
            c += w[j] * (float(j) - a) * (float(j) - a)
        if math.sqrt(c) > 0.001 * float(n - 1):
            b = b / c
            for j in range(nleft, nright + 1):
                w[j] = w[j] * (b * (float(j) - a) + 1.0)
    ys = 0.0
    for j in range(nleft, nright + 1):
        ys += w[j] * y[j]
    return True, ys


def ess(y, n, length, deg, userw, rw):
    """the whole series smoothed with jump 1; 1-based in, 1-based out"""
    ys = [0.0] * (n + 1)
    if n < 2:
        ys[1] = y[1]
        return ys
    if length >= n:
        nleft, nright = 1, n
        for i in range(1, n + 1):
            ok, v = est(y, n, length, deg, i, nleft, nright, userw, rw)
            ys[i] = v if ok else y[i]
        return ys
    nsh = (length + 1) // 2
    nleft, nright = 1, length
    for i in range(1, n + 1):
        if i > nsh and nright != n:
            nleft += 1
            nright += 1
        ok, v = est(y, n, length, deg, i, nleft, nright, userw, rw)
        ys[i] = v if ok else y[i]
    return ys


def moving_average(x, n, length):
    """running-sum moving average of x[1 .. n]: n - length + 1 values, 1-based"""
    newn = n - length + 1
    out = [0.0] * (newn + 1)
    v = 0.0
    for i in range(1, length + 1):
        v += x[i]
    out[1] = v / float(length)
    k, m = length, 0
    for j in range(2, newn + 1):
        k += 1
        m += 1
        v = v - x[m] + x[k]
        out[j] = v / float(length)
    return out


def inner_pass(y, n, np_, ns, nt, nl, isdeg, itdeg, ildeg, userw, rw, trend):
    """one inner pass; returns the new (seasonal, trend), 1-based"""
    w = [0.0] + [y[i] - trend[i] for i in range(1, n + 1)]
    c = [0.0] * (n + 2 * np_ + 1)
    for j in range(1, np_ + 1):
        k = (n - j) // np_ + 1
        sub = [0.0] + [w[(i - 1) * np_ + j] for i in range(1, k + 1)]
        rsub = [0.0] + [rw[(i - 1) * np_ + j] for i in range(1, k + 1)]
        sm = ess(sub, k, ns, isdeg, userw, rsub)
        ok, first = est(sub, k, ns, isdeg, 0, 1, min(ns, k), userw, rsub)
        if not ok:
            first = sm[1]
        ok, last = est(sub, k, ns, isdeg, k + 1, max(1, k - ns + 1), k, userw, rsub)
        if not ok:
            last = sm[k]
        ext = [first] + sm[1:] + [last]                      # positions 0 .. k + 1
        for m in range(0, k + 2):
            c[m * np_ + j] = ext[m]
    a1 = moving_average(c, n + 2 * np_, np_)
    a2 = moving_average(a1, n + np_ + 1, np_)
    a3 = moving_average(a2, n + 2, 3)
    low = ess(a3, n, nl, ildeg, False, rw)
    seasonal = [0.0] + [c[np_ + i] - low[i] for i in range(1, n + 1)]
    d = [0.0] + [y[i] - seasonal[i] for i in range(1, n + 1)]
    return seasonal, ess(d, n, nt, itdeg, userw, rw)


def robustness_weights(y, n, trend, seasonal):
    r = [abs(y[i] - trend[i] - seasonal[i]) for i in range(1, n + 1)]
    s = sorted(r)
    m1 = n // 2 + 1
    m2 = n - m1 + 1
    cmad = 3.0 * (s[m1 - 1] + s[m2 - 1])
    rw = [0.0] * (n + 1)
    for i in range(1, n + 1):
        if r[i - 1] <= 0.001 * cmad:
            rw[i] = 1.0
        elif r[i - 1] <= 0.999 * cmad:
            q = r[i - 1] / cmad
            u = 1.0 - q * q
            rw[i] = u * u
        else:
            rw[i] = 0.0
    return rw, cmad


def stl_series(y, period, seasonal, trend, low_pass, seasonal_deg=1, trend_deg=1, low_pass_deg=1, inner_iter=5, outer_iter=0):
    """STL of one series: fp64 arrays (trend, seasonal, resid, weights) and the cmad behind the weights, repeated T times
    (inf without an outer iteration).  outer_iter + 1 outer passes of inner_iter inner passes each; the robustness weights
    are renewed after every outer pass but the last."""
    n = len(y)
    y1 = [0.0] + [float(v) for v in y]
    tr = [0.0] * (n + 1)
    se = [0.0] * (n + 1)
    rw = [1.0] * (n + 1)
    userw = False
    cmad = math.inf
    k = 0
    while True:
        for _ in range(inner_iter):
            se, tr = inner_pass(y1, n, period, seasonal, trend, low_pass, seasonal_deg, trend_deg, low_pass_deg, userw, rw, tr)
        k += 1
        if k > outer_iter:
            break
        rw, cmad = robustness_weights(y1, n, tr, se)
        userw = True
    t, s = np.array(tr[1:]), np.array(se[1:])
    yv = np.array(y1[1:])
    return t, s, yv - s - t, np.array(rw[1:]), np.full(n, cmad)


_CACHE = {}


def oracle(y, columns=None, **kw):
    """stl_series of the chosen columns of y (T, M): five (T, len(columns)) arrays.  Results are kept per (data, column,
    parameters), so the cases that share a series pay for it once."""
    y = np.asarray(y, dtype=np.float64).reshape(y.shape[0], -1)
    cols = range(y.shape[1]) if columns is None else columns
    out = []
    for c in cols:
        key = (y[:, c].tobytes(), tuple(sorted(kw.items())))
        if key not in _CACHE:
            _CACHE[key] = stl_series(y[:, c], **kw)
        out.append(_CACHE[key])
    return tuple(np.stack([o[i] for o in out], axis=1) for i in range(5))


# ---- the series of the two test files --------------------------------------------------------------------------------------
def closed_form(t_len, period, m, seed=0):
    """y_t = a + b t + s_(t mod p) with sum(s) = 0 over a period, |y| <= 6: (y, trend, seasonal), each (T, m)"""
    rs = np.random.RandomState(seed)
    t = np.arange(t_len, dtype=np.float64)[:, None]
    a = rs.uniform(-1.0, 1.0, (1, m))
    b = rs.uniform(-2.0, 2.0, (1, m)) / t_len
    s = rs.uniform(-1.0, 1.0, (period, m))
    s -= s.mean(axis=0, keepdims=True)
    s -= s.mean(axis=0, keepdims=True)                       # the second pass takes the mean's own rounding out
    seas = s[np.arange(t_len) % period]
    trend = a + b * t
    return trend + seas, trend, seas


def noisy(t_len, period, m, seed=1):
    """a trend, a seasonal cycle and N(0, 0.3) noise, a different mix in every column"""
    rs = np.random.RandomState(seed)
    t = np.arange(t_len, dtype=np.float64)[:, None]
    amp = rs.uniform(0.5, 2.0, (1, m))
    ph = rs.uniform(0.0, 2.0 * np.pi, (1, m))
    return (rs.uniform(-1.0, 1.0, (1, m)) + rs.uniform(-3.0, 3.0, (1, m)) * t / t_len + amp * np.sin(2.0 * np.pi * t / period + ph)
            + 0.3 * rs.standard_normal((t_len, m)))


OUTLIERS = (40, 97, 150)


def contaminated_sine(t_len=181, seed=2):
    """(T, 2): column 0 is sin(2 pi t / 12) + 0.3 noise, column 1 the same with +15 at the three OUTLIERS"""
    rs = np.random.RandomState(seed)
    t = np.arange(t_len, dtype=np.float64)
    clean = np.sin(2.0 * np.pi * t / 12.0) + 0.3 * rs.standard_normal(t_len)
    dirty = clean.copy()
    dirty[list(OUTLIERS)] += 15.0
    return np.stack([clean, dirty], axis=1)


def params(period=12, seasonal=13, trend=None, low_pass=None, seasonal_deg=1, trend_deg=1, low_pass_deg=1, robust=False,
           inner_iter=None, outer_iter=None):
    """the explicit parameter set of a call, with the defaults of section "Defaults and rules" written out here"""
    if trend is None:
        trend = int(math.ceil(1.5 * period / (1.0 - 1.5 / seasonal)))
        trend += 1 if trend % 2 == 0 else 0
    if low_pass is None:
        low_pass = period + 1
        low_pass += 1 if low_pass % 2 == 0 else 0
    if inner_iter is None:
        inner_iter = 2 if robust else 5
    if outer_iter is None:
        outer_iter = 15 if robust else 0
    return dict(period=period, seasonal=seasonal, trend=trend, low_pass=low_pass, seasonal_deg=seasonal_deg, trend_deg=trend_deg,
                low_pass_deg=low_pass_deg, inner_iter=inner_iter, outer_iter=outer_iter)


def ulp32(x):
    """the spacing of fp32 at |x|, elementwise"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def white(t_len, m, seed=0):
    """N(0, 1) noise, (T, m), column c drawn with seed + 4 c"""
    return np.stack([np.random.RandomState(seed + 4 * c).standard_normal(t_len) for c in range(m)], axis=1)


def cases():
    """name -> (y (T, M <= 5), keyword arguments of params(), closed form (trend, seasonal) or None): the case list of the
    host entry, which the device tests run as well"""
    out = {}
    for name, (t_len, period, kw) in {"closed_t181": (181, 12, {}), "closed_t24": (24, 12, {}), "closed_t25": (25, 12, {}),
                                      "closed_t40": (40, 12, {}), "closed_t30_trend35": (30, 12, dict(trend=35)),
                                      "closed_p2_t9": (9, 2, dict(seasonal=7)), "closed_p7_t30": (30, 7, dict(seasonal=7)),
                                      "closed_p12_t30": (30, 12, {})}.items():
        y, tr, se = closed_form(t_len, period, 3, seed=t_len + period)
        out[name] = (y, dict(period=period, **kw), (tr, se))
    out["noisy_t181"] = (noisy(181, 12, 5), {}, None)
    out["noisy_t24"] = (noisy(24, 12, 3), {}, None)                   # subseries of 2 points: len >= n with the (len - n) / 2 term
    out["noisy_t25"] = (noisy(25, 12, 3), {}, None)                   # subseries of 2 and 3 points
    out["noisy_t30_trend35"] = (noisy(30, 12, 3), dict(trend=35), None)   # the trend window is longer than the series
    out["noisy_p2_t9"] = (noisy(9, 2, 3), dict(period=2, seasonal=7), None)
    out["noisy_p7_t30"] = (noisy(30, 7, 3), dict(period=7, seasonal=7), None)
    out["deg_000"] = (noisy(181, 12, 2), dict(seasonal_deg=0, trend_deg=0, low_pass_deg=0), None)
    out["deg_011"] = (noisy(181, 12, 2), dict(seasonal_deg=0), None)
    out["robust"] = (contaminated_sine(), dict(robust=True), None)
    out["robust_1_1"] = (contaminated_sine(), dict(robust=True, inner_iter=1, outer_iter=1), None)
    # white noise on two periods and a sample: whole windows of the short subseries get weight 0, so est reports not ok at
    # positions 0, k + 1 and inside (the oracle counts 20 such calls per column)
    out["not_ok"] = (white(25, 2), dict(robust=True, inner_iter=2, outer_iter=3), None)
    return out


def weight_bound(y, cmad):
    """the bound on |weights - oracle's|: with q = r / cmad and rw = (1 - q^2)^2, |d rw / d r| <= 1.54 / cmad and
    |d rw / d cmad| <= 1 / cmad; r is off by at most d = TOL max|y| and cmad, six times a median of r, by 6 d"""
    return 8.0 * TOL * np.abs(y).max() / cmad
