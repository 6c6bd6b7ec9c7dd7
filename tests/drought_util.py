"""Oracles and bounds for the drought tests (test_cabi_drought.py, test_gpu_drought.py).  Nothing here shares code with
csrc/drought_core.h: the climatology comes from exact rational arithmetic (fractions), the parametric indices from numpy
longdouble on the exact climatology, the rank indices from scipy.stats.rankdata(method="average") per calendar slot, the
events from itertools.groupby over the dry flags with math.fsum for the severities, the area series from numpy.

Test data: seeded AR(1) noise quantised to multiples of 1/8 (so equal samples, samples exactly on a threshold that is a
multiple of 1/8 and runs of every short length occur), column 1 with a one-step NaN gap, column 2 with a many-step gap,
column 3 all NaN, column 4 constant (M2 == 0).  Every case is a corner [:T, :M] of one base array, so a column's oracle does
not depend on M and is computed once.

Bounds (derived, not measured).  u = 2^-53, g(k) = k u / (1 - k u).  For one slot with the n samples x_1 .. x_n in time
order, X = max |x_k|, exact running means m_k (m_0 = 0), d_k = x_k - m_(k-1), and the recurrence of the kernel
    m^_k = fl(m^_(k-1) + fl(fl(x_k - m^_(k-1)) * fl(1 / k))),   M2^_k = fl(M2^_(k-1) + fl(fl(d^_k * d^_k) * fl((k - 1) * fl(1 / k)))):
  mean   the increment carries three roundings (subtraction, reciprocal, product), |d_k| <= 2 X, and the sum one more on
         |m_k| <= X: a local error <= (6 / k + 1) u X per step.  An error e in m_(k-1) enters m_k as e (1 - 1 / k), so the
         local error of step k reaches the end damped by k / n:  |m^_n - m_n| <= 6 u X + u X (n + 1) / 2 <= g(n + 8) X =: E.
  M2     the exact M2 is sum d_k^2 (k - 1) / k (Welford).  The computed term is (d_k - e_(k-1))^2 (k - 1) / k (1 + theta_6)
         (subtraction, square, reciprocal, two products: six roundings with the squared one), |e| <= E, and the n sums of
         non-negative terms add g(n):  |M2^ - M2| <= g(n + 6) M2 + 2.01 E sum |d_k| + 1.01 n E^2 =: E2.
  anomaly        a^ = fl(x - m^):  |a^ - a| <= E + u (|a| + E) =: Ea;  fp32 storage adds 2^-24 (|a| + Ea) (+ 2^-150).
  standardized   sd^ = fl(sqrt(fl(M2^ / dof))) = sd (1 + rho'), |rho'| <= rho = E2 / M2 + 2 u (the square root at most
         keeps the relative error of M2, and adds its own and the division's rounding);  z^ = fl(a^ / sd^):
         |z^ - z| <= (Ea / sd + |z| rho) / (1 - rho) + u (|z| + that) =: Ez;  fp32 storage adds 2^-24 (|z| + Ez).
  severity       sums of d fp64 terms (threshold - v), each formed as the kernel forms it: an event's terms in time order,
         then the events in time order -- any term passes through fewer than d additions, so |got - fsum| <= g(d) sum|term|.
  counts, durations, starts, ranks (the table entry), in_event, the indicator and unweighted area fractions: exact.
  weighted area fractions: count 2^-52 mean|w x| / mean w, the bound of tests/test_gpu_basins.py for gd_zone_mean.
"""
import itertools
import math
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53
T_MAX, M_MAX = 181, 1025
TS = (1, 2, 11, 12, 13, 25, 181)
MS = (1, 63, 64, 65, 257, 1025)
# (T, period, phase, baseline): period 12 at every T -- with a phase and a baseline strictly inside the record, so that
# samples lie outside it, at two of them -- and period 1, T and 366 at one T each
CASES = ((1, 12, 0, None), (2, 12, 0, None), (11, 12, 0, None), (12, 12, 3, None), (13, 12, 0, None), (25, 12, 0, (3, 20)),
         (181, 12, 0, None), (181, 12, 5, (24, 144)), (25, 1, 0, None), (13, 13, 0, None), (181, 366, 7, None))
EV_MAPS = ("n_valid", "n_dry", "n_events", "event_steps", "max_duration", "mean_duration", "max_severity", "total_severity", "peak",
           "longest_start", "worst_start", "last_run")
EXACT_MAPS = ("n_valid", "n_dry", "n_events", "event_steps", "max_duration", "mean_duration", "peak", "longest_start", "last_run")
THRESHOLD = -0.5            # a multiple of 1/8: samples lie exactly on it
_BASE = {}
_CACHE = {}


def gamma(k):
    return k * U53 / (1.0 - k * U53)


def base(dtype=np.float64):
    key = np.dtype(dtype).name
    if key not in _BASE:
        rng = np.random.default_rng(20261020)
        e = rng.standard_normal((T_MAX, M_MAX))
        x = np.empty_like(e)
        x[0] = e[0]
        for t in range(1, T_MAX):
            x[t] = 0.7 * x[t - 1] + 0.71 * e[t]
        x = np.round(x * 8.0) / 8.0
        x[0, 1] = np.nan                      # a gap of one step (present at every T)
        x[7, 1] = np.nan
        x[1:2, 2] = np.nan                    # many steps: 1, 5 .. 10, 30 .. 89
        x[5:11, 2] = np.nan
        x[30:90, 2] = np.nan
        x[:, 3] = np.nan                      # no sample at all
        x[:, 4] = -1.25                       # constant: M2 == 0, dry at every step
        x[:2, 5] = -2.0                       # a run of two from step 0 (an event at min_duration <= 2), then wet
        x[2, 5] = 1.0
        x[0, 6] = -1.0                        # a run of one at step 0
        x[1, 6] = 1.0
        _BASE[key] = np.ascontiguousarray(x.astype(dtype))
    return _BASE[key]


def series(T, M, dtype=np.float64):
    return np.ascontiguousarray(base(dtype)[:T, :M])


def mask_of(M):
    """the first (when there are at least 8 series), a middle and the last series left out"""
    mask = np.ones(M, dtype=np.uint8)
    if M >= 8:
        mask[[0, M // 2, M - 1]] = 0
    return mask


def oracle_columns(M):
    """the special columns, both ends, the middle, and both sides of every wave / workgroup boundary"""
    want = {0, 1, 2, 3, 4, 5, 6, M // 2, M - 2, M - 1, 62, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, 767, 768, 1023, 1024}
    return sorted(c for c in want if 0 <= c < M)


def slot_steps(T, period, phase, lo, hi):
    """per slot, the steps lo <= t < hi of the slot in time order"""
    out = [[] for _ in range(period)]
    for t in range(lo, hi):
        out[(t + phase) % period].append(t)
    return out


def durations(T):
    """the min_duration values a case is scanned with: 3 (the default), and what lets a record of one or two steps hold an
    event at all"""
    return (1, 2, 3) if T < 3 else (1, 3)


# ---- climatology -----------------------------------------------------------------------------------------------------------
def clim_oracle_column(x, period, phase, b0, b1):
    """(n, mean, m2, E, E2) per slot of one series: exact n, correctly rounded exact mean and M2, and the bounds of the
    docstring; also the exact mean and M2 as Fractions for the index oracle"""
    T = x.shape[0]
    n, mean, m2, eb, e2b = np.zeros(period), np.full(period, np.nan), np.full(period, np.nan), np.zeros(period), np.zeros(period)
    exact = [None] * period
    for s, steps in enumerate(slot_steps(T, period, phase, b0, b1)):
        v = [Fraction(float(x[t])) for t in steps if not np.isnan(x[t])]
        k = len(v)
        n[s] = k
        if k == 0:
            continue
        run, d1 = Fraction(0), Fraction(0)
        for i, f in enumerate(v):
            d1 += abs(f - run)
            run += (f - run) / (i + 1)
        mu = sum(v) / k
        assert run == mu
        ss = sum((f - mu) ** 2 for f in v)
        big = float(max(abs(f) for f in v))
        mean[s], m2[s] = float(mu), float(ss)
        eb[s] = gamma(k + 8) * big
        e2b[s] = gamma(k + 6) * float(ss) + 2.01 * eb[s] * float(d1) + 1.01 * k * eb[s] ** 2
        exact[s] = (mu, ss)
    return n, mean, m2, eb, e2b, exact


def clim_oracle(dtype, T, period, phase, baseline, cols):
    """{col: clim_oracle_column} over the columns ``cols`` of the base array's first T steps"""
    b0, b1 = (0, T) if baseline is None else baseline
    x = base(dtype)[:T].astype(np.float64)
    out = {}
    for c in cols:
        key = ("clim", np.dtype(dtype).name, T, period, phase, b0, b1, int(c))
        if key not in _CACHE:
            _CACHE[key] = clim_oracle_column(x[:, c], period, phase, b0, b1)
        out[c] = _CACHE[key]
    return out


def check_clim(rec, cols, want, masked=()):
    """``rec`` (3, period, M) against the oracle of its columns ``cols``: n exact, mean and M2 within E and E2, NaN exactly
    where a slot is empty; the largest error over its bound (mean, M2)"""
    worst = [0.0, 0.0]
    for c in cols:
        n, mean, m2, eb, e2b, _ = want[c]
        if c in masked:
            assert np.all(rec[0, :, c] == 0) and np.isnan(rec[1:, :, c]).all(), c
            continue
        assert np.array_equal(rec[0, :, c], n), c
        has = n > 0
        assert np.isnan(rec[1:, ~has, c]).all() and np.isfinite(rec[1:, has, c]).all(), c
        for j, (w, b) in enumerate(((mean, eb), (m2, e2b))):
            err = np.abs(rec[1 + j, has, c] - w[has])
            assert np.all(err <= b[has]), (c, j, err, b[has])
            pos = b[has] > 0
            if pos.any():
                worst[j] = max(worst[j], float((err[pos] / b[has][pos]).max()))
    return tuple(worst)


# ---- parametric indices ----------------------------------------------------------------------------------------------------
def _ld(fr):
    return np.longdouble(fr.numerator) / np.longdouble(fr.denominator)


def index_oracle_column(x, clim, period, phase, kind, ddof, f32):
    """(want, bound) of one series as fp64 arrays (the longdouble value rounded for the comparison), NaN where the index
    is NaN: a NaN sample, an empty slot, n - ddof <= 0, M2 == 0"""
    n, mean, m2, eb, e2b, exact = clim
    T = x.shape[0]
    want, bound = np.full(T, np.nan), np.zeros(T)
    for t in range(T):
        s = (t + phase) % period
        if np.isnan(x[t]) or n[s] == 0:
            continue
        mu, ss = exact[s]
        a = np.longdouble(x[t]) - _ld(mu)
        ea = eb[s] + U53 * (abs(float(a)) + eb[s])
        if kind == "anomaly":
            val, err = a, ea
        else:
            dof = n[s] - ddof
            if dof <= 0 or ss == 0:
                continue
            sd = np.sqrt(_ld(ss) / np.longdouble(dof))
            rho = e2b[s] / float(ss) + 2.0 * U53
            assert rho < 0.5
            val = a / sd
            err = (ea / float(sd) + abs(float(val)) * rho) / (1.0 - rho)
            err += U53 * (abs(float(val)) + err)
        if f32:
            err += 2.0 ** -24 * (abs(float(val)) + err) + 2.0 ** -150
        want[t], bound[t] = float(val), err
    return want, bound


def check_index(got, dtype, T, period, phase, baseline, kind, ddof, cols, masked=()):
    """the columns ``cols`` of ``got`` (T, M) against the oracle; the largest error over its bound"""
    x = base(dtype)[:T].astype(np.float64)
    clim = clim_oracle(dtype, T, period, phase, baseline, cols)
    worst = 0.0
    for c in cols:
        g = got[:, c].astype(np.float64)
        if c in masked:
            assert np.isnan(g).all(), c
            continue
        key = ("index", np.dtype(dtype).name, T, period, phase, baseline, kind, ddof, int(c))
        if key not in _CACHE:
            _CACHE[key] = index_oracle_column(x[:, c], clim[c], period, phase, kind, ddof, np.dtype(dtype) == np.float32)
        want, bound = _CACHE[key]
        assert np.array_equal(np.isnan(g), np.isnan(want)), (kind, c)
        ok = ~np.isnan(want)
        err = np.abs(g[ok] - want[ok])
        assert np.all(err <= bound[ok]), (kind, c, float((err / np.maximum(bound[ok], 1e-300)).max()))
        pos = bound[ok] > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bound[ok][pos]).max()))
    return worst


# ---- rank indices ----------------------------------------------------------------------------------------------------------
def table_oracle(kind, nmax):
    """the table of drought.rank_table, restated: Gringorten's plotting position of the midrank, or its normal quantile"""
    import statistics
    out = np.zeros(nmax * nmax)
    for n in range(1, nmax + 1):
        for k in range(1, 2 * n):
            p = ((k + 1) / 2 - 0.44) / (n + 0.12)
            out[(n - 1) ** 2 + k - 1] = p if kind == "percentile" else statistics.NormalDist().inv_cdf(p)
    return out


def rank_oracle_column(x, period, phase, b0, b1):
    """(n_eff, k, ties) per step of one series by scipy's average ranks: k = 2 midrank - 1; n_eff = 0 for a NaN sample;
    ties = the samples that share their value with another member of their comparison set"""
    from scipy.stats import rankdata
    T = x.shape[0]
    n_eff, kk, ties = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64), 0
    inside = slot_steps(T, period, phase, b0, b1)
    for s, steps in enumerate(slot_steps(T, period, phase, 0, T)):
        members = [t for t in inside[s] if not np.isnan(x[t])]
        vals = x[members]
        ranks = rankdata(vals, method="average") if len(members) else np.zeros(0)
        for t in steps:
            if np.isnan(x[t]):
                continue
            if b0 <= t < b1:
                r, n = ranks[members.index(t)], len(members)
                ties += int(np.sum(vals == x[t]) > 1)
            else:
                r, n = rankdata(np.append(vals, x[t]), method="average")[-1], len(members) + 1
                ties += int(np.sum(vals == x[t]) > 0)
            k2 = 2.0 * r - 1.0
            assert k2 == int(k2) and 1 <= k2 <= 2 * n - 1
            n_eff[t], kk[t] = n, int(k2)
    return n_eff, kk, ties


def rank_want(dtype, T, period, phase, baseline, table, cols):
    """({col: expected (T,) values in ``dtype``}, the number of tied samples met)"""
    b0, b1 = (0, T) if baseline is None else baseline
    x = base(dtype)[:T]
    out, ties = {}, 0
    for c in cols:
        key = ("rank", np.dtype(dtype).name, T, period, phase, b0, b1, int(c))
        if key not in _CACHE:
            _CACHE[key] = rank_oracle_column(x[:, c].astype(np.float64), period, phase, b0, b1)
        n_eff, kk, tied = _CACHE[key]
        ties += tied
        want = np.full(T, np.nan)
        ok = n_eff > 0
        want[ok] = table[(n_eff[ok] - 1) ** 2 + kk[ok] - 1]
        out[c] = want.astype(dtype)
    return out, ties


def nmax_of(T, period, baseline):
    b0, b1 = (0, T) if baseline is None else baseline
    return -(-(b1 - b0) // period) + 1


# ---- events ----------------------------------------------------------------------------------------------------------------
def events_oracle_column(v, threshold, min_duration):
    """(maps dict, in_event, bound on the severities, runs that fail min_duration, gap between the two largest severities)"""
    T = v.shape[0]
    dry = [bool(val <= threshold) for val in v]
    runs, t = [], 0
    for flag, grp in itertools.groupby(dry):
        k = len(list(grp))
        if flag:
            runs.append((t, k))
        t += k
    events = [(t0, k) for t0, k in runs if k >= min_duration]
    in_event = np.zeros(T, dtype=np.uint8)
    sev, terms_abs, steps = [], 0.0, 0
    for t0, k in events:
        in_event[t0:t0 + k] = 1
        terms = [threshold - float(val) for val in v[t0:t0 + k]]
        sev.append(math.fsum(terms))
        terms_abs += math.fsum(abs(d) for d in terms)
        steps += k
    m = dict(n_valid=float(np.sum(~np.isnan(v))), n_dry=float(sum(dry)), n_events=float(len(events)), event_steps=float(steps),
             max_duration=float(max((k for _, k in events), default=0)), mean_duration=steps / len(events) if events else np.nan,
             max_severity=max(sev, default=0.0),
             total_severity=math.fsum(threshold - float(val) for t0, k in events for val in v[t0:t0 + k]),
             peak=min((float(np.min(v[t0:t0 + k])) for t0, k in events), default=np.nan),
             longest_start=float(next((t0 for t0, k in events if k == max(kk for _, kk in events)), -1)),
             worst_start=float(events[int(np.argmax(sev))][0]) if events else -1.0,
             last_run=float(runs[-1][1]) if runs and runs[-1][0] + runs[-1][1] == T else 0.0)
    top = sorted(sev, reverse=True)
    gap = top[0] - top[1] if len(top) > 1 else np.inf
    return m, in_event, gamma(max(steps, 1)) * terms_abs, sum(1 for _, k in runs if k < min_duration), gap


def check_events(got, steps, x, threshold, min_duration, cols, masked=()):
    """the columns ``cols`` of the maps ``got`` (name -> (M,)) and of ``steps`` (T, M) against the oracle of the cube ``x``:
    counts, durations, peak and starts exactly (worst_start where the two largest severities differ by more than twice the
    bound), severities within the bound.  Returns (events, runs that fail min_duration, the largest severity error over its
    bound)"""
    n_events = n_fail = 0
    worst = 0.0
    for c in cols:
        if c in masked:
            for name in EV_MAPS:
                zero = name in ("n_valid", "n_dry", "n_events", "event_steps", "max_duration", "last_run")
                assert got[name][c] == 0 if zero else np.isnan(got[name][c]), (name, c)
            assert not steps[:, c].any()
            continue
        m, in_event, bound, fail, gap = events_oracle_column(x[:, c].astype(np.float64), threshold, min_duration)
        n_events += int(m["n_events"])
        n_fail += fail
        for name in EXACT_MAPS:
            assert np.array_equal(got[name][c], m[name], equal_nan=True), (name, c, got[name][c], m[name])
        if gap > 2.0 * bound:
            assert got["worst_start"][c] == m["worst_start"], c
        for name in ("max_severity", "total_severity"):
            err = abs(got[name][c] - m[name])
            assert err <= bound, (name, c, err, bound)
            if bound > 0:
                worst = max(worst, err / bound)
        assert np.array_equal(steps[:, c], in_event), c
    return n_events, n_fail, worst


# ---- area ------------------------------------------------------------------------------------------------------------------
def exceed_oracle(x, threshold):
    out = np.where(x <= threshold, 1.0, 0.0).astype(x.dtype)
    out[np.isnan(x)] = np.nan
    return out
