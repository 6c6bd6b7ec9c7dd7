"""Oracles and bounds for the per-pixel time-series tests (test_cabi_series.py, test_gpu_series.py).  Nothing here shares
code with csrc/series_core.h: records come from exact rational arithmetic (fractions) and math.fsum, both correctly
rounded; fits from np.linalg.lstsq on the rows where the series is not NaN; block means from math.fsum.

Bounds (derived, not measured; every fp64 summation order of n terms stays within them):
  records        |got - want| <= 4 T 2^-53 S per entry, S = sum |term| of that entry; counts exact
  derived maps   16 T 2^-53 max(1, |value|) against numpy formulas on the oracle's records
  coefficients   ||got - want||_2 <= (T + 8 P) cond_2(A_valid)^2 2^-53 ||want||_2 per series
  rss            8 T 2^-53 sum r^2 + 2 sqrt(sum r^2) E + E^2, E = ||A_valid||_2 times the coefficient bound (the coefficient
                 error propagated through ||A||: r_got = r_want - A dc)
  block means    n_block 2^-52 mean|x| (inputs randn + 2), counts exact
"""
import math
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53
T_MAX, M_MAX = 181, 1003
TS = (1, 2, 7, 181)
MS = (1, 63, 64, 65, 257, 1003)
MAPS = ("n", "mean_p", "mean_t", "bias", "rmse", "mae", "std_p", "std_t", "cc", "nse", "kge", "crmsd")
_BASE = {}
_REC_CACHE = {}


def base(dtype=np.float64):
    """the (181, 1003) pair: t = randn + 2, p = 0.8 t + 0.6 randn + 0.3 (cc in roughly 0.5 .. 0.95, mean_t far from 0),
    rounded to ``dtype``; every smaller case is a corner [:T, :M] of it"""
    key = np.dtype(dtype).name
    if key not in _BASE:
        rng = np.random.default_rng(20260118)
        t = rng.standard_normal((T_MAX, M_MAX)) + 2.0
        p = 0.8 * t + 0.6 * rng.standard_normal((T_MAX, M_MAX)) + 0.3
        _BASE[key] = (np.ascontiguousarray(p.astype(dtype)), np.ascontiguousarray(t.astype(dtype)))
    return _BASE[key]


def pair(T, M, dtype=np.float64):
    p, t = base(dtype)
    return np.ascontiguousarray(p[:T, :M]), np.ascontiguousarray(t[:T, :M])


def oracle_columns(M):
    """columns the exact oracle visits: both ends, the middle, and both sides of every wave / workgroup boundary"""
    want = {0, 1, M // 2, M - 2, M - 1, 62, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, 767, 768}
    return sorted(c for c in want if 0 <= c < M)


def record_oracle(p, t, skip_nan=True):
    """(record, scale) of one series from its 1-D arrays: exact means, M2 / C / sum|d| / sum d^2 as exact sums of exactly
    formed terms, rounded once; scale[k] = sum |term| of entry k (what the bound multiplies)"""
    p = np.asarray(p, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    if skip_nan:
        ok = ~(np.isnan(p) | np.isnan(t))
        p, t = p[ok], t[ok]
    n = p.size
    rec, scale = np.zeros(8), np.zeros(8)
    rec[0] = n
    if n == 0:
        return rec, scale
    fp, ft = [Fraction(float(v)) for v in p], [Fraction(float(v)) for v in t]
    mp, mt = sum(fp) / n, sum(ft) / n
    dp, dt = [v - mp for v in fp], [v - mt for v in ft]
    d = [a - b for a, b in zip(fp, ft)]
    rec[1], rec[2] = float(mp), float(mt)
    rec[3], rec[4] = float(sum(v * v for v in dp)), float(sum(v * v for v in dt))
    rec[5] = float(sum(a * b for a, b in zip(dp, dt)))
    rec[6], rec[7] = float(sum(abs(v) for v in d)), float(sum(v * v for v in d))
    scale[1], scale[2] = math.fsum(np.abs(p)) / n, math.fsum(np.abs(t)) / n
    scale[3], scale[4], scale[6], scale[7] = rec[3], rec[4], rec[6], rec[7]
    scale[5] = float(sum(abs(a * b) for a, b in zip(dp, dt)))
    return rec, scale


def records_oracle(p, t, cols, skip_nan=True, key=None):
    """(8, len(cols)) records and scales of the columns ``cols`` of two (T, M) arrays; ``key`` caches per column"""
    recs, scales = np.zeros((8, len(cols))), np.zeros((8, len(cols)))
    for i, c in enumerate(cols):
        k = None if key is None else (key, p.shape[0], int(c), skip_nan)
        if k is None or k not in _REC_CACHE:
            r = record_oracle(p[:, c], t[:, c], skip_nan)
            if k is None:
                recs[:, i], scales[:, i] = r
                continue
            _REC_CACHE[k] = r
        recs[:, i], scales[:, i] = _REC_CACHE[k]
    return recs, scales


def record_bound(T, scales):
    return 4.0 * T * U53 * scales


def skill_numpy(rec, ddof=0):
    """the twelve maps from (8, M) records by the numpy formulas of include/gandanet.h"""
    rec = np.asarray(rec, dtype=np.float64)
    n, mp, mt, m2p, m2t, c, sae, sse = rec
    out = {}
    with np.errstate(all="ignore"):
        has = n > 0
        nan = np.full(n.shape, np.nan)
        out["n"] = n.copy()
        out["mean_p"], out["mean_t"], out["bias"] = np.where(has, mp, nan), np.where(has, mt, nan), np.where(has, mp - mt, nan)
        out["rmse"], out["mae"] = np.where(has, np.sqrt(sse / n), nan), np.where(has, sae / n, nan)
        dof = n - ddof
        out["std_p"] = np.where(has & (dof > 0), np.sqrt(m2p / dof), nan)
        out["std_t"] = np.where(has & (dof > 0), np.sqrt(m2t / dof), nan)
        var = has & (m2p > 0) & (m2t > 0)
        cc = np.where(var, np.clip(c / np.sqrt(m2p * m2t), -1.0, 1.0), nan)
        out["cc"] = cc
        out["nse"] = np.where(has, np.where(m2t > 0, 1.0 - sse / m2t, np.where(sse == 0, 1.0, 0.0)), nan)
        out["kge"] = np.where(var, 1.0 - np.sqrt((cc - 1.0) ** 2 + (np.sqrt(m2p / m2t) - 1.0) ** 2 + (mp / mt - 1.0) ** 2), nan)
        out["crmsd"] = np.where(has, np.sqrt(np.maximum((m2p + m2t - 2.0 * c) / n, 0.0)), nan)
    return out


def map_bound(T, want):
    return 16.0 * T * U53 * np.maximum(1.0, np.abs(want))


def check_maps(got, want, T, where=""):
    """every map of ``got`` (name -> array) against ``want`` within map_bound, NaN exactly where ``want`` has NaN; the
    largest error over bound"""
    worst = 0.0
    for name, g in got.items():
        w = want[name]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (where, name)
        if name == "n":
            assert np.array_equal(g, w), (where, name)
            continue
        fin = np.isfinite(w)
        assert np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (where, name)
        ratio = np.abs(g[fin] - w[fin]) / map_bound(T, w[fin])
        if ratio.size:
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (where, name, float(ratio.max()))
    return worst


# ---- least squares -------------------------------------------------------------------------------------------------------
def basis_for(P, T):
    """the design matrices of the tests: 1 | 1, tau | 1, tau, two harmonics | 1, tau, three harmonics (period 12)"""
    t = np.arange(T, dtype=np.float64)
    half = 0.5 * (T - 1) if T > 1 else 1.0
    cols = [np.ones(T)]
    if P >= 2:
        cols.append((t - 0.5 * (T - 1)) / half)
    for k in range(1, (P - 2) // 2 + 1):
        cols += [np.cos(2.0 * np.pi * k * t / 12.0), np.sin(2.0 * np.pi * k * t / 12.0)]
    a = np.stack(cols, axis=1)
    assert a.shape == (T, P)
    return np.ascontiguousarray(a)


# sample positions that keep a P x P sub-matrix of the harmonic basis well conditioned (distinct phases of the year), at
# T = 181 and at T = 2 P
SPREAD = (0, 13, 27, 52, 80, 95, 130, 177)
SPREAD_SHORT = (0, 1, 3, 4, 6, 7, 9, 10)


def fit_series(P, T, M, dtype=np.float64):
    """(y, basis): M series of T samples = basis @ random coefficients + 0.3 randn, with (when the shape allows) scattered
    NaNs in column 1, P - 1 valid samples in column 2, exactly P in column 3, none in column 4"""
    rng = np.random.default_rng(1000 + 10 * P + T)
    a = basis_for(P, T)
    y = a @ rng.standard_normal((P, M)) + 0.3 * rng.standard_normal((T, M)) + 2.0
    if M > 4 and T >= 2 * P:
        rows = list(SPREAD[:P] if T == 181 else SPREAD_SHORT[:P])
        assert len(rows) == P
        y[rng.choice(T, size=max(1, T // 10), replace=False), 1] = np.nan
        keep = np.zeros(T, dtype=bool)
        keep[rows[:P - 1]] = True
        y[~keep, 2] = np.nan
        keep[rows] = True
        y[~keep, 3] = np.nan
        y[:, 4] = np.nan
    return np.ascontiguousarray(y.astype(dtype)), a


def lstsq_oracle(y, a):
    """per series: coef (P, M), rss, n, cond_2 and ||.||_2 of the valid rows of the basis; NaN coef / rss below P samples"""
    T, M = y.shape
    P = a.shape[1]
    coef, rss, n = np.full((P, M), np.nan), np.full(M, np.nan), np.zeros(M)
    cond, norm = np.full(M, np.nan), np.full(M, np.nan)
    y = y.astype(np.float64)
    full = None
    for m in range(M):
        ok = ~np.isnan(y[:, m])
        n[m] = ok.sum()
        if n[m] < P:
            continue
        if ok.all():
            if full is None:
                sv = np.linalg.svd(a, compute_uv=False)
                full = (sv[0] / sv[-1], sv[0])
            cond[m], norm[m] = full
        else:
            sv = np.linalg.svd(a[ok], compute_uv=False)
            cond[m], norm[m] = sv[0] / sv[-1], sv[0]
        c = np.linalg.lstsq(a[ok], y[ok, m], rcond=None)[0]
        r = y[ok, m] - a[ok] @ c
        coef[:, m], rss[m] = c, math.fsum(r * r)
    return coef, rss, n, cond, norm


def check_fit(got, want, T, where=""):
    """(coef, rss, n) against lstsq_oracle's tuple within the stated bounds; the largest error over bound (coef, rss)"""
    coef, rss, n = got
    wc, wr, wn, cond, norm = want
    P = wc.shape[0]
    assert np.array_equal(n, wn), where
    bad = np.isnan(wr)
    assert np.all(np.isnan(coef[:, bad])) and np.all(np.isnan(rss[bad])), where
    assert np.all(np.isfinite(coef[:, ~bad])) and np.all(np.isfinite(rss[~bad])), where
    cb = (T + 8 * P) * cond[~bad] ** 2 * U53 * np.linalg.norm(wc[:, ~bad], axis=0)
    ce = np.linalg.norm(coef[:, ~bad] - wc[:, ~bad], axis=0)
    e = norm[~bad] * cb
    rb = 8.0 * T * U53 * wr[~bad] + 2.0 * np.sqrt(wr[~bad]) * e + e * e
    re = np.abs(rss[~bad] - wr[~bad])
    assert np.all(ce <= cb), (where, float((ce / cb).max()))
    assert np.all(re <= rb), (where, float((re / rb).max()))
    return (float((ce / cb).max()), float((re / rb).max())) if ce.size else (0.0, 0.0)


def synth_harmonic(T, times=None, period=12.0):
    """a noise-free series with a chosen mean, slope, two amplitudes and phases, and the coefficient vector it should give
    against harmonic_basis(times, period, 2, True): (y (T, 3), answers dict, want coefficients (6, 3))"""
    t = np.arange(T, dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64)
    t_mid, t_half = 0.5 * (t.max() + t.min()), 0.5 * (t.max() - t.min())
    mean = np.array([3.0, -1.25, 0.5])
    slope = np.array([0.02, -0.004, 0.0])
    amp = np.array([[1.5, 0.3, 2.0], [0.4, 0.9, 0.05]])
    phase = np.array([[0.7, -2.1, 3.0], [-1.2, 0.1, 1.9]])
    y = mean + slope * (t[:, None] - t_mid)
    want = [mean, slope * t_half]
    for k in (1, 2):
        w = 2.0 * np.pi * k / period
        # A cos(wt - phi) expanded, so that wt is rounded as the basis rounds it (at t near 2000 and period 1 the rounding of
        # wt - phi alone is 1e-12, the synthesis' error and not the fit's)
        want += [amp[k - 1] * np.cos(phase[k - 1]), amp[k - 1] * np.sin(phase[k - 1])]
        y = y + want[-2] * np.cos(w * t[:, None]) + want[-1] * np.sin(w * t[:, None])
    return np.ascontiguousarray(y), dict(mean=mean, slope=slope, amp=amp, phase=phase), np.stack(want)


def ulps(got, want):
    """|got - want| in units of the spacing of ``want``"""
    return np.abs(got - want) / np.spacing(np.abs(want))


# ---- block means ---------------------------------------------------------------------------------------------------------
def block_case(shape, dtype=np.float64, nan_block=True, seed=3):
    """randn + 2 of ``shape`` with a few NaNs scattered over plane 0 and (optionally) one block of NaNs at its origin"""
    rng = np.random.default_rng(seed + sum(shape))
    x = (rng.standard_normal(shape) + 2.0).astype(dtype)
    flat = x[0].reshape(-1)
    flat[rng.choice(flat.size, size=max(1, flat.size // 9), replace=False)] = np.nan
    return x


def block_mean_oracle(x, fy, fx, weights=None, min_count=1):
    """(mean fp64, count, mean|x| of each block's contributors) by math.fsum, members in any order"""
    planes = x.reshape((-1,) + x.shape[-2:]).astype(np.float64)
    H, W = planes.shape[1:]
    out = np.full((planes.shape[0], H // fy, W // fx), np.nan)
    cnt = np.zeros(out.shape, dtype=np.int32)
    mag = np.zeros(out.shape)
    for pl in range(planes.shape[0]):
        for i in range(H // fy):
            for j in range(W // fx):
                v = planes[pl, i * fy:(i + 1) * fy, j * fx:(j + 1) * fx].reshape(-1)
                w = np.ones(v.size) if weights is None else weights[i * fy:(i + 1) * fy, j * fx:(j + 1) * fx].reshape(-1)
                ok = ~np.isnan(v)
                cnt[pl, i, j] = ok.sum()
                sw = math.fsum(w[ok])
                if cnt[pl, i, j] >= max(min_count, 1) and sw != 0:
                    out[pl, i, j] = math.fsum(w[ok] * v[ok]) / sw
                    mag[pl, i, j] = math.fsum(np.abs(w[ok] * v[ok])) / abs(sw)
    shape = x.shape[:-2] + out.shape[1:]
    return out.reshape(shape), cnt.reshape(shape), mag.reshape(shape)


def check_block(got, count, want, fy, fx, dtype, where=""):
    wm, wc, mag = want
    assert np.array_equal(count, wc), where
    assert np.array_equal(np.isnan(got), np.isnan(wm)), where
    fin = ~np.isnan(wm)
    bound = fy * fx * 2.0 ** -52 * mag[fin]
    if np.dtype(dtype) == np.float32:   # one rounding to the fp32 output on top
        bound = bound + np.spacing(np.abs(wm[fin]).astype(np.float32)).astype(np.float64)
    err = np.abs(got[fin].astype(np.float64) - wm[fin])
    assert np.all(err <= bound), (where, float((err / bound).max()))
    return float((err / bound).max()) if err.size else 0.0
