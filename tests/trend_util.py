"""Generators and the brute-force oracle of the trend tests (test_cabi_trend.py, test_gpu_trend.py).  The oracle restates
the definitions of include/gandanet.h, "Per-pixel trend tests", in numpy: the full array of pairwise slopes and np.sort,
season by season and concatenated in the seasonal form.  It shares no code with csrc/trend_core.h.  Every compared map is
exact (np.array_equal, NaN == NaN) except p, which has the relative bound P_RTOL below.

The oracle also asserts a condition on its own inputs: wherever an interval is asked for, (nt +- zq sigma) / 2 lies further
than 1e-9 from a half-integer, so that an ulp in zq (scipy's norm.ppf against statistics.NormalDist) cannot move a rank.
sigma = 0 (an all-equal series) is exempt: zq sigma is then exactly 0 whatever zq is, and nt / 2 IS a half-integer for odd
nt, rounded to even by every side.
"""
import math
import statistics

import numpy as np

MAPS = ("n", "s", "var_s", "z", "p", "tau", "slope", "intercept", "slope_lo", "slope_hi")
EXACT = tuple(k for k, nm in enumerate(MAPS) if nm != "p")
SEN, CI, CONT = 1, 2, 4
# p against math.erfc of the same z, relative.  The largest error measured on an MI355X over the cases of
# test_gpu_trend.py was 3.518e-16 (|z| up to 25.8, p down to 4e-147); the bound is four times that, far below the cap of
# 2^-40 above which something other than rounding would be wrong.
P_MEASURED = 3.518e-16
P_RTOL = min(4 * P_MEASURED, 2.0 ** -40)
P_TINY = 2.2250738585072014e-308          # below this (subnormal or 0) the check is absolute, 1e-300
KINDS = ("gauss_trend", "up", "down", "equal", "ints", "two", "outlier", "gauss")
_CACHE = {}


def zq_of(alpha):
    a = 1.0 - alpha if alpha > 0.5 else alpha
    return statistics.NormalDist().inv_cdf(a / 2.0)


def times_of(T, uniform=True):
    if uniform:
        return np.arange(T, dtype=np.float64)
    rng = np.random.default_rng(977 + T)
    return 2002.0 + np.cumsum(rng.uniform(0.02, 0.15, T))


def series(T, M, dtype=np.float64, gaps=False, seed=0):
    """(T, M): column m is of kind KINDS[m % 8]; with ``gaps`` about one sample in seven is NaN, and the columns 8, 9, 10
    (where M has them) keep 0, 1 and 2 valid samples"""
    rng = np.random.default_rng(20260311 + 1000 * T + seed)
    k = np.arange(T, dtype=np.float64)[:, None]
    x = np.empty((T, M))
    for m in range(M):
        kind = KINDS[m % len(KINDS)]
        g = rng.standard_normal(T)
        if kind == "gauss_trend":
            col = g + 0.02 * (m % 5 - 2) * k[:, 0]
        elif kind == "up":
            col = np.cumsum(np.abs(g) + 0.125)
        elif kind == "down":
            col = -np.cumsum(np.abs(g) + 0.125)
        elif kind == "equal":
            col = np.full(T, 1.5 + m)
        elif kind == "ints":
            col = rng.integers(0, 4, T).astype(np.float64)
        elif kind == "two":
            col = np.where(g > 0.3, 2.5, -1.0)
        elif kind == "outlier":
            col = g.copy()
            col[rng.integers(0, T)] = 1e12
        else:
            col = g
        x[:, m] = col
    x = x.astype(dtype)
    if gaps:
        x[rng.random((T, M)) < 1.0 / 7.0] = np.nan
        for m, keep in ((8, 0), (9, 1), (10, 2)):
            if m < M:
                x[:, m] = np.nan
                x[rng.choice(T, size=min(keep, T), replace=False), m] = (1.0 + np.arange(min(keep, T))).astype(dtype)
    return np.ascontiguousarray(x)


def columns(M):
    """the columns the oracle visits: both ends, the middle and both sides of the multiples of 64"""
    want = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, M // 2, M - 2, M - 1, 62, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256}
    return sorted(c for c in want if 0 <= c < M)


def _mid(v, n):
    return (v[(n - 1) // 2] + v[n // 2]) * 0.5


def oracle_one(y, t, period=0, flags=SEN | CI | CONT, zq=0.0):
    """the ten maps of one series (NaN where a map is not asked for)"""
    y = np.asarray(y, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    out = np.full(len(MAPS), np.nan)
    idx = np.nonzero(~np.isnan(y))[0]
    yv, tv = y[idx], t[idx]
    sea = idx % period if period else np.zeros(idx.size, dtype=np.int64)
    n = int(yv.size)
    out[0], out[1] = n, 0.0
    if n < 2:
        return out
    s = k = tot = ytie = 0
    slopes = []
    for g in np.unique(sea):
        yy, tt = yv[sea == g], tv[sea == g]
        ng = int(yy.size)
        iu = np.triu_indices(ng, 1)
        dy = (yy[None, :] - yy[:, None])[iu]
        s += int(np.sign(dy).sum())
        c = np.unique(yy, return_counts=True)[1].astype(object)
        k += ng * (ng - 1) * (2 * ng + 5) - int(sum(c * (c - 1) * (2 * c + 5)))
        tot += ng * (ng - 1) // 2
        ytie += int(sum(c * (c - 1) // 2))
        slopes.append(dy / (tt[None, :] - tt[:, None])[iu])
    var_s = (1.0 / 18.0) * float(k)
    if var_s == 0:
        z = np.nan
    elif s == 0:
        z = 0.0
    else:
        z = float(s - np.sign(s) if flags & CONT else s) / np.sqrt(var_s)
    out[1], out[2], out[3] = s, var_s, z
    out[4] = math.erfc(abs(z) * 0.7071067811865476) if z == z else np.nan
    if ytie != tot:
        out[5] = min(1.0, max(-1.0, float(s) / np.sqrt(float(tot)) / np.sqrt(float(tot - ytie))))
    nt = tot
    if not flags & SEN or nt == 0:
        return out
    sl = np.sort(np.concatenate(slopes) + 0.0)
    assert sl.size == nt and np.all(np.isfinite(sl))
    out[6] = _mid(sl, nt)
    out[7] = _mid(np.sort(yv), n) - out[6] * _mid(np.sort(tv), n)
    if flags & CI:
        sigma = np.sqrt(var_s)
        a, b = (nt - zq * sigma) / 2.0, (nt + zq * sigma) / 2.0
        if sigma > 0:
            for v in (a, b):
                assert abs(v - math.floor(v) - 0.5) > 1e-9, ("a rank within 1e-9 of a tie of rint: choose another seed", v)
        ru = min(int(np.rint(a)), nt - 1)
        rl = max(int(np.rint(b)) - 1, 0)
        out[8], out[9] = sl[rl], sl[ru]
    return out


def oracle(x, t, cols, period=0, flags=SEN | CI | CONT, zq=0.0, mask=None):
    """(10, len(cols)): the maps of the columns ``cols`` of the (T, M) array ``x``"""
    out = np.empty((len(MAPS), len(cols)))
    for j, m in enumerate(cols):
        if mask is not None and not mask[m]:
            out[:, j] = np.nan
            out[0, j] = out[1, j] = 0.0
        else:
            out[:, j] = oracle_one(x[:, m], t, period, flags, zq)
    return out


def reference(key, x, t, period=0, flags=SEN | CI | CONT, zq=0.0, mask=None):
    """(host twin on every column, oracle on ``columns(M)``), computed once per ``key`` and never changed"""
    if key not in _CACHE:
        from gan_danet_amd import kern as K
        cols = columns(x.shape[1])
        host = K.trend_test_host(x, t, period, mask, flags, zq, out=np.full((len(MAPS), x.shape[1]), -7.0))
        host.setflags(write=False)
        want = oracle(x, t, cols, period, flags, zq, mask)
        want.setflags(write=False)
        _CACHE[key] = (host, cols, want)
    return _CACHE[key]


def planes_of(flags):
    return [k for k in EXACT if k < 6 or (k < 8 and flags & SEN) or (k >= 8 and flags & CI)]


def assert_exact(got, want, flags, what):
    """bit for bit on every plane that ``flags`` asks for but p (NaN equals NaN; np.array_equal takes -0.0 for 0.0)"""
    for k in planes_of(flags):
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, MAPS[k], np.nonzero(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))))[0][:8])


def p_error(p, z):
    """the largest error of p against math.erfc of the same z, as a fraction of its bound (relative P_RTOL; absolute 1e-300
    where the exact value is subnormal or 0), and the largest relative error itself"""
    worst = worst_rel = 0.0
    for pv, zv in zip(np.ravel(p), np.ravel(z)):
        if zv != zv:
            assert pv != pv
            continue
        want = math.erfc(abs(zv) * 0.7071067811865476)
        if want < P_TINY:
            worst = max(worst, abs(pv - want) / 1e-300)
        else:
            rel = abs(pv - want) / want
            worst_rel = max(worst_rel, rel)
            worst = max(worst, rel / P_RTOL)
    return worst, worst_rel
