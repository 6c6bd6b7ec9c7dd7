"""Oracle, inputs and bounds for the lagged-correlation tests (test_cabi_lagcorr.py, test_gpu_lagcorr.py).  Nothing here shares
code with csrc/lagcorr_core.h: per lag the oracle gathers the valid pairs and computes a two-pass Pearson r in np.longdouble
(the mean of the pairs, then the centred sums), the standard autocorrelation likewise from the series mean, and the best lag
with the tie rule written out.

Bounds (derived, not measured; u = 2^-53):

  r     The twin centres by the series mean ma' (any approximation of it: r does not depend on the shift), rounds u_t = a_t - ma'
        (relative error u), and forms va = Suu - Su Su / n, vb, c = Suv - Su Sv / n from sums of n terms added in order.  A sum
        of n products carries at most (n + 1) u times the sum of the magnitudes, the rounding of u_t another 2 u; Su Su / n
        carries at most (2 n + 3) u Suu because (sum |u|)^2 <= n Suu.  So |d va| <= (3 n + 6) u Suu, and with Cauchy-Schwarz
        |d c| <= (3 n + 6) u sqrt(Suu Svv).  With kappa_a = Suu / va and kappa_b = Svv / vb -- the raw second moment of the
        centred values over their variance on the pairs of that lag, 1 when the pairs' mean equals the series mean --
          |d r| <= |d c| / sqrt(va vb) + |r| (d va / va + d vb / vb) / 2 + 3 u <= (3 n + 6) u (kappa_a + kappa_b) + 3 u
        to first order; R_BOUND doubles it for the second-order terms and the oracle's own rounding to fp64:
          r_bound = 2 (3 n + 8) u (kappa_a + kappa_b).
        It is first order, so the inputs must keep (3 n + 8) u kappa far below 1: the CPU test asserts kappa <= KAPPA_MAX.
  acf   "standard": c_k / c_0 does depend on the mean.  The recurrence m += (x - m) / k leaves |m' - m| <= 4 n u max|x| (a
        local error of at most 4 u max|x| per step, damped by 1 - 1 / k afterwards); it moves the numerator by at most
        2 |m' - m| sum|u| and sum|u| / Suu <= 1 / rms(u).  With the (n + 3) u of each of the two sums and |acf| <= 1 (to
        first order), doubled as above:
          acf_bound = 2 u ((2 n + 8) + 16 n max|x| / rms(u)).
  z, p  the device's atanh and erfc are within 5 and 16 ulp (the OpenCL limits that the ROCm device library documents),
        math.atanh and math.erfc within 1 ulp, sqrt is correctly rounded and the two products add 1 ulp: z within
        Z_RTOL = 10 * 2^-52 of math.atanh(r) * math.sqrt(n_eff - 3) on the device's own n_eff (which numpy reproduces exactly,
        every operation being rounded on its own), p within P_RTOL = 17 * 2^-52 of math.erfc(|z| * 0.7071067811865476) on the
        device's own z, absolute 2^-1022 where p is subnormal.
"""
import math

import numpy as np

U53 = 2.0 ** -53
T_MAX, M_MAX = 181, 1003
TS = (1, 2, 7, 181)
MS_CPU = (1, 63, 64, 65, 257)
MS_GPU = (1, 63, 64, 65, 257, 1003)
RANGES = ((0, 0), (-1, 1), (-12, 12), (0, 12), (-64, 64), (3, 7))
KAPPA_MAX = 2.0 ** 20
Z_RTOL, P_RTOL = 10.0 * 2.0 ** -52, 17.0 * 2.0 ** -52
SELECT = ("abs", "max", "min")
_BASE = {}
_ORACLE = {}
LD = np.longdouble


def base(dtype=np.float64, nans=True):
    """the (181, 1003) pair: a = randn + 2, b[t] = 0.8 a[t - 3] + 0.6 randn + 0.3 (b follows a by 3), rounded to ``dtype``;
    every smaller case is a corner [:T, :M].  With ``nans``: column 1 has scattered NaNs in a, column 2 in b, column 3 is all
    NaN in a, column 4 has a NaN run of 141 steps in b (longer than any lag range), column 5 is all NaN in b, and every 7th
    column from 7 on has scattered NaNs in both."""
    key = (np.dtype(dtype).name, nans)
    if key not in _BASE:
        rng = np.random.default_rng(20260929)
        a = rng.standard_normal((T_MAX, M_MAX)) + 2.0
        b = 0.6 * rng.standard_normal((T_MAX, M_MAX)) + 0.3
        b[3:] += 0.8 * a[:-3]
        b[:3] += 0.8 * 2.0
        if nans:
            a[rng.choice(T_MAX, 20, replace=False), 1] = np.nan
            b[rng.choice(T_MAX, 20, replace=False), 2] = np.nan
            a[:, 3] = np.nan
            b[20:161, 4] = np.nan
            b[:, 5] = np.nan
            for c in range(7, M_MAX, 7):
                a[rng.choice(T_MAX, 9, replace=False), c] = np.nan
                b[rng.choice(T_MAX, 9, replace=False), c] = np.nan
        _BASE[key] = (np.ascontiguousarray(a.astype(dtype)), np.ascontiguousarray(b.astype(dtype)))
    return _BASE[key]


def pair(T, M, dtype=np.float64, nans=True):
    a, b = base(dtype, nans)
    return np.ascontiguousarray(a[:T, :M]), np.ascontiguousarray(b[:T, :M])


def mask_for(M):
    m = np.ones(M, dtype=np.uint8)
    m[[c for c in (0, 6, 63, 64, M - 1) if c < M]] = 0
    return m


def _series_mean(x):
    ok = ~np.isnan(x)
    n = ok.sum(axis=0)
    with np.errstate(all="ignore"):
        return np.where(ok, x, 0).astype(LD).sum(axis=0) / np.maximum(n, 1), n


def lag_oracle(a, b, lo, hi, min_pairs=3):
    """(r (NL, M) fp64, n (NL, M) int, kappa (NL, M): max(kappa_a, kappa_b) of the bound above) of a[t] against b[t + l];
    ``a`` (T, M) or (T,)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.ndim == 1:
        a = np.repeat(a[:, None], b.shape[1], axis=1)
    T, M = b.shape
    nl = hi - lo + 1
    r, n, kappa = np.full((nl, M), np.nan), np.zeros((nl, M), dtype=np.int64), np.full((nl, M), np.nan)
    ma, _ = _series_mean(a)
    mb, _ = _series_mean(b)
    for k in range(nl):
        l = lo + k
        t0, t1 = max(0, -l), min(T, T - l)
        if t1 <= t0:
            continue
        x, y = a[t0:t1].astype(LD), b[t0 + l:t1 + l].astype(LD)
        ok = ~(np.isnan(x) | np.isnan(y))
        cnt = ok.sum(axis=0)
        n[k] = cnt
        with np.errstate(all="ignore"):
            den = np.maximum(cnt, 1)
            mx, my = np.where(ok, x, 0).sum(axis=0) / den, np.where(ok, y, 0).sum(axis=0) / den
            dx, dy = np.where(ok, x - mx, 0), np.where(ok, y - my, 0)
            va, vb, c = (dx * dx).sum(axis=0), (dy * dy).sum(axis=0), (dx * dy).sum(axis=0)
            good = (cnt >= min_pairs) & (va > 0) & (vb > 0)
            rk = np.clip(c / np.sqrt(va * vb), -1, 1)
            r[k] = np.where(good, rk, np.nan).astype(np.float64)
            ux, uy = np.where(ok, x - ma, 0), np.where(ok, y - mb, 0)       # centred by the series means, as the twin centres
            kap = np.maximum((ux * ux).sum(axis=0) / va, (uy * uy).sum(axis=0) / vb)
            kappa[k] = np.where(good, kap, np.nan).astype(np.float64)
    return r, n, kappa


def r_bound(n, kappa):
    return 2.0 * (3.0 * n + 8.0) * U53 * 2.0 * kappa          # kappa_a + kappa_b <= 2 max(kappa_a, kappa_b)


def best_oracle(r, n, lo, hi, select="abs"):
    """the (4, M) planes from a curve: visit 0, +1, -1, +2, -2, ... and keep the first of equals"""
    nl, M = r.shape
    out = np.full((4, M), np.nan)
    out[2] = 0.0
    order = [l for d in range(0, max(hi, -lo) + 1) for l in ((d,) if d == 0 else (d, -d)) if lo <= l <= hi]
    for m in range(M):
        best = None
        for l in order:
            v = r[l - lo, m]
            if np.isnan(v):
                continue
            key = abs(v) if select == "abs" else (v if select == "max" else -v)
            if best is None or key > best[0]:
                best = (key, l, v, n[l - lo, m])
        if best is not None:
            out[0, m], out[1, m], out[2, m] = best[1], best[2], best[3]
        if lo <= 0 <= hi:
            out[3, m] = r[-lo, m]
    return out


def cached_oracle(T, lo, hi, dtype, min_pairs=3):
    """the oracle of pair(T, 257, dtype): a series' result does not depend on M, so smaller M are its first columns"""
    key = (T, lo, hi, np.dtype(dtype).name, min_pairs)
    if key not in _ORACLE:
        a, b = pair(T, 257, dtype)
        _ORACLE[key] = lag_oracle(a, b, lo, hi, min_pairs)
    return _ORACLE[key]


def check_curve(r, n, want, where=""):
    """the twin's curve against the oracle's (r, n, kappa) within r_bound: counts exact, NaN in the same places, kappa under
    KAPPA_MAX; returns the largest error over its bound and the largest kappa"""
    wr, wn, kap = want
    assert np.array_equal(n, wn), where
    assert np.array_equal(np.isnan(r), np.isnan(wr)), where
    fin = ~np.isnan(wr)
    if not fin.any():
        return 0.0, 0.0
    assert kap[fin].max() <= KAPPA_MAX, (where, float(kap[fin].max()))
    assert np.all(np.abs(r[fin]) <= 1.0), where
    ratio = np.abs(r[fin] - wr[fin]) / r_bound(wn[fin], kap[fin])
    assert ratio.max() <= 1.0, (where, float(ratio.max()))
    return float(ratio.max()), float(kap[fin].max())


def check_best(best, r, n, lo, hi, select, where=""):
    """the twin's planes against best_oracle on the twin's OWN curve (the choice is exact given the curve)"""
    want = best_oracle(r, n, lo, hi, select)
    assert np.array_equal(best, want, equal_nan=True), where


def acf_oracle(x, K, kind="standard", min_pairs=3):
    """(acf (K + 1, M), n, bound (K + 1, M)) of the "standard" autocorrelation; "pearson" is lag_oracle(x, x, 0, K)"""
    x = np.asarray(x, dtype=np.float64)
    T, M = x.shape
    m, n0 = _series_mean(x)
    ok = ~np.isnan(x)
    u = np.where(ok, x.astype(LD) - m, 0)
    with np.errstate(all="ignore"):
        suu = (u * u).sum(axis=0)
        acf, n, bound = np.full((K + 1, M), np.nan), np.zeros((K + 1, M), dtype=np.int64), np.full((K + 1, M), np.nan)
        xmax = np.where(ok, np.abs(x), 0).max(axis=0)
        rms = np.sqrt((suu / np.maximum(n0, 1)).astype(np.float64))
        for k in range(K + 1):
            if k >= T:
                continue
            both = ok[:T - k] & ok[k:]
            n[k] = both.sum(axis=0)
            num = np.where(both, u[:T - k] * u[k:], 0).sum(axis=0)
            good = (n[k] >= min_pairs) & (suu > 0)
            acf[k] = np.where(good, num / suu, np.nan).astype(np.float64)
            bound[k] = 2.0 * U53 * ((2.0 * n0 + 8.0) + 16.0 * n0 * xmax / rms)
    return acf, n, bound


def neff_numpy(r, n, r1a, r1b):
    """n_eff by the formula of include/gandanet.h, every operation rounded on its own: the device's bits"""
    with np.errstate(all="ignore"):
        q = r1a * r1b
        ne = n * (1.0 - q) / (1.0 + q)
        ne = np.where(ne < 0.0, 0.0, np.where(ne > n, n, ne))
        bad = np.isnan(r) | np.isnan(n) | np.isnan(r1a * np.ones_like(r)) | np.isnan(r1b)
        return np.where(bad, np.nan, ne)


def check_signif(r, neff, z, p, where=""):
    """z against math.atanh / math.sqrt on the device's n_eff, p against math.erfc on the device's z; the largest errors over
    their bounds"""
    worst_z = worst_p = 0.0
    for i in range(r.size):
        if np.isnan(r[i]) or np.isnan(neff[i]) or not neff[i] > 3.0:
            assert np.isnan(z[i]) and np.isnan(p[i]), (where, i)
            continue
        if abs(r[i]) == 1.0:
            assert np.isinf(z[i]) and np.sign(z[i]) == np.sign(r[i]) and p[i] == 0.0, (where, i)
            continue
        wz = math.atanh(r[i]) * math.sqrt(neff[i] - 3.0)
        ez = abs(z[i] - wz) / (Z_RTOL * abs(wz)) if wz != 0.0 else (0.0 if z[i] == 0.0 else np.inf)
        wp = math.erfc(abs(z[i]) * 0.7071067811865476)
        ep = abs(p[i] - wp) / (P_RTOL * wp + 2.0 ** -1022)
        worst_z, worst_p = max(worst_z, ez), max(worst_p, ep)
        assert ez <= 1.0 and ep <= 1.0, (where, i, ez, ep)
    return worst_z, worst_p


def bh_numpy(p, alpha=0.05, mask=None):
    """Benjamini-Hochberg: (threshold, significant)"""
    valid = ~np.isnan(p) if mask is None else (~np.isnan(p) & (mask != 0))
    pv = np.sort(p[valid])
    ok = pv <= alpha * np.arange(1, pv.size + 1) / max(pv.size, 1)
    thr = float(pv[ok].max()) if ok.any() else 0.0
    return thr, (valid & (p <= thr)) if ok.any() else np.zeros(p.shape, dtype=bool)
