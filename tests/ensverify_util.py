"""Generators, the numpy oracle and the derived tolerances of the ensemble-verification tests (test_cabi_ensverify.py,
test_gpu_ensverify.py).  The oracle restates the definitions of include/gandanet.h, "Ensemble verification", in numpy fp64
and shares no code with csrc/ensverify_core.h: the CRPS is the brute-force mean|x_i - y| - sum_ij |x_i - x_j| / (2 M^2)
(no sorting), the rank comes from np.sum(x < y) and np.sum(x == y), mean error and spread from np.mean and
np.var(ddof=1) of the differences, the Gaussian part from math.erf and math.exp.  ``crps_exact`` gives the CRPS of a few
hundred elements in exact rationals.

Exact (np.array_equal): rank map, n, the tie count, the histogram and the coverage counts.  A coverage bit is a threshold,
so the oracle asserts on its own values that no valid element has | |e| - z_k s | <= 1e-9 z_k s, except where s == 0 exactly
(then the bit is e == 0 on every side); the seeds below were chosen so that this holds with no element left out.

Tolerances, with u = 2^-53, A = mean|d_i|, P = sum_{i<j}|x_i - x_j| / M^2 (M (M - 1) in the fair form); none is tuned:
  crps       |err| <= (M + 3) u (A + P) per element (issue; the sorted form measured 1.06 u (A + P) against exact rationals),
             plus one ulp of the storage dtype for a map;
  e          the sum of M terms then one division: (M + 1) u A on each side, so 2 (M + 2) u A between two evaluations;
  s          s^2 is a sum of M squares of rounded differences over M - 1: relative (M + 3) u on each side, (M + 5) u on s
             between two evaluations; an error de of the mean moves s^2 by at most 2 de^2, hence s by at most sqrt(2) de:
             another 2 (M + 2) u A, absolute;
  sums       the per-element bounds added up, plus n u times the sum of the absolute terms (any summation order);
  crps_gauss against this file's formula evaluated on the device's own fp64 err and spread maps, so that only erf and exp
             differ: relative to s (|z| + 1).  The largest error measured on an MI355X over the elements of
             test_gpu_ensverify.py::test_crps_gauss_per_element was G_MEASURED; the bound is four times that (the P_RTOL
             precedent of trend_util.py), capped at 2^-40 above which something other than rounding would be wrong.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
Z = (0.674489750196082, 1.0, 1.644853626951472, 1.959963984540054)
N, TIED, CRPS, CRPS_GAUSS, ABS_E, E2, S2, COVER, HIST, BINS, REC = 0, 1, 2, 3, 4, 5, 6, 7, 11, 33, 44
G_MEASURED = 2.461e-16
G_RTOL = min(4 * G_MEASURED, 2.0 ** -40)
KINDS = ("gauss", "ints", "identical", "equal_truth", "outlier", "near")
SENTINEL, SENTINEL_U8 = -7777.0, 99
_CACHE = {}


def even_m(M):
    """Integer data can sit exactly on a coverage threshold: d = (0, 1, 2) has |e| = s = 1, the level z = 1.  |e| = s means
    S^2 (2 M - 1) = M^2 Q for S = sum d, Q = sum d^2; at odd M in-range integers solve it (M = 3: S = 3, Q = 5), and the
    oracle's assertion finds such elements at every odd M > 1 tried.  At even M it finds none, so the integer kind runs there."""
    return M + (M % 2)


def make(kind, M, planes, hw, dtype=np.float32, seed=0, nans=False, stride_pad=5, offset=0):
    """members (M, planes, hw) -- a view into a slab whose members are planes * hw + stride_pad elements apart and start
    `offset` elements into their buffers -- and the truth (planes, hw)"""
    rng = np.random.default_rng(20261019 + 7919 * M + 104729 * planes + hw + 15485863 * seed + KINDS.index(kind))
    n = planes * hw
    if kind == "gauss":
        y = rng.standard_normal(n)
        x = y + 0.3 * rng.standard_normal(n) + 0.8 * rng.standard_normal((M, n))
    elif kind == "ints":
        y = rng.integers(0, 4, n).astype(np.float64)
        x = rng.integers(0, 4, (M, n)).astype(np.float64)
    elif kind == "identical":                       # multiples of 1/8: every sum below is exact, so s == 0 exactly
        y = rng.integers(-40, 41, n) / 8.0
        x = np.broadcast_to(np.where(rng.random(n) < 0.25, y, rng.integers(-40, 41, n) / 8.0), (M, n)).copy()
    elif kind == "equal_truth":
        y = rng.standard_normal(n)
        x = np.broadcast_to(y, (M, n)).copy()
    elif kind == "outlier":
        y = rng.standard_normal(n)
        x = y + rng.standard_normal((M, n))
        x[rng.integers(0, M, n), np.arange(n)] = 1e12
    elif kind == "near":
        y = 1e4 + 1e-3 * rng.standard_normal(n)
        x = 1e4 + 1e-3 * rng.standard_normal((M, n))
    else:
        raise ValueError(kind)
    y = y.astype(dtype)
    x = x.astype(dtype)
    if kind == "equal_truth":
        x[:] = y
    if nans:
        y[rng.random(n) < 0.05] = np.nan
        hit = rng.random(n) < 0.08
        x[rng.integers(0, M, n)[hit], np.arange(n)[hit]] = np.nan
    slab = np.full(offset + M * (n + stride_pad), SENTINEL, dtype=dtype)
    xv = np.lib.stride_tricks.as_strided(slab[offset:], shape=(M, n), strides=((n + stride_pad) * slab.itemsize, slab.itemsize))
    xv[:] = x
    ybuf = np.full(offset + n, SENTINEL, dtype=dtype)
    ybuf[offset:] = y
    return xv.reshape(M, planes, hw), ybuf[offset:].reshape(planes, hw)


def oracle(x, y, mask=None, scale=1.0, fair=False):
    """per-element values (fp64, NaN / 255 where invalid), the record and the tolerances of every compared quantity"""
    M = x.shape[0]
    shape = y.shape
    x64 = np.asarray(x, dtype=np.float64).reshape(M, -1)
    y64 = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y64.size
    valid = ~np.isnan(y64) & ~np.isnan(x64).any(0)
    if mask is not None:
        valid &= np.tile(np.asarray(mask).reshape(-1) != 0, n // np.asarray(mask).size)
    xs, ys = np.where(valid, x64, 0.0), np.where(valid, y64, 0.0)
    d = xs - ys
    A = np.mean(np.abs(d), axis=0)
    pair = np.zeros(n)
    for i in range(M):
        pair += np.abs(xs[i][None, :] - xs).sum(0)
    P = pair / (2.0 * (M * (M - 1) if fair else M * M))
    crps = A - P
    less, ties = np.sum(xs < ys, axis=0), np.sum(xs == ys, axis=0)
    rank = less + ties // 2
    e = np.mean(d, axis=0)
    s2 = np.var(d, axis=0, ddof=1) if M > 1 else np.zeros(n)
    s = np.sqrt(s2)
    gauss = gauss_formula(e, s)
    cover = np.zeros((4, n), dtype=bool)
    for k, zk in enumerate(Z):
        cover[k] = np.abs(e) <= zk * s
        near = valid & (s > 0) & (np.abs(np.abs(e) - zk * s) <= 1e-9 * zk * s)
        assert not near.any(), f"oracle: {int(near.sum())} elements sit on the coverage threshold z = {zk}: pick another seed"
    nan = np.where(valid, 0.0, np.nan)
    out = {"valid": valid.reshape(shape), "M": M, "n": int(valid.sum())}
    out["crps"] = (crps * scale + nan).reshape(shape)
    out["err"] = (e * scale + nan).reshape(shape)
    out["spread"] = (s * scale + nan).reshape(shape)
    out["gauss"] = (gauss * scale + nan).reshape(shape)
    out["rank"] = np.where(valid, rank, 255).astype(np.uint8).reshape(shape)
    # tolerances per element (fp64 values; a map adds one ulp of its dtype)
    tol_c = (M + 3) * U * (A + P) * scale
    tol_e = 2 * (M + 2) * U * A * scale
    tol_s = ((M + 5) * U * s + 2 * (M + 2) * U * A) * scale
    out["tol"] = {"crps": tol_c.reshape(shape), "err": tol_e.reshape(shape), "spread": tol_s.reshape(shape)}
    v = valid
    rec = np.zeros(REC)
    rec[N] = v.sum()
    rec[TIED] = (v & (ties > 0)).sum()
    rec[CRPS] = math.fsum(crps[v] * scale)
    rec[CRPS_GAUSS] = math.fsum(gauss[v] * scale)
    rec[ABS_E] = math.fsum(np.abs(e[v]) * scale)
    rec[E2] = math.fsum((e[v] * scale) ** 2)
    rec[S2] = math.fsum(s2[v] * scale * scale)
    for k in range(4):
        rec[COVER + k] = (v & cover[k]).sum()
    rec[HIST:HIST + M + 1] = np.bincount(rank[v], minlength=M + 1)
    out["rec"] = rec
    nu = float(rec[N]) * U
    ae = np.abs(e[v]) * scale
    out["rec_tol"] = {
        CRPS: math.fsum(tol_c[v]) + nu * math.fsum(np.abs(crps[v]) * scale),
        ABS_E: math.fsum(tol_e[v]) + nu * rec[ABS_E],
        E2: math.fsum(2 * ae * tol_e[v] + tol_e[v] ** 2 + 2 * U * ae * ae) + nu * rec[E2],
        S2: math.fsum((2 * (M + 4) * U * s2[v] + 2 * ((M + 2) * U * A[v]) ** 2) * scale * scale) + nu * rec[S2],
    }
    return out


_erf, _exp = np.vectorize(math.erf, otypes=[float]), np.vectorize(math.exp, otypes=[float])


def gauss_formula(e, s):
    """the CRPS of N(mean, s^2) at the truth, with e = mean - truth: s (z erf(z / sqrt 2) + 2 phi(z) - 1 / sqrt pi), z = -e / s"""
    e, s = np.asarray(e, dtype=np.float64), np.asarray(s, dtype=np.float64)
    ok = s > 0
    z = -e / np.where(ok, s, 1.0)
    g = np.where(ok, s, 0.0) * (z * _erf(z / math.sqrt(2.0)) + 2.0 * _exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) - 1.0 / math.sqrt(math.pi))
    return np.where(ok, g, np.abs(e))


def gauss_weight(e, s):
    """what the crps_gauss error is measured against: s (|z| + 1) = |e| + s"""
    return np.abs(np.asarray(e, dtype=np.float64)) + np.asarray(s, dtype=np.float64)


def crps_exact(x, y, fair=False):
    """the CRPS of every element in exact rationals from the stored values; inputs without NaN"""
    M = x.shape[0]
    xs = np.asarray(x).reshape(M, -1)
    ys = np.asarray(y).reshape(-1)
    out = []
    for j in range(ys.size):
        v = [Fraction(float(t)) for t in xs[:, j]]
        t = Fraction(float(ys[j]))
        a = sum(abs(q - t) for q in v) / M
        p = sum(abs(v[i] - v[k]) for i in range(M) for k in range(i + 1, M))
        out.append(a - p / (M * (M - 1) if fair else M * M))
    return out


def ulp(v, dtype):
    """one ulp of the storage dtype at |v| (0 where v is NaN)"""
    a = np.nan_to_num(np.abs(np.asarray(v, dtype=np.float64)), nan=0.0).astype(dtype)
    return np.spacing(a).astype(np.float64)


def check_maps(got, ref, dtype, what=""):
    """got: dict crps / err / spread / rank of arrays in the storage dtype.  Returns the largest error / bound per map."""
    worst = {}
    valid = ref["valid"]
    assert np.array_equal(got["rank"], ref["rank"]), what + " rank map"
    for k in ("crps", "err", "spread"):
        g = np.asarray(got[k], dtype=np.float64)
        assert np.array_equal(np.isnan(g), ~valid), f"{what} {k}: NaN exactly at the invalid elements"
        bound = ref["tol"][k] + ulp(ref[k], dtype)
        err = np.abs(g - ref[k])[valid]
        ok = err <= bound[valid]
        assert ok.all(), f"{what} {k}: {int((~ok).sum())} elements outside the bound, worst {np.max(err / np.maximum(bound[valid], 1e-300)):.3g}"
        worst[k] = float(np.max(err / np.maximum(bound[valid], 1e-300))) if err.size else 0.0
    return worst


def check_rec(rec, ref, what=""):
    """counts exact, float sums inside their bounds (crps_gauss is checked by its own tests)"""
    r = ref["rec"]
    for f in [N, TIED] + list(range(COVER, COVER + 4)) + list(range(HIST, HIST + BINS)):
        assert rec[f] == r[f], f"{what} record field {f}: {rec[f]} != {r[f]}"
    worst = {}
    for f, tol in ref["rec_tol"].items():
        assert abs(rec[f] - r[f]) <= tol, f"{what} record field {f}: {rec[f]} vs {r[f]}, bound {tol}"
        worst[f] = abs(rec[f] - r[f]) / tol if tol > 0 else 0.0
    return worst


def check_gauss_sum(rec_gauss, err_map64, spread_map64, valid, scale, what=""):
    """sum crps_gauss against the formula on the run's own fp64 err / spread maps (both already scaled: the formula is
    homogeneous of degree one, so the scale needs no separate handling)"""
    e, s = err_map64[valid], spread_map64[valid]
    ref = gauss_formula(e, s)
    tol = G_RTOL * math.fsum(gauss_weight(e, s)) + e.size * U * math.fsum(np.abs(ref)) + 4 * U * math.fsum(np.abs(ref))
    want = math.fsum(ref)
    assert abs(rec_gauss - want) <= tol, f"{what} sum crps_gauss {rec_gauss} vs {want}, bound {tol}"
    return abs(rec_gauss - want) / tol if tol > 0 else 0.0


def metrics_np(rec, M):
    """the derived metrics of gd_ens_verify_merge_host in numpy"""
    n = rec[N]
    if not n > 0:
        return None
    rmse, spread = math.sqrt(rec[E2] / n), math.sqrt(rec[S2] / n)
    hist = rec[HIST:HIST + M + 1] / n
    return {"crps": rec[CRPS] / n, "crps_gauss": rec[CRPS_GAUSS] / n, "mae": rec[ABS_E] / n, "rmse": rmse, "spread": spread,
            "spread_skill": math.sqrt((M + 1) / M) * spread / rmse if (M > 1 and rmse > 0) else math.nan,
            "coverage": [rec[COVER + k] / n for k in range(4)], "rank_hist": list(hist),
            "reliability": float(np.sum(np.abs(hist - 1.0 / (M + 1)))), "tied": rec[TIED] / n}
