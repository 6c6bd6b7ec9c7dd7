"""Oracle, inputs and bounds for the triple-collocation tests (test_cabi_tcol.py, test_gpu_tcol.py).  Nothing here shares code
with csrc/tcol_core.h: the oracle deletes listwise, takes np.cov-style covariances (two-pass, about the mean of the counted
steps) in np.longdouble, evaluates the eight formulas there, and summarises replicates with np.nanquantile / np.nanmean /
np.nanstd.

Inputs: an AR(1) truth t (coefficient 0.6, unit variance) per pixel and x = 5 + t + 0.3 e1, y = -2 + 0.8 t + 0.4 e2,
z = 1.3 t + 0.5 e3 with independent standard normal e.  Every third pixel has three NaN steps (in x, y, z at three different
steps), pixel 1 has NaNs in y only, pixel 4 is all NaN (in all three cubes) and pixel 5 has y = -y (negative cross-covariances:
the undefined branch).  Every smaller case is a corner [:T, :M] of the (181, 257) base.

Bounds (eps = 2^-52).  The scales are Qxx, Qyy, Qzz for the error variances, 1 for rho2 and |beta| for the betas, and an
error is |twin - oracle| / scale.  MEASURED on the grid of test_cabi_tcol.py, fp64 and fp32 storage:
  point estimates (T in {1, 2, 3, 24, 181} x M in {1, 63, 64, 65, 257}, the six covariances included, those against
  sqrt(Qaa Qbb)): the largest error was 9.70 eps (T = 181).  POINT_BOUND_EPS = 4 x 9.70 = 39 eps.
  bootstrap replicates (T, block in {(24, 3), (40, 4), (181, 6)}, B = 128, 65 pixels: 8 x 128 x 65 values per case, none
  skipped): 2180.5 eps at T = 24 (fp32 storage; 647.5 eps with fp64), 13.8 eps at T = 40, 22.1 eps at T = 181.  The T = 24
  figure is one replicate whose Qyz = 0.0023 is a hundredth of Qxx (rho2_x = 50 there): the statistics divide by that
  cross-covariance, so its rounding error of a few eps of sqrt(Qyy Qzz) is amplified by Qxy Qxz / Qyz^2 -- conditioning of the
  formulas at the edge of the undefined branch, which the scales the method prescribes do not see; the 99.9th percentile of
  the same case is 6.6 eps.  REPLICATE_BOUND_EPS = 4 x 2180.5 = 8722 eps (1.9e-12).  The margin of 4 is for other seeds and
  for libm-free rounding differences.
Closed form (T = 32, exactly orthogonal columns of a QR factor): the largest deviation from the real-arithmetic values was
3.23 eps of the same scales; CLOSED_BOUND_EPS = 4 x 3.23 = 13 eps.
Bootstrap mean and std against the long-double mean and std (ddof 1) of the twin's own replicates, relative to the replicates'
largest magnitude: at most 4.74 eps over the grid above; MOMENT_BOUND_EPS = 4 x 4.74 = 19 eps.  The quantiles equal
np.nanquantile bit for bit and n_ok the count of replicates that are not NaN.
"""
import numpy as np

EPS = 2.0 ** -52
POINT_BOUND_EPS = 39.0
REPLICATE_BOUND_EPS = 8722.0
CLOSED_BOUND_EPS = 13.0
MOMENT_BOUND_EPS = 19.0
LD = np.longdouble
T_MAX, M_MAX = 181, 257
TS_EST = (1, 2, 3, 24, 181)
MS_EST = (1, 63, 64, 65, 257)
STATS = ("err_var_x", "err_var_y", "err_var_z", "rho2_x", "rho2_y", "rho2_z", "beta_y", "beta_z")
F_MASKED, F_FEW, F_NONPOS, F_NEG_X, F_NEG_Y, F_NEG_Z, F_RHO2 = 1, 2, 4, 8, 16, 32, 64
_BASE = {}


def base(dtype=np.float64):
    key = np.dtype(dtype).name
    if key not in _BASE:
        rng = np.random.default_rng(20261021)
        t = np.empty((T_MAX, M_MAX))
        t[0] = rng.standard_normal(M_MAX)
        for k in range(1, T_MAX):
            t[k] = 0.6 * t[k - 1] + np.sqrt(1.0 - 0.36) * rng.standard_normal(M_MAX)
        x = 5.0 + t + 0.3 * rng.standard_normal(t.shape)
        y = -2.0 + 0.8 * t + 0.4 * rng.standard_normal(t.shape)
        z = 1.3 * t + 0.5 * rng.standard_normal(t.shape)
        for c in range(0, M_MAX, 3):
            x[(2 + c) % 19, c] = np.nan
            y[(7 + c) % 23, c] = np.nan
            z[(11 + c) % 17, c] = np.nan
        y[[3, 9, 15], 1] = np.nan
        x[:, 4] = y[:, 4] = z[:, 4] = np.nan
        y[:, 5] = -y[:, 5]
        _BASE[key] = tuple(np.ascontiguousarray(a.astype(dtype)) for a in (x, y, z))
    return _BASE[key]


def triple(T, M, dtype=np.float64):
    return tuple(np.ascontiguousarray(a[:T, :M]) for a in base(dtype))


def mask_for(M):
    m = np.ones(M, dtype=np.uint8)
    m[[c for c in (0, 6, 63, 64, M - 1) if c < M]] = 0
    return m


def indices(T, B, block, seed=0):
    """the recipe of collocation.bootstrap_indices, written out independently"""
    nb = -(-T // block)
    starts = np.random.default_rng(seed).integers(0, T, size=(B, nb))
    out = np.empty((T, B), dtype=np.uint16)
    for b in range(B):
        steps = np.concatenate([(s + np.arange(block)) % T for s in starts[b]])[:T]
        out[:, b] = steps
    return out


def formulas(q):
    """the eight statistics (8, ...) from the covariances q = (Qxx, Qyy, Qzz, Qxy, Qxz, Qyz), NaN where a cross-covariance is not > 0"""
    qxx, qyy, qzz, qxy, qxz, qyz = q
    with np.errstate(all="ignore"):
        st = np.stack([qxx - qxy * qxz / qyz, qyy - qxy * qyz / qxz, qzz - qxz * qyz / qxy, qxy * qxz / (qxx * qyz),
                       qxy * qyz / (qyy * qxz), qxz * qyz / (qzz * qxy), qyz / qxz, qyz / qxy])
    bad = ~((qxy > 0) & (qxz > 0) & (qyz > 0))
    st[:, bad] = np.nan
    return st


def oracle(x, y, z, min_samples=10, mask=None):
    """(stats (8, M) longdouble, cov (6, M) longdouble, n (M,)): every pixel at once, the arrays may carry a replicate axis in
    front of the pixels ((T, ..., M))"""
    x, y, z = (np.asarray(a, dtype=np.float64).astype(LD) for a in (x, y, z))
    ok = ~(np.isnan(x) | np.isnan(y) | np.isnan(z))
    if mask is not None:
        ok = ok & (np.asarray(mask) != 0)
    n = ok.sum(axis=0)
    with np.errstate(all="ignore"):
        den = np.maximum(n, 1).astype(LD)
        d = [np.where(ok, a - np.where(ok, a, 0).sum(axis=0) / den, 0) for a in (x, y, z)]
        n1 = np.maximum(n - 1, 1).astype(LD)
        cov = np.stack([(d[a] * d[b]).sum(axis=0) / n1 for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))])
    few = n < min_samples
    cov[:, few] = np.nan
    st = formulas(cov)
    st[:, few] = np.nan
    return st, cov, n


def scales(cov):
    """the scale of every statistic's error: (8, ...) from the oracle's covariances and statistics"""
    st = formulas(cov)
    one = np.ones_like(cov[0])
    return np.stack([cov[0], cov[1], cov[2], one, one, one, np.abs(st[6]), np.abs(st[7])]).astype(np.float64)


def worst_error(got, want_st, want_cov, where=""):
    """the largest |got - want| / scale in units of eps; NaN in the same places"""
    want = want_st.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want_st)), where
    fin = ~np.isnan(want)
    if not fin.any():
        return 0.0
    err = np.abs(got.astype(LD) - want_st)[fin] / scales(want_cov)[fin]
    return float(err.max() / EPS)


def oracle_replicates(x, y, z, idx, min_samples=10):
    """(stats (8, B, M), cov (6, B, M)) of the resampled series: replicate b takes the steps idx[:, b]"""
    xs, ys, zs = (np.asarray(a)[idx] for a in (x, y, z))          # (T, B, M)
    st, cov, _ = oracle(xs, ys, zs, min_samples)
    return st, cov


def flags_of(stats, n, min_samples, mask=None):
    """the flag word implied by a statistics array (8, M) and the counts: what the definitions say, from the twin's own values"""
    M = n.shape[0]
    f = np.zeros(M, dtype=np.int32)
    masked = np.zeros(M, dtype=bool) if mask is None else (np.asarray(mask) == 0)
    few = ~masked & (n < min_samples)
    und = ~masked & ~few & np.isnan(stats[0])
    f[masked] |= F_MASKED
    f[few] |= F_FEW
    f[und] |= F_NONPOS
    with np.errstate(invalid="ignore"):
        f[stats[0] < 0] |= F_NEG_X
        f[stats[1] < 0] |= F_NEG_Y
        f[stats[2] < 0] |= F_NEG_Z
        f[(stats[3] > 1) | (stats[4] > 1) | (stats[5] > 1)] |= F_RHO2
    return f


def check_summary(summary, n_ok, rep, q, where=""):
    """the bootstrap summaries against numpy on the twin's own replicate planes rep (B, 8, M): quantiles bit for bit, n_ok
    exact, mean and std within MOMENT_BOUND_EPS; returns the largest moment error in eps"""
    B = rep.shape[0]
    cnt = (~np.isnan(rep)).sum(axis=0)
    assert np.array_equal(n_ok, cnt), where
    worst = 0.0
    for s in range(8):
        for m in range(rep.shape[2]):
            v = rep[:, s, m]
            got = summary[s, :, m]
            if cnt[s, m] < 2:
                assert np.isnan(got).all(), (where, s, m)
                continue
            assert np.array_equal(got[2:], np.nanquantile(v, q)), (where, s, m)
            fin = v[~np.isnan(v)]
            mag = np.abs(fin).max()
            em = abs(got[0] - fin.astype(LD).mean()) / mag / EPS
            es = abs(got[1] - np.sqrt(((fin.astype(LD) - fin.astype(LD).mean()) ** 2).sum() / (fin.size - 1))) / mag / EPS
            worst = max(worst, float(em), float(es))
    assert B >= 1 and worst <= MOMENT_BOUND_EPS, (where, worst)
    return worst
