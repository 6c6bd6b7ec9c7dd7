"""Oracles and bounds of the EOF tests (tests/test_cabi_eof.py on the host twins, tests/test_gpu_eof.py on the device).

The oracle forms the weighted anomaly matrix a[t, m] = sqrt(w_m) (x[t, m] - mean_m) in numpy ``longdouble`` (64-bit
mantissa) from the GIVEN fp64 mean, its Gram matrix in longdouble ("exact" next to 2^-53), and the modes by
``numpy.linalg.svd`` of the fp64 rounding of a.

The entrywise Gram bound is  B[t, s] = (n_valid + 3) 2^-53 sum_m |a[t, m]| |a[s, m]|.  It holds for any order of the sum:
n - 1 additions and one rounding of every product make n, the subtraction x - mean of either factor two more; one is left.
sqrt(w) and its product with the difference add up to four roundings, so for general weights the first-order worst case is
n + 6: the cases with fewer than 8 valid series therefore use unit weights or powers of 4, whose square root and product are
exact, and the bound is rigorous there (largest observed 0.70 of B, at one series); from 31 valid series on, errors that all
line up are out of the question (largest observed 0.13 of B).

gamma(k) = k u / (1 - k u), u = 2^-53, bounds a chain of k roundings (Higham, Accuracy and Stability, lemma 3.1).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
CHUNK, SPLIT_MIN, SPLIT_MAX = 32, 8, 256           # csrc/eof_core.h
GRAM_TS = (2, 15, 16, 17, 33, 181, 256)
# 1, 3, chunk - 1, chunk, chunk + 1, one past a full split (two splits, the second one series), three splits with a ragged end
GRAM_MS = (1, 3, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK * SPLIT_MIN + 1, 600)


def gamma(k):
    return k * U / (1.0 - k * U)


def geom(T, M):
    """(nb, nblk, splits) of gd_eof_gram, restated from include/gandanet.h"""
    nb = (T + 15) // 16
    chunks = -(-M // CHUNK)
    s = min(max(-(-chunks // SPLIT_MIN), 1), SPLIT_MAX)
    per = -(-chunks // s)
    return nb, nb * (nb + 1) // 2, -(-chunks // per)


def cube(T, M, dtype=np.float64, seed=0):
    """a (T, M) cube with a level, a trend and noise per series"""
    rng = np.random.default_rng(1000 * T + M + seed)
    t = np.arange(T)[:, None]
    x = rng.normal(0, 3, (1, M)) + 0.02 * t * rng.normal(0, 1, (1, M)) + rng.standard_normal((T, M))
    return np.ascontiguousarray(x.astype(dtype))


def pow4_weights(M, seed=0):
    return 4.0 ** np.random.default_rng(seed).integers(-2, 3, M).astype(np.float64)


def coslat_weights(M):
    return np.cos(np.deg2rad(np.linspace(-89.5, 89.5, M)))


def int_cube(T, M, centred, seed=0):
    """integers in [-8, 8]; ``centred``: every column sums to zero over t (rows come in pairs v, -v, an odd T ends in 0)"""
    rng = np.random.default_rng(7 * T + M + seed)
    x = rng.integers(-8, 9, (T, M))
    if centred:
        x[T // 2:2 * (T // 2)] = -x[:T // 2]
        x[2 * (T // 2):] = 0
    return x


def valid_oracle(x, mask=None, weight=None):
    ok = np.isfinite(x.astype(np.float64)).all(axis=0)
    if mask is not None:
        ok &= np.asarray(mask).reshape(-1) != 0
    if weight is not None:
        ok &= np.isfinite(weight) & (weight > 0)
    return ok


def mean_oracle(x, valid, center=True):
    """(the exact mean in longdouble rounded to fp64, the bound of the sequential fp64 sum over T and its division)"""
    T = x.shape[0]
    xv = np.where(valid[None, :], x.astype(np.float64), 0.0).astype(LD)
    mean = (xv.sum(axis=0) / T).astype(np.float64) if center else np.zeros(x.shape[1])
    bound = gamma(T) * np.abs(xv).sum(axis=0).astype(np.float64) / T + U * np.abs(mean)
    return mean, bound


def anomalies(x, mean, valid, weight=None):
    """the weighted anomaly matrix in longdouble, exactly zero at invalid series"""
    d = x.astype(LD) - np.asarray(mean, dtype=np.float64).astype(LD)[None, :]
    if weight is not None:
        d = d * np.sqrt(np.where(valid, weight, 1.0).astype(LD))[None, :]
    return np.where(np.asarray(valid, dtype=bool)[None, :], d, LD(0))


def gram_bound(a, n_valid):
    aa = np.abs(a).astype(np.float64)
    return (n_valid + 3) * U * (aa @ aa.T)


def check_gram(G, a, n_valid, what=""):
    """asserts |G - oracle| <= B entrywise and bitwise symmetry; returns the largest error / bound"""
    want = (a @ a.T).astype(np.float64)
    B = gram_bound(a, n_valid)
    err = np.abs(G - want)
    assert np.array_equal(G, G.T), f"{what}: G is not bitwise symmetric"
    assert np.all(err <= B), f"{what}: error / bound up to {float((err / np.maximum(B, 1e-300)).max()):.3f}"
    return float((err / np.maximum(B, 1e-300)).max()) if B.max() > 0 else 0.0


def project_oracle(x, mean, valid, coef, weight=None):
    """(out (K, M) in longdouble rounded to fp64 with NaN at invalid series, its bound): T products and T - 1 additions, the
    subtraction, sqrt and the final product: T + 3 roundings on sum_t |c| |x - mean| sqrt(w)"""
    T = x.shape[0]
    ok = np.asarray(valid, dtype=bool)
    d = np.where(ok[None, :], x.astype(np.float64), 0.0).astype(LD) - np.where(ok, mean, 0.0).astype(LD)[None, :]
    s = np.sqrt(np.where(ok, weight, 1.0).astype(LD)) if weight is not None else np.ones(x.shape[1], dtype=LD)
    c = coef.astype(LD)
    out = (c.T @ d) * s[None, :]
    bound = gamma(T + 3) * ((np.abs(c).T @ np.abs(d)) * s[None, :])
    out, bound = out.astype(np.float64), bound.astype(np.float64)
    out[:, ~ok] = np.nan
    return out, bound


def reconstruct_oracle(eofs, pcs, mean, valid, weight=None, dtype=np.float64):
    """(out (T, M) in longdouble with NaN at invalid series, its bound): K products, K - 1 additions, sqrt and the division
    make K + 2 roundings on sum_k |p| |e| / sqrt(w); the addition of the mean and the rounding to ``dtype`` act on the result"""
    K = eofs.shape[0]
    ok = np.asarray(valid, dtype=bool)
    e = np.where(ok[None, :], eofs, 0.0).astype(LD)
    s = np.sqrt(np.where(ok, weight, 1.0).astype(LD)) if weight is not None else np.ones(eofs.shape[1], dtype=LD)
    p = pcs.astype(LD)
    out = np.where(ok, mean, 0.0).astype(LD)[None, :] + (p @ e) / s[None, :]
    u_out = 2.0 ** -24 if np.dtype(dtype) == np.float32 else U
    bound = gamma(K + 2) * ((np.abs(p) @ np.abs(e)) / s[None, :]) + (U + u_out) * (1 + 2 * U) * np.abs(out)
    out, bound = out.astype(np.float64), bound.astype(np.float64)
    out[:, ~ok] = np.nan
    return out, bound


def fix_signs(u):
    u = u.copy()
    for k in range(u.shape[1]):
        if u[np.argmax(np.abs(u[:, k])), k] < 0:
            u[:, k] = -u[:, k]
    return u


def svd_modes(a):
    """(sigma^2 descending, U (T, r) with fixed signs, V (r, M) with the matching signs) of the anomaly matrix"""
    u, s, vt = np.linalg.svd(a.astype(np.float64), full_matrices=False)
    uf = fix_signs(u)
    flip = np.sign((uf * u).sum(axis=0))
    return s * s, uf, vt * flip[:, None]


def sin_angle(a, b):
    """sin of the angle between two vectors"""
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return float(np.linalg.norm(a - b * (a @ b)))


def low_rank_cube(T, shape, sigmas, noise=1e-3, seed=0, dtype=np.float64):
    """mean field + sum_k sigma_k u_k v_k^T + noise: orthonormal u_k (orthogonal to the constant) and v_k, sigma well apart"""
    rng = np.random.default_rng(seed)
    M = int(np.prod(shape))
    q, _ = np.linalg.qr(np.column_stack([np.ones(T), rng.standard_normal((T, len(sigmas)))]))
    v, _ = np.linalg.qr(rng.standard_normal((M, len(sigmas))))
    x = 5.0 + rng.standard_normal(M)[None, :] + (q[:, 1:] * np.asarray(sigmas)) @ v.T + noise * rng.standard_normal((T, M))
    return np.ascontiguousarray(x.astype(dtype)).reshape((T,) + tuple(shape))


def full_rank_bound(x2, mean, valid, weight, gram):
    """The entrywise bound of |reconstruct() - x| at the valid series when all T modes are kept, from the reference tool's
    own decomposition of ``gram`` (numpy.linalg.eigh: lambda, U).  The rebuilt weighted anomaly is U U^T a with every mode
    of lambda > 0 (a null mode has a zero pattern), so with A = |U| |U|^T |a| (entrywise) the error is at most
      ||U U^T - I||_2 ||a[:, m]||_2                the loss of orthogonality of eigh, measured on its output
      + sum over the modes with lambda <= 0 of |U[t, k]| |U[:, k]^T a[:, m]|                    the modes left out
      + (gamma(T + 3) + 4 u) A                     the projection (project_oracle), sqrt and quotient in U / sqrt(lambda), sqrt
                                                   and product in sqrt(lambda) U: sqrt(lambda) itself cancels
      + gamma(T + 2) A                             the sum over k = T modes, sqrt(w) and the division (reconstruct_oracle),
    all divided by sqrt(w), plus 2 u |x| for the addition of the mean and the rounding of the result; x = mean + a / sqrt(w)
    holds exactly for the oracle's a.  Second-order terms are covered by the factor 1 + gamma(T + 3)."""
    T = x2.shape[0]
    ok = np.asarray(valid, dtype=bool)
    a = anomalies(x2, mean, valid, weight)
    lam, u = np.linalg.eigh(gram)
    orth = float(np.linalg.norm(u @ u.T - np.eye(T), 2))
    a64 = np.abs(a).astype(np.float64)
    A = np.abs(u) @ (np.abs(u).T @ a64)
    tol = orth * np.linalg.norm(a64, axis=0)[None, :] + (gamma(T + 3) + gamma(T + 2) + 4 * U) * A
    for k in np.nonzero(lam <= 0)[0]:
        tol = tol + np.abs(u[:, k:k + 1]) * np.abs(u[:, k].astype(LD) @ a).astype(np.float64)[None, :]
    s = np.sqrt(np.where(ok, weight, 1.0)) if weight is not None else np.ones(x2.shape[1])
    tol = (1 + gamma(T + 3)) * tol / s[None, :] + 2 * U * np.abs(x2.astype(np.float64))
    return tol[:, ok]
