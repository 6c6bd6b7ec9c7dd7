"""numpy (fp64) restatement of what the evaluation kernels compute, shared by the CPU and GPU evaluation tests."""
import numpy as np


def record(p, t):
    """the 8-double record of include/gandanet.h ("evaluation") of fp32 or fp64 arrays, in fp64"""
    p, t = np.asarray(p, dtype=np.float64).ravel(), np.asarray(t, dtype=np.float64).ravel()
    if p.size == 0:
        return np.zeros(8)
    dp, dt = p - p.mean(), t - t.mean()
    return np.array([p.size, p.mean(), t.mean(), (dp * dp).sum(), (dt * dt).sum(), (dp * dt).sum(),
                     np.abs(p - t).sum(), ((p - t) ** 2).sum()])


def metrics(p, t):
    """mean_squared_error / mean_absolute_error / r2_score / np.corrcoef(t, p)[0, 1] in fp64; sklearn's own functions
    are used as well where the module is installed"""
    p, t = np.asarray(p, dtype=np.float64).ravel(), np.asarray(t, dtype=np.float64).ravel()
    out = {"n": float(p.size), "mse": ((p - t) ** 2).mean(), "mae": np.abs(p - t).mean(),
           "r2": 1.0 - ((p - t) ** 2).sum() / ((t - t.mean()) ** 2).sum(), "cc": np.corrcoef(t, p)[0, 1]}
    try:
        from sklearn.metrics import mean_absolute_error, mean_squared_error, r2_score
    except ImportError:
        return out
    sk = {"mse": mean_squared_error(t, p), "mae": mean_absolute_error(t, p), "r2": r2_score(t, p)}
    for k, v in sk.items():
        assert abs(v - out[k]) <= 1e-12 * max(1.0, abs(v)), (k, v, out[k])
    return out


def check_metrics(got, want, where=""):
    """the bounds of the issue: mse / mae 1e-9 relative, r2 / cc 1e-9 absolute (fp64 accumulation: n 2^-53 < 1e-11 at
    these sizes, two decades left for the co-moment cross terms)"""
    assert got["n"] == want["n"], (where, got["n"], want["n"])
    for k in ("mse", "mae"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (where, k, got[k], want[k])
    for k in ("r2", "cc"):
        assert abs(got[k] - want[k]) <= 1e-9, (where, k, got[k], want[k])


def offset_pair(n, seed=0):
    """x = 1000 + 0.01 randn, y = x + 0.003 randn as fp32: raw fp32 sums of squares lose everything here"""
    rng = np.random.default_rng(seed)
    x = (1000.0 + 0.01 * rng.standard_normal(n)).astype(np.float32)
    y = (x.astype(np.float64) + 0.003 * rng.standard_normal(n)).astype(np.float32)
    return x, y
