"""The numpy oracle of the SSA tests (include/gandanet.h, "Singular spectrum analysis"): the lag covariance in np.longdouble,
numpy.linalg.eigh, the sort and sign rule, diagonal averaging and the staged gap-filling iteration, with the series
generators and, for every float output, a forward-error bound.

Bounds.  The oracle centres a series exactly as the twin does -- y = x - mean in fp64 with the twin's own mean plane, which
the tests hold to the longdouble mean separately -- so both decompose the same y, and what differs is the fp64 summation of
C and the Jacobi solve; both are backward stable, so the twin's eigenvalues are those of C + dC with

    ||dC||_F <= g(M) * eps * ||C||_F,    g(M) = G * sqrt(M)    (Jacobi's rotations per entry grow with M; sqrt is the usual
                                                                statistical growth)

and Weyl's inequality gives |d lambda| <= ||dC||_2 <= ||dC||_F.  The eigenvector of an eigenvalue whose gap to its
neighbours is `gap` moves by about ||dC|| / gap (Davis-Kahan), and a reconstructed component, e e^T applied to windows of y
and averaged, by about twice that times sqrt(M) * max|y|.  A group of components moves by ||dC|| / (its gap to the rest).

The constants were not chosen in advance.  MEASURED_* below are the largest (error / (eps * its scale)) that the HOST TWIN
showed against this oracle on the CPU over every shape, method, dtype and generator of tests/test_cabi_ssa.py
(python -m pytest tests/test_cabi_ssa.py -s prints them); the tests assert MARGIN = 4 times the measured value, the room
the change-point tests leave for other libm and compiler versions.
"""
import numpy as np

EPS = 2.0 ** -52
MARGIN = 4.0
MEASURED_EIG = 2.798       # |eig - oracle| / (eps * sqrt(M) * ||C||_F), largest seen
MEASURED_RC = 0.886        # |rc - oracle| / (eps * sqrt(M) * ||C||_F / gap * 2 * sqrt(M) * max|y|), largest seen
MEASURED_ORTH = 0.333       # max|E^T E - I| / (sweeps * M * eps), largest seen
MEASURED_RESID = 0.110      # ||C e - lambda e||_2 / (eps * sqrt(M) * ||C||_F + 2 ||C||_F * orthogonality bound), largest seen
MEASURED_ITERATE = 2.9e-14 # |twin filled - oracle filled| / sd over the fill cases of the suite, largest seen
MEASURED_SWEEPS = 14       # the most Jacobi sweeps any series of the suite took (GD_SSA_MAX_SWEEPS = 30)
G_EIG = MARGIN * MEASURED_EIG
G_RC = MARGIN * MEASURED_RC
G_ORTH = MARGIN * MEASURED_ORTH
G_RESID = MARGIN * MEASURED_RESID
ITERATE_RTOL = MARGIN * MEASURED_ITERATE

MAPS = ("n", "n_gaps", "mean", "sd", "trace", "sweeps", "iterations", "last_change", "flags")
IX = {nm: k for k, nm in enumerate(MAPS)}
MASKED, FEW, CONSTANT, NONFINITE, GAPS, SWEEPS, ITER = 1, 2, 4, 8, 16, 32, 64
METHODS = ("bk", "vg")
TS = (3, 8, 9, 24, 47, 64, 65, 181)
MS = (2, 3, 4, 5, 12, 24, 31, 32, 33, 63, 64)


def shapes(ts=TS, ms=MS):
    return [(T, M) for T in ts for M in ms if T >= 2 * M - 1]


# ---- generators ---------------------------------------------------------------------------------------------------------------
def planted_values(T: int, P: int = 4):
    """noiseless trend + annual + semi-annual (rank <= 6), fp64, one phase per column"""
    t = np.arange(T, dtype=np.float64)[:, None]
    ph = np.arange(P, dtype=np.float64)[None, :]
    return 0.02 * t + 1.5 * np.sin(2 * np.pi * t / 12.0 + 0.7 * ph) + 0.6 * np.cos(2 * np.pi * t / 6.0 + 0.3 * ph) + 3.0


def series(T: int, dtype=np.float64, seed: int = 0):
    """(T, 8) complete series of every kind: planted, planted + noise, white noise, a random walk, a pure sinusoid (one
    separated pair), an offset of 50 sd, integers 0 .. 3, a damped oscillation"""
    rng = np.random.default_rng(1000 * T + seed)
    t = np.arange(T, dtype=np.float64)
    p = planted_values(T, 2)
    cols = [p[:, 0], p[:, 1] + 0.3 * rng.standard_normal(T), rng.standard_normal(T), np.cumsum(rng.standard_normal(T)),
            2.0 * np.sin(2 * np.pi * t / 7.3 + 0.4), 50.0 + rng.standard_normal(T), rng.integers(0, 4, T).astype(np.float64),
            np.exp(-t / max(T, 2) * 2.0) * np.cos(2 * np.pi * t / 9.0) + 0.05 * rng.standard_normal(T)]
    if T < 5:
        cols[6] = np.arange(T, dtype=np.float64) ** 2          # short integer series could be constant
    return np.ascontiguousarray(np.stack(cols, 1).astype(dtype))


def grace_gaps(T: int, seed: int = 0):
    """the GRACE pattern scaled to T: one run of 11 steps and about T / 9 scattered single steps (bool (T,), True = gap)"""
    rng = np.random.default_rng(seed)
    g = np.zeros(T, dtype=bool)
    a = int(0.6 * T)
    g[a:a + 11] = True
    g[rng.choice(np.setdiff1d(np.arange(T), np.arange(a - 1, a + 12)), size=max(1, T // 9), replace=False)] = True
    return g


# ---- the definitions ------------------------------------------------------------------------------------------------------------
def covariance(y, M: int, method: str):
    """C of the complete centred series y (any float type; sums in np.longdouble)"""
    y = np.asarray(y, dtype=np.longdouble)
    T = y.size
    K = T - M + 1
    if method == "bk":
        X = np.stack([y[i:i + K] for i in range(M)], 1)
        return (X.T @ X) / np.longdouble(K)
    c = np.array([np.dot(y[:T - l], y[l:]) / np.longdouble(T - l) for l in range(M)])
    return c[np.abs(np.subtract.outer(np.arange(M), np.arange(M)))]


def eigen(C):
    """eigenpairs of the fp64 image of C: descending eigenvalue (ties to the lower original index of eigh's ascending order
    reversed), first entry of largest magnitude positive"""
    w, v = np.linalg.eigh(np.asarray(C, dtype=np.float64))
    order = np.argsort(-w, kind="stable")
    w, v = w[order], v[:, order]
    for k in range(v.shape[1]):
        if v[np.argmax(np.abs(v[:, k])), k] < 0:
            v[:, k] = -v[:, k]
    return w, v


def components(y, E, ks):
    """RC_k (len(ks), T) of the complete centred fp64 series y"""
    T, M = y.size, E.shape[0]
    K = T - M + 1
    X = np.stack([y[i:i + K] for i in range(M)], 1)            # (K, M)
    out = np.zeros((len(ks), T))
    cnt = np.zeros(T)
    for j in range(M):
        cnt[j:j + K] += 1
    for a, k in enumerate(ks):
        pc = X @ E[:, k]
        for j in range(M):
            out[a, j:j + K] += pc * E[j, k]
        out[a] /= cnt
    return out


def stats(col):
    """n, mean, sd (fp64 values of longdouble sums) and the flags that do not depend on the entry point"""
    col = np.asarray(col, dtype=np.float64)
    ok = ~np.isnan(col)
    n = int(ok.sum())
    if np.isinf(col[ok]).any():
        return n, np.nan, np.nan, NONFINITE
    if n == 0:
        return 0, np.nan, np.nan, 0
    v = col[ok].astype(np.longdouble)
    mean = v.sum() / n
    sd = np.sqrt(((v - mean) ** 2).sum() / n)
    return n, float(mean), float(sd), (0 if float(sd) > 0.0 else CONSTANT)


def decompose(col, M: int, method: str, mean_plane=None):
    """the oracle of one series: dict with n, n_gaps, mean, sd, flags and, for a complete regular series, eig (M), E, trace, rc
    (M, T), C (fp64), eig_bound (scalar, without G), gap (M): the distance of eigenvalue k to its nearest neighbour.
    ``mean_plane``: the twin's mean of this series; the series is then centred with it in fp64, as the twin centres it"""
    col = np.asarray(col, dtype=np.float64)
    T = col.size
    n, mean, sd, flags = stats(col)
    if n < T:
        flags |= GAPS
    out = dict(n=n, n_gaps=T - n, mean=mean, sd=sd, flags=flags)
    if flags:
        return out
    y = col - (mean if mean_plane is None else float(mean_plane))
    C = covariance(y, M, method)
    w, E = eigen(C)
    gap = np.array([min([abs(w[k] - w[j]) for j in range(M) if j != k]) for k in range(M)])
    out.update(eig=w, E=E, trace=float(w.sum()), rc=components(y, E, range(M)), y=y, gap=gap,
               C=np.asarray(C, dtype=np.float64), eig_bound=EPS * np.sqrt(M) * np.linalg.norm(np.asarray(C, dtype=np.float64)))
    return out


def rc_bound(o, M: int, gap):
    """the bound (without G_RC) of a component, or of a group, whose eigenvalues keep `gap` from the others"""
    return o["eig_bound"] / gap * 2.0 * np.sqrt(M) * np.abs(o["y"]).max()


def fill(col, M: int, rank: int, method: str = "bk", tol: float = 1e-3, max_iter: int = 20, min_valid=None):
    """the oracle of gd_ssa_fill for one series: dict with n, n_gaps, mean, sd, flags, and for a regular series filled (T), eig
    (rank), iterations, last_change, changes: [(change, tol * sd)] of every iteration"""
    col = np.asarray(col, dtype=np.float64)
    T = col.size
    min_valid = 2 * M if min_valid is None else min_valid
    n, mean, sd, flags = stats(col)
    if n < min_valid:
        flags |= FEW
    out = dict(n=n, n_gaps=T - n, mean=mean, sd=sd, flags=flags)
    if flags:
        return out
    gapm = np.isnan(col)
    y = np.where(gapm, 0.0, col - mean)
    changes, iters, last = [], 0, 0.0
    if not gapm.any():
        w, E = eigen(covariance(y, M, method))
    else:
        for q in range(1, rank + 1):
            done = False
            for _ in range(max_iter):
                w, E = eigen(covariance(y, M, method))
                R = components(y, E, range(q)).sum(0)
                last = float(np.abs(R[gapm] - y[gapm]).max())
                y[gapm] = R[gapm]
                iters += 1
                changes.append((last, tol * sd))
                if last <= tol * sd:
                    done = True
                    break
            if not done:
                out["flags"] |= ITER
    out.update(filled=np.where(gapm, mean + y, col), eig=w[:rank], iterations=iters, last_change=last, changes=changes, trace=float(w.sum()))
    return out
