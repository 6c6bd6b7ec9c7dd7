"""Cases and the oracle of the neighbourhood-verification tests (test_cabi_neighborhood.py, test_gpu_neighborhood.py).

The oracle holds no prefix sum: the window counts cf, co, cv are scipy.ndimage correlations of the int64 indicator with a
box of ones in mode="constant" (positions outside the domain count zero) -- ``scipy.ndimage.correlate(ind, np.ones((n, n)))``
wherever its n^2 taps per pixel are affordable, and otherwise the same box applied as two ``correlate1d`` passes with
``np.ones(n)`` (a box of ones is separable and the arithmetic is exact int64, so the two are one function;
``check_box_forms_agree`` holds them against each other).  The sums are Python / NumPy int64 in window mode and ``math.fsum``
of the fp64 terms in valid mode.

The bound of the valid mode.  Every term -- (pf - po)^2, pf^2, po^2 with pf = cf / cv, po = co / cv -- is formed by the same
correctly rounded fp64 operations here and in the code under test, so the terms are the same numbers and only the order of
their addition differs.  N non-negative terms added in ANY order with N - 1 roundings give a sum within gamma_{N-1} = (N - 1) u
/ (1 - (N - 1) u) of the true sum, relative (Higham, Accuracy and Stability, 4.2; u = 2^-53), and fsum is the true sum rounded
once (u more).  ``sum_bound`` is N u / (1 - N u) times the fsum, which covers both; it is zero for an empty or all-zero sum,
where every order is exact.  Nothing in it is tuned to the device.
"""
import functools
import math

import numpy as np
from scipy import ndimage

U64 = 2.0 ** -53
LITERAL_TAPS = 4_000_000     # n * n * H * W up to which the box is one 2-D correlate


class Case:
    """two (T, H, W) cubes whose values are exact in fp32 (so the fp32 and the fp64 twin share one oracle), (T, K)
    threshold tables, an optional (H, W) mask"""

    def __init__(self, name, f, o, thr_f, thr_o, mask=None):
        self.name, self.f, self.o, self.mask = name, f, o, mask
        T = f.shape[0]
        self.thr_f = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_f, dtype=np.float64), (T, np.shape(thr_f)[-1])))
        self.thr_o = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_o, dtype=np.float64), (T, np.shape(thr_o)[-1])))
        hw = max(f.shape[1], f.shape[2])
        self.scales = (1, 3, 5, 9, 33, 2 * hw + 1)     # the last: the whole domain, clipped on every side

    def __repr__(self):
        return f"{self.name}{tuple(self.f.shape)}"

    def cubes(self, dtype):
        return self.f.astype(dtype), self.o.astype(dtype)


def _fields(shape, seed):
    rng = np.random.default_rng(seed)
    f = rng.normal(size=shape).astype(np.float32).astype(np.float64)
    o = (0.6 * f + 0.8 * rng.normal(size=shape)).astype(np.float32).astype(np.float64)
    return rng, f, o


def _plain(name, shape, seed, thr):
    rng, f, o = _fields(shape, seed)
    if f.size > 40:
        f.reshape(-1)[rng.integers(f.size)] = np.nan
        o.reshape(-1)[rng.integers(o.size)] = np.nan
    return Case(name, f, o, thr, thr)


def _full(shape=(4, 70, 129), seed=5):
    """a mask, NaNs placed separately in f and in o, values EQUAL to a threshold, per-step per-field tables, K = 3"""
    rng, f, o = _fields(shape, seed)
    T, H, W = shape
    mask = (rng.random((H, W)) < 0.85).astype(np.uint8)
    thr_f = np.sort(rng.normal(scale=0.7, size=(T, 3)).astype(np.float32).astype(np.float64), axis=1)
    thr_o = np.sort(rng.normal(scale=0.7, size=(T, 3)).astype(np.float32).astype(np.float64), axis=1)
    for t in range(T):
        for k in range(3):     # a dozen voxels of each field sit exactly on each of their thresholds
            f[t].reshape(-1)[rng.choice(H * W, 12, replace=False)] = thr_f[t, k]
            o[t].reshape(-1)[rng.choice(H * W, 12, replace=False)] = thr_o[t, k]
    f.reshape(-1)[rng.choice(f.size, 60, replace=False)] = np.nan
    o.reshape(-1)[rng.choice(o.size, 60, replace=False)] = np.nan
    return Case("full", f, o, thr_f, thr_o, mask)


CASES = [
    _plain("sub-wave", (3, 5, 7), 1, (-0.5, 0.3)),            # smaller than a wave
    _plain("carry", (2, 37, 131), 2, (-0.5, 0.3)),            # a row crosses two 64-lane segments plus a tail
    _plain("one-row", (1, 1, 300), 3, (-0.5, 0.3)),           # a single row longer than a workgroup
    _plain("one-column", (1, 300, 1), 4, (-0.5, 0.3)),
    _full(),
]
BY_NAME = {c.name: c for c in CASES}
DTYPES = (np.float32, np.float64)
# an fp32 and an fp64 twin of every case; both values of `below` on the full case
TWINS = [(c, dt, below) for c in CASES for dt in DTYPES for below in ((True, False) if c.name == "full" else (True,))]


def twin_id(v):
    return repr(v) if isinstance(v, Case) else ("below" if v else "above") if isinstance(v, bool) else np.dtype(v).name


def check_case_properties():
    c = BY_NAME["full"]
    assert c.mask is not None and 0 < c.mask.sum() < c.mask.size
    nf, no = np.isnan(c.f), np.isnan(c.o)
    assert nf.any() and no.any() and (nf & ~no).any() and (no & ~nf).any()
    assert c.thr_f.shape == (4, 3) and not np.array_equal(c.thr_f, c.thr_o) and not np.array_equal(c.thr_f[0], c.thr_f[1])
    for t in range(4):
        for k in range(3):
            assert (c.f[t] == c.thr_f[t, k]).sum() >= 6 and (c.o[t] == c.thr_o[t, k]).sum() >= 6
    for case in CASES:
        for x in (case.f, case.o):
            assert np.array_equal(x.astype(np.float32).astype(np.float64), x, equal_nan=True)
        assert case.scales[-1] == 2 * max(case.f.shape[1:]) + 1


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def box_2d(ind, n):
    return ndimage.correlate(ind, np.ones((n, n), dtype=np.int64), mode="constant", cval=0)


def box_separable(ind, n):
    ones = np.ones(n, dtype=np.int64)
    return ndimage.correlate1d(ndimage.correlate1d(ind, ones, axis=0, mode="constant", cval=0), ones, axis=1, mode="constant", cval=0)


def box(ind, n):
    """the sum of the int64 (H, W) indicator over the n x n window around every pixel, outside = 0"""
    ind = np.ascontiguousarray(ind, dtype=np.int64)
    return box_2d(ind, n) if n * n * ind.size <= LITERAL_TAPS else box_separable(ind, n)


def check_box_forms_agree():
    rng = np.random.default_rng(11)
    for shape in ((5, 7), (1, 40), (40, 1), (23, 31)):
        ind = (rng.random(shape) < 0.4).astype(np.int64)
        for n in (1, 3, 5, 9, 33, 2 * max(shape) + 1):
            assert np.array_equal(box_2d(ind, n), box_separable(ind, n)), (shape, n)


def indicators(f, o, thr_f, thr_o, below, mask):
    """(valid, I_f, I_o) bool (H, W) of one step at one threshold pair; comparisons in fp64"""
    valid = ~np.isnan(f) & ~np.isnan(o)
    if mask is not None:
        valid &= mask != 0
    with np.errstate(invalid="ignore"):
        ef = (f <= thr_f) if below else (f >= thr_f)
        eo = (o <= thr_o) if below else (o >= thr_o)
    return valid, valid & ef, valid & eo


def sum_bound(total, n_terms):
    return 0.0 if n_terms == 0 else n_terms * U64 / (1.0 - n_terms * U64) * total


class Oracle:
    """window: sums (T, K, S, 3) uint64 and their per-pixel terms (T, K, S, H, W, 3) int64; valid: fsum sums (T, K, S, 3),
    their bounds and per-pixel fp64 terms; base (T, K, 3) uint64; counts cf, cv (T, K, S, H, W) and the valid centres"""


@functools.lru_cache(maxsize=None)
def oracle(name, below):
    case = BY_NAME[name]
    T, H, W = case.f.shape
    K, S = case.thr_f.shape[1], len(case.scales)
    r = Oracle()
    r.sums_w = np.zeros((T, K, S, 3), dtype=np.uint64)
    r.terms_w = np.zeros((T, K, S, H, W, 3), dtype=np.int64)
    r.sums_v, r.bound_v = np.zeros((T, K, S, 3)), np.zeros((T, K, S, 3))
    r.terms_v = np.zeros((T, K, S, H, W, 3))
    r.base = np.zeros((T, K, 3), dtype=np.uint64)
    r.cf, r.cv = np.zeros((T, K, S, H, W), dtype=np.int64), np.zeros((T, K, S, H, W), dtype=np.int64)
    r.valid = np.zeros((T, K, H, W), dtype=bool)
    for t in range(T):
        for k in range(K):
            valid, i_f, i_o = indicators(case.f[t], case.o[t], case.thr_f[t, k], case.thr_o[t, k], below, case.mask)
            r.valid[t, k] = valid
            r.base[t, k] = (int(i_f.sum()), int(i_o.sum()), int(valid.sum()))
            for s, n in enumerate(case.scales):
                cf, co, cv = box(i_f, n), box(i_o, n), box(valid, n)
                r.cf[t, k, s], r.cv[t, k, s] = cf, cv
                d = cf - co
                tw = np.stack([d * d, cf * cf, co * co], axis=-1) * valid[..., None]
                r.terms_w[t, k, s] = tw
                r.sums_w[t, k, s] = [int(tw[..., c].sum()) for c in range(3)]
                den = np.where(valid, cv, 1)
                pf, po = cf / den, co / den
                dv = pf - po
                tv = np.stack([dv * dv, pf * pf, po * po], axis=-1) * valid[..., None]
                r.terms_v[t, k, s] = tv
                n_terms = int(valid.sum())
                for c in range(3):
                    r.sums_v[t, k, s, c] = math.fsum(tv[..., c][valid].tolist())
                    r.bound_v[t, k, s, c] = sum_bound(r.sums_v[t, k, s, c], n_terms)
    return r


def worst_over_bound(got, want, bound):
    """the largest |got - want| / bound; where the bound is zero the two must be equal (inf otherwise)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(q.max()) if q.size else 0.0


def fraction_oracle(case, k, s, below, normalize):
    """(T, H, W): c / n^2 or c / cv of the forecast cube at threshold column k, NaN at an invalid centre (a NaN of f or a
    masked pixel; the observed cube plays no part)"""
    T, H, W = case.f.shape
    n = case.scales[s]
    out = np.full((T, H, W), np.nan)
    for t in range(T):
        valid, i_f, _ = indicators(case.f[t], case.f[t], case.thr_f[t, k], case.thr_f[t, k], below, case.mask)
        cf, cv = box(i_f, n), box(valid, n)
        frac = cf / (n * n) if normalize == "window" else cf / np.where(valid, cv, 1)
        out[t] = np.where(valid, frac, np.nan)
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def displaced(d=4, shape=(1, 41, 61), at=(20, 20)):
    """one event pixel in each field, the observed one d columns to the right, well inside the domain: A = 2 n min(d, n),
    B = C = n^2 for every n whose windows stay inside"""
    f, o = np.zeros(shape), np.zeros(shape)
    f[0, at[0], at[1]] = -1.0
    o[0, at[0], at[1] + d] = -1.0
    return f, o, (-0.5,), (1, 3, 5, 7, 9, 11)
