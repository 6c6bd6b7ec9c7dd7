"""CPU: the host twins of the lagged-correlation family (gd_lag_corr_host, gd_series_acf_host; csrc/lagcorr_core.h) against the
independent numpy oracle of tests/lagcorr_util.py within the bounds derived there, the exact properties of the definitions
(symmetry, tie rule, independence of M and of the column), the argument checks, and fdr_threshold against a numpy
Benjamini-Hochberg.  Each bound test prints its largest error over its bound (python -m pytest -s).

Measured: the largest |r_twin - r_oracle| over r_bound was 0.043 (T = 7, where three-pair overlaps reach kappa = 4.5e4 against
the cap 2^20; 0.007 at T = 181, kappa at most 1.4), the largest standard-acf error over acf_bound 0.0026."""
import numpy as np
import pytest

import lagcorr_util as U


def _K():
    from gan_danet_amd import kern
    return kern


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("lo,hi", U.RANGES)
@pytest.mark.parametrize("T", U.TS)
def test_twin_against_oracle(T, lo, hi, dtype):
    """every M: scattered NaNs, whole-NaN series and a NaN run longer than the lag range are columns 1 .. 5 of the inputs"""
    K = _K()
    worst = kmax = 0.0
    for M in U.MS_CPU:
        a, b = U.pair(T, M, dtype)
        r, n, best = K.lag_corr_host(a, b, lo, hi)
        wr, wn, kap = U.cached_oracle(T, lo, hi, dtype)
        w, k = U.check_curve(r, n, (wr[:, :M], wn[:, :M], kap[:, :M]), (T, M, lo, hi))
        worst, kmax = max(worst, w), max(kmax, k)
        U.check_best(best, r, n, lo, hi, "abs", (T, M, lo, hi))
        assert _eq(best[2], U.best_oracle(wr[:, :M], wn[:, :M], lo, hi)[2])          # best_n equals the oracle's integers
        if M > 5 and T == 181:
            assert np.isnan(r[:, [3, 5]]).all() and not n[:, [3, 5]].any() and np.isnan(best[0, [3, 5]]).all()
    print(f"T = {T}, lags {lo} .. {hi}, {np.dtype(dtype).name}: r at most {worst:.4f} of its bound, kappa at most {kmax:.1f}")


def test_invalid_lags():
    K = _K()
    a, b = U.pair(7, 5, nans=False)
    r, n, best = K.lag_corr_host(a, b, -6, 6, min_pairs=3)
    wr, wn, _ = U.lag_oracle(a, b, -6, 6, 3)
    assert np.array_equal(n, wn) and np.array_equal(n[:, 0], [1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1])     # n is kept
    assert np.isnan(r[[0, 1, 11, 12]]).all() and not np.isnan(r[2:11]).any()
    # every lag beyond the series: all NaN, best_lag NaN, best_n 0
    r, n, best = K.lag_corr_host(a, b, 7, 12)
    assert np.isnan(r).all() and not n.any() and np.isnan(best[[0, 1, 3]]).all() and not best[2].any()
    a1, b1 = U.pair(2, 3, nans=False)
    r, n, best = K.lag_corr_host(a1, b1, -3, 3)
    assert np.isnan(r).all() and np.isnan(best[0]).all() and np.array_equal(n[:, 0], [0, 0, 1, 2, 1, 0, 0])
    # a constant series: NaN at every lag
    c = a.copy()
    c[:, 2] = 1.25
    r, _, best = K.lag_corr_host(c, b, -3, 3)
    assert np.isnan(r[:, 2]).all() and np.isnan(best[0, 2]) and not np.isnan(r[:, [0, 1, 3, 4]]).any()
    r, _, _ = K.lag_corr_host(a, c, -3, 3)
    assert np.isnan(r[:, 2]).all()
    # constant on the overlap of one lag only: lag 5 pairs a[0], a[1] with b[5], b[6]; with two equal values the sums are
    # exact (2 q and (2 c)^2 / 2), so vb is exactly 0 there and nowhere else
    d = b.copy()
    d[6, 1] = d[5, 1]
    r, n, _ = K.lag_corr_host(a, d, 0, 5, min_pairs=2)
    assert np.isnan(r[5, 1]) and n[5, 1] == 2 and not np.isnan(r[:5, 1]).any() and not np.isnan(r[:, 0]).any()


@pytest.mark.parametrize("s", (-5, 0, 3))
def test_known_shift(s):
    K = _K()
    rng = np.random.default_rng(5 + s)
    T, M = 60, 9
    a = rng.standard_normal((T, M)) + 1.0
    b = rng.standard_normal((T, M))                     # b[t + s] = a[t] wherever both exist
    if s >= 0:
        b[s:] = a[:T - s]
    else:
        b[:T + s] = a[-s:]
    for select in ("abs", "max"):
        r, n, best = K.lag_corr_host(a, b, -8, 8, select=select)
        assert np.all(best[0] == s) and np.all(best[2] == T - abs(s))
        assert np.all(best[1] <= 1.0) and np.all(1.0 - best[1] <= U.r_bound(T - abs(s), 2.0))


def test_bit_for_bit_properties():
    K = _K()
    for dtype in (np.float64, np.float32):
        a, b = U.pair(181, 65, dtype)
        r, n, best = K.lag_corr_host(a, b, -12, 12)
        r2, n2, _ = K.lag_corr_host(b, a, -12, 12)
        assert _eq(r, r2[::-1]) and np.array_equal(n, n2[::-1])                      # (a, b) at l is (b, a) at -l
        acf, na = K.series_acf_host(b, 12, "pearson")
        rx, nx, _ = K.lag_corr_host(b, b, 0, 12)
        assert _eq(acf, rx) and np.array_equal(na, nx)
        # an index (T,) is the series tiled
        idx = np.ascontiguousarray(a[:, 7])
        ri, ni, bi = K.lag_corr_host(idx, b, -12, 12)
        rt, nt, bt = K.lag_corr_host(np.repeat(idx[:, None], 65, axis=1), b, -12, 12)
        assert _eq(ri, rt) and np.array_equal(ni, nt) and _eq(bi, bt)
        assert _eq(K.lag_corr_host(idx[:, None], b, -12, 12)[0], ri)
        # a series' outputs do not change with its column or with M
        perm = np.random.default_rng(1).permutation(65)
        rp, np_, bp = K.lag_corr_host(np.ascontiguousarray(a[:, perm]), np.ascontiguousarray(b[:, perm]), -12, 12)
        assert _eq(rp, r[:, perm]) and np.array_equal(np_, n[:, perm]) and _eq(bp, best[:, perm])
        rs, ns, bs = K.lag_corr_host(np.ascontiguousarray(a[:, :9]), np.ascontiguousarray(b[:, :9]), -12, 12)
        assert _eq(rs, r[:, :9]) and np.array_equal(ns, n[:, :9]) and _eq(bs, best[:, :9])
        # the curve asked for or not
        r0, n0, b0 = K.lag_corr_host(a, b, -12, 12, curve=False)
        assert r0 is None and n0 is None and _eq(b0, best)
        assert K.lag_corr_host(a, b, -12, 12, best=False)[2] is None


def test_tie_rule():
    K = _K()
    a, _ = U.pair(40, 6, nans=False)
    wr, wn, _ = U.lag_oracle(a, a, -6, 6)
    r, n, best = K.lag_corr_host(a, a, -6, 6, select="min")
    assert np.array_equal(r, r[::-1])                                               # +l and -l tie bitwise
    want = U.best_oracle(r, n, -6, 6, "min")
    lmin = want[0].astype(int)
    assert np.all(lmin > 0)                                                         # the positive lag of the pair wins
    for m in range(6):                                                              # the tie exists in the oracle's curve too
        assert abs(wr[6 + lmin[m], m] - wr[6 - lmin[m], m]) <= 2 * U.r_bound(40, 2.0) and np.argmin(wr[:, m]) in (6 + lmin[m], 6 - lmin[m])
    assert _eq(best, want)
    # select="abs" with a = b: lag 0 (r = 1) wins; "max" as well
    assert np.all(K.lag_corr_host(a, a, -6, 6, select="abs")[2][0] == 0)


def test_mask_bytes():
    K = _K()
    a, b = U.pair(181, 65)
    mask = U.mask_for(65)
    r, n, best = K.lag_corr_host(a, b, -3, 3, mask=mask)
    rf, nf, bf = K.lag_corr_host(a, b, -3, 3)
    off = mask == 0
    assert np.isnan(r[:, off]).all() and not n[:, off].any() and np.isnan(best[:, off][[0, 1, 3]]).all() and not best[2, off].any()
    assert _eq(r[:, ~off], rf[:, ~off]) and np.array_equal(n[:, ~off], nf[:, ~off]) and _eq(best[:, ~off], bf[:, ~off])
    acf, na = K.series_acf_host(b, 3, mask=mask)
    assert np.isnan(acf[:, off]).all() and not na[:, off].any()
    with pytest.raises(K.L.GandanetError):
        K.lag_corr_host(a, b, -3, 3, mask=np.ones(64, dtype=np.uint8))


def test_argument_errors():
    K = _K()
    E = K.L.GandanetError
    a, b = U.pair(7, 5, nans=False)
    for bad in (lambda: K.lag_corr_host(a, b, 2, 1), lambda: K.lag_corr_host(a, b, -65, 0), lambda: K.lag_corr_host(a, b, 0, 65),
                lambda: K.lag_corr_host(a, b, 0, 1.0), lambda: K.lag_corr_host(a, b, 0, 1, min_pairs=1),
                lambda: K.lag_corr_host(np.zeros((2049, 2)), np.zeros((2049, 2)), 0, 1), lambda: K.lag_corr_host(a[:, :2], b, 0, 1),
                lambda: K.lag_corr_host(a[:6], b, 0, 1), lambda: K.lag_corr_host(a.astype(np.float32), b, 0, 1),
                lambda: K.lag_corr_host(a, b, 0, 1, select="median"), lambda: K.lag_corr_host(a, b, 0, 1, curve=False, best=False),
                lambda: K.series_acf_host(a, 65), lambda: K.series_acf_host(a, -1), lambda: K.series_acf_host(a, 2, "yule"),
                lambda: K.series_acf_host(a, 2, min_pairs=1), lambda: K.series_acf_host(a[0], 2)):
        with pytest.raises(E):
            bad()
    lib = K.lib()
    p = a.ctypes.data
    assert lib.gd_lag_corr_host(p, p, 1, 7, 5, 5, 0, 1, 3, 0, None, None, None, None) == -1 and "every output is NULL" in K.L.last_error()
    assert lib.gd_lag_corr_host(p, p, 1, 7, 5, 2, 0, 1, 3, 0, None, p, None, None) == -1 and "a_M" in K.L.last_error()
    assert lib.gd_lag_corr_host(p, p, 1, 7, 5, 5, 0, 1, 3, 3, None, p, None, None) == -1 and "select" in K.L.last_error()


def test_standard_acf():
    K = _K()
    worst = 0.0
    for dtype in (np.float64, np.float32):
        for T in U.TS:
            _, x = U.pair(T, 65, dtype)
            acf, n = K.series_acf_host(x, 12)
            wa, wn, bound = U.acf_oracle(x, 12)
            assert np.array_equal(n, wn) and np.array_equal(np.isnan(acf), np.isnan(wa)), T
            fin = ~np.isnan(wa)
            assert np.all(acf[0][fin[0]] == 1.0)                                     # acf_0 == 1 exactly
            if fin.any():
                ratio = np.abs(acf[fin] - wa[fin]) / bound[fin]
                worst = max(worst, float(ratio.max()))
                assert ratio.max() <= 1.0, (T, float(ratio.max()))
    # gap-free input: the textbook formula sum (x_t - m)(x_(t+k) - m) / sum (x_t - m)^2
    _, x = U.pair(181, 8, nans=False)
    acf, n = K.series_acf_host(x, 5)
    d = x - x.mean(axis=0)
    for k in range(6):
        want = (d[:181 - k] * d[k:]).sum(axis=0) / (d * d).sum(axis=0)
        assert np.allclose(acf[k], want, rtol=0, atol=1e-13) and np.all(n[k] == 181 - k)
    print(f"standard acf at most {worst:.4f} of its bound")


def test_neff_clamp():
    """the formula of n_eff as numpy evaluates it: clamped to [0, n] (r1a r1b < 0 would give more than n, r1a r1b near 1 gives ~0)"""
    r = np.array([0.5, 0.5, 0.5, 0.5, np.nan])
    n = np.array([100.0, 100.0, 100.0, 100.0, 100.0])
    ne = U.neff_numpy(r, n, np.array([-0.5, 0.9, 1.0, -1.0, 0.1]), np.array([0.5, 0.9, 1.0, 1.0, 0.1]))
    assert ne[0] == 100.0 and 0.0 < ne[1] < 100.0 and ne[2] == 0.0 and ne[3] == 100.0 and np.isnan(ne[4])


def test_fdr_threshold():
    import torch
    from gan_danet_amd import lagcorr as LC
    rng = np.random.default_rng(11)
    p = rng.uniform(0.0, 1.0, (23, 17))
    p[rng.uniform(size=p.shape) < 0.3] *= 1e-3                                       # a share of true discoveries
    p[rng.uniform(size=p.shape) < 0.1] = np.nan
    mask = (rng.uniform(size=p.shape) < 0.8).astype(np.uint8)
    for alpha in (0.05, 0.2):
        for mk in (None, mask):
            thr, sig = LC.fdr_threshold(torch.from_numpy(p), alpha, None if mk is None else torch.from_numpy(mk))
            wt, ws = U.bh_numpy(p, alpha, mk)
            assert thr == wt and np.array_equal(sig.numpy(), ws) and 0 < ws.sum() < ws.size
    thr, sig = LC.fdr_threshold(torch.full((4, 4), 0.9, dtype=torch.float64), 0.05)
    assert thr == 0.0 and not sig.any()
    thr, sig = LC.fdr_threshold(torch.full((3,), float("nan")), 0.05)
    assert thr == 0.0 and not sig.any()
    with pytest.raises(LC.L.GandanetError):
        LC.fdr_threshold(torch.zeros(3), 1.5)
