"""CPU: the trend entry points of the C ABI (include/gandanet.h, "Per-pixel trend tests") are declared and bound, reject
every bad argument before any launch, and the host twin -- plain C++ over csrc/trend_core.h that sorts the stored slopes of
a series -- equals the brute-force numpy oracle of tests/trend_util.py bit for bit on every map but p, and scipy itself
(theilslopes, kendalltau) in the non-seasonal case.  Each test prints its largest p error over its bound
(python -m pytest -s)."""
import os

import numpy as np
import pytest
import torch

import trend_util as U

NAMES = ("gd_trend_test", "gd_trend_test_host")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_trend_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import build, kern, trend
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    assert "Per-pixel trend tests" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
    assert hasattr(kern, "trend_test") and hasattr(kern, "trend_test_host")
    assert f"#define GD_TREND_MAX_T {L.TREND_MAX_T}" in src and L.TREND_MAX_T == 2048
    for k, name in enumerate(L.TREND_MAPS):
        assert f"GD_TREND_{name.upper()} = {k}" in src
    assert f"GD_TREND_MAPS = {len(L.TREND_MAPS)}" in src and L.TREND_MAPS == U.MAPS
    assert f"GD_TREND_SEN = {L.TREND_SEN}, GD_TREND_CI = {L.TREND_CI}, GD_TREND_CONTINUITY = {L.TREND_CONTINUITY}" in src
    assert (L.TREND_SEN, L.TREND_CI, L.TREND_CONTINUITY) == (U.SEN, U.CI, U.CONT)
    assert "trend.hip" in build.SOURCES
    assert gan_danet_amd.trend is trend and trend.TrendTest._fields == U.MAPS
    for name in ("TrendTest", "trend_test", "mann_kendall", "sen_slope", "normal_quantile"):
        assert getattr(gan_danet_amd, name) is getattr(trend, name)


def test_trend_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses) are not
    touched"""
    L, lib = _lib()
    a, b, c = 0x1000, 0x2000, 0x3000
    order = ("x", "dtype", "T", "M", "times", "period", "mask", "flags", "zq", "out")
    good = dict(x=a, dtype=1, T=181, M=7, times=b, period=12, mask=None, flags=7, zq=-1.96, out=c)
    rules = [(dict(x=None), "null"), (dict(times=None), "null"), (dict(out=None), "null"), (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"),
             (dict(T=1), "T outside"), (dict(T=0), "T outside"), (dict(T=2049, period=0), "T outside"), (dict(M=0), "M <= 0"),
             (dict(M=-3), "M <= 0"), (dict(M=1 << 31), "too many"), (dict(period=1), "period"), (dict(period=182), "period"),
             (dict(period=-12), "period"), (dict(flags=8), "flag"), (dict(flags=-1), "flag"), (dict(flags=2), "needs the slope"),
             (dict(flags=6), "needs the slope"), (dict(zq=float("nan")), "zq"), (dict(zq=float("-inf")), "zq"), (dict(x=a + 4), "aligned"),
             (dict(x=a + 2, dtype=0), "aligned"), (dict(times=b + 4), "aligned"), (dict(out=c + 4), "aligned")]
    for host, fn in ((False, lib.gd_trend_test), (True, lib.gd_trend_test_host)):
        for kw, word in rules:
            v = dict(good, **kw)
            args = [v[k] for k in order]
            rc = fn(*args) if host else fn(*args, None)
            assert rc == -1, (fn.__name__, kw, rc)
            assert word in L.last_error(), (fn.__name__, kw, L.last_error())
    # the host twin looks at the times itself
    from gan_danet_amd import kern as K
    x = U.series(5, 3)
    for bad in ([0, 1, 1, 2, 3], [0, 1, 3, 2, 4], [0, 1, np.nan, 3, 4], [0, 1, 2, 3, np.inf]):
        with pytest.raises(L.GandanetError, match="times"):
            K.trend_test_host(x, bad)
    with pytest.raises(L.GandanetError):
        K.trend_test_host(x, np.arange(4.0))
    with pytest.raises(L.GandanetError):
        K.trend_test_host(x.astype(np.int32), np.arange(5.0))


TS = (2, 3, 4, 5, 12, 13, 25, 63, 64, 65, 181)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", TS)
def test_host_twin_against_the_oracle(T, dtype):
    """every kind of series, with and without NaN gaps, uniform and non-uniform times: equal on n, s, var_s, z, tau, slope,
    intercept, slope_lo, slope_hi; p within its bound of math.erfc of the twin's z"""
    worst = 0.0
    for gaps in (False, True):
        x = U.series(T, 65, dtype, gaps)
        t = U.times_of(T, uniform=not gaps)
        zq = U.zq_of(0.05)
        host, cols, want = U.reference(("plain", T, np.dtype(dtype).name, gaps), x, t, 0, 7, zq)
        U.assert_exact(host[:, cols], want, 7, (T, gaps))
        if gaps:
            assert list(host[0, 8:11]) == [0, min(1, T), min(2, T)] and np.isnan(host[2:, 8:10]).all() and np.all(host[1, 8:10] == 0)
        w, _ = U.p_error(host[4], host[3])
        worst = max(worst, w)
        assert w <= 1.0
        assert np.array_equal(np.isnan(host[3]), np.isnan(host[4]))
    print(f"T = {T} {np.dtype(dtype).name}: host twin == oracle on every compared map; p at most {worst:.3f} of its bound")


@pytest.mark.parametrize("T", [13, 25, 181])
def test_host_twin_seasonal(T):
    """period 12, with and without gaps: T = 13 leaves one season with a single pair and eleven with none"""
    for gaps in (False, True):
        for dtype in (np.float64, np.float32):
            x = U.series(T, 65, dtype, gaps)
            t = U.times_of(T, uniform=not gaps)
            zq = U.zq_of(0.05)
            host, cols, want = U.reference(("seasonal", T, np.dtype(dtype).name, gaps), x, t, 12, 7, zq)
            U.assert_exact(host[:, cols], want, 7, (T, gaps))
            assert U.p_error(host[4], host[3])[0] <= 1.0
    if T == 13:
        x = U.series(T, 65)
        host = U.reference(("seasonal", T, "float64", False), x, U.times_of(T), 12, 7, U.zq_of(0.05))[0]
        assert np.all(host[0] == 13) and np.all(np.abs(host[1]) <= 1)          # one pair: s is -1, 0 or 1
        assert host[6, 1] == (x[12, 1] - x[0, 1]) / 12.0 and host[8, 1] == host[6, 1] == host[9, 1]
        gone = x.copy()
        gone[12] = np.nan                                                       # no season keeps a pair: nt = 0
        from gan_danet_amd import kern as K
        none = K.trend_test_host(gone, U.times_of(T), 12, None, 7, U.zq_of(0.05))
        assert np.all(none[0] == 12) and np.all(none[1] == 0) and np.all(none[2] == 0) and np.isnan(none[3:]).all()


@pytest.mark.parametrize("alpha", [0.05, 0.32, 0.95])
def test_host_twin_flags_alpha_and_mask(alpha):
    from gan_danet_amd import kern as K
    from gan_danet_amd import trend
    T, M = 64, 65
    x = U.series(T, M, gaps=True, seed=3)
    t = U.times_of(T, uniform=False)
    zq = trend.normal_quantile((1.0 - alpha if alpha > 0.5 else alpha) / 2.0)
    assert zq == U.zq_of(alpha) and zq < 0
    mask = np.ones(M, dtype=np.uint8)
    mask[[0, 31, M - 1]] = 0
    cols = U.columns(M)
    for flags in (0, U.CONT, U.SEN, U.SEN | U.CONT, U.SEN | U.CI, 7):
        for period in (0, 12):
            got = K.trend_test_host(x, t, period, mask, flags, zq, out=np.full((10, M), -7.0))
            U.assert_exact(got[:, cols], U.oracle(x, t, cols, period, flags, zq, mask), flags, (flags, period))
            assert np.all(got[0, [0, 31, M - 1]] == 0) and np.isnan(got[2:6, [0, 31, M - 1]]).all()
            untouched = [k for k in range(6, 10) if k not in U.planes_of(flags)]
            assert np.all(got[untouched] == -7.0), (flags, untouched)          # planes that were not asked for stay as they were
    lo, hi = K.trend_test_host(x, t, 0, None, 7, zq)[[8, 9]]
    ok = ~np.isnan(lo)
    assert np.all(lo[ok] <= hi[ok])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_twin_against_scipy(dtype):
    """non-seasonal: slope, intercept, low and high equal scipy.stats.theilslopes(y, t, 1 - alpha) and tau equals
    scipy.stats.kendalltau(t, y) bit for bit; without the continuity correction p matches kendalltau's asymptotic p"""
    from scipy import stats
    from gan_danet_amd import kern as K
    worst = 0.0
    for T, gaps, alpha in ((181, False, 0.05), (64, True, 0.32), (25, False, 0.95), (5, False, 0.05), (2, False, 0.05)):
        x = U.series(T, 16, dtype, gaps)
        t = U.times_of(T, uniform=not gaps)
        got = K.trend_test_host(x, t, 0, None, U.SEN | U.CI, U.zq_of(alpha))
        U.oracle(x, t, range(16), 0, U.SEN | U.CI, U.zq_of(alpha))              # the oracle's check of the ranks' distance to a tie
        for m in range(16):
            ok = ~np.isnan(x[:, m])
            y, tt = x[ok, m].astype(np.float64), t[ok]
            if y.size < 2:
                continue
            ref = stats.theilslopes(y, tt, 1.0 - alpha)
            assert np.array_equal(got[6:10, m], [ref.slope, ref.intercept, ref.low_slope, ref.high_slope]), (T, m)
            kt = stats.kendalltau(tt, y, method="asymptotic" if y.size > 2 else "auto")      # its variance divides by n - 2
            assert np.array_equal(got[5, m], kt.statistic, equal_nan=True), (T, m, got[5, m], kt.statistic)
            if y.size > 2 and kt.pvalue == kt.pvalue and kt.pvalue >= U.P_TINY:
                # kendalltau forms the variance by another expression ((m (2 n + 5) - y1) / 18 against (1 / 18) K), so its
                # z may differ from ours by 2 ulp, which erfc magnifies by d ln erfc(x) / d ln x <= 1 + 2 x^2 = 1 + z^2
                tol = U.P_RTOL + 2 * 2.0 ** -52 * (1.0 + got[3, m] ** 2)
                rel = abs(got[4, m] - kt.pvalue) / kt.pvalue
                worst = max(worst, rel / tol)
                assert rel <= tol, (T, m, got[4, m], kt.pvalue)
    print(f"{np.dtype(dtype).name}: theilslopes and tau equal bit for bit; p at most {worst:.3f} of its bound from kendalltau's")


def test_cpu_and_bad_arguments_are_refused():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import trend
    x = torch.zeros(24, 4, 6, dtype=torch.float64)
    for call in (lambda: trend.trend_test(x), lambda: trend.mann_kendall(x), lambda: trend.sen_slope(x), lambda: trend.trend_test(x.numpy()),
                 lambda: trend.normal_quantile(0.0), lambda: trend.normal_quantile(1.0)):
        with pytest.raises(L.GandanetError):
            call()
    assert trend.normal_quantile(0.5) == 0.0 and abs(trend.normal_quantile(0.025) + 1.959963984540054) < 1e-12
