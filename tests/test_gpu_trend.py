"""GPU: the trend module (gan_danet_amd/trend.py, csrc/trend.hip) against its host twin bit for bit on every column and
every map but p, and against the brute-force numpy oracle of tests/trend_util.py on the columns at both ends and around the
multiples of 64.  The device selects the order statistics by a radix select that stores no slope, the twin sorts the stored
slopes, the oracle is np.sort: three methods, one set of bits.  p is compared with math.erfc of the device's own z within
trend_util.P_RTOL.  Each test prints its largest p error over its bound (python -m pytest -s).

Measured on an MI355X: the device equalled the host twin bit for bit in every case; the largest relative error of p was
3.518e-16 (T = 12 and 13; |z| up to 25.8 at T = 300, where it was 1.342e-16), which is P_MEASURED of tests/trend_util.py: the
bound P_RTOL is four times that, 1.407e-15.  Where the exact p is subnormal or 0 (T = 2048, monotone) the check is absolute."""
import numpy as np
import pytest
import torch

import trend_util as U

pytestmark = pytest.mark.gpu

FILL = -7.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _off(a):
    """a copy of ``a`` on the device whose first element lies one element past a 16-byte boundary"""
    buf = torch.empty(a.size + 1, device="cuda", dtype=torch.from_numpy(a[:0].reshape(-1)).dtype)
    v = buf[1:].view(a.shape)
    v.copy_(_dev(a))
    assert v.data_ptr() % 16 == a.itemsize
    return v


def _run(x, t, period=0, flags=7, zq=0.0, mask=None, xd=None):
    """the (10, M) planes of the kernel itself, on a buffer filled with FILL"""
    from gan_danet_amd import kern as K
    out = torch.full((10, x.shape[1]), FILL, device="cuda", dtype=torch.float64)
    K.trend_test(_dev(x) if xd is None else xd, _dev(t), period, None if mask is None else _dev(mask), flags, zq, out)
    return out.cpu().numpy()


def _check(got, ref, flags, what):
    host, cols, want = ref
    U.assert_exact(got, host, flags, what)
    U.assert_exact(got[:, cols], want, flags, what)
    w, rel = U.p_error(got[4], got[3])
    assert w <= 1.0, (what, w, rel)
    return w, rel


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", (2, 3, 4, 5, 12, 13, 25, 63, 64, 65, 181))
def test_device_against_twin_and_oracle(T, dtype):
    """every kind of series (Gaussian with a trend, monotone up and down, all equal, integers 0 .. 3, two-valued, an
    outlier of 1e12), without gaps on uniform times and with NaN gaps (series left with 0, 1 and 2 samples) on non-uniform
    times"""
    worst = worst_rel = 0.0
    for gaps in (False, True):
        x = U.series(T, 65, dtype, gaps)
        t = U.times_of(T, uniform=not gaps)
        zq = U.zq_of(0.05)
        ref = U.reference(("plain", T, np.dtype(dtype).name, gaps), x, t, 0, 7, zq)
        w, rel = _check(_run(x, t, 0, 7, zq), ref, 7, (T, gaps))
        worst, worst_rel = max(worst, w), max(worst_rel, rel)
    print(f"T = {T} {np.dtype(dtype).name}: device == host twin on every column; p at most {worst:.3f} of its bound ({worst_rel:.3e} relative)")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_result_does_not_depend_on_m(dtype):
    """M on both sides of 64: the columns of a smaller cube are the first columns of the larger, bit for bit"""
    T = 25
    zq = U.zq_of(0.05)
    t = U.times_of(T)
    big = U.series(T, 257, dtype, gaps=True, seed=1)
    kept = {}
    for M in (257, 65, 64, 63, 2, 1):
        x = np.ascontiguousarray(big[:, :M])
        got = _run(x, t, 0, 7, zq)
        kept[M] = got
        _check(got, U.reference(("m", M, np.dtype(dtype).name), x, t, 0, 7, zq), 7, M)
        assert np.array_equal(got, kept[257][:, :M], equal_nan=True), M
    assert np.array_equal(kept[257][:, :65], kept[65], equal_nan=True)
    assert np.array_equal(_run(big, t, 0, 7, zq), kept[257], equal_nan=True)                    # two runs, the same bits
    assert np.array_equal(_run(big, t, 0, 7, zq, xd=_off(big)), kept[257], equal_nan=True)      # a view 16-byte misaligned


@pytest.mark.parametrize("T,M", [(300, 5), (2048, 3)])
def test_long_series(T, M):
    """T = 2048: 2 096 128 slopes per series, the 32-bit counts and every digit pass (column 1 is monotone, column 2 -- of
    integers 0 .. 3 -- has bins that never thin out to a single slope)"""
    for dtype in (np.float64, np.float32):
        x = U.series(T, 8, dtype)[:, [0, 2, 4, 6, 1][:M]]
        x = np.ascontiguousarray(x)
        t = U.times_of(T, uniform=dtype == np.float64)
        zq = U.zq_of(0.05)
        w, rel = _check(_run(x, t, 0, 7, zq), U.reference(("long", T, np.dtype(dtype).name), x, t, 0, 7, zq), 7, T)
        print(f"T = {T} {np.dtype(dtype).name}: device == host twin; p at most {w:.3f} of its bound ({rel:.3e} relative)")


@pytest.mark.parametrize("T", [13, 25, 181])
def test_seasonal(T):
    """period 12 with and without gaps; T = 13 leaves one season with a single pair and eleven with none"""
    worst = 0.0
    for gaps in (False, True):
        for dtype in (np.float64, np.float32):
            x = U.series(T, 65, dtype, gaps)
            t = U.times_of(T, uniform=not gaps)
            zq = U.zq_of(0.05)
            ref = U.reference(("seasonal", T, np.dtype(dtype).name, gaps), x, t, 12, 7, zq)
            worst = max(worst, _check(_run(x, t, 12, 7, zq), ref, 7, (T, gaps))[0])
    if T == 13:
        gone = U.series(T, 65)
        gone[12] = np.nan                                                     # no season keeps a pair: nt = 0
        none = _run(gone, U.times_of(T), 12, 7, U.zq_of(0.05))
        assert np.all(none[0] == 12) and np.all(none[1] == 0) and np.all(none[2] == 0) and np.isnan(none[3:]).all()
    print(f"T = {T}, period 12: device == host twin on every column; p at most {worst:.3f} of its bound")


@pytest.mark.parametrize("alpha", [0.05, 0.32, 0.95])
def test_flags_alpha_and_mask(alpha):
    """sen / ci on and off, with and without the continuity correction and the period; a run leaves the planes it was not
    asked for untouched; masked series have n = 0"""
    T, M = 64, 65
    x = U.series(T, M, gaps=True, seed=3)
    t = U.times_of(T, uniform=False)
    zq = U.zq_of(alpha)
    mask = np.ones(M, dtype=np.uint8)
    mask[[0, 31, M - 1]] = 0
    for flags in (0, U.CONT, U.SEN, U.SEN | U.CONT, U.SEN | U.CI, 7):
        for period in (0, 12):
            got = _run(x, t, period, flags, zq, mask)
            _check(got, U.reference(("flags", alpha, flags, period), x, t, period, flags, zq, mask), flags, (flags, period))
            assert np.all(got[0, [0, 31, M - 1]] == 0) and np.isnan(got[2:6, [0, 31, M - 1]]).all()
            untouched = [k for k in range(6, 10) if k not in U.planes_of(flags)]
            assert np.all(got[untouched] == FILL), (flags, untouched)


def test_public_interface():
    import gan_danet_amd as G
    from gan_danet_amd import _lib as L
    T = 25
    x = U.series(T, 24, np.float32, gaps=True)
    t = U.times_of(T, uniform=False)
    xd = _dev(x.reshape(T, 4, 6))
    mask = torch.ones(4, 6, dtype=torch.bool, device="cuda")
    mask[1, 2] = False
    flat = mask.reshape(-1).cpu().numpy().astype(np.uint8)
    for alpha in (0.05, 0.95):
        r = G.trend_test(xd, t, mask=mask, alpha=alpha)
        assert isinstance(r, G.TrendTest) and all(v.shape == (4, 6) and v.dtype == torch.float64 for v in r)
        want = _run(x, t, 0, 7, U.zq_of(alpha), flat)
        assert all(np.array_equal(v.cpu().numpy().reshape(-1), want[k], equal_nan=True) for k, v in enumerate(r))
    assert G.normal_quantile(0.025) == U.zq_of(0.05) and G.normal_quantile((1.0 - 0.95) / 2.0) == U.zq_of(0.95)
    r = G.trend_test(xd, period=12, continuity=False)                         # default times 0 .. T - 1
    want = _run(x, U.times_of(T), 12, U.SEN | U.CI, U.zq_of(0.05))
    assert all(np.array_equal(v.cpu().numpy().reshape(-1), want[k], equal_nan=True) for k, v in enumerate(r))
    mk = G.mann_kendall(xd, t)
    assert mk.slope is None and mk.intercept is None and mk.slope_lo is None and mk.slope_hi is None
    want = _run(x, t, 0, U.CONT)
    assert all(np.array_equal(mk[k].cpu().numpy().reshape(-1), want[k], equal_nan=True) for k in range(6))
    sl = G.sen_slope(xd, t, ci=False)
    assert sl.slope.shape == (4, 6) and sl.slope_lo is None and sl.slope_hi is None
    assert np.array_equal(sl.slope.cpu().numpy(), G.sen_slope(xd, t).slope.cpu().numpy(), equal_nan=True)
    one = G.trend_test(_dev(x[:, 0]))
    assert one.slope.shape == () and one.n.item() == np.count_nonzero(~np.isnan(x[:, 0]))
    for bad in (lambda: G.trend_test(xd, np.arange(T - 1.0)), lambda: G.trend_test(xd, t[::-1].copy()), lambda: G.trend_test(xd, period=1),
                lambda: G.trend_test(xd, period=T + 1), lambda: G.trend_test(xd, period=12.0), lambda: G.trend_test(xd, sen=False),
                lambda: G.trend_test(xd, alpha=0.0), lambda: G.trend_test(xd[:1]), lambda: G.trend_test(xd.int()),
                lambda: G.trend_test(xd, mask=mask[:3]), lambda: G.trend_test(torch.zeros(2049, 2, device="cuda"))):
        with pytest.raises(L.GandanetError):
            bad()
