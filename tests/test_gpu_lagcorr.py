"""GPU: the lagged-correlation kernels (csrc/lagcorr.hip) against their host twins bit for bit on the curve, the counts, the
best-lag planes and both kinds of autocorrelation, around the kernel's time-chunk length and at its limits; gd_corr_signif
against math.atanh / math.erfc within the bounds of tests/lagcorr_util.py; and the public module gan_danet_amd.lagcorr.
The twins themselves are held against an independent numpy oracle in test_cabi_lagcorr.py.

Measured on an MI355X: the device equalled the host twin bit for bit in every case; z was at most 0.160 of its bound (10 ulp),
p at most 0.143 of its bound (17 ulp); the file takes 3 s."""
import numpy as np
import pytest
import torch

import lagcorr_util as U

pytestmark = pytest.mark.gpu


def _K():
    from gan_danet_amd import kern
    return kern


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _np(t):
    return None if t is None else t.cpu().numpy()


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _same(got, want, what):
    for g, w in zip(got, want):
        assert (g is None) == (w is None), what
        if g is not None:
            assert _eq(_np(g), w), what


def _both(a, b, lo, hi, what, **kw):
    K = _K()
    mask = kw.pop("mask", None)
    got = K.lag_corr(_dev(a), _dev(b), lo, hi, mask=_dev(mask), **kw)
    _same(got, K.lag_corr_host(a, b, lo, hi, mask=mask, **kw), what)
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", U.TS)
def test_device_equals_twin(T, dtype):
    """the grid of shapes and lag ranges, NaN columns included, with and without a mask"""
    for M in U.MS_GPU:
        a, b = U.pair(T, M, dtype)
        for lo, hi in U.RANGES:
            _both(a, b, lo, hi, (T, M, lo, hi), mask=U.mask_for(M) if (M + hi) % 2 else None)


def test_around_the_chunk_length():
    K = _K()
    Tc = K.L.LAG_CHUNK
    assert Tc == 32
    rng = np.random.default_rng(3)
    for lo, hi in ((-3, 3), (-12, 12), (0, 5)):
        for T in (Tc - 1, Tc, Tc + 1, 2 * Tc + (hi - lo) + 1):
            a = rng.standard_normal((T, 65)) + 1.0
            b = rng.standard_normal((T, 65)) + 0.5 * a
            a[rng.choice(T, 3, replace=False), 2] = np.nan
            _both(a, b, lo, hi, (T, lo, hi), select="max")
            _both(a.astype(np.float32), b.astype(np.float32), lo, hi, (T, lo, hi, "f32"), select="min")


def test_longest_series_and_widest_range():
    rng = np.random.default_rng(4)
    a = rng.standard_normal((2048, 65)) + 3.0
    b = rng.standard_normal((2048, 65))
    b[40:] += a[:-40]
    b[100:900, 7] = np.nan
    got = _both(a, b, -64, 64, "T = 2048")
    assert np.all(_np(got[2])[0, :7] == 40)


@pytest.mark.parametrize("kind", ["standard", "pearson"])
def test_acf_equals_twin(kind):
    K = _K()
    for dtype in (np.float64, np.float32):
        for T, M in ((1, 1), (2, 63), (7, 65), (181, 257), (181, 1003), (33, 64)):
            _, x = U.pair(T, M, dtype)
            for Kmax in (0, 1, 12, 64):
                mask = U.mask_for(M) if Kmax == 12 else None
                _same(K.series_acf(_dev(x), Kmax, kind, _dev(mask)), K.series_acf_host(x, Kmax, kind, mask), (kind, T, M, Kmax))


def test_corr_signif():
    K = _K()
    rng = np.random.default_rng(6)
    M = 1003
    r = np.clip(rng.uniform(-1.05, 1.05, M), -1.0, 1.0)
    n = rng.integers(2, 200, M).astype(np.float64)
    r1a, r1b = rng.uniform(-0.95, 0.95, M), rng.uniform(-0.95, 0.95, M)
    r[:4] = [1.0, -1.0, 0.0, np.nan]
    n[:2], r1a[:2], r1b[:2] = 100.0, 0.3, 0.3
    n[4:8] = [3.0, 4.0, np.nan, 50.0]
    r1a[8:11] = [np.nan, 1.0, -1.0]
    r1b[9:11] = [1.0, 1.0]
    r[11], n[11], r1a[11], r1b[11] = 0.999999, 180.0, 0.0, 0.0                       # |z| about 96: p underflows towards 0
    for one in (False, True):
        ra = r1a[500:501] if one else r1a
        ne, z, p = (_np(v) for v in K.corr_signif(_dev(r), _dev(n), _dev(ra), _dev(r1b)))
        assert _eq(ne, U.neff_numpy(r, n, ra, r1b)), one                              # n_eff: the same bits as numpy
        assert np.isnan(z[3]) and np.isnan(z[6]) and (one or np.isnan(ne[8])) and np.isnan(z[4])
        wz, wp = U.check_signif(r, ne, z, p, one)
        print(f"corr_signif (r1a single: {one}): z at most {wz:.3f} of its bound, p at most {wp:.3f}")
    assert np.isinf(z[0]) and p[0] == 0.0 and p[1] == 0.0


def test_reruns_streams_and_inputs_untouched():
    K = _K()
    a, b = U.pair(181, 257)
    ad, bd = _dev(a), _dev(b)
    first = K.lag_corr(ad, bd, -12, 12)
    again = K.lag_corr(ad, bd, -12, 12)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = K.lag_corr(ad, bd, -12, 12)
    side.synchronize()
    for x, y, z in zip(first, again, other):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
        assert _eq(_np(x), _np(z))
    assert _eq(_np(ad), a) and _eq(_np(bd), b)
    idx = np.ascontiguousarray(a[:, 9])                                              # an index against every series
    _both(idx, b, -12, 12, "index")
    _both(a, b, -12, 12, "no curve", curve=False)
    _both(a, b, 0, 0, "curve only", best=False)


def test_public_interface():
    import gan_danet_amd as G
    from gan_danet_amd import _lib as L
    K = _K()
    T, H, W = 60, 5, 7                                                               # odd H W
    a, b = U.pair(T, H * W, np.float32)
    ad, bd = _dev(a.reshape(T, H, W)), _dev(b.reshape(T, H, W))
    mask = torch.ones(H, W, dtype=torch.bool, device="cuda")
    mask[2, 3] = False
    res = G.lag_correlation(ad, bd, 6, mask=mask, curve=True)
    flat = mask.reshape(-1).cpu().numpy().astype(np.uint8)
    wr, wn, wb = K.lag_corr_host(a, b, -6, 6, mask=flat)
    assert isinstance(res, G.LagCorrelation) and res.r.shape == (13, H, W) and res.n.dtype == torch.int32 and res.best_lag.shape == (H, W)
    assert _eq(_np(res.lags), np.arange(-6, 7)) and _eq(_np(res.r).reshape(13, -1), wr) and _eq(_np(res.n).reshape(13, -1), wn)
    assert all(_eq(_np(v).reshape(-1), wb[k]) for k, v in enumerate((res.best_lag, res.best_r, res.best_n, res.r0)))
    assert np.nanmax(np.abs(_np(res.best_lag))) <= 6 and np.isnan(_np(res.p)[2, 3]) and np.nanmedian(_np(res.best_lag)) == 3
    r1a, r1b = K.series_acf_host(a, 1, mask=flat)[0][1], K.series_acf_host(b, 1, mask=flat)[0][1]
    assert _eq(_np(res.n_eff).reshape(-1), U.neff_numpy(wb[1], wb[2], r1a, r1b))
    U.check_signif(wb[1], _np(res.n_eff).reshape(-1), _np(res.z).reshape(-1), _np(res.p).reshape(-1), "lag_correlation")
    plain = G.lag_correlation(ad, bd, lags=(0, 4), significance=False, select="max")
    assert plain.r is None and plain.p is None and _eq(_np(plain.best_lag).reshape(-1), K.lag_corr_host(a, b, 0, 4, select="max")[2][0])
    one = G.lag_correlation(ad[:, 1, 1].contiguous(), bd, 6)                          # an index (T,)
    assert _eq(_np(one.best_r).reshape(-1), K.lag_corr_host(np.ascontiguousarray(a[:, 8]), b, -6, 6)[2][1])
    acf, n = G.autocorrelation(bd, 5, mask=mask)
    wa, wn = K.series_acf_host(b, 5, "standard", flat)
    assert acf.shape == (6, H, W) and _eq(_np(acf).reshape(6, -1), wa) and _eq(_np(n).reshape(6, -1), wn)
    # driver_lags equals one call per channel
    aux = torch.stack([ad, bd, ad + bd], dim=1)
    lag, rr, pp = G.driver_lags(bd, aux, 4)
    for c in range(3):
        sep = G.lag_correlation(aux[:, c].contiguous(), bd, 4)
        assert torch.equal(torch.nan_to_num(lag[c], nan=-99.0), torch.nan_to_num(sep.best_lag, nan=-99.0))
        assert _eq(_np(rr[c]), _np(sep.best_r)) and _eq(_np(pp[c]), _np(sep.p))
    assert G.driver_lags(bd, aux, 4, channels=[2])[0].shape == (1, H, W)
    # skill_maps' cc and n get a p map; against the direct path at lag 0: skill_maps uses another recurrence, so within the
    # bound of r (kappa 1 at lag 0 up to the pairs' mean, doubled for two computed values) and the propagated bound of z
    sk = G.skill_maps(ad, bd, metrics=("cc", "n"))
    ne, z, p = G.correlation_significance(sk["cc"], sk["n"], ad, bd)
    zero = G.lag_correlation(ad, bd, 0)
    assert _eq(_np(sk["n"]), _np(zero.best_n))
    err = np.abs(_np(sk["cc"]) - _np(zero.r0))
    fin = ~np.isnan(_np(zero.r0))
    assert np.array_equal(np.isnan(_np(sk["cc"])), ~fin) and np.all(err[fin] <= 2.0 * U.r_bound(T, 2.0))
    assert _eq(_np(ne), _np(zero.n_eff)) and p.shape == (H, W)
    r1x, r1y = K.series_acf_host(a, 1)[0][1], K.series_acf_host(b, 1)[0][1]           # ready r1 maps: the same inputs, the same bits
    ne2, z2, p2 = G.correlation_significance(zero.r0, zero.best_n, r1x=_dev(r1x.reshape(H, W)), r1y=_dev(r1y.reshape(H, W)))
    assert _eq(_np(ne2), _np(zero.n_eff)) and _eq(_np(z2), _np(zero.z)) and _eq(_np(p2), _np(zero.p))
    for bad in (lambda: G.lag_correlation(ad.cpu(), bd.cpu()), lambda: G.autocorrelation(bd.cpu()), lambda: G.lag_correlation(ad, bd, 65),
                lambda: G.lag_correlation(ad, bd, lags=(3, 1)), lambda: G.lag_correlation(ad, bd, min_pairs=1),
                lambda: G.lag_correlation(ad[:10], bd), lambda: G.lag_correlation(ad.double(), bd), lambda: G.lag_correlation(ad, bd, select="x"),
                lambda: G.lag_correlation(ad, bd, mask=mask[:2]), lambda: G.correlation_significance(sk["cc"].cpu(), sk["n"].cpu(), ad, bd),
                lambda: G.correlation_significance(sk["cc"], sk["n"], ad), lambda: G.driver_lags(bd, ad, 4),
                lambda: K.corr_signif(sk["cc"].cpu().reshape(-1), sk["n"].reshape(-1), sk["n"].reshape(-1), sk["n"].reshape(-1)),
                lambda: K.lag_corr(ad.cpu().reshape(T, -1), bd.cpu().reshape(T, -1), 0, 1)):
        with pytest.raises(L.GandanetError):
            bad()
