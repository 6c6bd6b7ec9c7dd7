"""GPU: the triple-collocation kernels (csrc/tcol.hip) against their host twins bit for bit -- stats, cov, n and flags of the point
estimate; summary, n_ok and replicates of the bootstrap -- around the pixel-group size, the wave width in B and the limits of T
and B, with the full and with the smallest legal workspace, at two placements of one pixel; and the public module
gan_danet_amd.collocation.  The twins themselves are held against an independent long-double oracle in test_cabi_tcol.py.

Measured on an MI355X: the device equalled the host twin bit for bit in every case; the file takes 4 s."""
import numpy as np
import pytest
import torch

import tcol_util as U

pytestmark = pytest.mark.gpu

Q3 = (0.025, 0.5, 0.975)
Q8 = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 0.99, 1.0)


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


def _boot(x, y, z, idx, q, what, mask=None, ws=None, min_samples=10):
    K = _K()
    got = K.tc_bootstrap(_dev(x), _dev(y), _dev(z), _dev(idx), q, min_samples, _dev(mask), True, ws)
    _same(got, K.tc_bootstrap_host(x, y, z, idx, q, min_samples, mask, True), what)
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", U.TS_EST)
def test_estimate_equals_twin(T, dtype):
    K = _K()
    for M in U.MS_EST:
        x, y, z = U.triple(T, M, dtype)
        for mask in (None, U.mask_for(M)):
            got = K.tc_estimate(_dev(x), _dev(y), _dev(z), 10, _dev(mask))
            _same(got, K.tc_estimate_host(x, y, z, 10, mask), (T, M, mask is not None))
    x, y, z = U.triple(T, 65, dtype)
    assert K.tc_estimate(_dev(x), _dev(y), _dev(z), 3, cov=False)[1] is None


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", (3, 24, 181))
def test_bootstrap_shapes(T, dtype):
    """M around the pixel group of 8, with and without a mask; min_samples 3 so that T = 3 computes"""
    for M in (1, 7, 8, 9, 65):
        x, y, z = U.triple(T, M, dtype)
        idx = U.indices(T, 65, 3, seed=M)
        _boot(x, y, z, idx, Q3, (T, M), mask=U.mask_for(M) if M == 65 else None, min_samples=3 if T == 3 else 10)


@pytest.mark.parametrize("B", (1, 2, 63, 64, 65, 257))
def test_bootstrap_replicate_counts(B):
    x, y, z = U.triple(24, 9)
    _boot(x, y, z, U.indices(24, B, 3, seed=B), Q3, B)
    xf, yf, zf = U.triple(24, 9, np.float32)
    _boot(xf, yf, zf, U.indices(24, B, 1, seed=B), (0.5,), (B, "f32"))


def test_bootstrap_at_the_limits():
    """T = 2048 (one pixel per workgroup, 48 KB of LDS) with B = 2048 (the widest sort) at M = 3"""
    rng = np.random.default_rng(9)
    t = rng.standard_normal((2048, 3))
    x, y, z = 1.0 + t + 0.3 * rng.standard_normal(t.shape), 0.8 * t + 0.4 * rng.standard_normal(t.shape), 1.3 * t + 0.5 * rng.standard_normal(t.shape)
    y[100:140, 1] = np.nan
    from gan_danet_amd.collocation import bootstrap_indices
    _boot(x, y, z, bootstrap_indices(2048, 2048, 12, seed=1), Q3, "limits")


@pytest.mark.parametrize("T", (340, 341, 681, 682, 1364, 1365))
def test_bootstrap_group_thresholds(T):
    """the group of pixels per workgroup halves at T = 341, 682 and 1365 (3 T G + 3 G doubles in 64 KB)"""
    K = _K()
    assert K.lib().gd_tc_group(T) == {340: 8, 341: 4, 681: 4, 682: 2, 1364: 2, 1365: 1}[T]
    rng = np.random.default_rng(T)
    t = rng.standard_normal((T, 9))
    x, y, z = t + 0.3 * rng.standard_normal(t.shape), 0.8 * t + 0.4 * rng.standard_normal(t.shape), 1.3 * t + 0.5 * rng.standard_normal(t.shape)
    x[5, 2] = np.nan
    _boot(x, y, z, U.indices(T, 33, 6, seed=T), (0.5,), T)


def test_bootstrap_quantile_counts():
    x, y, z = U.triple(24, 9)
    idx = U.indices(24, 100, 3)
    _boot(x, y, z, idx, (0.5,), "Q = 1")
    _boot(x, y, z, idx, Q8, "Q = 8")


def test_workspace_independence():
    K = _K()
    x, y, z = U.triple(24, 65)
    idx = U.indices(24, 65, 3)
    full = _boot(x, y, z, idx, Q3, "full workspace")
    need = K.tc_bootstrap_min_workspace(24, 65)
    small = _boot(x, y, z, idx, Q3, "smallest workspace", ws=torch.empty(need, dtype=torch.uint8, device="cuda"))
    odd = _boot(x, y, z, idx, Q3, "three groups", ws=torch.empty(3 * (need - 8) + 8 + 5, dtype=torch.uint8, device="cuda"))
    for a, b, c in zip(full, small, odd):
        assert _eq(_np(a), _np(b)) and _eq(_np(a), _np(c))
    with pytest.raises(K.L.GandanetError, match="bytes needed"):
        K.tc_bootstrap(_dev(x), _dev(y), _dev(z), _dev(idx), Q3, 10, ws=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    bad = idx.copy()
    bad[7, 3] = 24
    with pytest.raises(K.L.GandanetError, match="index is >= T"):
        K.tc_bootstrap(_dev(x), _dev(y), _dev(z), _dev(bad), Q3, 10)


def test_placement_independence():
    """one pixel at column 3 of M = 9 and at column 70 of M = 131: equal bits"""
    K = _K()
    x, y, z = U.triple(24, 131)
    idx = U.indices(24, 65, 3)
    a = [np.ascontiguousarray(c[:, :9]) for c in (x, y, z)]
    b = [c.copy() for c in (x, y, z)]
    for ca, cb in zip(a, b):
        cb[:, 70] = ca[:, 3]
    ga = K.tc_bootstrap(*(_dev(c) for c in a), _dev(idx), Q3, 10, None, True)
    gb = K.tc_bootstrap(*(_dev(c) for c in b), _dev(idx), Q3, 10, None, True)
    for u, v in zip(ga, gb):
        assert _eq(_np(u)[..., 3], _np(v)[..., 70])
    ea, eb = K.tc_estimate(*(_dev(c) for c in a), 10), K.tc_estimate(*(_dev(c) for c in b), 10)
    for u, v in zip(ea, eb):
        assert _eq(_np(u)[..., 3], _np(v)[..., 70])


def test_public_module():
    import gan_danet_amd as G
    from gan_danet_amd import _lib as L
    K = _K()
    T, H, W = 24, 5, 13                                                              # odd H W, 65 pixels
    x, y, z = U.triple(T, H * W, np.float32)
    xd, yd, zd = (_dev(c.reshape(T, H, W)) for c in (x, y, z))
    mask = torch.ones(H, W, dtype=torch.bool, device="cuda")
    mask[2, 3] = False
    flat = mask.reshape(-1).cpu().numpy().astype(np.uint8)
    res = G.triple_collocation(xd, yd, zd, mask=mask, names=("grace", "product", "gldas"))
    st, cov, n, fl = K.tc_estimate_host(x, y, z, 10, flat)
    assert isinstance(res, G.TripleCollocation) and res.n.shape == (H, W) and res.n.dtype == torch.int32 and res.flags.dtype == torch.int32
    assert _eq(_np(res.stats).reshape(8, -1), st) and _eq(_np(res.n).reshape(-1), n) and _eq(_np(res.flags).reshape(-1), fl)
    for i, k in enumerate(res.names):
        assert _eq(_np(res.err_var[k]).reshape(-1), st[i]) and _eq(_np(res.rho2[k]).reshape(-1), st[3 + i])
        with np.errstate(invalid="ignore"):
            assert _eq(_np(res.err_std[k]).reshape(-1), np.where(st[i] >= 0, np.sqrt(np.abs(st[i])), np.nan))
            assert _eq(_np(res.rho[k]).reshape(-1), np.sqrt(st[3 + i]))
    assert _eq(_np(res.beta["product"]).reshape(-1), st[6]) and _eq(_np(res.beta["gldas"]).reshape(-1), st[7])
    valid = _np(res.valid).reshape(-1)
    assert np.array_equal(valid, ~np.isnan(st[6])) and not valid[[4, 5, 2 * W + 3]].any() and valid.sum() == H * W - 3
    assert np.all(_np(res.beta["grace"]).reshape(-1)[valid] == 1.0)
    assert _eq(_np(res.cov[("grace", "gldas")]).reshape(-1), cov[4]) and len(res.cov) == 6
    w = res.merge_weights()
    tot = _np(w["grace"] + w["product"] + w["gldas"]).reshape(-1)
    pos = valid & (st[:3] > 0).all(axis=0)
    assert pos.any() and np.all(np.abs(tot[pos] - 1.0) <= 4 * U.EPS) and np.isnan(tot[~pos]).all()
    snr = _np(res.snr_db()["grace"]).reshape(-1)
    inside = valid & (st[3] > 0) & (st[3] < 1)
    assert np.allclose(snr[inside], 10 * np.log10(st[3][inside] / (1 - st[3][inside])), rtol=1e-12) and np.isnan(snr[~inside]).all()
    # the bootstrap: the table of the recipe, the summaries of the twin, the interval, the replicates
    bs = G.triple_collocation_bootstrap(xd, yd, zd, B=65, block=3, seed=5, mask=mask, keep_replicates=True)
    idx = G.bootstrap_indices(T, 65, 3, seed=5)
    summ, nok, rep = K.tc_bootstrap_host(x, y, z, idx, Q3, 10, flat, True)
    assert isinstance(bs, G.TripleCollocationBootstrap) and np.array_equal(bs.indices, idx) and bs.q == Q3
    assert bs.replicates.shape == (65, 8, H, W) and _eq(_np(bs.replicates).reshape(65, 8, -1), rep)
    for i, k in enumerate(G.collocation.STATS):
        assert _eq(_np(bs.mean[k]).reshape(-1), summ[i, 0]) and _eq(_np(bs.std[k]).reshape(-1), summ[i, 1])
        assert _eq(_np(bs.quantiles[k]).reshape(3, -1), summ[i, 2:]) and _eq(_np(bs.n_ok[k]).reshape(-1), nok[i])
    lo, hi = bs.interval("err_var_x")
    assert _eq(_np(lo).reshape(-1), summ[0, 2]) and _eq(_np(hi).reshape(-1), summ[0, 4])
    assert np.all(_np(lo).reshape(-1)[valid] <= _np(hi).reshape(-1)[valid])
    assert _eq(_np(bs.estimate.stats), _np(res.stats))
    own = G.triple_collocation_bootstrap(xd, yd, zd, indices=_dev(idx), mask=mask, q=(0.5,))
    assert own.replicates is None and _eq(_np(own.quantiles["beta_y"])[0].reshape(-1), summ[6, 3])
    for bad in (lambda: G.triple_collocation(xd.cpu(), yd.cpu(), zd.cpu()), lambda: G.triple_collocation_bootstrap(xd.cpu(), yd.cpu(), zd.cpu()),
                lambda: G.triple_collocation(xd, yd[:10], zd), lambda: G.triple_collocation(xd, yd.double(), zd),
                lambda: G.triple_collocation(xd, yd, zd, min_samples=2), lambda: G.triple_collocation(xd, yd, zd, mask=mask[:2]),
                lambda: G.triple_collocation(xd, yd, zd, names=("a", "a", "b")), lambda: G.triple_collocation(xd[:, 0, 0], yd[:, 0, 0], zd[:, 0, 0]),
                lambda: G.triple_collocation_bootstrap(xd, yd, zd, B=4000), lambda: G.triple_collocation_bootstrap(xd, yd, zd, q=(2.0,)),
                lambda: G.triple_collocation_bootstrap(xd, yd, zd, indices=idx[:10]), lambda: bs.interval("nope"),
                lambda: K.tc_estimate(_dev(x).cpu(), _dev(y).cpu(), _dev(z).cpu(), 10)):
        with pytest.raises(L.GandanetError):
            bad()
