"""GPU: the EOF module (gan_danet_amd/eof.py, csrc/eof.hip) against the longdouble oracle of tests/eof_util.py.

gd_eof_gram (v_mfma_f64_16x16x4_f64): exact on integer data, within the entrywise bound B on random data, bitwise
symmetric, the same bits on two runs, nothing written outside G and the workspace, nothing added by invalid series.
prepare, project and reconstruct: nothing written outside their outputs, bit for bit their host twins (held to the oracle on the CPU by tests/test_cabi_eof.py)
and within their gamma bounds.  eof_analysis: eigenvalues within ||B||_F plus the residual of numpy's eigh on the same
matrix (Weyl), PCs within the Davis-Kahan angle and EOFs within that angle plus the rounding of the projection, against
numpy.linalg.svd; the full-rank reconstruction within the entrywise bound of eof_util.full_rank_bound.  Each test prints its largest error over its
bound (python -m pytest -s)."""
import numpy as np
import pytest
import torch

import eof_util as U

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _off(a):
    """a copy of ``a`` on the device whose first element lies one element past a 16-byte boundary"""
    buf = torch.empty(a.size + 1, device="cuda", dtype=torch.from_numpy(a[:0].reshape(-1)).dtype)
    v = buf[1:].view(a.shape)
    v.copy_(_dev(a))
    assert v.data_ptr() % 16 == a.itemsize
    return v


def _gram(x, mean, valid, w=None, off=False):
    """G of the device with sentinels around G and the workspace; asserts that they are untouched"""
    from gan_danet_amd import kern as K
    T, M = x.shape
    nbytes = K.eof_gram_ws_bytes(T, M)
    assert nbytes == U.geom(T, M)[1] * U.geom(T, M)[2] * 2048
    gbuf = torch.full((T * T + 64,), SENTINEL, device="cuda", dtype=torch.float64)
    wbuf = torch.full((nbytes // 8 + 64,), SENTINEL, device="cuda", dtype=torch.float64)
    ws = wbuf[32:32 + nbytes // 8].view(torch.uint8)
    K.eof_gram(_off(x) if off else _dev(x), _dev(mean), _dev(valid), _dev(w), out=gbuf[32:32 + T * T], ws=ws)
    g, wv = gbuf.cpu().numpy(), wbuf.cpu().numpy()
    assert np.all(g[:32] == SENTINEL) and np.all(g[32 + T * T:] == SENTINEL), "written outside G"
    assert np.all(wv[:32] == SENTINEL) and np.all(wv[32 + nbytes // 8:] == SENTINEL), "written outside the workspace"
    assert not np.any(g[32:32 + T * T] == SENTINEL), "an entry of G was not written"
    return g[32:32 + T * T].reshape(T, T).copy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", U.GRAM_TS)
def test_gram_random(T, dtype):
    from gan_danet_amd import kern as K
    worst = 0.0
    for M in U.GRAM_MS:
        x = U.cube(T, M, dtype)
        w = U.pow4_weights(M) if M < 31 else U.coslat_weights(M)
        for wt in (None, w):
            mean, valid = K.eof_prepare_host(x, None, wt)
            G = _gram(x, mean, valid, wt)
            worst = max(worst, U.check_gram(G, U.anomalies(x, mean, valid, wt), int(valid.sum()), f"T={T} M={M}"))
            assert np.array_equal(_gram(x, mean, valid, wt), G), (T, M)                # the same input again: the same bits
            assert np.array_equal(_gram(x, mean, valid, wt, off=True), G), (T, M)      # x one element past a 16-byte boundary
    print(f"gram T = {T} {np.dtype(dtype).name}: at most {worst:.3f} of B; symmetric, repeatable, sentinels untouched")


@pytest.mark.parametrize("T", U.GRAM_TS)
def test_gram_exact_integers(T):
    """any error in the fragment layout, the C/D map or the ownership of a block changes an integer"""
    from gan_danet_amd import kern as K
    for M in U.GRAM_MS:
        for centred in (False, True):
            xi = U.int_cube(T, M, centred)
            for dtype in (np.float64, np.float32):
                x = xi.astype(dtype)
                mean, valid = (t.cpu().numpy() for t in K.eof_prepare(_dev(x), center=centred))
                assert np.all(mean == 0) and np.all(valid == 1)
                assert np.array_equal(_gram(x, mean, valid), (xi @ xi.T).astype(np.float64)), (T, M, centred, dtype)


def _messy(T, M, dtype):
    x = U.cube(T, M, dtype)
    mask = np.ones(M, dtype=np.uint8)
    w = U.coslat_weights(M)
    x[T // 2, 1] = np.nan
    x[0, 2] = np.inf
    x[T - 1, 33] = -np.inf
    mask[[4, M - 1]] = 0
    w[5] = 0.0
    w[40] = np.nan
    return x, mask, w


@pytest.mark.parametrize("T", (2, 181, 256))
def test_gram_invalid_series(T):
    from gan_danet_amd import kern as K
    M = 300
    x, mask, w = _messy(T, M, np.float64)
    mean, valid = K.eof_prepare_host(x, mask, w)
    assert valid.sum() == M - 7
    keep = valid.astype(bool)
    G = _gram(x, mean, valid, w)
    ratio = U.check_gram(G, U.anomalies(x[:, keep], mean[keep], valid[keep], w[keep]), int(keep.sum()), f"T={T} reduced")
    x[:, ~keep] = np.nan                                   # whatever an invalid series holds
    assert np.array_equal(_gram(x, mean, valid, w), G)
    assert np.all(_gram(x, mean, np.zeros(M, np.uint8), w) == 0)
    print(f"gram T = {T}: invalid series add nothing ({ratio:.3f} of B on the reduced matrix); all invalid gives exactly 0")


def test_gram_refuses_t_outside_2_to_256():
    from gan_danet_amd import kern as K
    from gan_danet_amd._lib import GandanetError
    for T in (1, 257):
        x = _dev(U.cube(T, 5))
        with pytest.raises(GandanetError, match="T outside"):
            K.eof_gram(x, _dev(np.zeros(5)), _dev(np.ones(5, np.uint8)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_prepare_project_reconstruct_equal_their_twins(dtype):
    from gan_danet_amd import eof as E
    from gan_danet_amd import kern as K
    rng = np.random.default_rng(11)
    worst_p = worst_r = 0.0
    for T, M, kk in ((2, 1, 1), (17, 257, 4), (181, 300, 16), (33, 65, 17)):
        x, mask, w = (U.cube(T, M, dtype), None, None) if M < 50 else _messy(T, M, dtype)
        xd = _off(x)
        for mk, wt, center in ((mask, w, True), (None, None, True), (mask, None, False)):
            mbuf = torch.full((M + 16,), SENTINEL, device="cuda", dtype=torch.float64)
            vbuf = torch.full((M + 32,), 0xA5, device="cuda", dtype=torch.uint8)
            K.eof_prepare(xd, _dev(mk), _dev(wt), center, mean=mbuf[8:8 + M], valid=vbuf[16:16 + M])
            mb, vb = mbuf.cpu().numpy(), vbuf.cpu().numpy()
            assert np.all(mb[:8] == SENTINEL) and np.all(mb[8 + M:] == SENTINEL), "written outside mean"
            assert np.all(vb[:16] == 0xA5) and np.all(vb[16 + M:] == 0xA5), "written outside valid"
            mean, valid = K.eof_prepare_host(x, mk, wt, center)
            assert np.array_equal(mb[8:8 + M], mean) and np.array_equal(vb[16:16 + M], valid), (T, M)
        mean, valid = K.eof_prepare_host(x, mask, w)
        ok = valid.astype(bool)
        coef = rng.standard_normal((T, kk))
        for wt, use in ((w, w is not None), (w, False)):
            buf = torch.full((kk * M + 16,), SENTINEL, device="cuda", dtype=torch.float64)
            if kk <= 16:
                K.eof_project(xd, _dev(mean), _dev(valid), _dev(coef), _dev(wt), use, out=buf[8:8 + kk * M].view(kk, M))
                b = buf.cpu().numpy()
                assert np.all(b[:8] == SENTINEL) and np.all(b[8 + kk * M:] == SENTINEL)
                got = b[8:8 + kk * M].reshape(kk, M)
            else:                                          # 17 columns: the module's chunks of 16 and 1
                got = E._project(xd, _dev(mean), _dev(valid), coef, _dev(wt), use).cpu().numpy()
            host = np.concatenate([K.eof_project_host(x, mean, valid, coef[:, k:k + 16], wt, use) for k in range(0, kk, 16)])
            assert np.array_equal(got, host, equal_nan=True), (T, M, kk, use)
            want, bound = U.project_oracle(x, mean, valid, coef, wt if use else None)
            assert np.isnan(got[:, ~ok]).all() and np.all(np.abs(got - want)[:, ok] <= bound[:, ok])
            worst_p = max(worst_p, float((np.abs(got - want)[:, ok] / np.maximum(bound[:, ok], 1e-300)).max()))
        kr = min(kk, 16)
        eofs, pcs = rng.standard_normal((kr, M)), rng.standard_normal((T, kr))
        for wt in (w, None):
            for od, td in ((np.float64, torch.float64), (np.float32, torch.float32)):
                rbuf = torch.full((T * M + 16,), SENTINEL, device="cuda", dtype=td)
                K.eof_reconstruct(_dev(eofs), _dev(pcs), _dev(mean), _dev(valid), _dev(wt), td, out=rbuf[8:8 + T * M].view(T, M))
                rb = rbuf.cpu().numpy()
                assert np.all(rb[:8] == SENTINEL) and np.all(rb[8 + T * M:] == SENTINEL), "written outside the reconstruction"
                got = rb[8:8 + T * M].reshape(T, M)
                assert np.array_equal(got, K.eof_reconstruct_host(eofs, pcs, mean, valid, wt, od), equal_nan=True), (T, M, kr)
                want, bound = U.reconstruct_oracle(eofs, pcs, mean, valid, wt, od)
                assert np.isnan(got[:, ~ok]).all() and np.all(np.abs(got - want)[:, ok] <= bound[:, ok])
                worst_r = max(worst_r, float((np.abs(got - want)[:, ok] / np.maximum(bound[:, ok], 1e-300)).max()))
    print(f"{np.dtype(dtype).name}: device == host twin bit for bit; project at most {worst_p:.3f} of its bound, reconstruct {worst_r:.3f}")


def _check_against_svd(res, x, w, mask=None, what=""):
    """eigenvalues (Weyl) and modes (Davis-Kahan) of an EOFResult against numpy.linalg.svd of the oracle's anomalies"""
    T = x.shape[0]
    x2 = x.reshape(T, -1)
    mean, valid = res.mean.cpu().numpy().reshape(-1), res.valid.cpu().numpy().reshape(-1)
    assert np.array_equal(valid, U.valid_oracle(x2, mask, w)) and res.n_valid == valid.sum()
    a = U.anomalies(x2, mean, valid, w)
    lam, u, v = U.svd_modes(a)
    bf = float(np.linalg.norm(U.gram_bound(a, int(valid.sum()))))           # ||G^ - G||_2 <= ||B||_F
    lam_np, u_np = np.linalg.eigh(res.gram)                                 # the reference tool on the same matrix
    resid = np.linalg.norm(res.gram @ u_np - u_np * lam_np, axis=0)[::-1]
    K = res.n_modes
    dof = T - 1
    got_lam = res.eigenvalues.cpu().numpy() * dof
    pcs, eofs = res.pcs.cpu().numpy(), res.eofs.cpu().numpy().reshape(K, -1)
    worst = 0.0
    for k in range(K):
        tol = bf + resid[k]
        assert abs(got_lam[k] - lam[k]) <= tol, (what, k, got_lam[k], lam[k], tol)
        worst = max(worst, abs(got_lam[k] - lam[k]) / tol)
        others = np.delete(lam[:T], k)
        gap = float(np.min(np.abs(others - lam[k])))
        dk = 2.0 * tol / gap
        assert pcs[:, k] @ u[:, k] > 0, (what, k, "sign")
        s = U.sin_angle(pcs[:, k], u[:, k])
        assert s <= dk, (what, k, s, dk)
        assert abs(np.linalg.norm(pcs[:, k]) - np.sqrt(lam[k])) <= tol / np.sqrt(lam[k]) + 4 * U.U * np.sqrt(lam[k])
        # the pattern a^T u^ / sqrt(lambda^): the same Davis-Kahan angle, plus the rounding of the projection
        # (project_oracle's gamma(T + 3) on |u_k|^T |a| / sigma_k, the norm of a unit pattern's error)
        c = np.abs(u[:, k:k + 1]) / np.sqrt(lam[k])
        proj = U.gamma(T + 3) * float(np.linalg.norm(c.T @ np.abs(a).astype(np.float64)))
        e = np.where(valid, eofs[k], 0.0)
        se = U.sin_angle(e, v[k])
        assert np.isnan(eofs[k][~valid]).all() and e @ v[k] > 0 and se <= dk + proj, (what, k, se, dk, proj)
        # |e|^2 = u^^T G u^ / lambda^: G^ for G costs ||B||_F, u^ for an eigenvector the residual
        assert abs(np.linalg.norm(e) - 1.0) <= tol / lam[k] + proj + 4 * U.U, (what, k)
        worst = max(worst, s / dk, se / (dk + proj))
    return worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_eof_analysis_low_rank(dtype):
    from gan_danet_amd import eof as E
    T, shape = 12, (20, 30)
    x = U.low_rank_cube(T, shape, (40.0, 15.0, 6.0), noise=1e-3, dtype=dtype)
    lat = np.linspace(-59.5, 59.5, shape[0])
    w = np.repeat(np.cos(np.deg2rad(lat))[:, None], shape[1], axis=1).reshape(-1)
    res = E.eof_analysis(_dev(x), n_modes=3, lat=lat)
    worst = _check_against_svd(res, x, w, what="lat")
    explicit = E.eof_analysis(_dev(x), n_modes=3, weights=_dev(w.reshape(shape)))
    assert torch.equal(res.eofs, explicit.eofs) and torch.equal(res.pcs, explicit.pcs)              # lat= equals explicit weights
    assert float(res.variance_fraction.sum()) > 0.999 and res.eofs.shape == (3,) + shape and res.pcs.shape == (T, 3)
    assert torch.allclose(res.north_error, res.eigenvalues * np.sqrt(2.0 / T), rtol=1e-15)
    assert np.allclose(res.pattern_correlation(explicit).cpu().numpy(), 1.0, atol=1e-12)
    # covariance maps: eof sqrt(eigenvalue) / sqrt(w)
    cov = res.eofs_as_covariance().cpu().numpy().reshape(3, -1)
    want = res.eofs.cpu().numpy().reshape(3, -1) * np.sqrt(res.eigenvalues.cpu().numpy())[:, None] / np.sqrt(w)[None, :]
    assert np.allclose(cov, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    # all T modes: the fractions sum to 1 and the reconstruction returns the cube
    full = E.eof_analysis(_dev(x), n_modes=T, weights=_dev(w.reshape(shape)))
    assert abs(float(full.variance_fraction.sum()) - 1.0) <= T * T * U.U * 4
    assert abs(full.total_variance - float(np.trace(full.gram)) / (T - 1)) <= 1e-15 * full.total_variance
    rec = full.reconstruct(dtype=torch.float64).cpu().numpy().reshape(T, -1)
    x2 = np.ascontiguousarray(x.reshape(T, -1))
    mean, valid = full.mean.cpu().numpy().reshape(-1), full.valid.cpu().numpy().reshape(-1)
    tol = U.full_rank_bound(x2, mean, valid, w, full.gram)                      # derived there, entrywise
    ratio = float((np.abs(rec - x2.astype(np.float64))[:, valid] / tol).max())
    err, tol = float(np.abs(rec - x2.astype(np.float64)).max()), float(tol.max())
    assert ratio <= 1.0, ratio
    assert full.reconstruct().dtype == _dev(x).dtype and full.reconstruct(2).shape == (T,) + shape
    print(f"eof_analysis {np.dtype(dtype).name}: eigenvalues, PC and EOF angles at most {worst:.3f} of their bounds; full-rank "
          f"reconstruction at most {ratio:.3f} of its entrywise bound (largest error {err:.2e}, largest bound {tol:.2e})")


def test_eof_analysis_gaps_masks_and_errors():
    from gan_danet_amd import eof as E
    from gan_danet_amd._lib import GandanetError
    T, shape = 12, (9, 31)
    x = U.low_rank_cube(T, shape, (30.0, 10.0), noise=1e-3, seed=3)
    base = E.eof_analysis(_dev(x), n_modes=2)
    worst = _check_against_svd(base, x, None, what="plain")
    # two months missing altogether: NaN rows in the PCs, the same modes
    gappy = np.insert(x, [3, 7], np.nan, axis=0)
    res = E.eof_analysis(_dev(gappy), n_modes=2)
    kept = np.ones(T + 2, bool)
    kept[[3, 8]] = False
    assert np.array_equal(res.kept_steps.cpu().numpy(), kept)
    pcs = res.pcs.cpu().numpy()
    assert np.isnan(pcs[~kept]).all() and np.array_equal(pcs[kept], base.pcs.cpu().numpy())
    assert torch.equal(res.eofs, base.eofs) and torch.equal(res.eigenvalues, base.eigenvalues)
    rec = res.reconstruct().cpu().numpy()
    assert rec.shape == gappy.shape and np.isnan(rec[~kept]).all() and np.array_equal(rec[kept], base.reconstruct().cpu().numpy())
    # a pixel with a gap at a kept step is left out whole; a mask leaves pixels out
    holed = x.copy()
    holed[5, 2, 7] = np.nan
    mask = np.ones(shape, bool)
    mask[0, :] = False
    res = E.eof_analysis(_dev(holed), n_modes=2, mask=_dev(mask))
    assert res.n_valid == x[0].size - shape[1] - 1 and not bool(res.valid[2, 7]) and torch.isnan(res.eofs[:, 2, 7]).all()
    worst = max(worst, _check_against_svd(res, holed, None, mask=mask.reshape(-1), what="mask"))
    assert float(res.pattern_correlation(base).min()) > 0.99
    with pytest.raises(GandanetError, match="no valid pixel"):
        E.eof_analysis(_dev(x), mask=_dev(np.zeros(shape, bool)), drop_empty_steps=False)
    with pytest.raises(GandanetError, match="at least 2"):
        E.eof_analysis(_dev(np.where(np.arange(T)[:, None, None] > 0, np.nan, x)))
    with pytest.raises(GandanetError, match="at most"):
        E.eof_analysis(_dev(np.zeros((257, 4))))
    with pytest.raises(GandanetError, match="GPU tensor"):
        E.eof_analysis(torch.zeros(4, 4))
    print(f"eof_analysis with gaps and masks: at most {worst:.3f} of the bounds")


@pytest.mark.parametrize("M", [255, 256])
def test_launcher_edges(M):
    """prepare, project and reconstruct with T = 5 at the series counts on either side of a whole 256-thread workgroup (1 and
    257 are in test_prepare_project_reconstruct_equal_their_twins): outputs in the middle of sentinel buffers, the
    sentinels intact, bit for bit the host twins"""
    from gan_danet_amd import kern as K
    T, kk = 5, 4
    x = U.cube(T, M, np.float32)
    x[::2, 3] = np.nan
    w = U.coslat_weights(M)
    rng = np.random.default_rng(M)
    mbuf = torch.full((M + 16,), SENTINEL, device="cuda", dtype=torch.float64)
    vbuf = torch.full((M + 32,), 0xA5, device="cuda", dtype=torch.uint8)
    K.eof_prepare(_dev(x), None, _dev(w), True, mean=mbuf[8:8 + M], valid=vbuf[16:16 + M])
    mb, vb = mbuf.cpu().numpy(), vbuf.cpu().numpy()
    assert np.all(mb[:8] == SENTINEL) and np.all(mb[8 + M:] == SENTINEL) and np.all(vb[:16] == 0xA5) and np.all(vb[16 + M:] == 0xA5)
    mean, valid = K.eof_prepare_host(x, None, w, True)
    assert np.array_equal(mb[8:8 + M], mean, equal_nan=True) and np.array_equal(vb[16:16 + M], valid)
    coef = rng.standard_normal((T, kk))
    buf = torch.full((kk * M + 16,), SENTINEL, device="cuda", dtype=torch.float64)
    K.eof_project(_dev(x), _dev(mean), _dev(valid), _dev(coef), _dev(w), True, out=buf[8:8 + kk * M].view(kk, M))
    b = buf.cpu().numpy()
    assert np.all(b[:8] == SENTINEL) and np.all(b[8 + kk * M:] == SENTINEL)
    assert np.array_equal(b[8:8 + kk * M].reshape(kk, M), K.eof_project_host(x, mean, valid, coef, w, True), equal_nan=True)
    eofs, pcs = rng.standard_normal((kk, M)), rng.standard_normal((T, kk))
    rbuf = torch.full((T * M + 16,), SENTINEL, device="cuda", dtype=torch.float32)
    K.eof_reconstruct(_dev(eofs), _dev(pcs), _dev(mean), _dev(valid), _dev(w), torch.float32, out=rbuf[8:8 + T * M].view(T, M))
    rb = rbuf.cpu().numpy()
    assert np.all(rb[:8] == SENTINEL) and np.all(rb[8 + T * M:] == SENTINEL)
    assert np.array_equal(rb[8:8 + T * M].reshape(T, M), K.eof_reconstruct_host(eofs, pcs, mean, valid, w, np.float32), equal_nan=True)
