"""CPU: the host twins of the triple-collocation family (gd_tc_estimate_host, gd_tc_bootstrap_host; csrc/tcol_core.h) against the
independent long-double oracle of tests/tcol_util.py within the bounds recorded there, a closed form on exactly orthogonal
columns, the bootstrap summaries against numpy on the twin's own replicates (quantiles bit for bit), the exact properties of
the definitions (independence of M and of the column, the mask, the flags), the index recipe and the argument checks.  Each
bound test prints its largest error (python -m pytest -s)."""
import numpy as np
import pytest

import tcol_util as U

Q3 = (0.025, 0.5, 0.975)
BOOT_GRID = ((24, 3), (40, 4), (181, 6))                              # (T, block), B = 128, M = 65


def _K():
    from gan_danet_amd import kern
    return kern


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", U.TS_EST)
def test_estimate_twin_against_oracle(T, dtype):
    K = _K()
    worst = 0.0
    for M in U.MS_EST:
        x, y, z = U.triple(T, M, dtype)
        st, cov, n, fl = K.tc_estimate_host(x, y, z, 10)
        wst, wcov, wn = U.oracle(x, y, z, 10)
        assert np.array_equal(n, wn), (T, M)
        worst = max(worst, U.worst_error(st, wst, wcov, (T, M)))
        assert np.array_equal(np.isnan(cov), np.isnan(wcov)), (T, M)
        fin = ~np.isnan(wcov)
        if fin.any():                                                 # the covariances: Qaa-scaled, sqrt(Qaa Qbb) for the cross terms
            sc = np.sqrt(np.stack([wcov[0] * wcov[0], wcov[1] * wcov[1], wcov[2] * wcov[2], wcov[0] * wcov[1], wcov[0] * wcov[2],
                                   wcov[1] * wcov[2]]).astype(np.float64))
            ec = float((np.abs(cov.astype(U.LD) - wcov)[fin] / sc[fin]).max() / U.EPS)
            worst = max(worst, ec)
        assert np.array_equal(fl, U.flags_of(st, n, 10)), (T, M)
        if T >= 24 and M > 5:
            assert fl[4] == U.F_FEW and n[4] == 0 and fl[5] == U.F_NONPOS and np.isnan(st[:, 5]).all() and not np.isnan(cov[:, 5]).any()
            assert n[1] == T - 3 and n[0] == T - 3 and n[2] == T
        if T < 10:
            assert np.isnan(st).all() and np.all(fl == U.F_FEW)
    print(f"T = {T}, {np.dtype(dtype).name}: point estimates at most {worst:.2f} eps of their scales (bound {U.POINT_BOUND_EPS})")
    assert worst <= U.POINT_BOUND_EPS


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T,block", BOOT_GRID)
def test_bootstrap_twin_against_oracle(T, block, dtype):
    """every replicate of every pixel against the oracle on the resampled series, none skipped; the summaries against numpy on
    the twin's own replicates; at T = 24 the reference data alone exercise the undefined branch and the negative variances"""
    K = _K()
    x, y, z = U.triple(T, 65, dtype)
    idx = U.indices(T, 128, block)
    summary, n_ok, rep = K.tc_bootstrap_host(x, y, z, idx, Q3, 10, replicates=True)
    ost, ocov = U.oracle_replicates(x, y, z, idx, 10)
    worst = U.worst_error(rep.transpose(1, 0, 2), ost, ocov, (T, "replicates"))
    wm = U.check_summary(summary, n_ok, rep, Q3, T)
    valid = [c for c in range(65) if c not in (4, 5)]
    undefined = int(np.isnan(rep[:, 0, valid]).sum())
    negative = int((rep[:, :3, valid] < 0).any(axis=1).sum())
    print(f"T = {T}, {np.dtype(dtype).name}: replicates at most {worst:.1f} eps (bound {U.REPLICATE_BOUND_EPS}), moments at most {wm:.2f} eps "
          f"(bound {U.MOMENT_BOUND_EPS}); {undefined} undefined and {negative} with a negative variance of {128 * len(valid)}")
    assert worst <= U.REPLICATE_BOUND_EPS
    if T == 24:
        assert undefined > 0 and negative > 0
        assert (n_ok[:, valid] < 128).any() and (n_ok[:, valid] >= 2).all()
    assert not n_ok[:, 4].any() and not n_ok[:, 5].any() and np.isnan(summary[:, :, [4, 5]]).all()


def test_closed_form():
    """columns of a QR factor of [1, random(32, 4)]: an exactly orthogonal, zero-mean truth and three errors, so that
    err_var_x = s1^2 var(e1), rho2_x = b1^2 var(t) / Qxx and beta_y = b2 / b1 hold in real arithmetic"""
    K = _K()
    T, M = 32, 9
    rng = np.random.default_rng(7)
    worst = 0.0
    cubes = np.empty((3, T, M))
    want = np.empty((8, M))
    scale = np.empty((8, M))
    for m in range(M):
        qf, _ = np.linalg.qr(np.concatenate([np.ones((T, 1)), rng.standard_normal((T, 4))], axis=1))
        t, e = 3.0 * qf[:, 1], qf[:, 2:]
        b = np.array([1.0, 0.8, 1.3]) * (1.0 + 0.1 * m)
        s = np.array([0.9, 1.2, 1.5])
        off = np.array([5.0, -2.0, 0.0])
        for c in range(3):
            cubes[c, :, m] = off[c] + b[c] * t + s[c] * e[:, c]
        var_t, var_e = 9.0 / (T - 1), 1.0 / (T - 1)                   # the columns have unit norm and zero mean
        qaa = b * b * var_t + s * s * var_e
        want[0:3, m] = s * s * var_e
        want[3:6, m] = b * b * var_t / qaa
        want[6, m], want[7, m] = b[1] / b[0], b[2] / b[0]
        scale[0:3, m], scale[3:6, m], scale[6:8, m] = qaa, 1.0, want[6:8, m]
    st, cov, n, fl = K.tc_estimate_host(cubes[0], cubes[1], cubes[2], 3)
    assert np.all(n == T) and not fl.any()
    worst = float((np.abs(st - want) / scale).max() / U.EPS)
    print(f"closed form: at most {worst:.2f} eps of the scales (bound {U.CLOSED_BOUND_EPS})")
    assert worst <= U.CLOSED_BOUND_EPS


def test_bit_for_bit_properties():
    K = _K()
    for dtype in (np.float64, np.float32):
        x, y, z = U.triple(24, 65, dtype)
        idx = U.indices(24, 65, 3, seed=2)
        full = K.tc_estimate_host(x, y, z, 10)
        boot = K.tc_bootstrap_host(x, y, z, idx, Q3, 10, replicates=True)
        # a series' outputs do not change with its column or with M
        perm = np.random.default_rng(1).permutation(65)
        xp, yp, zp = (np.ascontiguousarray(a[:, perm]) for a in (x, y, z))
        for got, want in zip(K.tc_estimate_host(xp, yp, zp, 10), full):
            assert _eq(got, want[..., perm])
        for got, want in zip(K.tc_bootstrap_host(xp, yp, zp, idx, Q3, 10, replicates=True), boot):
            assert _eq(got, want[..., perm])
        for got, want in zip(K.tc_bootstrap_host(x[:, :9], y[:, :9], z[:, :9], idx, Q3, 10, replicates=True), boot):
            assert _eq(got, want[..., :9])
        # the identity table reproduces the point estimate in every replicate
        ident = np.repeat(np.arange(24, dtype=np.uint16)[:, None], 2, axis=1)
        _, nk, rep = K.tc_bootstrap_host(x, y, z, ident, (0.5,), 10, replicates=True)
        assert _eq(rep[0], full[0]) and _eq(rep[1], full[0])
        # the statistics do not depend on which cube comes second and third beyond their own relabelling
        sw = K.tc_estimate_host(x, z, y, 10)[0]
        assert _eq(sw[0], full[0][0]) and _eq(sw[[1, 2]], full[0][[2, 1]]) and _eq(sw[[6, 7]], full[0][[7, 6]])
        # cov asked for or not; replicates asked for or not
        assert K.tc_estimate_host(x, y, z, 10, cov=False)[1] is None
        s2, n2, r2 = K.tc_bootstrap_host(x, y, z, idx, Q3, 10)
        assert r2 is None and _eq(s2, boot[0]) and _eq(n2, boot[1])
        # Q = 1 and Q = 8: a quantile does not depend on its neighbours
        q8 = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 0.99, 1.0)
        s8 = K.tc_bootstrap_host(x, y, z, idx, q8, 10)[0]
        s1 = K.tc_bootstrap_host(x, y, z, idx, (0.5,), 10)[0]
        assert s8.shape == (8, 10, 65) and s1.shape == (8, 3, 65) and _eq(s8[:, 5], s1[:, 2]) and _eq(s8[:, :2], boot[0][:, :2])
        with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):                                  # pixels 4 and 5 are all NaN
            lo, hi = np.nanmin(boot[2], axis=0), np.nanmax(boot[2], axis=0)
        assert (boot[1] >= 2).sum() == (boot[1] > 0).sum() and _eq(s8[:, 2], lo) and _eq(s8[:, 9], hi)  # q = 0 and q = 1


def test_mask_bytes():
    K = _K()
    x, y, z = U.triple(24, 65)
    mask = U.mask_for(65)
    idx = U.indices(24, 16, 3)
    off = mask == 0
    st, cov, n, fl = K.tc_estimate_host(x, y, z, 10, mask)
    ref = K.tc_estimate_host(x, y, z, 10)
    assert np.isnan(st[:, off]).all() and np.isnan(cov[:, off]).all() and not n[off].any() and np.all(fl[off] == U.F_MASKED)
    for got, want in zip((st, cov, n, fl), ref):
        assert _eq(got[..., ~off], want[..., ~off])
    assert np.array_equal(fl, U.flags_of(st, n, 10, mask))
    s, nk, rep = K.tc_bootstrap_host(x, y, z, idx, Q3, 10, mask, replicates=True)
    sr, nr, rr = K.tc_bootstrap_host(x, y, z, idx, Q3, 10, replicates=True)
    assert np.isnan(s[..., off]).all() and not nk[:, off].any() and np.isnan(rep[..., off]).all()
    assert _eq(s[..., ~off], sr[..., ~off]) and _eq(nk[:, ~off], nr[:, ~off]) and _eq(rep[..., ~off], rr[..., ~off])
    with pytest.raises(K.L.GandanetError):
        K.tc_estimate_host(x, y, z, 10, np.ones(64, dtype=np.uint8))


def test_index_recipe():
    from gan_danet_amd import collocation as C
    for T, B, block in ((24, 128, 3), (181, 100, 6), (7, 5, 1), (7, 5, 7), (7, 5, 12), (10, 4, 3)):
        got = C.bootstrap_indices(T, B, block, seed=3)
        assert got.dtype == np.uint16 and got.shape == (T, B) and got.flags["C_CONTIGUOUS"] and int(got.max()) < T
        assert np.array_equal(got, U.indices(T, B, block, seed=3))
        assert np.array_equal(got, C.bootstrap_indices(T, B, block, seed=3))
        assert not np.array_equal(got, C.bootstrap_indices(T, B, block, seed=4))
        k = min(block, T)                                             # inside a block the steps follow each other modulo T
        assert np.all((got[1:k].astype(int) - got[:k - 1]) % T == 1 % T)
    lin = C.bootstrap_indices(10, 50, 4, seed=1, circular=False)
    assert int(lin.max()) < 10 and np.all(np.diff(lin[:4].astype(int), axis=0) == 1)           # no block wraps
    for bad in (lambda: C.bootstrap_indices(0, 5, 1), lambda: C.bootstrap_indices(5, 0, 1), lambda: C.bootstrap_indices(5, 5, 0),
                lambda: C.bootstrap_indices(2049, 5, 1), lambda: C.bootstrap_indices(5, 2049, 1),
                lambda: C.bootstrap_indices(5, 5, 6, circular=False), lambda: C.bootstrap_indices(5.0, 5, 1)):
        with pytest.raises(C.L.GandanetError):
            bad()


def test_argument_errors():
    K = _K()
    E = K.L.GandanetError
    x, y, z = U.triple(24, 5)
    idx = U.indices(24, 8, 3)
    big = idx.copy()
    big[5, 3] = 24
    for bad in (lambda: K.tc_estimate_host(x, y, z, 2), lambda: K.tc_estimate_host(x, y[:, :4], z, 10),
                lambda: K.tc_estimate_host(x, y.astype(np.float32), z, 10), lambda: K.tc_estimate_host(x[0], y[0], z[0], 10),
                lambda: K.tc_estimate_host(np.zeros((2049, 2)), np.zeros((2049, 2)), np.zeros((2049, 2)), 10),
                lambda: K.tc_estimate_host(x, y, z, 10.0), lambda: K.tc_bootstrap_host(x, y, z, idx, Q3, 2),
                lambda: K.tc_bootstrap_host(x, y, z, big, Q3, 10), lambda: K.tc_bootstrap_host(x, y, z, idx[:23], Q3, 10),
                lambda: K.tc_bootstrap_host(x, y, z, idx.astype(np.int32), Q3, 10), lambda: K.tc_bootstrap_host(x, y, z, idx, (), 10),
                lambda: K.tc_bootstrap_host(x, y, z, idx, np.linspace(0, 1, 9), 10), lambda: K.tc_bootstrap_host(x, y, z, idx, (1.5,), 10),
                lambda: K.tc_bootstrap_host(x, y, z, np.zeros((24, 2049), dtype=np.uint16), Q3, 10),
                lambda: K.tc_bootstrap_host(x, y, z, np.zeros((24, 0), dtype=np.uint16), Q3, 10)):
        with pytest.raises(E):
            bad()
    lib = K.lib()
    p, ip = x.ctypes.data, idx.ctypes.data
    q = np.array(Q3)
    out = np.empty(8 * 5 * 5)
    cnt = np.empty(8 * 5, dtype=np.int32)
    o, c, qp = out.ctypes.data, cnt.ctypes.data, q.ctypes.data

    def est(**kw):
        a = dict(x=p, y=p, z=p, dtype=1, T=24, M=5, ms=10, mask=None, stats=o, cov=None, n=c, flags=c)
        a.update(kw)
        return lib.gd_tc_estimate_host(a["x"], a["y"], a["z"], a["dtype"], a["T"], a["M"], a["ms"], a["mask"], a["stats"], a["cov"], a["n"], a["flags"])

    def boot(fn=lib.gd_tc_bootstrap_host, tail=(), **kw):
        a = dict(x=p, y=p, z=p, dtype=1, T=24, M=5, idx=ip, B=8, ms=10, q=qp, Q=3, mask=None, summary=o, n_ok=c, rep=None)
        a.update(kw)
        return fn(a["x"], a["y"], a["z"], a["dtype"], a["T"], a["M"], a["idx"], a["B"], a["ms"], a["q"], a["Q"], a["mask"], a["summary"],
                  a["n_ok"], a["rep"], *tail)

    assert est() == 0 and boot() == 0
    for kw, word in ((dict(y=None), "null"), (dict(stats=None), "null"), (dict(dtype=2), "dtype"), (dict(T=0), "T outside"),
                     (dict(T=2049), "T outside"), (dict(M=0), "M <= 0"), (dict(ms=2), "min_samples"), (dict(x=p + 4), "aligned"),
                     (dict(cov=o + 4), "aligned")):
        assert est(**kw) == -1 and word in K.L.last_error(), kw
    for kw, word in ((dict(z=None), "null"), (dict(idx=None), "null"), (dict(q=None), "null"), (dict(dtype=-1), "dtype"),
                     (dict(T=0), "T outside"), (dict(B=0), "B outside"), (dict(B=2049), "B outside"), (dict(Q=0), "Q outside"),
                     (dict(Q=9), "Q outside"), (dict(ms=2), "min_samples"), (dict(idx=big.ctypes.data), "index is >= T"),
                     (dict(idx=ip + 1), "aligned"), (dict(summary=o + 4), "aligned"), (dict(T=23), "index is >= T")):
        assert boot(**kw) == -1 and word in K.L.last_error(), kw
    # the device entry makes the same checks before it touches the GPU, and names the bytes of one group of pixels
    need = K.tc_bootstrap_min_workspace(24, 8)
    assert need == 8 + 8 * 8 * 8 * 8 and lib.gd_tc_group(24) == 8 and lib.gd_tc_group(341) == 4 and lib.gd_tc_group(2048) == 1
    assert lib.gd_tc_group(0) == 0 and lib.gd_tc_group(2049) == 0
    assert K.tc_bootstrap_workspace(24, 5, 8) == need and K.tc_bootstrap_workspace(24, 9, 8) == 8 + 16 * 8 * 8 * 8
    dev = lambda **kw: boot(lib.gd_tc_bootstrap, (kw.pop("ws", o), kw.pop("ws_bytes", need), None), **kw)
    assert dev(B=0) == -1 and "B outside" in K.L.last_error()
    assert dev(ws=None) == -1 and "workspace" in K.L.last_error()
    assert dev(ws_bytes=need - 1) == -1 and f"{need} bytes needed" in K.L.last_error()
    assert dev(ws_bytes=0) == -1 and "smaller than one group" in K.L.last_error()
    assert lib.gd_tc_estimate(p, p, p, 1, 24, 5, 2, None, o, None, c, c, None) == -1 and "min_samples" in K.L.last_error()
