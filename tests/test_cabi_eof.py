"""CPU: the EOF entry points of the C ABI (include/gandanet.h, "EOF analysis") are declared and bound, reject every bad
argument before any launch, and the host twins -- plain loops over csrc/eof_core.h, the arithmetic the device kernels
share -- hold the bounds of tests/eof_util.py against its longdouble oracle: gd_eof_gram_host within the entrywise bound
B and exact on integer data, means, pattern maps and reconstructions within their gamma bounds.  Each test prints its
largest error over its bound (python -m pytest -s)."""
import os

import numpy as np
import pytest

import eof_util as U

NAMES = ("gd_eof_prepare", "gd_eof_prepare_host", "gd_eof_gram_ws_bytes", "gd_eof_gram", "gd_eof_gram_host", "gd_eof_project",
         "gd_eof_project_host", "gd_eof_reconstruct", "gd_eof_reconstruct_host")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_eof_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import build, eof
    L, lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gandanet.h")).read()
    core = open(os.path.join(root, "gan-danet_amd", "csrc", "eof_core.h")).read()
    assert "EOF analysis" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
    assert f"#define GD_EOF_MAX_T {L.EOF_MAX_T}" in src and f"#define GD_EOF_MAX_K {L.EOF_MAX_K}" in src
    assert f"#define GD_EOF_CHUNK {L.EOF_CHUNK}" in core and f"#define GD_EOF_SPLIT_MIN {L.EOF_SPLIT_MIN}" in core
    assert f"#define GD_EOF_SPLIT_MAX {L.EOF_SPLIT_MAX}" in core
    assert (L.EOF_CHUNK, L.EOF_SPLIT_MIN, L.EOF_SPLIT_MAX) == (U.CHUNK, U.SPLIT_MIN, U.SPLIT_MAX)
    assert "eof.hip" in build.SOURCES
    assert gan_danet_amd.eof is eof and gan_danet_amd.eof_analysis is eof.eof_analysis and gan_danet_amd.EOFResult is eof.EOFResult
    # the workspace is one slab of nblk * 256 doubles per split; 0 for a refused shape
    for T in U.GRAM_TS:
        for M in U.GRAM_MS + (396000,):
            nb, nblk, splits = U.geom(T, M)
            assert lib.gd_eof_gram_ws_bytes(T, M) == splits * nblk * 2048, (T, M)
    assert U.geom(181, 396000)[1:] == (78, 253) and U.geom(256, 600)[1:] == (136, 3) and U.geom(2, 257)[2] == 2
    assert lib.gd_eof_gram_ws_bytes(1, 5) == 0 and lib.gd_eof_gram_ws_bytes(257, 5) == 0 and lib.gd_eof_gram_ws_bytes(5, 0) == 0


def test_eof_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the device pointers (never-dereferenced addresses) are
    not touched"""
    L, lib = _lib()
    a, b, c, d, e, f = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000

    def sweep(fns, order, good, rules):
        for host, fn, extra in fns:
            for kw, word in rules:
                v = dict(good, **kw)
                args = [v[k] for k in order if host is False or k not in extra]
                rc = fn(*args) if host else fn(*args, None)
                assert rc == -1, (fn.__name__, kw, rc)
                assert word in L.last_error(), (fn.__name__, kw, L.last_error())

    sweep(((False, lib.gd_eof_prepare, ()), (True, lib.gd_eof_prepare_host, ())),
          ("x", "dtype", "T", "M", "mask", "w", "center", "mean", "valid"),
          dict(x=a, dtype=1, T=181, M=7, mask=None, w=None, center=1, mean=b, valid=c),
          [(dict(x=None), "null"), (dict(mean=None), "null"), (dict(valid=None), "null"), (dict(dtype=2), "dtype"), (dict(T=0), "<= 0"),
           (dict(M=0), "<= 0"), (dict(M=1 << 31), "too many"), (dict(center=2), "center"), (dict(x=a + 4), "aligned"),
           (dict(w=d + 4), "aligned"), (dict(mean=b + 4), "aligned")])
    sweep(((False, lib.gd_eof_gram, ()), (True, lib.gd_eof_gram_host, ("ws", "nbytes"))),
          ("x", "dtype", "T", "M", "mean", "valid", "w", "G", "ws", "nbytes"),
          dict(x=a, dtype=0, T=181, M=7, mean=b, valid=c, w=None, G=d, ws=e, nbytes=1 << 30),
          [(dict(x=None), "null"), (dict(mean=None), "null"), (dict(valid=None), "null"), (dict(G=None), "null"), (dict(dtype=-1), "dtype"),
           (dict(T=1), "T outside"), (dict(T=257), "T outside"), (dict(T=0), "<= 0"), (dict(M=0), "<= 0"), (dict(M=1 << 31), "too many"),
           (dict(x=a + 2), "aligned"), (dict(G=d + 4), "aligned")])
    for kw in (dict(ws=None), dict(nbytes=78 * 2048 - 1), dict(ws=e + 4)):
        v = dict(x=a, dtype=0, T=181, M=7, mean=b, valid=c, w=None, G=d, ws=e, nbytes=78 * 2048)
        v.update(kw)
        assert lib.gd_eof_gram(v["x"], 0, 181, 7, b, c, None, d, v["ws"], v["nbytes"], None) == -1 and "workspace" in L.last_error()
    sweep(((False, lib.gd_eof_project, ()), (True, lib.gd_eof_project_host, ())),
          ("x", "dtype", "T", "M", "mean", "valid", "w", "use", "coef", "K", "out"),
          dict(x=a, dtype=1, T=181, M=7, mean=b, valid=c, w=d, use=1, coef=e, K=4, out=f),
          [(dict(x=None), "null"), (dict(coef=None), "null"), (dict(out=None), "null"), (dict(dtype=3), "dtype"), (dict(T=0), "<= 0"),
           (dict(K=0), "K outside"), (dict(K=17), "K outside"), (dict(use=2), "use_weight"), (dict(w=None), "use_weight"),
           (dict(coef=e + 4), "aligned"), (dict(out=f + 4), "aligned")])
    sweep(((False, lib.gd_eof_reconstruct, ()), (True, lib.gd_eof_reconstruct_host, ())),
          ("eofs", "pcs", "mean", "valid", "w", "T", "M", "K", "out", "dtype"),
          dict(eofs=a, pcs=b, mean=c, valid=d, w=None, T=181, M=7, K=4, out=e, dtype=0),
          [(dict(eofs=None), "null"), (dict(pcs=None), "null"), (dict(out=None), "null"), (dict(dtype=2), "dtype"), (dict(M=0), "<= 0"),
           (dict(K=0), "K outside"), (dict(K=17), "K outside"), (dict(out=e + 2), "aligned"), (dict(eofs=a + 4), "aligned")])


def _messy(T, M, dtype, seed=0):
    """a cube with a NaN, an infinity, a masked series and one of weight zero; (x, mask, weight)"""
    x = U.cube(T, M, dtype, seed)
    mask = np.ones(M, dtype=np.uint8)
    w = U.coslat_weights(M)
    if M >= 8:
        x[T // 2, 1] = np.nan
        x[0, 2] = np.inf
        x[T - 1, 3] = -np.inf
        mask[4] = 0
        w[5] = 0.0
        w[6] = np.nan
    return x, mask, w


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_prepare_host(dtype):
    from gan_danet_amd import kern as K
    worst = 0.0
    for T, M in ((2, 1), (17, 9), (181, 70)):
        x, mask, w = _messy(T, M, dtype)
        for mk, wt, center in ((None, None, True), (mask, w, True), (mask, None, False)):
            mean, valid = K.eof_prepare_host(x, mk, wt, center)
            ok = U.valid_oracle(x, mk, wt)
            assert np.array_equal(valid, ok.astype(np.uint8)) and valid.dtype == np.uint8
            want, bound = U.mean_oracle(x, ok, center)
            assert np.all(mean[~ok] == 0) and np.all(np.abs(mean - want) <= bound)
            worst = max(worst, float((np.abs(mean - want) / np.maximum(bound, 1e-300)).max()))
            if not center:
                assert np.all(mean == 0)
    print(f"prepare_host {np.dtype(dtype).name}: mean error at most {worst:.3f} of the bound")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", U.GRAM_TS)
def test_gram_host_random(T, dtype):
    from gan_danet_amd import kern as K
    worst = 0.0
    for M in U.GRAM_MS:
        x = U.cube(T, M, dtype)
        w = U.pow4_weights(M) if M < 31 else U.coslat_weights(M)
        for wt in (None, w):
            mean, valid = K.eof_prepare_host(x, None, wt)
            G = K.eof_gram_host(x, mean, valid, wt)
            worst = max(worst, U.check_gram(G, U.anomalies(x, mean, valid, wt), int(valid.sum()), f"T={T} M={M}"))
    print(f"gram_host T = {T} {np.dtype(dtype).name}: at most {worst:.3f} of B")


@pytest.mark.parametrize("T", U.GRAM_TS)
def test_gram_host_exact_and_invalid(T):
    from gan_danet_amd import kern as K
    for M in (3, 33, 257):
        for centred in (False, True):
            xi = U.int_cube(T, M, centred)
            for dtype in (np.float64, np.float32):
                x = xi.astype(dtype)
                mean, valid = K.eof_prepare_host(x, None, None, center=centred)
                assert np.all(mean == 0) and np.all(valid == 1)
                assert np.array_equal(K.eof_gram_host(x, mean, valid), (xi @ xi.T).astype(np.float64)), (T, M, centred)
    x, mask, w = _messy(T, 70, np.float64)
    mean, valid = K.eof_prepare_host(x, mask, w)
    assert valid.sum() == 70 - 6
    G = K.eof_gram_host(x, mean, valid, w)
    keep = valid.astype(bool)
    ratio = U.check_gram(G, U.anomalies(x[:, keep], mean[keep], valid[keep], w[keep]), int(keep.sum()), f"T={T} reduced")
    assert np.all(K.eof_gram_host(x, mean, np.zeros(70, np.uint8), w) == 0)
    print(f"gram_host T = {T}: exact on integers; invalid series add nothing ({ratio:.3f} of B on the reduced matrix)")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_project_and_reconstruct_host(dtype):
    from gan_danet_amd import kern as K
    rng = np.random.default_rng(5)
    worst_p = worst_r = 0.0
    for T, M, kk in ((2, 1, 1), (17, 9, 4), (181, 70, 16), (33, 65, 5)):
        x, mask, w = _messy(T, M, dtype)
        mean, valid = K.eof_prepare_host(x, mask, w)
        coef = rng.standard_normal((T, kk))
        for wt, use in ((w, True), (w, False), (None, False)):
            got = K.eof_project_host(x, mean, valid, coef, wt, use)
            want, bound = U.project_oracle(x, mean, valid, coef, wt if use else None)
            ok = valid.astype(bool)
            assert np.isnan(got[:, ~ok]).all() and np.all(np.abs(got - want)[:, ok] <= bound[:, ok])
            worst_p = max(worst_p, float((np.abs(got - want)[:, ok] / np.maximum(bound[:, ok], 1e-300)).max()))
        eofs, pcs = rng.standard_normal((kk, M)), rng.standard_normal((T, kk))
        for wt in (w, None):
            for od in (np.float64, np.float32):
                got = K.eof_reconstruct_host(eofs, pcs, mean, valid, wt, od)
                want, bound = U.reconstruct_oracle(eofs, pcs, mean, valid, wt, od)
                ok = valid.astype(bool)
                assert got.dtype == od and np.isnan(got[:, ~ok]).all() and np.all(np.abs(got - want)[:, ok] <= bound[:, ok])
                worst_r = max(worst_r, float((np.abs(got - want)[:, ok] / np.maximum(bound[:, ok], 1e-300)).max()))
    print(f"{np.dtype(dtype).name}: project_host at most {worst_p:.3f} of its bound, reconstruct_host {worst_r:.3f}")


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_host_twin_launcher_edges(M):
    """the host side of the per-item launcher, T = 5: gd_eof_prepare_host, gd_eof_project_host and gd_eof_reconstruct_host
    write through the C entries into the middle of buffers of sentinels, leave the sentinels alone, and a column's bits are
    those the wrappers give on the 257-series cube (the device side: tests/test_gpu_eof.py::test_launcher_edges)"""
    from gan_danet_amd import kern as K
    L, lib = _lib()
    T, kk, pad = 5, 4, 64

    def guarded(n, dtype):
        return np.full(n + 2 * pad, 7, dtype=dtype)

    def ptr(buf):
        return buf[pad:].ctypes.data

    def middle(buf, n, shape):
        assert np.all(buf[:pad] == 7) and np.all(buf[pad + n:] == 7), "written outside the output"
        return buf[pad:pad + n].reshape(shape)

    rng = np.random.default_rng(7)
    coef, eofs_w, pcs = rng.standard_normal((T, kk)), rng.standard_normal((kk, 257)), rng.standard_normal((T, kk))
    w_wide = U.coslat_weights(257)
    for dtype in (np.float64, np.float32):
        wide = U.cube(T, 257, dtype)
        wide[::2, 0] = np.nan                                            # a series with gaps, present at every M
        x, w, eofs = np.ascontiguousarray(wide[:, :M]), np.ascontiguousarray(w_wide[:M]), np.ascontiguousarray(eofs_w[:, :M])
        dt = int(dtype == np.float64)
        mean_w, valid_w = K.eof_prepare_host(wide, None, w_wide, True)
        mb, vb = guarded(M, np.float64), guarded(M, np.uint8)
        L.check(lib.gd_eof_prepare_host(x.ctypes.data, dt, T, M, None, w.ctypes.data, 1, ptr(mb), ptr(vb)), "gd_eof_prepare_host")
        mean, valid = middle(mb, M, (M,)).copy(), middle(vb, M, (M,)).copy()
        assert np.array_equal(mean, mean_w[:M], equal_nan=True) and np.array_equal(valid, valid_w[:M])
        pb = guarded(kk * M, np.float64)
        L.check(lib.gd_eof_project_host(x.ctypes.data, dt, T, M, mean.ctypes.data, valid.ctypes.data, w.ctypes.data, 1, coef.ctypes.data, kk,
                                        ptr(pb)), "gd_eof_project_host")
        assert np.array_equal(middle(pb, kk * M, (kk, M)), K.eof_project_host(wide, mean_w, valid_w, coef, w_wide, True)[:, :M], equal_nan=True)
        rb = guarded(T * M, dtype)
        L.check(lib.gd_eof_reconstruct_host(eofs.ctypes.data, pcs.ctypes.data, mean.ctypes.data, valid.ctypes.data, w.ctypes.data, T, M, kk,
                                            ptr(rb), dt), "gd_eof_reconstruct_host")
        want = K.eof_reconstruct_host(eofs_w, pcs, mean_w, valid_w, w_wide, dtype)[:, :M]
        assert np.array_equal(middle(rb, T * M, (T, M)), want, equal_nan=True)
