"""CPU: the spatial-spectra entry points of the C ABI (include/gandanet.h, "Spatial spectra") are declared and bound, reject
every bad argument before any launch, and the host twins -- plain loops over csrc/spectra_core.h, the arithmetic the
device kernels share -- hold the bounds of tests/spectra_util.py against its longdouble oracle.  gd_spec_bins_host is
checked against an independent Fraction binning, the twiddle table against the longdouble one, and numpy.fft.rfft2
against the oracle (a check of the oracle).  Each test prints its largest error over its bound (python -m pytest -s)."""
import os

import numpy as np
import pytest

import spectra_util as U

NAMES = ("gd_spec_twiddle_host", "gd_spec_default_bins", "gd_spec_bins_host", "gd_spec_prepare", "gd_spec_prepare_host",
         "gd_spec_power_ws_bytes", "gd_spec_power", "gd_spec_power_host", "gd_spec_cross_ws_bytes", "gd_spec_cross",
         "gd_spec_cross_host")
DETRENDS, WINDOWS = ("none", "mean", "plane"), ("none", "hann", ("tukey", 0.4))


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_spectra_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import build, spectra
    L, lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gandanet.h")).read()
    assert "Spatial spectra" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
    for name, v in (("GD_SPEC_MAX_H", L.SPEC_MAX_H), ("GD_SPEC_MAX_W", L.SPEC_MAX_W), ("GD_SPEC_MAX_BINS", L.SPEC_MAX_BINS)):
        assert f"#define {name} {v}" in src
    assert "spectra.hip" in build.SOURCES and os.path.exists(os.path.join(root, "gan-danet_amd", "csrc", "spectra_core.h"))
    for name in ("power_spectrum", "cross_spectrum", "spectral_ratio", "effective_resolution", "Spectrum", "CrossSpectrum"):
        assert getattr(gan_danet_amd, name) is getattr(spectra, name)
    # one slab of nbins + 1 doubles per field and tile of 8 (cross: 4 values, tiles of 4) kx; 0 for a refused shape
    for T, H, W, nb in ((1, 1, 1, 1), (3, 17, 33, 9), (181, 440, 900, 450)):
        kx = W // 2 + 1
        assert lib.gd_spec_power_ws_bytes(T, H, W, nb) == T * -(-kx // 8) * (nb + 1) * 8
        assert lib.gd_spec_cross_ws_bytes(T, H, W, nb) == T * -(-kx // 4) * 4 * (nb + 1) * 8
    for f in (lib.gd_spec_power_ws_bytes, lib.gd_spec_cross_ws_bytes):
        for T, H, W, nb in ((0, 4, 4, 2), (1, 0, 4, 2), (1, 4, 0, 2), (1, 1025, 4, 2), (1, 4, 2049, 2), (1 << 12, 1024, 1024, 2),
                            (1, 4, 4, 0), (1, 4, 4, 1025)):
            assert f(T, H, W, nb) == 0, (T, H, W, nb)


def test_spectra_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the device pointers (never-dereferenced addresses) are
    not touched"""
    L, lib = _lib()
    a, b, c, d, e, f, g, h, i, j, k = (0x1000 * n for n in range(1, 12))

    def sweep(fns, order, good, rules):
        for host, fn, extra in fns:
            for kw, word in rules:
                if host and any(key in extra for key in kw):
                    continue
                v = dict(good, **kw)
                args = [v[key] for key in order if host is False or key not in extra]
                rc = fn(*args) if host else fn(*args, None)
                assert rc == -1, (fn.__name__, kw, rc)
                assert word in L.last_error(), (fn.__name__, kw, L.last_error())

    shapes = [(dict(dtype=2), "dtype"), (dict(T=0), "< 1"), (dict(H=0), "< 1"), (dict(W=0), "< 1"), (dict(H=1025), "GD_SPEC_MAX_H"),
              (dict(W=2049), "GD_SPEC_MAX_W"), (dict(T=1 << 12, H=1024, W=1024), "too many"), (dict(T=1 << 31, H=1, W=1), "too many")]
    sweep(((False, lib.gd_spec_prepare, ()), (True, lib.gd_spec_prepare_host, ())),
          ("x", "dtype", "T", "H", "W", "mask", "wy", "wx", "detrend", "coef", "S"),
          dict(x=a, dtype=1, T=3, H=17, W=33, mask=None, wy=None, wx=None, detrend=1, coef=b, S=c),
          [(dict(x=None), "null"), (dict(coef=None), "null"), (dict(S=None), "null"), (dict(detrend=3), "detrend"),
           (dict(detrend=-1), "detrend"), (dict(x=a + 4), "aligned"), (dict(wy=d + 4), "aligned"), (dict(wx=d + 2), "aligned"),
           (dict(coef=b + 4), "aligned"), (dict(S=c + 4), "aligned")] + shapes)
    tables = [(dict(nbins=0), "nbins"), (dict(nbins=1025), "nbins"), (dict(th=None), "null"), (dict(tw=None), "null"),
              (dict(bin=None), "null"), (dict(th=d + 4), "aligned"), (dict(bin=f + 2), "aligned")]
    good = dict(x=a, dtype=0, T=3, H=17, W=33, mask=None, wy=None, wx=None, coef=b, S=c, th=d, tw=e, bin=f, nbins=9, power=g, dropped=h,
                p2d=None, ws=i, nbytes=1 << 30)
    sweep(((False, lib.gd_spec_power, ()), (True, lib.gd_spec_power_host, ("ws", "nbytes"))),
          ("x", "dtype", "T", "H", "W", "mask", "wy", "wx", "coef", "S", "th", "tw", "bin", "nbins", "power", "dropped", "p2d", "ws", "nbytes"),
          good, [(dict(x=None), "null"), (dict(coef=None), "null"), (dict(S=None), "null"), (dict(power=None), "null"),
                 (dict(dropped=None), "null"), (dict(x=a + 2), "aligned"), (dict(power=g + 4), "aligned"), (dict(p2d=j + 4), "aligned"),
                 (dict(ws=None), "workspace"), (dict(ws=i + 4), "workspace"), (dict(nbytes=3 * 3 * 10 * 8 - 1), "workspace")]
          + tables + shapes)
    good = dict(xa=a, xb=k, dtype=1, T=3, H=17, W=33, mask=None, wy=None, wx=None, ca=b, sa=c, cb=b, sb=c, th=d, tw=e, bin=f, nbins=9,
                out=g, dropped=h, ws=i, nbytes=1 << 30)
    sweep(((False, lib.gd_spec_cross, ()), (True, lib.gd_spec_cross_host, ("ws", "nbytes"))),
          ("xa", "xb", "dtype", "T", "H", "W", "mask", "wy", "wx", "ca", "sa", "cb", "sb", "th", "tw", "bin", "nbins", "out", "dropped", "ws",
           "nbytes"),
          good, [(dict(xa=None), "null"), (dict(xb=None), "null"), (dict(cb=None), "null"), (dict(sb=None), "null"), (dict(out=None), "null"),
                 (dict(xb=k + 4), "aligned"), (dict(out=g + 4), "aligned"), (dict(ws=None), "workspace"),
                 (dict(nbytes=3 * 5 * 4 * 10 * 8 - 1), "workspace")] + tables + shapes)
    ok = np.zeros(64, np.int64)
    p = ok.ctypes.data
    for args, word in (((0, 4, 1.0, 1.0, 2, 0.0, p, p, p), "outside"), ((4, 4, 0.0, 1.0, 2, 0.0, p, p, p), "positive"),
                       ((4, 4, 1.0, float("inf"), 2, 0.0, p, p, p), "positive"), ((4, 4, 1.0, 1.0, 0, 0.0, p, p, p), "nbins"),
                       ((4, 4, 1.0, 1.0, 2, float("nan"), p, p, p), "NaN"), ((4, 4, 1.0, 1.0, 2, 0.0, None, p, p), "null")):
        assert lib.gd_spec_bins_host(*args) == -1 and word in L.last_error(), (args, L.last_error())
    assert lib.gd_spec_twiddle_host(0, p) == -1 and lib.gd_spec_twiddle_host(4, None) == -1
    assert lib.gd_spec_default_bins(4, 4, 0.0, 1.0) == 0


def test_twiddles_within_one_ulp_and_exact_on_the_axes():
    from gan_danet_amd import kern as K
    worst = 0.0
    for N in (1, 2, 4, 5, 7, 8, 12, 31, 33, 90, 440, 900, 2048):
        tw = K.spec_twiddle_host(N)
        c, s = U.twiddles(N)
        for got, want in ((tw[:N], c), (tw[N:], s)):
            ulp = np.spacing(np.abs(want.astype(np.float64)))
            err = np.abs(got.astype(U.LD) - want).astype(np.float64)
            exact = np.abs(want) < 1e-30
            assert np.all(got[exact] == 0) and np.all(err <= ulp), N
            worst = max(worst, float((err / ulp).max()))
        if N % 4 == 0:
            assert tw[N // 4] == 0 and tw[N + N // 4] == 1 and tw[N // 2] == -1 and tw[N + N // 2] == 0 and tw[N + 3 * N // 4] == -1
        assert tw[0] == 1 and tw[N] == 0
    print(f"twiddles: at most {worst:.3f} ulp")


@pytest.mark.parametrize("dy,dx", [(1.0, 1.0), (0.5, 0.5), (0.25, 0.5), (0.05, 0.05), (0.3, 0.7), (1.0 / 3.0, 0.1234567)])
def test_bins_host_against_fractions(dy, dx):
    from gan_danet_amd import kern as K
    for H, W in U.SHAPES + ((3, 4), (5, 6), (20, 40), (100, 200)):
        nb = K.spec_default_bins(H, W, dy, dx)
        P, Q = H * dy, W * dx
        assert nb == min(int(np.floor(0.5 / max(dx, dy) * max(P, Q) * (1 + 2.0 ** -40))) + 1, 1024)
        for nbins, kmax in ((nb, 0.5 / max(dx, dy)), (nb, 0.0), (max(nb // 2, 1), 0.0)):
            bins, kc, count = K.spec_bins_host(H, W, dy, dx, nbins, kmax)
            want = U.bins_fraction(H, W, dy, dx, nbins, kmax)
            assert np.array_equal(bins, want), (H, W, nbins, kmax)
            assert bins.min() >= -1 and bins.max() < nbins and count.sum() == H * (W // 2 + 1) - (bins < 0).sum()
            assert np.array_equal(count, np.bincount(bins[bins >= 0], minlength=nbins))
            assert np.allclose(kc, (np.arange(nbins) + 0.5) / max(P, Q), rtol=1e-15)
        assert bins[0, 0] == 0
    # a 3-4-5 triangle lands on the edge of bin 5, exactly
    assert K.spec_bins_host(16, 16, 1.0, 1.0, 9)[0][3, 4] == 5 and K.spec_bins_host(16, 16, 1.0, 1.0, 9)[0][13, 4] == 5


def test_hermitian_weights_through_p2d():
    """a delta at the origin has Z = 1 everywhere, S = H W: p2d = weight / (H W)^2, weight 1, 2, .., 2, 1 on even W and
    1, 2, .., 2 on odd W -- the code's own weights, not the oracle's"""
    from gan_danet_amd import kern as K
    for H, W in ((4, 8), (5, 7), (1, 2), (3, 1), (16, 16), (17, 33)):
        x = np.zeros((1, H, W))
        x[0, 0, 0] = 1.0
        coef, S = K.spec_prepare_host(x, detrend="none")
        bins, _, _ = K.spec_bins_host(H, W, 1.0, 1.0, 1)
        power, dropped, p2d = K.spec_power_host(x, coef, S, bins, 1, two_d=True)
        w = np.full(W // 2 + 1, 2.0)
        w[0] = 1.0
        if W % 2 == 0:
            w[-1] = 1.0
        want = np.broadcast_to(w / float(H * W) ** 2, (H, W // 2 + 1))
        P, BP, _, _ = U.power_oracle(x[0], coef[0])                # the oracle's bound; `want` is exact up to its own roundings
        assert np.all(np.abs(p2d[0] - want) <= BP + 4 * U.U * want), (H, W)
        assert abs(power[0, 0] + dropped[0] - 1.0 / (H * W)) <= float(BP.sum()) + U.gamma(H * W + 8) / (H * W)   # Parseval: sum x^2 / S


def test_rfft2_agrees_with_the_oracle():
    """a cross-check of the oracle, not of the code under test: numpy's fp64 FFT to its own tolerance"""
    for H, W in U.SHAPES:
        x = U.field(H, W)[0]
        zre, zim = U.dft(x.astype(U.LD))
        z = np.fft.rfft2(x)
        tol = 64 * U.U * np.log2(max(H * W, 2)) * np.abs(x).sum()
        assert np.abs(z.real - zre.astype(np.float64)).max() <= tol and np.abs(z.imag - zim.astype(np.float64)).max() <= tol, (H, W)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_prepare_host(dtype):
    from gan_danet_amd import kern as K
    worst = 0.0
    for H, W in U.SHAPES:
        x, mask = U.messy(H, W, dtype)
        i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        x[2] += (0.7 * i - 0.2 * j + 5.0).astype(dtype)
        for mk in (None, mask):
            for win in ("none", "hann"):
                wy, wx = U.windows(win, H, W)
                for det in DETRENDS:
                    coef, S = K.spec_prepare_host(x, mk, wy, wx, det)
                    for t in range(x.shape[0]):
                        ok = U.valid_of(x[t], mk)
                        want = U.detrend_oracle(x[t], ok, det)
                        bound = U.coef_bound(x[t], ok, det, want)
                        err = np.abs(coef[t].astype(U.LD) - want).astype(np.float64)
                        assert np.all(err <= bound), (H, W, det, t, err, bound)
                        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                        _, _, Sw = U.sample(x[t], ok, want, wy, wx)
                        assert S[t, 1] == ok.sum() and abs(S[t, 0] - float(Sw)) <= U.gamma(H * W + 4) * float(Sw)
    print(f"prepare_host {np.dtype(dtype).name}: coefficients at most {worst:.3f} of their bound")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_power_host(dtype):
    from gan_danet_amd import kern as K
    worst = 0.0
    for H, W in U.SHAPES:
        x, mask = U.messy(H, W, dtype)
        nbins = K.spec_default_bins(H, W, 0.5, 0.5)
        bins, _, _ = K.spec_bins_host(H, W, 0.5, 0.5, nbins, 1.0)
        for det, win, mk in (("none", "none", None), ("mean", "hann", mask), ("plane", ("tukey", 0.4), mask), ("plane", "hann", None)):
            wy, wx = U.windows(win, H, W)
            coef, S = K.spec_prepare_host(x, mk, wy, wx, det)
            power, dropped, p2d = K.spec_power_host(x, coef, S, bins, nbins, mk, wy, wx, two_d=True)
            for t in range(x.shape[0]):
                worst = max(worst, U.check_power(power[t], dropped[t], p2d[t], x[t], coef[t], bins, nbins, mk, wy, wx, (H, W, det, win, t)))
    print(f"power_host {np.dtype(dtype).name}: at most {worst:.3f} of the bounds (p2d, bins, Parseval)")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cross_host(dtype):
    from gan_danet_amd import kern as K
    worst = 0.0
    for H, W in U.SHAPES:
        xa, xb = U.field(H, W, dtype, seed=1, T=2), U.field(H, W, dtype, seed=2, T=2)
        nbins = K.spec_default_bins(H, W, 1.0, 1.0)
        bins, _, _ = K.spec_bins_host(H, W, 1.0, 1.0, nbins, 0.5)
        for det, win in (("mean", "hann"), ("plane", "none")):
            wy, wx = U.windows(win, H, W)
            ca, sa = K.spec_prepare_host(xa, None, wy, wx, det)
            cb, sb = K.spec_prepare_host(xb, None, wy, wx, det)
            out, dropped = K.spec_cross_host(xa, xb, ca, sa, cb, sb, bins, nbins, None, wy, wx)
            for t in range(2):
                worst = max(worst, U.check_cross(out[:, t], dropped[t], xa[t], ca[t], xb[t], cb[t], bins, nbins, None, wy, wx, (H, W, det, t)))
            same, sd = K.spec_cross_host(xa, xa, ca, sa, ca, sa, bins, nbins, None, wy, wx)
            if np.all(sa[:, 0] > 0):                      # a one-point Hann taper is zero: S = 0, NaN
                assert np.all(same[3] == 0) and np.array_equal(same[0], same[1]) and np.all(sd[:, 3] == 0)
    print(f"cross_host {np.dtype(dtype).name}: at most {worst:.3f} of the bounds; a against a: quad exactly 0")
