"""CPU: the filter entry points of the C ABI (include/gandanet.h, "filters") are declared and bound,
gd_gaussian_weights_host reproduces scipy's Gaussian taps, every device entry point rejects bad arguments before any
launch, the Savitzky-Golay tables agree with scipy and with the hat matrix, and the public module refuses CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.signal
import torch

NAMES = ("gd_gaussian_weights_host", "gd_correlate1d_axis", "gd_savgol_edges_axis", "gd_median_nd", "gd_fill_ratio",
         "gd_fill_prepare")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_filter_symbols_are_declared_and_bound():
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name


def _numpy_taps(sigma, radius):
    """scipy.ndimage's formula (_gaussian_kernel1d, order 0) written out in numpy"""
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


@pytest.mark.parametrize("sigma,radius", [(2.0, 8), (3.0, 12), (0.4, 2)])
def test_gaussian_weights_host(sigma, radius):
    L, lib = _lib()
    w = (C.c_double * 129)()
    assert lib.gd_gaussian_weights_host(sigma, 4.0, w, 129) == radius
    got, want = np.array(w[:2 * radius + 1]), _numpy_taps(sigma, radius)
    ulps = np.max(np.abs(got - want) / np.spacing(want))
    print(f"sigma {sigma}: max {ulps} ulp from numpy, |sum - 1| = {abs(got.sum() - 1.0):.3e}")
    assert ulps <= 2.0
    assert abs(got.sum() - 1.0) <= 1e-15
    assert np.all(np.array(w[2 * radius + 1:]) == 0.0)            # nothing beyond the taps is written


def test_gaussian_weights_host_errors():
    L, lib = _lib()
    w = (C.c_double * 129)()
    assert lib.gd_gaussian_weights_host(2.0, 4.0, w, 16) < 0 and "capacity" in L.last_error()   # 17 taps
    assert lib.gd_gaussian_weights_host(2.0, 4.0, w, 17) == 8
    assert lib.gd_gaussian_weights_host(0.0, 4.0, w, 129) < 0 and "sigma" in L.last_error()
    assert lib.gd_gaussian_weights_host(-1.0, 4.0, w, 129) < 0 and "sigma" in L.last_error()
    assert lib.gd_gaussian_weights_host(2.0, 4.0, None, 129) < 0 and "null" in L.last_error()
    from gan_danet_amd import kern as K
    with pytest.raises(L.GandanetError):
        K.gaussian_weights_host(17.0)                               # radius 68 > 64


def test_filter_argument_errors_before_any_launch():
    """negative code + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses)
    are not touched"""
    L, lib = _lib()
    p, q, r, s = 0x1000, 0x2000, 0x3000, 0x4000
    w = (C.c_double * 129)(*([1.0] + [0.0] * 128))

    def bad(rc, word):
        assert rc < 0, rc
        assert word in L.last_error(), L.last_error()

    cor = lib.gd_correlate1d_axis
    bad(cor(None, q, 0, 2, 10, 3, w, 1, 0, None), "null")
    bad(cor(p, None, 0, 2, 10, 3, w, 1, 0, None), "null")
    bad(cor(p, q, 0, 2, 10, 3, None, 1, 0, None), "null")
    bad(cor(p, p, 0, 2, 10, 3, w, 1, 0, None), "src == dst")
    bad(cor(p, q, 0, 2, 0, 3, w, 1, 0, None), "L <= 0")
    bad(cor(p, q, 0, 2, -5, 3, w, 1, 0, None), "L <= 0")
    bad(cor(p, q, 0, 0, 10, 3, w, 1, 0, None), "<= 0")
    bad(cor(p, q, 0, 2, 10, 0, w, 1, 0, None), "<= 0")
    bad(cor(p, q, 0, 2, 10, 3, w, 65, 0, None), "radius")
    bad(cor(p, q, 0, 2, 10, 3, w, -1, 0, None), "radius")
    bad(cor(p, q, 2, 2, 10, 3, w, 1, 0, None), "dtype")
    bad(cor(p, q, -1, 2, 10, 3, w, 1, 0, None), "dtype")
    bad(cor(p, q, 0, 2, 10, 3, w, 1, 2, None), "edge mode")
    bad(cor(p + 4, q, 1, 2, 10, 3, w, 1, 0, None), "aligned")

    sg = lib.gd_savgol_edges_axis
    bad(sg(None, q, 0, 2, 10, 3, r, 5, None), "null")
    bad(sg(p, None, 0, 2, 10, 3, r, 5, None), "null")
    bad(sg(p, q, 0, 2, 10, 3, None, 5, None), "null")
    bad(sg(p, p, 0, 2, 10, 3, r, 5, None), "src == dst")
    bad(sg(p, q, 0, 2, 0, 3, r, 5, None), "L <= 0")
    bad(sg(p, q, 3, 2, 10, 3, r, 5, None), "dtype")
    bad(sg(p, q, 0, 2, 10, 3, r, 4, None), "odd")
    bad(sg(p, q, 0, 2, 100, 3, r, 35, None), "odd and <= 33")
    bad(sg(p, q, 0, 2, 10, 3, r, 11, None), "longer than the axis")
    bad(sg(p, q, 0, 2, 10, 3, r, 0, None), "odd")

    med = lib.gd_median_nd
    shape, size = (C.c_int64 * 4)(2, 3, 8, 8), (C.c_int * 4)(1, 1, 3, 3)

    def sizes(*v):
        return (C.c_int * 4)(*v)

    bad(med(None, q, 0, shape, size, None), "null")
    bad(med(p, None, 0, shape, size, None), "null")
    bad(med(p, q, 0, None, size, None), "null")
    bad(med(p, q, 0, shape, None, None), "null")
    bad(med(p, p, 0, shape, size, None), "src == dst")
    bad(med(p, q, 2, shape, size, None), "dtype")
    bad(med(p, q, 0, (C.c_int64 * 4)(2, 0, 8, 8), size, None), "shape")
    bad(med(p, q, 0, shape, sizes(1, 1, 2, 3), None), "size outside")
    bad(med(p, q, 0, shape, sizes(1, 1, 7, 1), None), "size outside")
    bad(med(p, q, 0, shape, sizes(1, 1, 0, 3), None), "size outside")
    bad(med(p, q, 0, shape, sizes(1, 1, 1, 1), None), "window count")        # 1
    bad(med(p, q, 0, shape, sizes(1, 1, 3, 5), None), "window count")        # 15
    bad(med(p, q, 0, shape, sizes(1, 5, 5, 5), None), "window count")        # 125
    bad(med(p, q, 0, shape, sizes(3, 3, 3, 5), None), "window count")        # 135
    bad(med(p, q, 0, shape, sizes(5, 5, 5, 5), None), "window count")        # 625

    prep = lib.gd_fill_prepare
    bad(prep(None, -9999.0, q, r, 0, 10, None), "null")
    bad(prep(p, -9999.0, None, r, 0, 10, None), "null")
    bad(prep(p, -9999.0, q, None, 0, 10, None), "null")
    bad(prep(p, -9999.0, p, r, 0, 10, None), "three buffers")
    bad(prep(p, -9999.0, q, q, 0, 10, None), "three buffers")
    bad(prep(p, -9999.0, q, r, 5, 10, None), "dtype")
    bad(prep(p, -9999.0, q, r, 0, 0, None), "n <= 0")

    rat = lib.gd_fill_ratio
    bad(rat(None, q, r, -9999.0, s, 0, 10, None), "null")
    bad(rat(p, None, r, -9999.0, s, 0, 10, None), "null")
    bad(rat(p, q, None, -9999.0, s, 0, 10, None), "null")
    bad(rat(p, q, r, -9999.0, None, 0, 10, None), "null")
    bad(rat(p, q, r, -9999.0, p, 0, 10, None), "buffer of its own")
    bad(rat(p, q, r, -9999.0, s, -3, 10, None), "dtype")
    bad(rat(p, q, r, -9999.0, s, 1, 0, None), "n <= 0")


def _hat(window, polyorder):
    """the least-squares hat matrix of the window's Vandermonde system, by the pseudo-inverse (the module uses QR)"""
    t = np.arange(window, dtype=np.float64) - window // 2
    a = np.vander(t, polyorder + 1, increasing=True)
    return a @ np.linalg.pinv(a)


@pytest.mark.parametrize("window,polyorder", [(5, 2), (11, 3), (33, 4)])
def test_savgol_tables(window, polyorder):
    from gan_danet_amd import filters
    coeffs, edges = filters.savgol_tables(window, polyorder)
    h, hat = window // 2, _hat(window, polyorder)
    assert coeffs.shape == (window,) and edges.shape == (2, h, window)
    assert coeffs.dtype == np.float64 and edges.dtype == np.float64
    ref = scipy.signal.savgol_coeffs(window, polyorder)
    e_c = max(np.abs(coeffs - ref).max(), np.abs(coeffs - ref[::-1]).max())
    e_l, e_r = np.abs(edges[0] - hat[:h]).max(), np.abs(edges[1] - hat[window - h:]).max()
    print(f"({window}, {polyorder}): coeffs vs savgol_coeffs {e_c:.3e}, edges vs hat rows {e_l:.3e} / {e_r:.3e}, "
          f"coeffs vs hat centre row {np.abs(coeffs - hat[h]).max():.3e}")
    assert e_c <= 1e-12
    assert e_l <= 1e-12 and e_r <= 1e-12
    # the centre row against the hat matrix: within 1e-12 plus whatever scipy's own coefficients are away from it (4e-16
    # at (5, 2) and (11, 3); 1.06e-12 at (33, 4), where matching scipy and matching the exact row exclude each other)
    scipy_off = np.abs(ref[::-1] - hat[h]).max()
    assert np.abs(coeffs - hat[h]).max() <= 1e-12 + scipy_off
    # the edge rule in full: the rows applied to a window of samples are scipy's polynomial fit at the edge positions
    x = np.random.RandomState(window).randn(window)
    want = scipy.signal.savgol_filter(x, window, polyorder)
    got = np.concatenate([edges[0] @ x, [coeffs @ x], edges[1] @ x])
    assert np.abs(got - want).max() <= 1e-12 * np.abs(x).max() * window


def test_savgol_value_errors():
    from gan_danet_amd import filters
    for w, p in ((4, 2), (0, 0), (5, 5), (5, 7)):
        with pytest.raises(ValueError):
            filters.savgol_tables(w, p)


def test_cpu_tensors_are_refused():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import filters
    x = torch.zeros(3, 4, 6, 9)
    calls = [lambda: filters.gaussian_filter(x, 2), lambda: filters.median_filter(x, 3),
             lambda: filters.savgol_filter(x, 5, 2), lambda: filters.fill_masked(x),
             lambda: filters.smooth_data_gaussian(x), lambda: filters.smooth_data_median(x),
             lambda: filters.smooth_data_savitzky_golay(x)]
    for call in calls:
        with pytest.raises(L.GandanetError):
            call()
    import gan_danet_amd
    assert gan_danet_amd.filters is filters


def test_dataset_rejects_unknown_smoothing():
    from gan_danet_amd.data import DeviceTileDataset
    a, b, c = np.zeros((2, 4, 4), np.float32), np.zeros((2, 8, 8), np.float32), np.zeros((2, 8, 8, 3), np.float32)
    with pytest.raises(ValueError):
        DeviceTileDataset(a, b, c, smoothing="nonsense")
    with pytest.raises(ValueError):
        DeviceTileDataset(a, b, c, smoothing=3)
