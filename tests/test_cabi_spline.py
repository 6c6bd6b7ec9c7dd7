"""CPU: the spline-zoom entry points of the C ABI (include/gandanet.h, "spline zoom") are declared and bound, every device
entry point rejects bad arguments before any launch, the public module raises ValueError for what it does not support,
applies scipy's output-shape rule and refuses CPU tensors."""
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

NAMES = ("gd_zoom_axis_ws_bytes", "gd_zoom_axis", "gd_spline_prefilter_axis", "gd_restore_units",
         "gd_masked_plane_mean_f64_ws_bytes", "gd_masked_plane_mean_f64")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_spline_symbols_are_declared_and_bound():
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
    assert "GD_ZOOM_MIRROR = 0" in src and "GD_ZOOM_NEAREST = 1" in src
    assert (L.ZOOM_MIRROR, L.ZOOM_NEAREST) == (0, 1)
    from gan_danet_amd import build
    assert "spline.hip" in build.SOURCES


def test_zoom_workspace_size():
    L, lib = _lib()
    ws = lib.gd_zoom_axis_ws_bytes
    assert ws(3, 10, 7, 0, 0) == 0 and ws(3, 10, 7, 1, 1) == 0
    assert ws(3, 10, 7, 3, L.ZOOM_MIRROR) == 3 * 10 * 7 * 8
    assert ws(3, 10, 7, 3, L.ZOOM_NEAREST) == 3 * (10 + 24) * 7 * 8       # 12 edge samples on either side
    assert ws(3, 0, 7, 3, 0) == 0 and ws(3, 10, 7, 2, 0) == 0


def test_spline_argument_errors_before_any_launch():
    """negative code + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses)
    are not touched"""
    L, lib = _lib()
    p, q, r, s = 0x1000, 0x2000, 0x3000, 0x4000
    big = 1 << 20

    def bad(rc, word):
        assert rc < 0, rc
        assert word in L.last_error(), L.last_error()

    z = lib.gd_zoom_axis
    bad(z(None, q, 0, 0, 2, 10, 20, 3, 1, 0, None, 0, None), "null")
    bad(z(p, None, 0, 0, 2, 10, 20, 3, 1, 0, None, 0, None), "null")
    bad(z(p, p, 0, 0, 2, 10, 20, 3, 1, 0, None, 0, None), "src == dst")
    bad(z(p, q, 0, 0, 2, 0, 20, 3, 1, 0, None, 0, None), "L <= 0")
    bad(z(p, q, 0, 0, 2, -4, 20, 3, 1, 0, None, 0, None), "L <= 0")
    bad(z(p, q, 0, 0, 0, 10, 20, 3, 1, 0, None, 0, None), "<= 0")
    bad(z(p, q, 0, 0, 2, 10, 20, 0, 1, 0, None, 0, None), "<= 0")
    bad(z(p, q, 0, 0, 2, 10, 0, 3, 1, 0, None, 0, None), "Lout <= 0")
    bad(z(p, q, 0, 0, 2, 10, -1, 3, 1, 0, None, 0, None), "Lout <= 0")
    for order in (2, 4, 5, -1):
        bad(z(p, q, 0, 0, 2, 10, 20, 3, order, 0, r, big, None), "order")
    bad(z(p, q, 0, 0, 2, 10, 20, 3, 3, 2, r, big, None), "mode")
    bad(z(p, q, 0, 0, 2, 10, 20, 3, 1, -1, None, 0, None), "mode")
    bad(z(p, q, 2, 0, 2, 10, 20, 3, 1, 0, None, 0, None), "dtype")
    bad(z(p, q, 0, -1, 2, 10, 20, 3, 1, 0, None, 0, None), "dtype")
    bad(z(p + 4, q, 1, 0, 2, 10, 20, 3, 1, 0, None, 0, None), "aligned")
    bad(z(p, q + 4, 0, 1, 2, 10, 20, 3, 1, 0, None, 0, None), "aligned")
    need = lib.gd_zoom_axis_ws_bytes(2, 10, 3, 3, 0)
    bad(z(p, q, 0, 0, 2, 10, 20, 3, 3, 0, None, need, None), "null")              # order 3 without a workspace
    bad(z(p, q, 0, 0, 2, 10, 20, 3, 3, 0, r, need - 1, None), "workspace smaller")
    bad(z(p, q, 0, 0, 2, 10, 20, 3, 3, 1, r, need, None), "workspace smaller")     # 'nearest' needs the padded lines
    bad(z(p, q, 0, 0, 2, 10, 20, 3, 3, 0, r + 4, need, None), "workspace")

    f = lib.gd_spline_prefilter_axis
    bad(f(None, q, 0, 2, 10, 3, None), "null")
    bad(f(p, None, 0, 2, 10, 3, None), "null")
    bad(f(p, p, 1, 2, 10, 3, None), "src == dst")
    bad(f(p, q, 3, 2, 10, 3, None), "dtype")
    bad(f(p, q, 0, 2, 0, 3, None), "L <= 0")
    bad(f(p, q, 0, 0, 10, 3, None), "<= 0")
    bad(f(p, q + 4, 0, 2, 10, 3, None), "aligned")

    u = lib.gd_restore_units
    bad(u(None, 0, q, 0, r, 3, 10, 1.0, 0.0, 1.0, s, 1, None), "null")
    bad(u(p, 0, q, 0, r, 3, 10, 1.0, 0.0, 1.0, None, 1, None), "null")
    bad(u(p, 2, q, 0, r, 3, 10, 1.0, 0.0, 1.0, s, 1, None), "dtype")
    bad(u(p, 0, q, 5, r, 3, 10, 1.0, 0.0, 1.0, s, 1, None), "dtype")
    bad(u(p, 0, q, 0, r, 3, 10, 1.0, 0.0, 1.0, s, -1, None), "dtype")
    bad(u(p, 0, q, 0, r, 0, 10, 1.0, 0.0, 1.0, s, 1, None), "n <= 0")
    bad(u(p, 0, q, 0, r, 3, 0, 1.0, 0.0, 1.0, s, 1, None), "n <= 0")
    bad(u(p, 0, q, 0, r, 3, 10, 1.0, 0.0, 1.0, p, 1, None), "aliases x")           # fp32 x, fp64 dst, same address
    bad(u(p, 0, q, 0, r, 3, 10, 1.0, 0.0, 1.0, q, 0, None), "aliases trend")
    bad(u(p + 4, 1, q, 0, r, 3, 10, 1.0, 0.0, 1.0, s, 1, None), "aligned")

    m = lib.gd_masked_plane_mean_f64
    need = lib.gd_masked_plane_mean_f64_ws_bytes(3, 10)
    assert need > 0
    bad(m(None, 3, 10, None, q, r, s, need, None), "null")
    bad(m(p, 3, 10, None, q, r, None, need, None), "null")
    bad(m(p, 0, 10, None, q, r, s, need, None), "n <= 0")
    bad(m(p, 70000, 10, None, q, r, s, 1 << 30, None), "65535")
    bad(m(p, 3, 10, None, q, r, s, need - 1, None), "workspace smaller")
    bad(m(p + 4, 3, 10, None, q, r, s, need, None), "aligned")


def test_output_shape_rule():
    """int(round(n * f)) with Python's round: halves go to even"""
    from gan_danet_amd import spline
    assert spline.output_shape((10,), 0.25) == (2,)                  # 2.5 -> 2
    assert spline.output_shape((14,), 0.25) == (4,)                  # 3.5 -> 4
    assert spline.output_shape((6,), 0.25) == (2,)                   # 1.5 -> 2
    assert spline.output_shape((5, 8, 9), (1, 5, 5)) == (5, 40, 45)
    assert spline.output_shape((5, 16, 20), (1, 1.25, 1.25)) == (5, 20, 25)
    assert spline.output_shape((6, 30, 25), (1, 0.4, 0.4)) == (6, 12, 10)
    assert spline.output_shape((30, 20, 5), (0.1, 0.1, 1)) == (3, 2, 5)
    assert spline.output_shape((4, 3), 0.25) == (1, 1)
    for shape, f in (((10,), 0.25), ((7, 9), (1.5, 0.5)), ((4, 3), 0.25), ((18, 8, 9), (1, 5, 5))):
        assert spline.output_shape(shape, f) == ndi.zoom(np.zeros(shape), f, order=0).shape
    with pytest.raises(ValueError):
        spline.output_shape((4, 5), (2, 2, 2))


def test_unsupported_arguments_raise_value_error():
    """before the tensor is looked at: a CPU tensor reaches the ValueError, not the device check"""
    from gan_danet_amd import spline
    x = torch.zeros(4, 5)
    for order in (2, 4, 5, -1, 1.5):
        with pytest.raises(ValueError):
            spline.zoom(x, 2, order=order)
    for mode in ("reflect", "wrap", "grid-constant", "grid-mirror", "grid-wrap", "nonsense"):
        with pytest.raises(ValueError):
            spline.zoom(x, 2, mode=mode)
    with pytest.raises(ValueError):
        spline.zoom(x, 2, cval=1.0)
    with pytest.raises(ValueError):
        spline.zoom(x, 2, grid_mode=True)
    with pytest.raises(ValueError):
        spline.zoom(x, 2, prefilter=False)
    with pytest.raises(ValueError):
        spline.zoom(x, (2, 2, 2))


def test_cpu_tensors_are_refused():
    import gan_danet_amd
    from gan_danet_amd import _lib as L
    from gan_danet_amd import inference, spline
    assert gan_danet_amd.spline is spline
    x = torch.zeros(3, 4, 6)
    calls = [lambda: spline.zoom(x, 2), lambda: spline.zoom(x, (1, 2, 2), order=0, mode="nearest"),
             lambda: spline.zoom(x.double(), 2, order=1), lambda: spline.spline_filter(x),
             lambda: inference.restore_units(x), lambda: inference.restore_units(x, x, 2.0, 1.0, 10.0),
             lambda: inference.zoom_mask(x[0], 5), lambda: inference.assemble_product(x, x, 1.0, 0.0, trend_zoom=1)]
    for call in calls:
        with pytest.raises(L.GandanetError):
            call()
