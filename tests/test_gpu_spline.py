"""Device spline zoom (gan_danet_amd/spline.py, csrc/spline.hip) and the inference product assembly against scipy and
numpy on the CPU.

The kernels compute in fp64 with scipy's formulas, so the bounds are bounds on rounding order, from the operation count.
Write e = 2^-52, M = max|x| entering an axis.

  order 0          exact: samples are copied
  order 1          4 e M per axis: 1 - t, two products and a sum round (t itself is the same number on both sides: the
                   coordinate is one IEEE product), on each of the two sides compared; the result is a convex combination,
                   so M does not grow
  order 3          48 e M per axis.  The prefilter scales by 6 and runs c+[i] = 6 x[i] + z c+[i-1] (|c+| <= 6 M / (1 - |z|) =
                   8.2 M; three roundings per step, summed along the recursion with 1 / (1 - |z|) = 1.37: 17 e M), then
                   c[i] = z (c[i+1] - c+[i]) (passes the causal error on with |z| / (1 - |z|) = 0.37 and adds two roundings on
                   |.| <= 10 M: 10 e M in all); the four weights take about 6 operations each and the sum four products:
                   12 roundings on |c| <= sqrt(3) M (the prefilter's gain): 10 e M.  About 21 e M a side when every rounding
                   is taken at half an ulp, 42 e M for two sides; 48 leaves room for the boundary sums.  M grows by sqrt(3)
                   per order-3 axis, and so does an error that enters it.
  chunking         a chunk's warm start leaves z^40 * 8.2 M = 1e-22 M, and the truncated boundary sums z^65: nothing
  fp32 input       ulp32(want) + the fp64 bound: both sides round one fp64 value once

The numpy restatement of these rules is 4.9e-15 from scipy on N(0, 1) data (two order-3 axes); the bound for that case is
2 * 48 e * sqrt(3) * 5 = 1.8e-13.  Each test prints its measured maximum error next to its bound before it asserts.

scipy's mode='constant' returns cval where rounding lifts the last coordinate (n_out - 1) * ((n - 1) / (n_out - 1)) above
n - 1 (n = 63 at factor 5, for one); the project treats 'constant' as 'mirror' there (test_constant_last_coordinate).
The 'constant' cases below are scipy's own result: none of them has such a coordinate, which _zoom_ref checks."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from gpu_util import DEV

pytestmark = pytest.mark.gpu

E = 2.0 ** -52
SQRT3 = np.sqrt(3.0)


def _rand(shape, seed, dtype=np.float64):
    return (np.random.RandomState(seed).randn(*shape) * 3.0 + 1.0).astype(dtype)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _factors(shape, zoom):
    return [float(zoom)] * len(shape) if np.isscalar(zoom) else [float(f) for f in zoom]


def _bound(x, zoom, order):
    """the rounding-order bound of the module docstring for the axes this call zooms"""
    mag, err = float(np.abs(x).max()), 0.0
    for f in _factors(x.shape, zoom):
        if f == 1.0 or order == 0:
            continue
        if order == 1:
            err += 4 * E * mag
        else:
            err = SQRT3 * err + 48 * E * mag
            mag *= SQRT3
    return err


def _overshoots(shape, zoom):
    for n, f in zip(shape, _factors(shape, zoom)):
        no = int(round(n * f))
        if no > 1 and (no - 1) * ((n - 1) / (no - 1)) > n - 1:
            return True
    return False


def _zoom_ref(x, zoom, order, mode):
    assert mode != "constant" or not _overshoots(x.shape, zoom), "pick another length: scipy returns cval here"
    return ndi.zoom(x.astype(np.float64), zoom, order=order, mode=mode)


def _check(x, zoom, order, mode, what, xd=None):
    from gan_danet_amd import spline
    xd = _dev(x) if xd is None else xd
    keep = xd.clone()
    got_t = spline.zoom(xd, zoom, order=order, mode=mode)
    assert torch.equal(xd, keep), "the input tensor was modified"
    assert got_t.dtype == xd.dtype and got_t.data_ptr() != xd.data_ptr() and got_t.is_contiguous()
    got = got_t.cpu().numpy()
    want = _zoom_ref(x, zoom, order, mode)                             # fp64 whatever x is: rounded below
    assert got.shape == want.shape, (got.shape, want.shape)
    tol = _bound(x, zoom, order)
    if order == 0:
        assert np.array_equal(got, want.astype(x.dtype)), f"{what}: order 0 is not bit-equal"
        print(f"zoom {what} {x.shape} x {zoom} order 0 {mode}: bit-equal")
        return
    err = np.abs(got.astype(np.float64) - want)
    if x.dtype == np.float32:
        slack = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + tol
        print(f"zoom {what} {x.shape} x {zoom} order {order} {mode} fp32: max err {err.max():.3e}, "
              f"max (err - ulp32) {np.max(err - slack + tol):.3e}, fp64 bound {tol:.3e}")
        assert np.all(err <= slack)
    else:
        print(f"zoom {what} {x.shape} x {zoom} order {order} {mode} fp64: max err {err.max():.3e}, bound {tol:.3e}")
        assert err.max() <= tol


# the reference's calls at reduced size
REFERENCE_CALLS = {
    "trend_5x_cubic": ((5, 8, 9), (1, 5, 5), 3, "constant"),
    "bias_1p25_cubic": ((5, 16, 20), (1, 1.25, 1.25), 3, "constant"),
    "uncertainty_5x_order0_nearest": ((4, 8, 9), (1, 5, 5), 0, "nearest"),
    "mask_5x_linear": ((8, 9), (5, 5), 1, "constant"),
    "mask_2x_linear": ((8, 9), (2, 2), 1, "constant"),
    "aux_0p4_cubic_nearest": ((6, 30, 25), (1, 0.4, 0.4), 3, "nearest"),
    "aux_0p1_cubic_nearest": ((30, 20, 5), (0.1, 0.1, 1), 3, "nearest"),
    "length_one_axis": ((3, 1, 7), (1, 1, 2), 3, "constant"),
    "to_one_sample": ((4, 3), 0.25, 3, "constant"),                   # every n_out is 1
    "to_one_sample_nearest": ((4, 5), 0.25, 3, "nearest"),
    "half_even_shape": ((10, 6), 0.25, 1, "constant"),                # 2.5 -> 2, 1.5 -> 2
}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", sorted(REFERENCE_CALLS))
def test_reference_calls(case, dtype):
    shape, zoom, order, mode = REFERENCE_CALLS[case]
    _check(_rand(shape, 31, dtype), zoom, order, mode, case)


# line lengths: 1 .. 4; 13 (just over the 12-sample pad); the horizon (40, 41); the boundary sum's 64 terms (65, 66) and
# its short-line rule (96, 97); inner > 1 cuts a line into chunks of 64 (63, 64, 65, 129); inner == 1 into chunks of 9
# (8, 9, 10, 19).  In 'nearest' mode the filtered line is 24 longer: 39, 40, 41 and 105 put it at 63, 64, 65 and 129.
LENGTHS = (1, 2, 3, 4, 8, 9, 10, 13, 19, 39, 40, 41, 63, 64, 65, 66, 96, 97, 105, 129)


@pytest.mark.parametrize("mode", ["mirror", "nearest"])
@pytest.mark.parametrize("outer,inner", [(1, 1), (5, 1), (5, 3), (1, 4), (5, 4), (5, 7)])
def test_cubic_line_lengths(outer, inner, mode):
    """every length above through the inner == 1 kernel (rows in LDS) and the inner > 1 kernel, fp64, factor 2 along the
    line; one scipy call and one device call per length"""
    for n in LENGTHS:
        _check(_rand((outer, n, inner), 100 + n), (1, 2, 1), 3, mode, f"L={n}")


@pytest.mark.parametrize("n", [2303, 2304, 2305, 4609])
def test_cubic_row_segments(n):
    """inner == 1: a workgroup takes a segment of 256 * 9 = 2304 samples of a row; one below, equal, one above, two
    segments plus one.  Two rows, fp32 in and out"""
    _check(_rand((2, n), n, np.float32), (1, 1.5), 3, "mirror", f"row L={n}")


@pytest.mark.parametrize("order,mode", [(0, "nearest"), (1, "constant"), (3, "constant"), (3, "nearest")])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_base_pointer_off_by_one_element(dtype, order, mode):
    """a contiguous view that starts one element into a larger buffer (8 mod 16 in fp64, 4 mod 16 in fp32), zoomed
    along both axes, so that the inner > 1 and the inner == 1 kernels both read it or what follows it"""
    from gan_danet_amd import spline  # noqa: F401
    shape = (3, 9, 14)
    x = _rand(shape, 41, dtype)
    buf = torch.zeros(x.size + 5, device=DEV, dtype=torch.from_numpy(x).dtype)
    xd = buf[1:1 + x.size].view(shape)
    xd.copy_(torch.from_numpy(x))
    assert xd.is_contiguous() and xd.data_ptr() % 16 == x.itemsize
    _check(x, (1, 2, 3), order, mode, "offset base", xd=xd)
    assert torch.count_nonzero(buf[:1]) == 0 and torch.count_nonzero(buf[1 + x.size:]) == 0


def test_constant_last_coordinate():
    """63 -> 315: 314 * (62 / 314) rounds to just above 62, where scipy's 'constant' returns cval for the last sample.  The
    project's 'constant' is 'mirror' there too, and everywhere else the two scipy modes agree"""
    from gan_danet_amd import spline
    x = _rand((63,), 5)
    assert _overshoots(x.shape, 5)
    got = spline.zoom(_dev(x), 5, order=3, mode="constant").cpu().numpy()
    want = ndi.zoom(x, 5, order=3, mode="mirror")
    assert np.array_equal(ndi.zoom(x, 5, order=3, mode="constant")[:-1], want[:-1])
    err, tol = np.abs(got - want).max(), _bound(x, 5, 3)
    print(f"zoom 63 x 5 'constant' against scipy 'mirror': max err {err:.3e}, bound {tol:.3e}")
    assert err <= tol


def test_unit_factors_copy():
    from gan_danet_amd import spline
    xd = _dev(_rand((3, 4, 5), 6, np.float32))
    out = spline.zoom(xd, 1, order=3)
    assert torch.equal(out, xd) and out.data_ptr() != xd.data_ptr()
    out = spline.zoom(xd, (1, 1.0, 1), order=0, mode="nearest")
    assert torch.equal(out, xd) and out.data_ptr() != xd.data_ptr()


@pytest.mark.parametrize("shape,axes", [((5, 9, 7), None), ((3, 70, 4), (1,)), ((6, 130), (1,)), ((4, 1, 5), None),
                                        ((2, 2305), (-1,))])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_spline_filter(shape, axes, dtype):
    """against scipy.ndimage.spline_filter(mode='mirror', output=float64): the prefilter's share of the order-3 bound,
    taken whole (48 e M per axis, growing by sqrt(3))"""
    from gan_danet_amd import spline
    x = _rand(shape, 51, dtype)
    xd = _dev(x)
    got_t = spline.spline_filter(xd, axes=axes)
    assert got_t.dtype == torch.float64 and got_t.shape == xd.shape
    want = x.astype(np.float64)
    todo = range(x.ndim) if axes is None else [a % x.ndim for a in axes]
    tol, mag = 0.0, float(np.abs(x).max())
    for a in todo:
        want = ndi.spline_filter1d(want, 3, axis=a, output=np.float64, mode="mirror")
        tol, mag = SQRT3 * tol + 48 * E * mag, mag * SQRT3
    if axes is None:
        assert np.abs(want - ndi.spline_filter(x.astype(np.float64), 3, output=np.float64, mode="mirror")).max() <= tol
    err = np.abs(got_t.cpu().numpy() - want).max()
    print(f"spline_filter {np.dtype(dtype).name} {shape} axes {axes}: max err {err:.3e}, bound {tol:.3e}")
    assert err <= tol


# ---- restore_units ------------------------------------------------------------------------------------------------------
SCALE, MEAN, UNIT = 3.7182818284590453, -1.2345678901234567, 10.0


def _restore_np(x, trend, mask):
    v = x.astype(np.float64)
    if trend is not None:
        v = v + trend.astype(np.float64)
    v = ((v * SCALE) + MEAN) * UNIT
    if mask is not None:
        v[..., mask == 0] = np.nan
    return v


@pytest.mark.parametrize("xdt,tdt", [(np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32),
                                     (np.float32, np.float32)])
def test_restore_units_bit_equal(xdt, tdt):
    from gan_danet_amd import inference
    x, trend = _rand((5, 13, 17), 61, xdt), _rand((5, 13, 17), 62, tdt)
    mask = (np.random.RandomState(63).rand(13, 17) > 0.3).astype(np.uint8)
    mask[0, :] = 0
    xd, td, md = _dev(x), _dev(trend), _dev(mask)
    keep = xd.clone()
    for tr, trd, m, mdev in ((trend, td, mask, md), (trend, td, None, None), (None, None, mask, md), (None, None, None, None)):
        got = inference.restore_units(xd, trd, SCALE, MEAN, UNIT, mdev).cpu().numpy()
        want = _restore_np(x, tr, m)
        assert got.dtype == np.float64
        assert np.array_equal(np.isnan(got), np.isnan(want))
        if m is not None:
            assert np.array_equal(np.isnan(got), np.broadcast_to(m == 0, got.shape))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "fp64 output is not bit-equal to numpy"
    assert torch.equal(xd, keep)
    # fp32 output: the same fp64 value rounded once; a float-valued mask works like bytes
    got32 = inference.restore_units(xd, td, SCALE, MEAN, UNIT, md.float(), out_dtype=torch.float32).cpu().numpy()
    assert got32.dtype == np.float32
    assert np.array_equal(got32, _restore_np(x, trend, mask).astype(np.float32), equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restore_units_in_place(dtype):
    from gan_danet_amd import inference
    x, trend = _rand((4, 9, 11), 64, dtype), _rand((4, 9, 11), 65, np.float64)
    mask = (np.random.RandomState(66).rand(9, 11) > 0.5).astype(np.uint8)
    xd = _dev(x)
    ptr = xd.data_ptr()
    out = inference.restore_units(xd, _dev(trend), SCALE, MEAN, UNIT, _dev(mask), out=xd)
    assert out.data_ptr() == ptr and out.dtype == xd.dtype
    assert np.array_equal(out.cpu().numpy(), _restore_np(x, trend, mask).astype(dtype), equal_nan=True)


def test_restore_units_refuses_aliasing_across_dtypes():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import kern as K
    buf = torch.zeros(64, device=DEV, dtype=torch.float64)
    x32 = buf.view(torch.float32)[:64]
    with pytest.raises(L.GandanetError):
        K.restore_units(x32, None, None, 1.0, 0.0, 1.0, buf)


# ---- zoom_mask and assemble_product --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,factor", [((8, 9), (5, 5)), ((8, 9), (2, 2)), ((7, 11), 3)])
def test_zoom_mask(shape, factor):
    from gan_danet_amd import inference
    m = (np.random.RandomState(71).rand(*shape) > 0.4).astype(np.float64)
    m[2:5, 3:6] = 0.0                                                      # a hole wide enough to survive the zoom
    want = (ndi.zoom(m, factor, order=1) != 0)
    for md in (_dev(m), _dev(m.astype(np.float32)), _dev(m.astype(np.uint8))):
        got = inference.zoom_mask(md, factor)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy() != 0, want)
    assert (~want).any() and want.any()


def _assemble_np(res, trend25, scale, mean, mask, bias, unc):
    """the post-loop chain of the 0.05-degree script with numpy and scipy"""
    import warnings
    out = res.astype(np.float64) + ndi.zoom(trend25.astype(np.float64), (1, 5, 5), order=3)
    out = (out * scale + mean) * 10.0
    if mask is not None:
        out[:, mask == 0] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                    # 'Mean of empty slice'
        series = np.nanmean(out, axis=(1, 2))
    if bias is not None:
        out = out + ndi.zoom(bias.astype(np.float64), (1, 1.25, 1.25), order=3)
    u = None if unc is None else ndi.zoom(unc, (1, 5, 5), order=0, mode="nearest")
    return out, series, u


@pytest.mark.parametrize("full", [True, False])
def test_assemble_product(full):
    """(6, 8, 9) trend tiles -> a (6, 40, 45) product.  The tiles of time step 2 are NaN throughout (a step the loader
    could not fill), so its series entry is NaN; with the mask, row 0 and a block are outside"""
    from gan_danet_amd import inference
    res = _rand((6, 40, 45), 81, np.float32)
    res[2] = np.nan
    trend25 = _rand((6, 8, 9), 82)
    bias = _rand((6, 32, 36), 83) if full else None
    unc = np.abs(_rand((6, 8, 9), 84, np.float32)) if full else None
    mask = None
    if full:
        mask = np.ones((40, 45), np.uint8)
        mask[0, :] = 0
        mask[10:20, 30:] = 0
    out = inference.assemble_product(_dev(res), _dev(trend25), SCALE, MEAN, mask=None if mask is None else _dev(mask),
                                     bias=None if bias is None else _dev(bias),
                                     uncertainty=None if unc is None else _dev(unc))
    want, series, u = _assemble_np(res, trend25, SCALE, MEAN, mask, bias, unc)
    got, got_series = out["product"].cpu().numpy(), out["series"].cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape and got_series.shape == (6,)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got_series[2]) and np.array_equal(np.isnan(got_series), np.isnan(series))
    # the zoomed trend's error passes through * scale * 10, the bias's is added; the sums round at the product's size
    big = float(np.nanmax(np.abs(want)))
    tol = _bound(trend25, (1, 5, 5), 3) * abs(SCALE) * 10.0 + 8 * E * big
    if full:
        tol += _bound(bias, (1, 1.25, 1.25), 3)
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]).max()
    npix = int(mask.sum()) if full else 40 * 45
    # a mean of npix terms: the terms' own error, plus a summation order's worth of roundings on the partial sums
    tol_s = tol + npix * E * big
    err_s = np.nanmax(np.abs(got_series - series))
    print(f"assemble_product full={full}: product max err {err:.3e} (bound {tol:.3e}), series {err_s:.3e} (bound {tol_s:.3e})")
    assert err <= tol and err_s <= tol_s
    if full:
        assert out["uncertainty"].dtype == torch.float32
        assert np.array_equal(out["uncertainty"].cpu().numpy(), u)
    else:
        assert out["uncertainty"] is None
