"""Device filters (gan_danet_amd/filters.py, csrc/filters.hip) against scipy on the CPU, and the dataset's ``smoothing=``
hook.  The kernels sum in fp64 and round once per pass, as scipy does, so the bounds are bounds on rounding order:

  Gaussian fp32   (k + 1) * 2^-23 * max|x| for k passes: every pass is a convex combination rounded once
  Gaussian fp64   k * (2 * radius + 2) * 2^-52 * max|x|
  Savitzky-Golay  2^-22 * A * max|x|, A = the largest absolute row sum of the coefficient tables
  median          exact
  fill_masked     the Gaussian bounds times 4 / d_min (a quotient of two smoothed fields, the divisor >= d_min)

Each test prints its measured maximum error before it asserts."""
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import scipy.signal
import torch

from gpu_util import DEV

pytestmark = pytest.mark.gpu


def _rand(shape, seed, dtype=np.float32):
    return (np.random.RandomState(seed).randn(*shape) * 3.0 + 1.0).astype(dtype)


def _dev(x):
    return torch.from_numpy(x).to(DEV)


def _run(fn, xd):
    """fn(xd) with the input checked bitwise untouched and the result a new tensor"""
    keep = xd.clone()
    out = fn(xd)
    assert torch.equal(xd, keep), "the input tensor was modified"
    assert out.data_ptr() != xd.data_ptr() and out.shape == xd.shape and out.dtype == xd.dtype
    return out.cpu().numpy()


def _passes(x, sigma, axes):
    axes = tuple(range(x.ndim)) if axes is None else axes
    sig = [sigma] * len(axes) if np.isscalar(sigma) else list(sigma)
    return sum(1 for s in sig if s > 1e-15), max([int(4.0 * s + 0.5) for s in sig] + [0])


GAUSS_F32 = {
    "multi_fold_reflection": ((5, 9, 7, 3), 2, None),            # radius 8 against lengths 5, 7 and 3
    "tiny_axes": ((4, 3, 2, 5), 2, None),
    "both_paths_off_tile": ((2, 3, 70, 130), 3, (2, 3)),         # inner = 130 and inner = 1; off every multiple of 4 and 64
    "identity_axes_and_long_row": ((1, 1, 1, 300), 3, None),     # L = 1 three times, then a 300-element row
    "skipped_axes": ((3, 5, 4, 6), (0, 2, 0, 1.5), None),
    "three_lds_segments": ((2, 2100), 3, (1,)),                  # a row longer than two 1024-element LDS segments
    "vector_columns_only": ((3, 37, 8), 3, (1,)),                # inner = 8: the 16-byte instance alone
    "scalar_columns_only": ((3, 37, 6), 3, (1,)),                # inner = 6: no whole vectors per row
    "radius_64": ((2, 40, 5), 16, (1,)),                         # the largest radius, folding around L = 40
}


@pytest.mark.parametrize("case", sorted(GAUSS_F32))
def test_gaussian_fp32(case):
    from gan_danet_amd import filters
    shape, sigma, axes = GAUSS_F32[case]
    x = _rand(shape, 11)
    want = ndi.gaussian_filter(x, sigma, axes=axes)
    got = _run(lambda t: filters.gaussian_filter(t, sigma, axes=axes), _dev(x))
    k, _ = _passes(x, sigma, axes)
    err, tol = np.abs(got.astype(np.float64) - want).max(), (k + 1) * 2.0 ** -23 * np.abs(x).max()
    print(f"gaussian fp32 {case} {shape}: max err {err:.3e}, bound {tol:.3e} ({k} passes)")
    assert err <= tol


def test_gaussian_fp32_base_pointer_off_by_one_element():
    """a contiguous view that starts one element into a larger buffer, through the public call: its first pass reads the
    offset view and writes a fresh (16-byte aligned) temporary, so source and destination disagree about their offset and
    every column goes through the scalar instance; the later passes run between aligned temporaries.  The 16-byte body
    with a scalar head and tail is reached when both share a non-zero offset: test_correlate_shared_offset below"""
    from gan_danet_amd import filters
    shape = (2, 3, 8, 12)
    x = _rand(shape, 12)
    buf = torch.zeros(x.size + 5, device=DEV)
    xd = buf[1:1 + x.size].view(shape)
    xd.copy_(torch.from_numpy(x))
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    want = ndi.gaussian_filter(x, 2)
    got = _run(lambda t: filters.gaussian_filter(t, 2), xd)
    assert torch.count_nonzero(buf[:1]) == 0 and torch.count_nonzero(buf[1 + x.size:]) == 0
    err, tol = np.abs(got.astype(np.float64) - want).max(), 5 * 2.0 ** -23 * np.abs(x).max()
    print(f"gaussian fp32 offset base {shape}: max err {err:.3e}, bound {tol:.3e}")
    assert err <= tol


def _sliced(x, off, fill=77.0):
    """x copied `off` elements into a larger device buffer filled with a sentinel: (buffer, contiguous view)"""
    buf = torch.full((x.size + off + 7,), fill, dtype=torch.from_numpy(x).dtype, device=DEV)
    view = buf[off:off + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    return buf, view


SHARED_OFFSET = [
    (np.float32, 1, (3, 9, 24), 1),       # 4 mod 16: head of 3 columns, 5 vectors, tail of 1
    (np.float32, 3, (3, 9, 24), 1),       # 12 mod 16: head 1, 5 vectors, tail 3
    (np.float32, 2, (2, 5, 4, 8), 1),     # 8 mod 16, inner = 32: head 2, 7 vectors, tail 2
    (np.float64, 1, (3, 9, 24), 1),       # fp64 at 8 mod 16: head 1, 11 vectors, tail 1
    (np.float32, 1, (3, 9, 4), 1),        # inner = 4: head 3, no whole vector, tail 1
    (np.float32, 1, (5, 37), 1),          # inner == 1: rows of 37 start at every offset from a 16-byte boundary
    (np.float64, 1, (4, 1101), 1),        # the same in fp64, two LDS segments
]


@pytest.mark.parametrize("dtype,off,shape,axis", SHARED_OFFSET)
def test_correlate_shared_offset(dtype, off, shape, axis):
    """gd_correlate1d_axis with src AND dst sliced the same number of elements into larger buffers: for inner > 1 the
    16-byte instance takes the aligned body (columns from `head` on) and the scalar instance the head and tail columns
    through its column remap; for inner == 1 rows start on and off 16-byte boundaries.  Against scipy, and with the
    elements around dst untouched"""
    from gan_danet_amd import kern as K
    x = _rand(shape, 21, dtype)
    es = x.itemsize
    _, src = _sliced(x, off)
    dbuf, dst = _sliced(np.zeros_like(x), off)
    assert src.data_ptr() % 16 == (off * es) % 16 != 0 and dst.data_ptr() % 16 == src.data_ptr() % 16
    keep = src.clone()
    w, radius = K.gaussian_weights_host(2.0)
    K.correlate1d_axis(src, dst, axis, w, radius)
    torch.cuda.synchronize()
    assert torch.equal(src, keep)
    assert bool((dbuf[:off] == 77.0).all()) and bool((dbuf[off + x.size:] == 77.0).all()), "wrote outside dst"
    want = ndi.correlate1d(x, np.array(w[:2 * radius + 1]), axis=axis, mode="reflect")
    err = np.abs(dst.cpu().numpy().astype(np.float64) - want).max()
    tol = (2 * 2.0 ** -23 if dtype == np.float32 else (2 * radius + 2) * 2.0 ** -52) * np.abs(x).max()
    print(f"correlate shared offset {np.dtype(dtype).name} +{off} {shape}: max err {err:.3e}, bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("shape", [(5, 9, 7, 3), (4, 3, 2, 5)])
def test_gaussian_fp64(shape):
    from gan_danet_amd import filters
    x = _rand(shape, 13, np.float64)
    want = ndi.gaussian_filter(x, 2)
    got = _run(lambda t: filters.gaussian_filter(t, 2), _dev(x))
    k, radius = _passes(x, 2, None)
    err, tol = np.abs(got - want).max(), k * (2 * radius + 2) * 2.0 ** -52 * np.abs(x).max()
    print(f"gaussian fp64 {shape}: max err {err:.3e}, bound {tol:.3e}")
    assert err <= tol


SAVGOL = [((3, 4, 6, 9), 5, 2, -1), ((2, 7, 5, 6), 5, 2, 1), ((2, 5), 5, 2, -1), ((3, 300), 11, 3, -1)]


@pytest.mark.parametrize("shape,window,order,axis", SAVGOL)
def test_savgol_fp32(shape, window, order, axis):
    from gan_danet_amd import filters
    x = _rand(shape, 14)
    want = scipy.signal.savgol_filter(x, window, order, axis=axis)
    got = _run(lambda t: filters.savgol_filter(t, window, order, axis=axis), _dev(x))
    coeffs, edges = filters.savgol_tables(window, order)
    a = max(np.abs(coeffs).sum(), np.abs(edges).sum(axis=-1).max())
    err, tol = np.abs(got.astype(np.float64) - want).max(), 2.0 ** -22 * a * np.abs(x).max()
    print(f"savgol fp32 {shape} ({window}, {order}) axis {axis}: max err {err:.3e}, bound {tol:.3e} (A = {a:.3f})")
    assert err <= tol


def test_savgol_value_errors_as_scipy():
    from gan_danet_amd import filters
    xd = _dev(_rand((2, 4), 15))
    for args in ((4, 2), (5, 5), (5, 2)):                        # even window, polyorder >= window, window > L = 4
        with pytest.raises(ValueError):
            filters.savgol_filter(xd, *args)


MEDIAN = [((3, 4, 5, 2), 3, None), ((2, 2, 37, 70), 3, (2, 3)), ((1, 1, 9, 11), 5, (2, 3)), ((2, 6, 7, 5), 3, (1, 2, 3))]


def _median_ref(x, size, axes):
    full = [1] * x.ndim
    for a in (range(x.ndim) if axes is None else axes):
        full[a] = size
    return ndi.median_filter(x, size=tuple(full))


@pytest.mark.parametrize("shape,size,axes", MEDIAN)
@pytest.mark.parametrize("data", ["continuous", "ties"])
def test_median_fp32(shape, size, axes, data):
    from gan_danet_amd import filters
    rs = np.random.RandomState(16)
    x = _rand(shape, 16) if data == "continuous" else rs.randint(-2, 3, size=shape).astype(np.float32)
    got = _run(lambda t: filters.median_filter(t, size, axes=axes), _dev(x))
    want = _median_ref(x, size, axes)
    print(f"median fp32 {shape} size {size} axes {axes} {data}: {int((got != want).sum())} of {x.size} differ")
    assert np.array_equal(got, want)


def test_median_fp64_and_one_axis():
    from gan_danet_amd import filters
    x = _rand((3, 4, 5, 2), 17, np.float64)
    assert np.array_equal(_run(lambda t: filters.median_filter(t, 3), _dev(x)), ndi.median_filter(x, size=3))
    y = _rand((4, 5, 23), 18)                                   # counts 3 and 5 along one axis, leading dims merged
    assert np.array_equal(_run(lambda t: filters.median_filter(t, 3, axes=(2,)), _dev(y)), ndi.median_filter(y, size=(1, 1, 3)))
    assert np.array_equal(_run(lambda t: filters.median_filter(t, 5, axes=(1,)), _dev(y)), ndi.median_filter(y, size=(1, 5, 1)))


@pytest.fixture(scope="module")
def fill_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "fill_nearest_6x20x18x2.npz"))
    fx = {k: z[k] for k in z.files}
    assert float(fx["d_min"]) >= 0.5                             # the condition the tolerance below rests on
    return fx


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fill_masked_against_the_reference_fixture(fill_fixture, dtype):
    from gan_danet_amd import filters
    x, want, d_min = fill_fixture["input"], fill_fixture["output"], float(fill_fixture["d_min"])
    ph, sigma = float(fill_fixture["placeholder"]), float(fill_fixture["sigma"])
    gaps = x <= ph
    k, radius, xmax = 3, int(4.0 * sigma + 0.5), np.abs(x[~gaps]).max()
    tol = (4 * k * (2 * radius + 2) * 2.0 ** -52 if dtype == np.float64 else 4 * (k + 1) * 2.0 ** -23) * xmax / d_min
    for v in range(x.shape[-1]):                                  # per variable, as the reference's loop
        xv = np.ascontiguousarray(x[..., v]).astype(dtype)
        got = _run(lambda t: filters.fill_masked(t, placeholder=ph, sigma=sigma, axes=(0, 1, 2)), _dev(xv))
        g = gaps[..., v]
        err = np.abs(got.astype(np.float64)[g] - want[..., v][g]).max()
        print(f"fill_masked {np.dtype(dtype).name} variable {v}: {int(g.sum())} gaps, max err {err:.3e}, bound {tol:.3e}")
        assert got.dtype == dtype and np.array_equal(got[~g], xv[~g])      # non-gap points bit for bit
        assert err <= tol


def _dataset_arrays(c=3):
    rs = np.random.RandomState(19)
    return (rs.randn(5, 4, 3).astype(np.float32), rs.randn(5, 9, 7).astype(np.float32),
            (rs.randn(5, 9, 7, c) * 2.0).astype(np.float32))


def test_dataset_smoothing_hook():
    from gan_danet_amd import filters
    from gan_danet_amd.data import DeviceTileDataset
    a, b, aux = _dataset_arrays()
    plain = DeviceTileDataset(a, b, aux)
    stored = torch.from_numpy(aux).to(DEV).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(plain.hr_aux, stored)
    assert torch.equal(DeviceTileDataset(a, b, aux, smoothing=None).hr_aux, stored)

    nchw = lambda arr: np.ascontiguousarray(arr.transpose(0, 3, 1, 2))
    ds = DeviceTileDataset(a, b, aux, smoothing="gaussian")
    want = nchw(ndi.gaussian_filter(aux, 2))
    err, tol = np.abs(ds.hr_aux.cpu().numpy().astype(np.float64) - want).max(), 5 * 2.0 ** -23 * np.abs(aux).max()
    print(f"dataset gaussian: max err {err:.3e}, bound {tol:.3e}")
    assert ds.hr_aux.shape == stored.shape and ds.hr_aux.is_contiguous() and err <= tol
    assert torch.equal(ds.lr_grace_05, plain.lr_grace_05) and torch.equal(ds.lr_grace_025, plain.lr_grace_025)

    ds = DeviceTileDataset(a, b, aux, smoothing="median")
    assert np.array_equal(ds.hr_aux.cpu().numpy(), nchw(ndi.median_filter(aux, size=3)))

    # the notebook's savgol_filter(data, 5, 2) runs along the channel axis and needs at least 5 channels: scipy raises on
    # the 3-channel array above, and so does the hook; the reference's hr_aux has more than five
    with pytest.raises(ValueError):
        scipy.signal.savgol_filter(aux, 5, 2)
    with pytest.raises(ValueError):
        DeviceTileDataset(a, b, aux, smoothing="savgol")
    a6, b6, aux6 = _dataset_arrays(c=6)
    ds = DeviceTileDataset(a6, b6, aux6, smoothing="savgol")
    coeffs, edges = filters.savgol_tables(5, 2)
    amax = max(np.abs(coeffs).sum(), np.abs(edges).sum(axis=-1).max())
    err = np.abs(ds.hr_aux.cpu().numpy().astype(np.float64) - nchw(scipy.signal.savgol_filter(aux6, 5, 2))).max()
    tol = 2.0 ** -22 * amax * np.abs(aux6).max()
    print(f"dataset savgol: max err {err:.3e}, bound {tol:.3e}")
    assert err <= tol

    calls = []

    def once(t):
        calls.append(tuple(t.shape))
        return t * 2.0

    ds = DeviceTileDataset(a, b, aux, smoothing=once)
    assert calls == [(5, 3, 9, 7)] and torch.equal(ds.hr_aux, stored * 2.0)
    _, _, c0 = ds.get(0, 2)
    assert torch.equal(c0, stored[:2] * 2.0)
