"""Dataset preparation on the device (gan_danet_amd/prepare.py, csrc/prepare.hip) against sklearn, numpy and scipy on the
CPU and against outputs recorded from the reference's own ``frequency_domain_augmentation`` (tests/golden/prepare_*.npz).

  scaler fit        mean_ within 4 * 2^-52 * max|x|; var_ within 8 * 2^-52 * (var + mean^2): the bound of a compensated or
                    Welford fp64 sum, far tighter than a naive E[x^2] - E[x]^2 would meet on the cancellation case
  transform         fp64 -> fp64 bit-equal to numpy's (x - mean) / scale and x * scale + mean (the same two IEEE operations in
                    the same order); fp32 out = the fp64 result rounded once
  frequency augm.   2 r + (K1 + 2) * 2^-52 * max|want|, r = max|real(ifft(fft(x))) - x| the reference chain's own round trip
                    on the same input in the input's precision (+ 2^-24 * max|want| for the one rounding to fp32)

Each test prints its measured maximum error before it asserts."""
import os

import numpy as np
import pytest
import scipy.fft
import torch
from sklearn.preprocessing import StandardScaler

from gpu_util import DEV

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _offset_view(x, off):
    """x copied ``off`` elements into a larger device buffer: (buffer, contiguous view)"""
    buf = torch.full((x.size + off + 7,), 77.0, dtype=torch.from_numpy(x).dtype, device=DEV)
    view = buf[off:off + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    return buf, view


# ---- scaler fit -------------------------------------------------------------------------------------------------------
def _fit_data(case):
    rs = np.random.RandomState(31)
    if case == "c45_f64":
        return rs.randn(3, 4, 5, 45) * rs.uniform(0.1, 20.0, 45) + rs.uniform(-50.0, 50.0, 45), -1
    if case == "c45_f32":
        return (rs.randn(3, 4, 5, 45) * rs.uniform(0.1, 20.0, 45) + rs.uniform(-50.0, 50.0, 45)).astype(np.float32), -1
    if case == "single_feature":
        return rs.randn(2, 3, 3, 1) * 7.0 + 0.1, None
    if case == "one_row":
        return rs.randn(1, 1, 1, 7) * 3.0, -1
    if case == "several_blocks":
        return rs.randn(5000, 3) * np.array([1.0, 5.0, 0.2]) + np.array([0.0, 3.0, -1.0]), -1
    if case == "off_tile":
        return rs.randn(7, 2, 130, 5) * 2.0 + 1.0, -1
    if case == "constant_channel":
        x = rs.randn(6, 5, 7, 4)
        x[..., 1] = 3.25
        x[..., 3] = 0.0
        return x, -1
    if case == "cancellation":
        x = rs.randn(4, 30, 25, 3)
        x[..., 1] = 1e4 + 1e-3 * rs.randn(4, 30, 25)
        return x, -1
    if case == "wide_c300":
        return rs.randn(9, 5, 300) * 2.0 - 1.0, -1                  # more than one 256-channel column block
    raise KeyError(case)


FIT_CASES = ["c45_f64", "c45_f32", "single_feature", "one_row", "several_blocks", "off_tile", "constant_channel",
             "cancellation", "wide_c300"]


class _Ref:
    pass


def _per_channel(rows):
    """StandardScaler fitted on one channel at a time, each an (M, 1) array of its own, as load_data's loop does.  (One fit
    of the whole (M, C) array is not the yardstick: numpy reduces its axis 0 row by row, not pairwise, and the mean of a
    channel near 1e4 over 3000 rows then sits about 19 ulp from the exact one.)"""
    fits = [StandardScaler().fit(np.ascontiguousarray(rows[:, i]).reshape(-1, 1)) for i in range(rows.shape[1])]
    ref = _Ref()
    ref.mean_, ref.var_, ref.scale_ = (np.concatenate([getattr(f, a) for f in fits]) for a in ("mean_", "var_", "scale_"))
    return ref


def _check_fit(sc, x, channel_axis, what):
    c = 1 if channel_axis is None else x.shape[-1]
    rows = x.reshape(-1, c).astype(np.float64)
    ref = _per_channel(rows)
    e_mean = np.abs(sc.mean_ - ref.mean_)
    e_var = np.abs(sc.var_ - ref.var_)
    b_mean = 4 * EPS * np.abs(rows).max(axis=0)
    b_var = 8 * EPS * (ref.var_ + ref.mean_ ** 2)
    print(f"fit {what} {x.shape}: mean_ err / bound max {np.max(e_mean / np.maximum(b_mean, 1e-300)):.3f}, "
          f"var_ err / bound max {np.max(e_var / np.maximum(b_var, 1e-300)):.3f}, max |mean err| {e_mean.max():.3e}, "
          f"max |var err| {e_var.max():.3e}")
    assert sc.mean_.dtype == sc.var_.dtype == sc.scale_.dtype == np.float64 and sc.mean_.shape == (c,)
    assert sc.n_samples_seen_ == rows.shape[0]
    assert np.all(e_mean <= b_mean) and np.all(e_var <= b_var)
    const = ref.scale_ == 1.0
    assert np.array_equal(sc.scale_ == 1.0, const)
    # scale_ = sqrt(var_): the bound on var_ divided by 2 * scale_, plus the rounding of the square root
    assert np.all(np.abs(sc.scale_ - ref.scale_) <= b_var / (2 * ref.scale_) + 2 * EPS * ref.scale_)
    return ref


@pytest.mark.parametrize("case", FIT_CASES)
def test_scaler_fit(case):
    from gan_danet_amd import prepare
    x, axis = _fit_data(case)
    xd = _dev(x)
    keep = xd.clone()
    sc = prepare.ChannelScaler().fit(xd, channel_axis=axis)
    assert torch.equal(xd, keep)
    ref = _check_fit(sc, x, axis, case)
    if case == "constant_channel":
        assert sc.scale_[1] == 1.0 and sc.scale_[3] == 1.0 and sc.var_[1] == 0.0 and sc.mean_[1] == 3.25
    if case == "one_row":
        assert np.all(sc.scale_ == 1.0) and np.array_equal(sc.mean_, x.reshape(-1))
    if case == "cancellation":
        print(f"cancellation channel: var_ {sc.var_[1]:.17e} (sklearn {ref.var_[1]:.17e})")
    again = prepare.ChannelScaler().fit(xd, channel_axis=axis)        # bit-reproducible
    assert np.array_equal(sc.mean_, again.mean_) and np.array_equal(sc.var_, again.var_) and np.array_equal(sc.scale_, again.scale_)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_scaler_fit_base_pointer_off_by_one_element(dtype):
    from gan_danet_amd import prepare
    x = (np.random.RandomState(32).randn(5, 6, 7, 9) * 3.0 + 2.0).astype(dtype)
    _, xd = _offset_view(x, 1)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == x.itemsize
    sc = prepare.ChannelScaler().fit(xd)
    _check_fit(sc, x, -1, f"offset view {np.dtype(dtype).name}")


# ---- transform / inverse ----------------------------------------------------------------------------------------------
TRANSFORM_SHAPES = [(2, 5, 7, 45), (1, 70, 130, 3), (3, 1, 1, 1), (2, 9, 8, 70)]


@pytest.mark.parametrize("shape", TRANSFORM_SHAPES)
@pytest.mark.parametrize("in_dtype", [np.float64, np.float32])
def test_transform_and_inverse(shape, in_dtype):
    from gan_danet_amd import prepare
    rs = np.random.RandomState(33)
    c = shape[-1]
    x = (rs.randn(*shape) * rs.uniform(0.5, 9.0, c) + rs.uniform(-20.0, 20.0, c)).astype(in_dtype)
    xd = _dev(x)
    keep = xd.clone()
    sc = prepare.ChannelScaler().fit(xd)
    x64 = x.astype(np.float64)
    fwd = (x64 - sc.mean_) / sc.scale_                               # numpy: two IEEE operations, as sklearn's transform
    inv = x64 * sc.scale_ + sc.mean_
    nchw = lambda a: np.ascontiguousarray(a.transpose(0, 3, 1, 2))
    for out_dtype, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        got = sc.transform(xd, out_dtype=tdt)
        assert got.data_ptr() != xd.data_ptr() and got.dtype == tdt and got.is_contiguous()
        ne = int((got.cpu().numpy() != fwd.astype(out_dtype)).sum())
        got_t = sc.transform(xd, out_dtype=tdt, to_nchw=True)
        assert got_t.shape == (shape[0], c, shape[1], shape[2]) and got_t.is_contiguous() and got_t.dtype == tdt
        ne_t = int((got_t.cpu().numpy() != nchw(fwd).astype(out_dtype)).sum())
        print(f"transform {shape} {np.dtype(in_dtype).name} -> {np.dtype(out_dtype).name}: {ne} elements differ from numpy, "
              f"{ne_t} with to_nchw")
        assert ne == 0 and ne_t == 0
    got = sc.transform(xd)
    assert got.dtype == xd.dtype                                   # the default output dtype is the input's
    back = sc.inverse_transform(xd)
    ne = int((back.cpu().numpy() != inv.astype(in_dtype)).sum())
    print(f"inverse {shape} {np.dtype(in_dtype).name}: {ne} elements differ from numpy")
    assert back.dtype == xd.dtype and back.data_ptr() != xd.data_ptr() and ne == 0
    assert torch.equal(xd, keep), "the input tensor was modified"
    ft = prepare.ChannelScaler().fit_transform(xd, to_nchw=True, out_dtype=torch.float32)
    assert torch.equal(ft, sc.transform(xd, out_dtype=torch.float32, to_nchw=True))


def test_transform_scalar_path_and_single_feature():
    from gan_danet_amd import prepare
    x = np.random.RandomState(34).randn(3, 11, 5) * 4.0 + 1.0
    _, xd = _offset_view(x, 1)                                      # 8 bytes off a 16-byte boundary
    assert xd.data_ptr() % 16 == 8
    sc = prepare.ChannelScaler().fit(xd)
    assert np.array_equal(sc.transform(xd).cpu().numpy(), (x - sc.mean_) / sc.scale_)
    assert np.array_equal(sc.inverse_transform(xd).cpu().numpy(), x * sc.scale_ + sc.mean_)
    g = np.random.RandomState(35).randn(6, 9, 11) * 7.0 - 0.5        # a GRACE field: one feature whatever the shape
    gd = _dev(g)
    s1 = prepare.ChannelScaler().fit(gd, channel_axis=None)
    ref = StandardScaler().fit(g.reshape(-1, 1))
    assert s1.mean_.shape == (1,) and abs(s1.mean_[0] - ref.mean_[0]) <= 4 * EPS * np.abs(g).max()
    assert np.array_equal(s1.transform(gd).cpu().numpy(), (g - s1.mean_[0]) / s1.scale_[0])
    assert np.array_equal(s1.inverse_transform(gd).cpu().numpy(), g * s1.scale_[0] + s1.mean_[0])


def test_recorded_scalers_round_trip(golden_dir):
    """the scalers the reference recorded (45 auxiliary channels, the two GRACE fields) through from_sklearn"""
    from gan_danet_amd import prepare
    z = np.load(os.path.join(golden_dir, "prepare_scalers.npz"))
    scalers = []
    for i in range(45):
        s = StandardScaler()
        s.mean_, s.scale_, s.var_ = z["aux_mean_"][i:i + 1], z["aux_scale_"][i:i + 1], z["aux_var_"][i:i + 1]
        s.n_samples_seen_ = int(z["aux_n_samples_seen_"][i])
        scalers.append(s)
    sc = prepare.ChannelScaler.from_sklearn(scalers)
    assert np.array_equal(sc.mean_, z["aux_mean_"]) and np.array_equal(sc.scale_, z["aux_scale_"])
    assert np.array_equal(sc.var_, z["aux_var_"]) and sc.n_samples_seen_ == int(z["aux_n_samples_seen_"][0])
    x = np.random.RandomState(36).randn(2, 4, 4, 45) * z["aux_scale_"] + z["aux_mean_"]
    xd = _dev(x)
    std = sc.transform(xd)
    assert np.array_equal(std.cpu().numpy(), (x - z["aux_mean_"]) / z["aux_scale_"])
    back = sc.inverse_transform(std).cpu().numpy()
    ratio = np.abs(back - x) / (np.spacing(np.abs(x) + np.abs(z["aux_mean_"])))
    print(f"recorded aux scalers: round trip max {ratio.max():.3f} ulp of |x| + |mean|")
    assert ratio.max() <= 2.0
    sk = sc.to_sklearn()
    assert np.allclose(sk.inverse_transform(std.cpu().numpy().reshape(-1, 45)).reshape(x.shape), back, rtol=1e-15, atol=0)
    for name in ("grace05", "grace025"):
        s = StandardScaler()
        s.mean_, s.scale_, s.var_ = z[name + "_mean_"], z[name + "_scale_"], z[name + "_var_"]
        s.n_samples_seen_ = int(z[name + "_n_samples_seen_"][0])
        g1 = prepare.ChannelScaler.from_sklearn(s)
        g = np.random.RandomState(37).randn(3, 5, 6) * s.scale_[0] + s.mean_[0]
        gd = _dev(g)
        back = g1.inverse_transform(g1.transform(gd)).cpu().numpy()
        ratio = np.abs(back - g) / np.spacing(np.abs(g) + abs(s.mean_[0]))
        print(f"recorded {name} scaler: round trip max {ratio.max():.3f} ulp")
        assert g1.mean_[0] == s.mean_[0] and g1.scale_[0] == s.scale_[0] and ratio.max() <= 2.0


# ---- frequency augmentation -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def freq_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "prepare_freq.npz"))
    return {k: z[k] for k in z.files}


def _round_trip(x, axis):
    """the FFT round trip's own error on x, in x's precision"""
    return float(np.abs(np.real(scipy.fft.ifft(scipy.fft.fft(x, axis=axis), axis=axis)) - x).max())


def _k1(freq, n):
    return min(freq, n - 1) + 1


def _tol(x, want, axis, freq):
    tol = 2 * _round_trip(x, axis) + (_k1(freq, x.shape[axis]) + 2) * EPS * np.abs(want).max()
    return tol + (2.0 ** -24 * np.abs(want).max() if x.dtype == np.float32 else 0.0)


def _run_freq(xd, freq, axis, noise, **kw):
    from gan_danet_amd import prepare
    keep = xd.clone()
    out = prepare.frequency_domain_augmentation(xd, freq, 0.1, axis, noise=noise, **kw)
    assert torch.equal(xd, keep), "the input tensor was modified"
    assert out.shape == xd.shape and out.dtype == xd.dtype
    return out


@pytest.mark.parametrize("name", ["t181", "clip", "inner_axis", "len1", "t25", "f32"])
@pytest.mark.parametrize("noise_form", ["full", "slices"])
def test_frequency_augmentation_against_the_reference(freq_fixture, name, noise_form):
    x, noise, want = (freq_fixture[f"{name}_{k}"] for k in ("input", "noise", "output"))
    axis, freq = int(freq_fixture[name + "_axis"]), int(freq_fixture[name + "_freq"])
    assert want.dtype == x.dtype
    if noise_form == "slices":
        noise = np.take(noise, np.arange(_k1(freq, x.shape[axis])), axis=axis)
    xd = _dev(x)
    out = _run_freq(xd, freq, axis, noise)
    assert out.data_ptr() != xd.data_ptr()
    got = out.cpu().numpy()
    err, tol = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(), _tol(x, want, axis, freq)
    print(f"freq augmentation {name} {x.shape} {x.dtype} axis {axis} freq {freq} ({noise_form} noise): max err {err:.3e}, "
          f"bound {tol:.3e}")
    if name == "len1":
        assert np.array_equal(got, want)                            # cos 0 / 1: the noise itself is added
    assert err <= tol


def _chain(x, noise, freq, axis):
    """the reference's chain stated with scipy.fft: real noise on the bins 0 .. freq that exist, real part of the inverse"""
    f = scipy.fft.fft(x, axis=axis)
    for idx in range(-freq, freq + 1):
        if 0 <= idx < x.shape[axis]:
            sl = [slice(None)] * x.ndim
            sl[axis] = idx
            f[tuple(sl)] += noise[tuple(sl)]
    return np.real(scipy.fft.ifft(f, axis=axis))


CHAIN_CASES = {
    "inner_axis_vector_columns": ((40, 3, 37, 8), 2, 12, 0),
    "k1_cap": ((3, 300), 1, 32, 0),
    "offset_base": ((9, 2, 6), 0, 12, 1),                           # base pointer 8 bytes off a 16-byte boundary
    "mean_only": ((30, 4, 6), 0, 0, 0),                             # seasonal_freq = 0 perturbs the mean alone
    "odd_inner": ((50, 7, 3), 0, 12, 0),                            # 21 series per row: the one-series-per-lane path
    "chunked_axis": ((3, 1000, 2), 1, 20, 0),                       # few series, long axis: several chunks per series
}


@pytest.mark.parametrize("case", sorted(CHAIN_CASES))
def test_frequency_augmentation_against_scipy(case):
    shape, axis, freq, off = CHAIN_CASES[case]
    rs = np.random.RandomState(41)
    x = rs.randn(*shape) * 5.0 + 2.0
    noise = rs.normal(scale=0.1, size=shape)
    want = _chain(x, noise, freq, axis)
    if off:
        _, xd = _offset_view(x, off)
        assert xd.data_ptr() % 16 == 8
    else:
        xd = _dev(x)
    got = _run_freq(xd, freq, axis, noise).cpu().numpy()
    err, tol = np.abs(got - want).max(), _tol(x, want, axis, freq)
    print(f"freq augmentation {case} {shape} axis {axis} freq {freq}: max err {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    if case == "mean_only":
        assert np.abs((got - x) - noise[:1] / shape[0]).max() <= 4 * EPS * np.abs(x).max()


def test_frequency_augmentation_out_slab():
    rs = np.random.RandomState(42)
    t, rest = 11, (5, 6)
    x, noise = rs.randn(t, *rest) * 3.0, rs.normal(scale=0.1, size=(t,) + rest)
    xd = _dev(x)
    buf = torch.full((3 * t,) + rest, 5.5, dtype=torch.float64, device=DEV)
    out = _run_freq(xd, 4, 0, noise, out=buf[t:2 * t])
    assert out.data_ptr() == buf[t:2 * t].data_ptr()
    assert bool((buf[:t] == 5.5).all()) and bool((buf[2 * t:] == 5.5).all()), "wrote outside the slab"
    assert torch.equal(buf[t:2 * t], _run_freq(xd, 4, 0, noise))


def test_frequency_augmentation_device_noise():
    """noise=None.  fft(out - x) holds noise[k] / 2 in bin k and in its mirror L - k for k >= 1 (the reference keeps the real
    part of the inverse transform, which symmetrises the spectrum) and noise[0] in bin 0: the draw is recovered as
    Re F[0] and Re F[k] + Re F[L - k], and nothing is left beyond bin 12 and its mirror"""
    from gan_danet_amd import prepare
    shape, level, freq = (64, 50, 40), 0.1, 12
    x = np.random.RandomState(43).randn(*shape) * 2.0
    xd = _dev(x)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1234)
    a = prepare.frequency_domain_augmentation(xd, freq, level, 0, generator=gen)
    gen.manual_seed(1234)
    b = prepare.frequency_domain_augmentation(xd, freq, level, 0, generator=gen)
    assert torch.equal(a, b)
    gen.manual_seed(99)
    assert not torch.equal(a, prepare.frequency_domain_augmentation(xd, freq, level, 0, generator=gen))
    f = scipy.fft.fft(a.cpu().numpy() - x, axis=0)
    beyond = np.abs(f[freq + 1:shape[0] - freq]).max()
    print(f"device noise: max |fft(out - x)| beyond bin {freq} and its mirror {beyond:.3e}, bound {64 * EPS * np.abs(x).max():.3e}")
    assert beyond <= 64 * EPS * np.abs(x).max()
    draw = np.concatenate([f[:1].real, f[1:freq + 1].real + f[:shape[0] - freq - 1:-1].real])
    assert draw.shape == (13, 50, 40)
    std = draw.std()
    print(f"device noise: sample std of the {draw.size} recovered draws {std:.5f} (noise_level {level}), mean {draw.mean():.2e}")
    assert abs(std - level) <= 0.05 * level
    assert np.abs(f[1:freq + 1].imag).max() <= 64 * EPS * np.abs(x).max()       # real noise only


# ---- augment_dataset and the split --------------------------------------------------------------------------------------
def test_augment_dataset():
    from gan_danet_amd import prepare
    from gan_danet_amd.data import DeviceTileDataset
    rs = np.random.RandomState(44)
    t, f = 6, 2
    d05, tr05 = rs.randn(t, 4, 6), rs.randn(t, 4, 6)
    d25, tr25 = rs.randn(t, 8, 12), rs.randn(t, 8, 12)
    aux = rs.randn(t, 8, 12, 5)
    noise = [[rs.normal(scale=0.1, size=a.shape) for a in (d05, d25, aux)] for _ in range(f)]
    dev = [_dev(a) for a in (d05, tr05, d25, tr25, aux)]
    keep = [a.clone() for a in dev]
    (o05, r05), (o25, r25), oaux = prepare.augment_dataset(*dev, augmentation_factor=f, seasonal_freq=12, noise_level=0.1,
                                                            noise=noise)
    assert all(torch.equal(a, b) for a, b in zip(dev, keep))
    assert o05.shape == (18, 4, 6) and o25.shape == (18, 8, 12) and oaux.shape == (18, 8, 12, 5)
    assert r05.shape == (18, 4, 6) and r25.shape == (18, 8, 12)
    for out, src, i in ((o05, dev[0], 0), (o25, dev[2], 1), (oaux, dev[4], 2)):
        assert torch.equal(out[:t], src)                             # slab 0 is the input, bit for bit
        for r in range(f):
            want = prepare.frequency_domain_augmentation(src, 12, 0.1, 0, noise=noise[r][i])
            assert torch.equal(out[(1 + r) * t:(2 + r) * t], want)
    assert np.array_equal(r05.cpu().numpy(), np.tile(tr05, (1 + f, 1, 1)))
    assert np.array_equal(r25.cpu().numpy(), np.tile(tr25, (1 + f, 1, 1)))
    ds = DeviceTileDataset(o05, o25, oaux)
    a, b, c = ds.get(0, 4)
    assert a.shape == (4, 1, 4, 6) and b.shape == (4, 1, 8, 12) and c.shape == (4, 5, 8, 12)
    assert torch.equal(c, oaux[:4].float().permute(0, 3, 1, 2))
    # drawn on the device: shapes, slab 0 and a perturbation of the right size
    (p05, _), _, paux = prepare.augment_dataset(*dev, augmentation_factor=1)
    assert p05.shape == (12, 4, 6) and torch.equal(paux[:t], dev[4]) and 0.0 < float((paux[t:] - dev[4]).abs().max()) < 1.0


def test_train_test_split():
    from gan_danet_amd import prepare
    rs = np.random.RandomState(45)
    n = 23
    arrays = [rs.randn(n, 4, 6).astype(np.float32), rs.randn(n, 8, 12), rs.randn(n, 8, 12, 5).astype(np.float32)]
    train, test = prepare.split_indices(n, 0.2, 42)
    assert len(test) == 5 and len(train) == 18 and sorted(np.concatenate([train, test])) == list(range(n))
    parts = prepare.train_test_split(*[_dev(a) for a in arrays], test_size=0.2, random_state=42)
    assert len(parts) == 6
    for i, a in enumerate(arrays):
        assert parts[2 * i].is_cuda and np.array_equal(parts[2 * i].cpu().numpy(), a[train])
        assert np.array_equal(parts[2 * i + 1].cpu().numpy(), a[test])
