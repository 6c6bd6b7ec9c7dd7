"""The float64 reference of the resize, pooling and tap-sum kernels (tests/resample_util.py) against ATen in float64
with autograd, on the CPU: the evidence that what tests/test_gpu_resample.py compares the kernels with is right,
including the tie and NaN rules of the max-pool."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_util as RU

TOL = 1e-12
SCALES = [2, 0.5, 0.25, 1.25, 1.5, 0.8]
SIZES = [(5, 7), (9, 12), (11, 30), (16, 16), (1, 9), (9, 1)]
EXPLICIT = [((1, 1), (4, 4)), ((2, 3), (8, 12)), ((1, 70), (4, 280)), ((5, 5), (5, 5)), ((9, 30), (4, 13)),
            ((7, 9), (14, 27)), ((10, 10), (3, 30))]


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b.detach().numpy() if hasattr(b, "detach") else b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    err = np.abs(a - b).max() / max(1.0, np.abs(b).max())
    assert err <= TOL, f"{what}: err {err:.3e} > {TOL:.0e}"


def _same(a, b, what):
    """equal including the places of NaNs and the signs of infinities"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b.detach().numpy() if hasattr(b, "detach") else b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"{what}:\n{a}\nvs\n{b}"


def _check_resize(mode, x, out, rs_y, rs_x, **kw):
    make = RU.cubic_axis if mode == "bicubic" else RU.linear_axis
    xr = x.clone().requires_grad_(True)
    yr = F.interpolate(xr, mode=mode, align_corners=False, **kw)
    assert tuple(yr.shape[2:]) == tuple(out)
    dy = _randn(tuple(yr.shape), 9)
    yr.backward(dy)
    ay, ax = make(x.shape[2], out[0], rs_y), make(x.shape[3], out[1], rs_x)
    _close(RU.resize_fwd(x, ay, ax), yr, f"{mode} forward")
    _close(RU.resize_bwd(dy, ay, ax), xr.grad, f"{mode} backward")
    # rows of the weight matrices sum to one, and the bound helper's images dominate the results
    _close(ay.W.sum(1), np.ones(out[0]), "row sums y")
    _close(ax.W.sum(1), np.ones(out[1]), "row sums x")
    assert (np.abs(RU.resize_fwd(x, ay, ax)) <= RU.abs_image(x, ay, ax) + 1e-12).all()
    assert (np.abs(RU.resize_bwd(dy, ay, ax)) <= RU.abs_image(dy, ay, ax, backward=True) + 1e-12).all()
    assert (RU.resize_bound(x, ay, ax, 10.0) >= 10.0 * RU.U * RU.abs_image(x, ay, ax) * (1 - 1e-12)).all()


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scale", SCALES)
def test_reference_matches_interpolate_at_scale_factors(scale, size, mode):
    out = (RU.out_size(size[0], scale), RU.out_size(size[1], scale))
    if min(out) == 0:
        with pytest.raises(RuntimeError):       # no such resize exists: ATen refuses it too
            F.interpolate(_randn((1, 1) + size, 1), scale_factor=scale, mode=mode, align_corners=False)
        return
    x = _randn((2, 3) + size, 3 + size[0])
    # with a scale factor (and recompute_scale_factor unset) ATen's ratio is 1 / scale, not in / out
    _check_resize(mode, x, out, 1.0 / scale, 1.0 / scale, scale_factor=scale)


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("size,out", EXPLICIT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_matches_interpolate_at_explicit_sizes(size, out, mode):
    x = _randn((2, 2) + size, 5 + size[1])
    _check_resize(mode, x, out, size[0] / out[0], size[1] / out[1], size=out)


def test_power_of_two_ratios_have_no_coordinate_term():
    for rs in (0.5, 2.0, 4.0, 0.25, 1.0):
        assert (RU.coord_delta(RU.source_coords(9, rs), rs) == 0).all()
        assert (RU.linear_axis(8, int(8 / rs), rs).E == 0).all()
        E = RU.cubic_axis(8, int(8 / rs), rs).E
        assert set(np.unique(E / (RU.W_EVAL * RU.U)).round(9)) <= {0.0, 1.0, 2.0, 3.0, 4.0}     # evaluation part only
    for rs in (0.8, 1.25, 1 / 1.5, RU.f32(1 / 2.2)):
        assert (RU.coord_delta(RU.source_coords(9, rs), rs) > 0).all()


def test_weight_error_bound_covers_the_float32_weights():
    """E must dominate |W_float32 - W| when the coordinate and the cubic polynomials are evaluated in float32 the way
    the kernels do (emulated here with numpy float32 scalars), floor changes included (x2.2: src of o = 5 is 2.0)"""
    f = np.float32
    for s in (2.2, 1.5, 1.25, 0.8, 0.3, 2.0, 0.5):
        rs = f(1.0 / s)
        for n_in in (1, 2, 9, 40):
            n_out = max(1, RU.out_size(n_in, s))
            ac, al = RU.cubic_axis(n_in, n_out, float(rs)), RU.linear_axis(n_in, n_out, float(rs))
            Wc, Wl = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
            for o in range(n_out):
                src = f(f(rs * f(f(o) + f(0.5))) - f(0.5))
                fl = np.floor(src)
                t = f(src - fl)
                a_, x0, x3, x2 = f(-0.75), f(t + f(1)), f(f(2) - t), f(f(1) - t)
                w = [f(f(f(f(f(f(a_ * x0) - f(5) * a_) * x0) + f(8) * a_) * x0) - f(4) * a_),
                     f(f(f(f(f(a_ + f(2)) * t) - f(a_ + f(3))) * t) * t + f(1)),
                     f(f(f(f(f(a_ + f(2)) * x2) - f(a_ + f(3))) * x2) * x2 + f(1)),
                     f(f(f(f(f(f(a_ * x3) - f(5) * a_) * x3) + f(8) * a_) * x3) - f(4) * a_)]
                for k in range(4):
                    Wc[o, min(max(int(fl) - 1 + k, 0), n_in - 1)] += float(w[k])
                sl = max(src, f(0))
                i0 = min(int(sl), n_in - 1)
                i1 = i0 + (1 if i0 < n_in - 1 else 0)
                lam = f(sl - f(i0))
                Wl[o, i0] += float(f(f(1) - lam))
                Wl[o, i1] += float(lam)
            assert (np.abs(Wc - ac.W) <= ac.E).all(), f"cubic x{s} n={n_in}: {np.abs(Wc - ac.W).max():.3e}"
            assert (np.abs(Wl - al.W) <= al.E + RU.U).all(), f"linear x{s} n={n_in}: {np.abs(Wl - al.W).max():.3e}"


def test_combine_inputs_is_two_resizes_and_a_cat():
    lr, aux = _randn((3, 2, 11, 14), 1), _randn((3, 3, 23, 29), 2)
    ref, bound = RU.combine_inputs(lr, aux, 2.0, 4.0, 5, 7)
    want = torch.cat([F.interpolate(lr, scale_factor=0.5, mode="bicubic"), F.interpolate(aux, scale_factor=0.25, mode="bicubic")], 1)
    _close(ref, want, "preamble")
    assert bound.shape == ref.shape and (bound > 0).all()


# ---- max-pool ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hand", "quantised-6x4", "quantised-2x514", "random"])
def test_reference_maxpool_matches_aten_ties_inf_nan(case):
    if case == "hand":
        x = torch.from_numpy(RU.hand_plane()).view(1, 1, 2, -1)
    elif case == "random":
        x = _randn((2, 3, 8, 10), 4)
    else:
        H, W = (6, 4) if case.endswith("6x4") else (2, 514)
        x = torch.randint(-1, 3, (2, 3, H, W), generator=torch.Generator().manual_seed(6)).double()
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    dy = _randn(tuple(yr.shape), 8)
    yr.backward(dy)
    _same(RU.maxpool2_fwd(x), yr, "pool forward")
    _same(RU.maxpool2_bwd(x, dy), xr.grad, "pool backward")
    gate = RU.maxpool2_bwd(x, dy, relu_mask=True)
    with np.errstate(invalid="ignore"):
        keep = np.repeat(np.repeat(RU.maxpool2_fwd(x) > 0, 2, -2), 2, -1)
    _same(gate, np.where(keep, xr.grad.numpy(), 0.0), "gated pool backward")
    if case == "hand":          # the sign of a zero maximum is the first element's
        assert np.array_equal(np.signbit(RU.maxpool2_fwd(x)), np.signbit(yr.detach().numpy()))


# ---- tap sum -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 30), (2, 3, 25), (1, 5, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("with_bias", [False, True])
def test_reference_tap_sum_is_the_one_hot_conv(shape, with_bias):
    B, H, W = shape
    E = torch.zeros(1, 9, 3, 3, dtype=torch.float64)
    for t in range(9):
        E[0, t, t // 3, t % 3] = 1.0
    u = _randn((B, 9, H, W), 3).requires_grad_(True)
    bias = _randn((1,), 4) if with_bias else None
    yr = F.conv2d(u, E, bias, padding=1)
    dy = _randn(tuple(yr.shape), 5)
    yr.backward(dy)
    _close(RU.shift_sum9_fwd(u, bias), yr, "tap sum")
    _close(RU.shift_sum9_bwd(dy), u.grad, "tap sum adjoint")
    assert (np.abs(RU.shift_sum9_fwd(u, bias)) <= RU.shift_sum9_abs(u, bias) + 1e-12).all()
    lhs = (RU.shift_sum9_fwd(u) * RU.f64(dy)).sum()
    rhs = (RU.f64(u) * RU.shift_sum9_bwd(dy)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
