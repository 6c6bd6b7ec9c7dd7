"""GPU parity, kernel level, for csrc/pointwise.hip: the scalar losses and their composition, TV, SSIM, the row softmax,
the SE/CBAM gate kernels, the pointwise glue and AdamW -- at the sizes where the capped grids, the grid-stride trips,
the ragged tails and the tie / overflow rules of those kernels actually run.

Every comparison is against a float64 reference computed on the CPU from the same float32 inputs cast to double
(``oracle.functional`` under double autograd where it has the op, plain torch double arithmetic otherwise).  Inputs are
seeded here; nothing is read from a fixture.  Tolerances are the ones the suite already applies to these kernels:
relmax 1e-5 for loss values and gradients (test_losses), 1e-4 / 2e-4 for the SSIM value / gradients
(test_ssim_module_gradients_vs_oracle), 1e-5 / 1e-4 for the row softmax forward / backward (test_softmax_rows) and
FP32_TOL for pointwise transcendental outputs.  They hold by construction at the sizes used: a thread of a reduction
adds at most five fp32 terms before the 256-wide block sum, and the final stage runs in double."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, assert_close, rell2, relmax, seeded

pytestmark = pytest.mark.gpu

FP32_TOL = 2e-5          # pointwise transcendental outputs (as in test_gpu_kernels.py)
LOSS_TOL = 1e-5          # loss values and gradients (test_losses)
SSIM_TOL_V, SSIM_TOL_G = 1e-4, 2e-4      # test_ssim_module_gradients_vs_oracle: value relmax, gradients rel-L2
ULP_TOL = 1e-6           # one or two fp32 roundings per element, measured against the largest element

# stage 1 of a scalar reduction: at most 1024 workgroups of 256 threads, four elements each
RED_SIZES = [1, 255, 257, 1025, 1 << 20, (1 << 20) + 1025]
EXTREME_LOGITS = [50.0, -50.0, 100.0, -100.0, 1e4, -1e4]


@pytest.fixture(scope="module")
def gd():
    import gan_danet_amd as g
    from gan_danet_amd import _lib
    _lib.load()
    return g


def _ops():
    from gan_danet_amd import kern, ops
    return ops, kern


def _of():
    from oracle import functional as OF
    return OF


def _err():
    from gan_danet_amd import _lib
    return _lib.GandanetError


def _check(a, b, tol, what, metric=relmax):
    """print the figure, then hold it to the bound"""
    if a.shape == b.shape:
        print(f"[pointwise] {what}: err {metric(a, b):.3e} (bound {tol:.1e})")
    assert_close(a, b, tol, what, metric)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _dleaf(t):
    return t.double().requires_grad_(True)


def _gleaf(t):
    return t.to(DEV).requires_grad_(True)


def _f32(v):
    """a Python float that float32 holds exactly: what the kernel receives, handed to the fp64 reference as well"""
    return float(np.float32(v))


# =====================================================================================================================
# 1. scalar-loss reductions
# =====================================================================================================================
def _logits(n, seed, repeat=1):
    """seeded logits at scale 2; entries 1.. hold +-50, +-100, +-1e4 (``repeat`` times over) wherever n leaves room.
    Entry 0 stays ordinary, so that n = 1 measures the kernel and not the 1 - sigmoid(50) cancellation of a lone
    saturated logit"""
    z = seeded((n,), seed, 2.0)
    ext = torch.tensor(EXTREME_LOGITS * repeat)
    k = max(0, min(n - 1, ext.numel()))
    z[1:1 + k] = ext[:k]
    return z


@pytest.mark.parametrize("label", [0.0, 1.0])
@pytest.mark.parametrize("n", RED_SIZES)
def test_bce_logits_constant_label(gd, n, label):
    ops, K = _ops()
    z = _logits(n, 100 + n % 97)
    zr = _dleaf(z)
    ref = _of().bce_with_logits(zr, torch.full_like(zr, label))
    (gr,) = torch.autograd.grad(ref, zr)
    zg = _gleaf(z)
    out = ops.bce_with_logits(zg, label)
    (gz,) = torch.autograd.grad(out, zg)
    _check(out, ref.detach(), LOSS_TOL, f"bce(label {label}) n={n}")
    _check(gz, gr, LOSS_TOL, f"dbce/dz(label {label}) n={n}")
    val, none = K.bce_logits(z.to(DEV), label, False)          # the value-only launch (null gradient pointer)
    assert none is None
    _check(val.view(()), ref.detach(), LOSS_TOL, f"K.bce_logits value only n={n}")


@pytest.mark.parametrize("n", RED_SIZES)
def test_bce_logits_target_tensor(gd, n):
    ops, K = _ops()
    E = len(EXTREME_LOGITS)
    z = _logits(n, 200 + n % 97, 3)                             # every extreme logit meets target 0, target 1 ...
    t = torch.rand(n, generator=torch.Generator().manual_seed(300 + n % 97))
    t[1:1 + E] = 0.0
    t[1 + E:1 + 2 * E] = 1.0                                    # ... and a target inside (0, 1)
    zr, tr = _dleaf(z), _dleaf(t)
    ref = _of().bce_with_logits(zr, tr)
    gzr, gtr = torch.autograd.grad(ref, (zr, tr))
    zg, tg = _gleaf(z), _gleaf(t)
    out = ops.bce_with_logits_target(zg, tg)
    gz, gt = torch.autograd.grad(out, (zg, tg))
    _check(out, ref.detach(), LOSS_TOL, f"bce(target) n={n}")
    _check(gz, gzr, LOSS_TOL, f"dbce/dz(target) n={n}")
    _check(gt, gtr, LOSS_TOL, f"dbce/dt(target) n={n}")
    if n > 1 + 3 * E:       # dt = -z / n: measured again without the 1e4 logits that set the scale of the line above
        _check(gt[1 + 3 * E:], gtr[1 + 3 * E:], LOSS_TOL, f"dbce/dt(target) ordinary logits n={n}")
    val, dz, dt = K.bce_logits_target(z.to(DEV), t.to(DEV), False, False)
    assert dz is None and dt is None
    _check(val.view(()), ref.detach(), LOSS_TOL, f"K.bce_logits_target value only n={n}")


def _pair(n, seed):
    a = seeded((n,), seed)
    b = a * 0.5 + seeded((n,), seed + 1) * 0.7
    return a, b


@pytest.mark.parametrize("wrt", ["a", "b", "ab"])
@pytest.mark.parametrize("n", RED_SIZES)
def test_mse_value_and_gradients_of_both_arguments(gd, n, wrt):
    """MSELoss()(a, b) with either argument, or both, requiring a gradient, under a non-unit upstream scalar that lives
    on the device.  The second argument's gradient was None (zero to autograd) before this file existed."""
    ops, K = _ops()
    a, b = _pair(n, 400 + n % 97)
    ar, br = _dleaf(a), _dleaf(b)
    ref = 3.0 * _of().mse(ar, br)
    gar, gbr = torch.autograd.grad(ref, (ar, br))
    ag = _gleaf(a) if "a" in wrt else a.to(DEV)
    bg = _gleaf(b) if "b" in wrt else b.to(DEV)
    out = ops.weighted_sum([3.0], [gd.MSELoss()(ag, bg)])
    out.backward()
    _check(out, ref.detach(), LOSS_TOL, f"3 * mse n={n}")
    if "a" in wrt:
        assert ag.grad is not None, "MSE gave its first argument no gradient"
        _check(ag.grad, gar, LOSS_TOL, f"dmse/da n={n} ({wrt})")
    if "b" in wrt:
        assert bg.grad is not None, "MSE gave its second argument no gradient"
        _check(bg.grad, gbr, LOSS_TOL, f"dmse/db n={n} ({wrt})")
    val, none = K.diff_loss("mse", a.to(DEV), b.to(DEV), False)
    assert none is None
    _check(3.0 * val.view(()), ref.detach(), LOSS_TOL, f"K.diff_loss(mse) value only n={n}")


@pytest.mark.parametrize("n", RED_SIZES)
def test_l1_value_gradients_and_exact_ties(gd, n):
    ops, K = _ops()
    a, b = _pair(n, 500 + n % 97)
    b[1::3] = a[1::3]                                           # exact ties: |a - b| has gradient exactly 0 there
    ar, br = _dleaf(a), _dleaf(b)
    ref = _of().l1(ar, br)
    gar, gbr = torch.autograd.grad(ref, (ar, br))
    ag, bg = _gleaf(a), _gleaf(b)
    out = ops.l1_loss(ag, bg)
    ga, gb = torch.autograd.grad(out, (ag, bg))
    _check(out, ref.detach(), LOSS_TOL, f"l1 n={n}")
    _check(ga, gar, LOSS_TOL, f"dl1/da n={n}")
    _check(gb, gbr, LOSS_TOL, f"dl1/db n={n}")
    assert (ga.cpu()[1::3] == 0).all() and (gb.cpu()[1::3] == 0).all(), "a tie must have gradient exactly 0"
    assert torch.equal(gb.cpu(), -ga.cpu()), "dL1/db must be -dL1/da"
    (ga1,) = torch.autograd.grad(ops.l1_loss(ag, b.to(DEV)), ag)   # first argument alone
    assert torch.equal(ga1.cpu(), ga.cpu())
    val, none = K.diff_loss("l1", a.to(DEV), b.to(DEV), False)
    assert none is None
    _check(val.view(()), ref.detach(), LOSS_TOL, f"K.diff_loss(l1) value only n={n}")


@pytest.mark.parametrize("n", RED_SIZES)
def test_dot_sum_and_accumulate(gd, n):
    """gd_dot: a.b, the plain sum (b = None) and accumulation into a non-zero output.  The inputs carry a mean of 0.5 so
    that the sums grow like n and the relative bound measures the reduction, not a cancellation of the data"""
    _, K = _ops()
    a = seeded((n,), 600 + n % 97) + 0.5
    b = a * 0.5 + seeded((n,), 601 + n % 97)
    ad, bd = a.to(DEV), b.to(DEV)
    ref_dot = (a.double() * b.double()).sum().view(1)
    ref_sum = a.double().sum().view(1)
    _check(K.dot(ad, bd), ref_dot, LOSS_TOL, f"dot n={n}")
    _check(K.dot(ad, None), ref_sum, LOSS_TOL, f"sum n={n}")
    out = torch.full((1,), 7.5, device=DEV)
    assert K.dot(ad, bd, out, accumulate=True) is out
    _check(out, ref_dot + 7.5, LOSS_TOL, f"dot accumulate n={n}")
    out = torch.full((1,), -3.25, device=DEV)
    K.dot(ad, None, out, accumulate=True)
    _check(out, ref_sum - 3.25, LOSS_TOL, f"sum accumulate n={n}")
    out = torch.full((1,), float("nan"), device=DEV)           # accumulate = False must not read the output
    K.dot(ad, bd, out, accumulate=False)
    _check(out, ref_dot, LOSS_TOL, f"dot overwrite n={n}")


def test_mean_of_and_weighted_sum_of_three_terms(gd):
    ops, _ = _ops()
    n = 1025
    a, b = _pair(n, 700)
    v = seeded((7,), 702) + 2.0
    coefs = [0.5, 2.0, -0.25]
    ar, br, vr = _dleaf(a), _dleaf(b), _dleaf(v)
    OF = _of()
    ref = coefs[0] * OF.mse(ar, br) + coefs[1] * OF.l1(ar, br) + coefs[2] * vr.mean()
    gar, gbr, gvr = torch.autograd.grad(ref, (ar, br, vr))
    ag, bg, vg = _gleaf(a), _gleaf(b), _gleaf(v)
    m = ops.mean_of(vg)
    _check(m, vr.mean().detach(), LOSS_TOL, "mean_of")
    out = ops.weighted_sum(coefs, [ops.mse_loss(ag, bg), ops.l1_loss(ag, bg), m])
    ga, gb, gv = torch.autograd.grad(out, (ag, bg, vg))
    _check(out, ref.detach(), LOSS_TOL, "weighted_sum of three")
    _check(ga, gar, LOSS_TOL, "weighted_sum d/da")
    _check(gb, gbr, LOSS_TOL, "weighted_sum d/db")
    _check(gv, gvr, LOSS_TOL, "weighted_sum d/dv (through mean_of)")


# =====================================================================================================================
# 2. TV
# =====================================================================================================================
@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (3, 2, 17, 45), (2, 3, 45, 17), (1, 1, 1031, 1021)])
def test_tv_non_square_multi_channel_and_capped_grid(gd, shape):
    ops, K = _ops()
    weight = 0.7
    x = seeded(shape, 800 + shape[2])
    xr = _dleaf(x)
    ref = _of().tv_loss(xr, weight)
    (gr,) = torch.autograd.grad(ref, xr)
    xg = _gleaf(x)
    out = ops.tv_loss(xg, weight)
    (g,) = torch.autograd.grad(out, xg)
    _check(out, ref.detach(), LOSS_TOL, f"tv {shape}")
    _check(g, gr, LOSS_TOL, f"dtv {shape}")
    val, none = K.tv(x.to(DEV), weight, False)
    assert none is None
    _check(val.view(()), ref.detach(), LOSS_TOL, f"K.tv value only {shape}")


@pytest.mark.parametrize("shape", [(2, 3, 1, 9), (2, 3, 9, 1), (1, 1, 1, 1)])
def test_tv_rejects_single_row_or_column(gd, shape):
    ops, K = _ops()
    x = seeded(shape, 810).to(DEV)
    with pytest.raises(_err()):
        ops.tv_loss(x, 1.0)
    with pytest.raises(_err()):
        K.tv(x, 1.0, True)


# =====================================================================================================================
# 3. SSIM
# =====================================================================================================================
def _ssim_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g) * 2 - 1
    b = (a + 0.3 * torch.randn(shape, generator=g)).clamp(-1.5, 1.5)
    w = torch.rand(shape[0], generator=g) + 0.5
    return a, b, w


def _ssim_reference(a, b, w, window, dtype=torch.float64):
    """oracle SSIM under autograd in ``dtype``: per-sample values, their mean, the gradients of the mean and of the
    w-weighted sum of the per-sample values with respect to both images"""
    ar, br = a.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    per = _of().ssim(ar, br, window, False)
    mean = per.mean()                      # every sample has C*H*W pixels: the mean of the means is the mean of the map
    gm = torch.autograd.grad(mean, (ar, br), retain_graph=True)
    gs = torch.autograd.grad((per * w.to(dtype)).sum(), (ar, br))
    return per.detach(), mean.detach(), gm, gs


def _ssim_device(a, b, w, window):
    ops, _ = _ops()
    val = ops.ssim_value(a.to(DEV), b.to(DEV), window)
    ag, bg = _gleaf(a), _gleaf(b)
    mean = ops.ssim(ag, bg, window, True)
    gm = torch.autograd.grad(mean, (ag, bg))
    per = ops.ssim(ag, bg, window, False)
    gs = torch.autograd.grad(per, (ag, bg), w.to(DEV))
    return val, per.detach(), mean.detach(), gm, gs


def _ssim_compare(shape, window, seed, tag):
    a, b, w = _ssim_inputs(shape, seed)
    rper, rmean, rgm, rgs = _ssim_reference(a, b, w, window)
    val, per, mean, gm, gs = _ssim_device(a, b, w, window)
    _check(val, rmean, SSIM_TOL_V, f"ssim_value {tag}")
    _check(mean, rmean, SSIM_TOL_V, f"ssim(size_average=True) {tag}")
    _check(per, rper, SSIM_TOL_V, f"ssim(size_average=False) {tag}")
    for name, g_, r_ in (("mean d/da", gm[0], rgm[0]), ("mean d/db", gm[1], rgm[1]),
                         ("weighted per-sample d/da", gs[0], rgs[0]), ("weighted per-sample d/db", gs[1], rgs[1])):
        _check(g_, r_, SSIM_TOL_G, f"ssim {name} {tag}", rell2)


@pytest.mark.parametrize("shape", [
    (1, 1, 3, 5),          # smaller than the 11-tap window in both dimensions
    (2, 2, 11, 4),         # smaller in one
    (1, 1, 260, 257),      # 66,820 pixels: grid-stride in the forward (> 16,384) and in the backward (> 65,536)
    (8, 5, 130, 127),      # 40 planes of 16,510 pixels: gx halved 64 -> 32, 160 partial sums per sample
])
def test_ssim_small_images_and_capped_grids(gd, shape):
    _ssim_compare(shape, 11, 900 + shape[3], f"{shape}")


@pytest.mark.parametrize("window", [1, 3, 15])
def test_ssim_window_sizes(gd, window):
    _ssim_compare((1, 2, 20, 23), window, 920 + window, f"window {window}")


@pytest.mark.parametrize("window", [0, 4, 10, 17])
def test_ssim_rejects_bad_windows(gd, window):
    ops, _ = _ops()
    a, b, _w = _ssim_inputs((1, 2, 20, 23), 930)
    with pytest.raises(_err()):
        ops.ssim_value(a.to(DEV), b.to(DEV), window)
    with pytest.raises(_err()):
        ops.ssim(_gleaf(a), _gleaf(b), window, True)


def test_ssim_rejects_more_planes_than_the_workspace_holds(gd):
    ops, _ = _ops()
    a, b, _w = _ssim_inputs((683, 3, 4, 4), 940)               # 2,049 planes
    with pytest.raises(_err(), match="too many planes"):
        ops.ssim_value(a.to(DEV), b.to(DEV), 11)
    for size_average in (True, False):
        with pytest.raises(_err(), match="too many planes"):
            ops.ssim(_gleaf(a), _gleaf(b), 11, size_average)


def test_ssim_offset_mean_low_variance_conditioning(gd):
    """a = 0.5 + 0.05 smooth + 0.01 noise, b = a + 0.01 noise on (2, 1, 64, 80): the offset-mean, low-variance fields of
    real normalised data, where E[x^2] - E[x]^2 cancels.  The bound is max(the bound of
    test_ssim_module_gradients_vs_oracle, 4 e_ref), e_ref being the error of the oracle itself run in float32 on the CPU
    (the factor 4 covers another order of the 121-tap accumulation and fma contraction against ATen's convolution).

    Measured on the MI355X (error of the fp32 oracle e_ref / error of the kernels / bound):
      value  1.98e-07 / 4.29e-06 / 1.0e-04      d/da  3.49e-05 / 7.05e-05 / 2.0e-04      d/db  4.33e-05 / 7.06e-05 / 2.0e-04
    so the plain-moment accumulation of the kernels stays within a factor of about two of ATen's fp32 convolutions here
    and both sit below the bound the suite already applies; 4 e_ref does not come into play."""
    shape = (2, 1, 64, 80)
    g = torch.Generator().manual_seed(950)
    yy = torch.arange(shape[2], dtype=torch.float32).view(1, 1, -1, 1) / shape[2]
    xx = torch.arange(shape[3], dtype=torch.float32).view(1, 1, 1, -1) / shape[3]
    phase = torch.tensor([0.3, 1.7]).view(2, 1, 1, 1)
    smooth = torch.sin(2 * torch.pi * 1.5 * yy + phase) * torch.cos(2 * torch.pi * 2.0 * xx - phase)
    a = 0.5 + 0.05 * smooth + 0.01 * torch.randn(shape, generator=g)
    b = a + 0.01 * torch.randn(shape, generator=g)
    w = torch.ones(shape[0])
    _, rmean, rgm, _ = _ssim_reference(a, b, w, 11)
    _, fmean, fgm, _ = _ssim_reference(a, b, w, 11, torch.float32)
    val, _, mean, gm, _ = _ssim_device(a, b, w, 11)
    e_ref = (relmax(fmean, rmean), rell2(fgm[0], rgm[0]), rell2(fgm[1], rgm[1]))
    e_dev = (max(relmax(val, rmean), relmax(mean, rmean)), rell2(gm[0], rgm[0]), rell2(gm[1], rgm[1]))
    floor = (SSIM_TOL_V, SSIM_TOL_G, SSIM_TOL_G)
    for name, er, ed, fl in zip(("value", "d/da", "d/db"), e_ref, e_dev, floor):
        print(f"[pointwise] ssim conditioning {name}: e_ref {er:.3e}  kernel {ed:.3e}  bound {max(fl, 4 * er):.3e}")
    assert torch.isfinite(mean).all() and all(torch.isfinite(t).all() for t in gm)
    for name, er, ed, fl in zip(("value", "d/da", "d/db"), e_ref, e_dev, floor):
        assert ed <= max(fl, 4 * er), f"ssim conditioning {name}: kernel {ed:.3e} > max({fl:.1e}, 4 * {er:.3e})"


# =====================================================================================================================
# 4. row softmax
# =====================================================================================================================
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("cols", [1, 63, 256, 257, 368, 1000])
def test_softmax_rows_beyond_one_trip(gd, cols, sign):
    _, K = _ops()
    x = seeded((3, cols), 1000 + cols, 5.0)
    x[1] += 80.0                                                # without the max subtraction exp() overflows here ...
    x[2] -= 80.0                                                # ... and here under sign = -1
    dp = seeded((3, cols), 1001 + cols)
    xr = _dleaf(x)
    pr = torch.softmax(sign * xr, -1)
    (gr,) = torch.autograd.grad(pr, xr, dp.double())
    p = K.softmax_rows(x.to(DEV), sign)
    _check(p, pr.detach(), 1e-5, f"softmax cols={cols} sign={sign}")
    rowsum = p.double().sum(-1).cpu()
    print(f"[pointwise] softmax cols={cols} sign={sign}: max |row sum - 1| {(rowsum - 1).abs().max().item():.3e}")
    assert ((rowsum - 1).abs() <= 1e-6).all(), f"softmax rows do not sum to 1: {rowsum.tolist()}"
    dx = K.softmax_rows_bwd(p, dp.to(DEV), sign)
    _check(dx, gr, 1e-4, f"softmax bwd cols={cols} sign={sign}")


# =====================================================================================================================
# 5. gate kernels
# =====================================================================================================================
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(3, 5, 7, 11), (2, 1, 1, 300)])
def test_gate_channels_and_pixels(gd, shape, mode):
    ops, _ = _ops()
    B, C, H, W = shape
    x = seeded(shape, 1100 + W)
    att = seeded((B, C) if mode == 0 else (B, 1, H, W), 1101 + W)
    dy = seeded(shape, 1102 + W)
    xr, ar = _dleaf(x), _dleaf(att)
    yr = xr * (ar.view(B, C, 1, 1) if mode == 0 else ar)
    gxr, gar = torch.autograd.grad(yr, (xr, ar), dy.double())
    xg, ag = _gleaf(x), _gleaf(att)
    y = ops.gate_channels(xg, ag) if mode == 0 else ops.gate_pixels(xg, ag)
    gx, ga = torch.autograd.grad(y, (xg, ag), dy.to(DEV))
    _check(y, yr.detach(), ULP_TOL, f"bcast_mul mode {mode} {shape}")
    _check(gx, gxr, ULP_TOL, f"bcast_mul mode {mode} {shape} dx")
    _check(ga, gar, LOSS_TOL, f"bcast_mul mode {mode} {shape} dgate")


@pytest.mark.parametrize("rows,n", [(8200, 5), (3, 1000), (2, 1)])
def test_row_dot_row_cap_and_long_rows(gd, rows, n):
    _, K = _ops()
    a = seeded((rows, n), 1200 + n) + 0.5
    b = a * 0.5 + seeded((rows, n), 1201 + n)
    out = K.row_dot(a.to(DEV), b.to(DEV), rows)
    _check(out, (a.double() * b.double()).sum(-1), LOSS_TOL, f"row_dot rows={rows} n={n}")


@pytest.mark.parametrize("C", [1, 7])
@pytest.mark.parametrize("sliced", [False, True])
def test_chan_dot_ragged_pixels_and_slab_slices(gd, C, sliced):
    _, K = _ops()
    B, N = 2, 257
    gamma = torch.tensor([0.37])
    if sliced:                                                  # a channel slice of a wider slab: batch stride > C * N
        slab_a, slab_o = seeded((B, C + 5, N), 1300 + C), seeded((B, C + 3, N), 1301 + C)
        a, o = slab_a[:, 2:2 + C], slab_o[:, 1:1 + C]
        ad, od = slab_a.to(DEV)[:, 2:2 + C], slab_o.to(DEV)[:, 1:1 + C]
        assert ad.stride(0) > C * N and od.stride(0) > C * N
    else:
        a, o = seeded((B, C, N), 1302 + C), seeded((B, C, N), 1303 + C)
        ad, od = a.to(DEV), o.to(DEV)
    ref = (a.double() * o.double()).sum(1)
    d_raw, delta = K.chan_dot(ad, od, gamma.to(DEV))
    _check(d_raw, ref, LOSS_TOL, f"chan_dot C={C} sliced={sliced}")
    _check(delta, ref * gamma.double(), LOSS_TOL, f"chan_dot * gamma C={C} sliced={sliced}")


@pytest.mark.parametrize("shape", [(2, 1, 5, 7), (3, 7, 9, 31)])
def test_chan_maxmean_ties_take_the_first_maximal_channel(gd, shape):
    ops, K = _ops()
    B, C, H, W = shape
    x = torch.round(seeded(shape, 1400 + W) * 2) / 2            # multiples of 0.5: many pixels have tied maxima
    am = torch.argmax(x, 1)                                     # documented to return the first maximal index
    if C > 1:
        srt = torch.sort(x, 1, descending=True).values
        assert (srt[:, 0] == srt[:, 1]).float().mean() > 0.1, "the fixture lost its ties"
    dy = seeded((B, 2, H, W), 1401 + W)
    y, idx = K.chan_maxmean_fwd(x.to(DEV))
    assert torch.equal(_bits(y[:, 0]), _bits(x.max(1).values)), "max plane is not bit-equal"
    assert torch.equal(idx.cpu().view(B, H, W).long(), am), "idx is not the first maximal channel"
    _check(y[:, 1], x.double().mean(1), LOSS_TOL, f"channel mean {shape}")
    xg = _gleaf(x)
    yg = ops.chan_maxmean(xg)
    assert torch.equal(_bits(yg), _bits(y))
    (gx,) = torch.autograd.grad(yg, xg, dy.to(DEV))
    ref = torch.zeros(shape, dtype=torch.float64)
    ref.scatter_(1, am.unsqueeze(1), dy[:, 0:1].double())
    ref += dy[:, 1:2].double() / C
    _check(gx, ref, LOSS_TOL, f"chan_maxmean backward {shape}")


def test_global_avg_pool_offset_mean(gd):
    ops, _ = _ops()
    shape = (2, 5, 150, 130)
    x = seeded(shape, 1500) + 3.0
    dy = seeded(shape[:2], 1501)
    xr = _dleaf(x)
    yr = xr.mean((2, 3))
    (gr,) = torch.autograd.grad(yr, xr, dy.double())
    xg = _gleaf(x)
    y = ops.global_avg_pool(xg)
    (gx,) = torch.autograd.grad(y, xg, dy.to(DEV))
    _check(y, yr.detach(), LOSS_TOL, "global_avg_pool")
    _check(gx, gr, LOSS_TOL, "global_avg_pool backward")


# =====================================================================================================================
# 6. pointwise glue
# =====================================================================================================================
def _act_ref(x, act, ops):
    """the activation in torch, in the dtype of x (leaky as where(x >= 0, x, 0.2 x): oracle.functional.leaky_relu)"""
    if act == ops.ACT_RELU:
        return torch.relu(x)
    if act == ops.ACT_LEAKY:
        return torch.where(x >= 0, x, x * 0.2)
    if act == ops.ACT_SIGMOID:
        return torch.sigmoid(x)
    return x * 1.0


def _act_input(n, seed):
    x = seeded((n,), seed, 3.0)
    special = torch.tensor([0.0, 100.0, -100.0, -0.0])
    k = min(n, 4)
    x[n - k:] = special[:k]                                     # at the ragged end of the array
    return x


def _act_compare(n, act, ops, K, seed):
    x, dy = _act_input(n, seed), seeded((n,), seed + 1)
    y = K.act_fwd(x.to(DEV), act)
    dx = K.act_bwd(y, dy.to(DEV), act)
    if act == ops.ACT_SIGMOID:
        xr = _dleaf(x)
        yr = _act_ref(xr, act, ops)
        (gr,) = torch.autograd.grad(yr, xr, dy.double())
        _check(y, yr.detach(), FP32_TOL, f"sigmoid n={n}")
        _check(dx, gr, FP32_TOL, f"sigmoid backward n={n}")
        return
    xr = x.clone().requires_grad_(True)
    yr = _act_ref(xr, act, ops)
    (gr,) = torch.autograd.grad(yr, xr, dy)
    # bit for bit, except the sign of a zero that ReLU produces from a zero input (max(-0, +0) may return either zero)
    free = (x == 0) if act == ops.ACT_RELU else torch.zeros_like(x, dtype=torch.bool)
    assert torch.equal(y.cpu(), yr.detach()), f"act {act} n={n}: forward differs"
    assert torch.equal(_bits(y)[~free], _bits(yr)[~free]), f"act {act} n={n}: forward is not bit-exact"
    assert torch.equal(_bits(dx), _bits(gr)), f"act {act} n={n}: backward is not bit-exact"


@pytest.mark.parametrize("act", ["ACT_NONE", "ACT_RELU", "ACT_LEAKY", "ACT_SIGMOID"])
@pytest.mark.parametrize("n", [1, 1023, 1025])
def test_act_fwd_bwd(gd, n, act):
    ops, K = _ops()
    _act_compare(n, getattr(ops, act), ops, K, 1600 + n)


def test_act_fwd_bwd_above_the_grid_cap(gd):
    """n = 8,388,611 > 8,192 blocks x 1,024: every thread makes a fifth grid-stride trip or stops before it"""
    ops, K = _ops()
    _act_compare(8192 * 1024 + 3, ops.ACT_LEAKY, ops, K, 1650)


def _within_one_ulp(out, ref64, what):
    """out (fp32) against a double reference: no further from it than the nearer fp32 neighbour's neighbour"""
    out = out.detach().cpu()
    assert torch.isfinite(out).all(), f"{what}: non-finite values"
    r = ref64.float()                                           # the correctly rounded result
    lo = torch.nextafter(r, torch.full_like(r, -float("inf")))
    hi = torch.nextafter(r, torch.full_like(r, float("inf")))
    bad = (out < lo) | (out > hi)
    print(f"[pointwise] {what}: {int((out != r).sum())} of {out.numel()} differ from the correctly rounded result")
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off by more than 1 ulp"


@pytest.mark.parametrize("n", [1, 1025, 4099])
def test_axpby_b_zero_never_reads_y(gd, n):
    _, K = _ops()
    a, b = _f32(0.3), _f32(-1.7)
    x, y0 = seeded((n,), 1700 + n), seeded((n,), 1701 + n)
    xd = x.to(DEV)
    y = torch.full((n,), float("nan"), device=DEV)
    assert K.axpby(xd, a, y, 0.0) is y
    assert torch.isfinite(y).all(), "b == 0 read the NaN-filled destination"
    assert torch.equal(_bits(y), _bits(x * a)), "b == 0 must give exactly a * x"
    y = y0.to(DEV).clone()
    K.axpby(xd, a, y, b)
    by = (y0 * b).double()                                      # the rounded fp32 product that goes into the fma
    _within_one_ulp(y, a * x.double() + by, f"axpby n={n}")
    z = x.to(DEV).clone()                                       # in place: x is y
    K.axpby(z, a, z, b)
    _within_one_ulp(z, a * x.double() + (x * b).double(), f"axpby in place n={n}")
    z = x.to(DEV).clone()
    K.axpby(z, a, z, 0.0)
    assert torch.equal(_bits(z), _bits(x * a))


@pytest.mark.parametrize("n", [1, 1025])
def test_scale_dev_plain_and_accumulate(gd, n):
    _, K = _ops()
    x, y0 = seeded((n,), 1800 + n), seeded((n,), 1801 + n)
    s = torch.tensor([_f32(-0.37)])
    out = K.scale_dev(x.to(DEV), s.to(DEV))
    _check(out, s.double() * x.double(), ULP_TOL, f"scale_dev n={n}")
    y = torch.full((n,), float("nan"), device=DEV)              # not accumulating: the destination is not read
    K.scale_dev(x.to(DEV), s.to(DEV), y, accumulate=False)
    _check(y, s.double() * x.double(), ULP_TOL, f"scale_dev into out n={n}")
    y = y0.to(DEV).clone()
    K.scale_dev(x.to(DEV), s.to(DEV), y, accumulate=True)
    _check(y, y0.double() + s.double() * x.double(), ULP_TOL, f"scale_dev accumulate n={n}")


def test_add_transpose(gd):
    _, K = _ops()
    a = seeded((2, 33, 33), 1900)
    out = K.add_transpose(a.to(DEV))
    assert torch.equal(_bits(out), _bits(a + a.transpose(1, 2))), "a + a^T is one exact fp32 addition per element"


def test_copy_rows_between_different_leading_dimensions(gd):
    _, K = _ops()
    B, R, Cc = 2, 5, 7
    s_ld, d_ld, s_rows, d_rows = 9, 10, 6, 8
    src = seeded((B, s_rows, s_ld), 2000)
    dst0 = seeded((B, d_rows, d_ld), 2001)
    dst = dst0.to(DEV)
    K.copy_rows(src.to(DEV), s_rows * s_ld, s_ld, dst, d_rows * d_ld, d_ld, B, R, Cc)
    ref = dst0.clone()
    ref[:, :R, :Cc] = src[:, :R, :Cc]
    assert torch.equal(_bits(dst), _bits(ref)), "copied block wrong or destination padding touched"


@pytest.mark.parametrize("region", [(0, 6, 20, 31), (3, 12, 5, 18)])     # top and right edges; interior, 9 x 13
def test_blend_region(gd, region):
    _, K = _ops()
    shape = (1, 3, 20, 31)
    sr, er, sc, ec = region
    gen, grace = seeded(shape, 2100), seeded(shape, 2101)
    mask = torch.rand(er - sr, ec - sc, generator=torch.Generator().manual_seed(2102))
    mask[0, 0], mask[-1, -1] = 0.0, 1.0
    g64, r64, m64 = gen.double().numpy(), grace.double().numpy(), mask.double().numpy()
    ref = g64.copy()
    ref[:, :, sr:er, sc:ec] = g64[:, :, sr:er, sc:ec] * (1.0 - m64) + r64[:, :, sr:er, sc:ec] * m64
    out = gen.to(DEV)
    assert K.blend_region(out, grace.to(DEV), mask.to(DEV), region) is out
    _check(out, torch.from_numpy(ref), ULP_TOL, f"blend_region {region}")
    outside = torch.ones(shape, dtype=torch.bool)
    outside[:, :, sr:er, sc:ec] = False
    assert torch.equal(_bits(out)[outside], _bits(gen)[outside]), "pixels outside the region changed"


@pytest.mark.parametrize("region", [(0, 21, 0, 5), (-1, 4, 0, 5), (0, 5, 27, 32), (5, 5, 0, 3)])
def test_blend_region_rejects_regions_outside_the_image(gd, region):
    _, K = _ops()
    shape = (1, 3, 20, 31)
    sr, er, sc, ec = region
    gen0 = seeded(shape, 2110)
    gen = gen0.to(DEV)
    mask = torch.full((max(er - sr, 0), max(ec - sc, 0)), 0.5, device=DEV)
    with pytest.raises(_err()):
        K.blend_region(gen, seeded(shape, 2111).to(DEV), mask, region)
    assert torch.equal(_bits(gen), _bits(gen0))


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", [1, 1025])
def test_adamw_single_step_vs_fp64(gd, n, step):
    """one K.adamw call at the given step against oracle.functional.adamw_update in double.  The hyper-parameters are
    float32-exact so that both sides see the same numbers (1 - float32(0.999) differs from 0.001 by 1.3e-5)"""
    _, K = _ops()
    lr, b1, b2, eps, wd, gs = _f32(1e-2), _f32(0.5), _f32(0.999), _f32(1e-8), _f32(0.1), 0.25
    p, g = seeded((n,), 2200 + n), seeded((n,), 2201 + n, 2.0)
    m = seeded((n,), 2202 + n, 0.3) if step > 1 else torch.zeros(n)
    v = seeded((n,), 2203 + n, 0.5) ** 2 if step > 1 else torch.zeros(n)
    pr, mr, vr = p.double(), m.double(), v.double()
    _of().adamw_update(pr, g.double() * gs, mr, vr, step, lr, b1, b2, eps, wd)
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    K.adamw(pd, g.to(DEV), md, vd, step, lr, b1, b2, eps, wd, gs)
    _check(pd, pr, ULP_TOL, f"adamw p n={n} step={step}")
    _check(md, mr, ULP_TOL, f"adamw m n={n} step={step}")
    _check(vd, vr, ULP_TOL, f"adamw v n={n} step={step}")
