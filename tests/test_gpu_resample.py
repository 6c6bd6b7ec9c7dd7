"""GPU parity, kernel level, for csrc/resample.hip and the pixel-major pooling of csrc/nhwc.hip: bicubic (the fixed x2
backward with its interior / border split, and the general gather backward), bilinear (with ``res`` and ``out`` +
``accumulate``), the fused input preamble, the nine-plane tap sum and its adjoint, the 2x2 max-pool in both layouts, and
the split of more than 65535 planes over several launches -- each through its ``kern`` / ``ops`` wrapper against the
float64 reference of tests/resample_util.py (held to ATen in tests/test_resample_reference.py).

Bounds.  Every bound is elementwise, u = 2^-24, and comes from ``resample_util.resize_bound``:

    |got - ref| <= c u (|Wy| + Ey) |x| (|Wx| + Ex)^T  +  [ (|Wy| + Ey) |x| (|Wx| + Ex)^T - |Wy| |x| |Wx|^T ]

The first term is the arithmetic term on the absolute-weight image: the kernel's sum of products, every product carrying
at most c roundings.  c = 10 for the bicubic forward (4 + 4 FMAs, margin 2), 8 for the bilinear forward (1 - lx, two
products and a sum, 1 - ly, two products and a sum), 32 for the backward kernels (up to 3 additions where clamped taps
are collected into one weight, then up to 14 FMAs along x and 14 along y; the fixed x2 interior has 8 + 8).  The bracket
is the weight term, E bounding the distance of the kernel's float32 weights from the reference's: the float32 source
coordinate is off by at most 2 u (|src| + 1) (two roundings) and the weights are Lipschitz in it, also across a change of
floor(src); plus, for bicubic, 40 u per tap for the Horner evaluation of the cubic polynomials (derivation in
resample_util's module text, checked against a float32 emulation on the CPU).  For a ratio that is a power of two the
coordinate is exact and the coordinate part of E is absent -- the x2 and the preamble cases run without it.  The
backward uses the transposed matrices in the same formula.  Added terms: ``res`` / ``accumulate`` add one rounding of
the sum each, u (|res| + image); the tap sum is ten additions at most, 10 u (|bias| + sum |u_tap|); the bias gradient is
a sum of n float32 terms in an order the test does not fix: n u sum |dy| holds for any order.  The pooling outputs and
the tap-sum adjoint are copies or zeros: compared exactly.

``_hold`` prints the largest error as a fraction of its bound before it asserts.

Not reached: a second trip of the pixel-major pooling kernels' grid-stride loop.  ``grid_n`` caps the grid at 16384
blocks of 256 lanes, one lane per channel octet of an output pixel, so a second trip needs more than 4.19 M octets: a
268 MB bf16 input and a float64 reference of a gigabyte.  Zero-sized outputs (a 1-row plane at x0.5, x0.25, x0.8) are
no resize at all: those combinations must raise instead."""
import numpy as np
import pytest
import torch

import resample_util as RU
from gpu_util import DEV, bf16_round, seeded
from resample_util import C_BWD, C_FWD_CUBIC, C_FWD_LINEAR, HAND_WINDOWS, U

pytestmark = pytest.mark.gpu

NPLANES = 65535 + 4


@pytest.fixture(scope="module")
def K():
    from gan_danet_amd import _lib, kern
    _lib.load()
    return kern


def _ops():
    from gan_danet_amd import ops
    return ops


def _err_type():
    from gan_danet_amd import _lib
    return _lib.GandanetError


def _sid(shape):
    return "x".join(str(s) for s in shape)


def _hold(name, what, got, ref, bound):
    """|got - ref| <= bound elementwise; prints the worst err / bound, then asserts"""
    got, ref = RU.f64(got), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max()
    print(f"[resample] {name} | {what}: err/bound {frac:.3e} (max err {err.max():.3e})")
    assert frac <= 1.0, f"{what}: {name} missed, err/bound {frac:.3e}, max err {err.max():.3e}"


def _exact(what, got, ref):
    """equal to the float64 reference value for value, NaNs in the same places, zeros of the same sign"""
    got, ref = RU.f64(got), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref))) | (np.signbit(got) != np.signbit(ref)) & ~np.isnan(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"got {got[bad][0]} want {ref[bad][0]}"


def _cubic_pair(Hi, Wi, Ho, Wo, rsh, rsw):
    return RU.cubic_axis(Hi, Ho, RU.f32(rsh)), RU.cubic_axis(Wi, Wo, RU.f32(rsw))


# =====================================================================================================================
# 1. the exact x2 bicubic: interior / border split of the fixed-weight backward
# =====================================================================================================================
UP2_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (4, 5), (5, 4), (6, 6), (9, 300)]


@pytest.mark.parametrize("size", UP2_SIZES, ids=_sid)
def test_bicubic_up2_forward_and_backward(K, size):
    """(6, 6) is the smallest plane with a fixed-weight interior; 2..4 have border pixels only; a 1-wide axis sends the
    launcher to the gather route; (9, 300) runs a second block along x in both directions.  B * C = 3 planes."""
    Hi, Wi = size
    x = seeded((1, 3, Hi, Wi), 301)
    dy = seeded((1, 3, 2 * Hi, 2 * Wi), 302)
    ay, ax = _cubic_pair(Hi, Wi, 2 * Hi, 2 * Wi, 0.5, 0.5)
    assert (ay.E <= 4 * RU.W_EVAL * U).all() and (ax.E <= 4 * RU.W_EVAL * U).all()      # no coordinate part at x2
    xg = x.to(DEV).requires_grad_(True)
    y = _ops().bicubic_up2(xg)
    y.backward(dy.to(DEV))
    what = f"up2 {_sid(size)}"
    _hold("bicubic x2 fwd", what + " y", y, RU.resize_fwd(x, ay, ax), RU.resize_bound(x, ay, ax, C_FWD_CUBIC))
    _hold("bicubic x2 bwd", what + " dx", xg.grad, RU.resize_bwd(dy, ay, ax), RU.resize_bound(dy, ay, ax, C_BWD, backward=True))


# =====================================================================================================================
# 2. the general bicubic: forward, and the gather backward through BicubicFn
# =====================================================================================================================
GEN_SCALES = [0.5, 0.25, 0.8, 1.25, 1.5, 2.2]
GEN_SIZES = [(1, 9), (9, 1), (5, 7), (11, 300)]
GEN_CASES = [(s, z) for s in GEN_SCALES for z in GEN_SIZES] + [(0.5, (7, 13)), (0.25, (9, 15)), (0.25, (11, 301))]


@pytest.mark.parametrize("scale,size", GEN_CASES, ids=lambda v: _sid(v) if isinstance(v, tuple) else f"x{v}")
def test_bicubic_general_forward_and_backward(K, scale, size):
    """inference.bicubic_resize = ops.BicubicFn at ratio 1 / scale, output floor(n * scale): every size here is odd
    somewhere, so floor drops a row or column at x0.5 and x0.25; (11, 300) runs a second x block forward (scale > 0.85)
    and backward.  x2.2 puts the source coordinate of output 5 on the integer 2 (a floor change the bound must carry)."""
    from gan_danet_amd import inference
    Hi, Wi = size
    Ho, Wo = RU.out_size(Hi, scale), RU.out_size(Wi, scale)
    x = seeded((2, 2, Hi, Wi), 311)
    xg = x.to(DEV).requires_grad_(True)
    if min(Ho, Wo) == 0:
        with pytest.raises(_err_type()):
            inference.bicubic_resize(xg, scale)
        return
    dy = seeded((2, 2, Ho, Wo), 312)
    rs = RU.f32(1.0 / scale)
    ay, ax = _cubic_pair(Hi, Wi, Ho, Wo, rs, rs)
    y = inference.bicubic_resize(xg, scale)
    assert tuple(y.shape) == (2, 2, Ho, Wo)
    y.backward(dy.to(DEV))
    what = f"bicubic x{scale} {_sid(size)}"
    _hold("bicubic fwd", what + " y", y, RU.resize_fwd(x, ay, ax), RU.resize_bound(x, ay, ax, C_FWD_CUBIC))
    _hold("bicubic gather bwd", what + " dx", xg.grad, RU.resize_bwd(dy, ay, ax),
          RU.resize_bound(dy, ay, ax, C_BWD, backward=True))


@pytest.mark.parametrize("scale", [3, 4])
def test_bicubic_backward_beyond_the_gather_window_raises(K, scale):
    """4 / rs + 5 > 14: the launcher's guard must refuse, through autograd and at the C ABI, and launch nothing"""
    from gan_danet_amd import _lib, inference
    x = seeded((1, 2, 5, 7), 321).to(DEV).requires_grad_(True)
    y = inference.bicubic_resize(x, scale)
    ay, ax = _cubic_pair(5, 7, 5 * scale, 7 * scale, 1.0 / scale, 1.0 / scale)
    _hold("bicubic fwd", f"bicubic x{scale} y", y, RU.resize_fwd(x, ay, ax), RU.resize_bound(x, ay, ax, C_FWD_CUBIC))
    with pytest.raises(_err_type()):
        y.backward(torch.ones_like(y))
    dy = torch.ones(2, 5 * scale, 7 * scale, device=DEV)
    dx = torch.full((2, 5, 7), -7.0, device=DEV)
    rc = _lib.load().gd_bicubic_bwd(K._ptr(dy), 2, 5, 7, K._ptr(dx), 5 * scale, 7 * scale, 1.0 / scale, 1.0 / scale, K._stream())
    torch.cuda.synchronize()
    assert rc != 0 and (dx == -7.0).all()


# =====================================================================================================================
# 3. bilinear
# =====================================================================================================================
BILINEAR_CASES = [((1, 1), (4, 4)), ((2, 3), (8, 12)), ((1, 70), (4, 280)), ((5, 5), (5, 5)), ((9, 300), (4, 131)),
                  ((7, 9), (14, 27))]


@pytest.mark.parametrize("size,out", BILINEAR_CASES, ids=_sid)
def test_bilinear_forward_backward_res_and_accumulate(K, size, out):
    (Hi, Wi), (Ho, Wo) = size, out
    x, dy = seeded((2, 2, Hi, Wi), 331), seeded((2, 2, Ho, Wo), 332)
    res, buf = seeded((2, 2, Ho, Wo), 333, 3.0), seeded((2, 2, Ho, Wo), 334, 3.0)
    ay, ax = RU.linear_axis(Hi, Ho), RU.linear_axis(Wi, Wo)
    ref, img = RU.resize_fwd(x, ay, ax), RU.abs_image(x, ay, ax)
    bnd = RU.resize_bound(x, ay, ax, C_FWD_LINEAR)
    what = f"bilinear {_sid(size)}->{_sid(out)}"
    xg = x.to(DEV).requires_grad_(True)
    y = _ops().BilinearFn.apply(xg, Ho, Wo)
    y.backward(dy.to(DEV))
    _hold("bilinear fwd", what + " y", y, ref, bnd)
    _hold("bilinear bwd", what + " dx", xg.grad, RU.resize_bwd(dy, ay, ax), RU.resize_bound(dy, ay, ax, C_BWD, backward=True))
    # res given: y = res + bilinear(x), one more rounding of the sum; res itself is left alone
    rg = res.to(DEV)
    yr = K.bilinear_fwd(x.to(DEV), Ho, Wo, res=rg)
    _hold("bilinear fwd + res", what + " res + y", yr, RU.f64(res) + ref, bnd + 1.01 * U * (np.abs(RU.f64(res)) + img + bnd))
    assert torch.equal(rg.cpu(), res)
    # out given, accumulate, twice on one buffer: buf + 2 bilinear(x), two roundings of a sum
    og = buf.to(DEV)
    for _ in range(2):
        assert K.bilinear_fwd(x.to(DEV), Ho, Wo, out=og, accumulate=True) is og
    _hold("bilinear fwd accumulate", what + " buf + 2 y", og, RU.f64(buf) + 2 * ref,
          2 * bnd + 2.02 * U * (np.abs(RU.f64(buf)) + 2 * img + 2 * bnd))
    # out given, no accumulate, over NaNs: the buffer must not be read
    ng = torch.full((2, 2, Ho, Wo), float("nan"), device=DEV)
    K.bilinear_fwd(x.to(DEV), Ho, Wo, out=ng, accumulate=False)
    assert torch.equal(ng, y.detach()), what + ": out= without accumulate differs from a fresh output"
    # res wins over a NaN-filled out as well (the kernel writes res + v and never reads out)
    ng.fill_(float("nan"))
    K.bilinear_fwd(x.to(DEV), Ho, Wo, out=ng, accumulate=False, res=rg)
    assert torch.equal(ng, yr), what + ": res + out= differs from res alone"


# =====================================================================================================================
# 4. sizes that do not follow from the ratio: an error or the right answer, never a truncated window
# =====================================================================================================================
LOOSE_CUBIC = [
    # Hi, Wi, Ho, Wo, rsh, rsw
    (5, 10, 6, 30, 0.8, 0.8),       # last column's window is 30 - 7 = 23 wide
    (5, 1, 6, 30, 0.8, 0.8),        # one column: column 0 is also the last, its window is all 30
    (10, 5, 30, 6, 0.8, 0.8),       # the same along y, where the kernel's row loop has no fixed width
    (5, 10, 6, 14, 0.8, 0.8),       # Wo = 14 where the ratio gives 12: the widened window (7 wide) still fits
    (5, 10, 6, 9, 0.8, 0.8),        # Wo short of the ratio's 12
]


def _error_or_reference(K, call, name, what, ref, bound):
    try:
        got = call()
        torch.cuda.synchronize()
    except _err_type() as e:
        print(f"[resample] {name} | {what}: refused ({e})")
        return
    _hold(name, what, got, ref, bound)


@pytest.mark.parametrize("case", LOOSE_CUBIC, ids=_sid)
def test_bicubic_backward_sizes_not_derived_from_the_ratio(K, case):
    """the C ABI takes (Ho, Wo) and (rsh, rsw) independently.  The last column's window is widened to Wo - 1 (column 0's
    narrowed to 0), so its width depends on Wo; column 0's own upper end is bounded by the ratio (2.5 / rs + 2.5 < 4 / rs
    + 5), so the mirrored case exists only where column 0 is also the last (Wi = 1)."""
    Hi, Wi, Ho, Wo, rsh, rsw = case
    dy = seeded((1, 2, Ho, Wo), 341)
    ay, ax = _cubic_pair(Hi, Wi, Ho, Wo, rsh, rsw)
    c = max(C_BWD, 3 + 14 + Ho)         # the row loop may run over all Ho rows here
    _error_or_reference(K, lambda: K.bicubic_bwd(dy.to(DEV), Hi, Wi, rsh, rsw), "bicubic gather bwd, loose sizes",
                        f"bicubic_bwd {_sid(case)}", RU.resize_bwd(dy, ay, ax), RU.resize_bound(dy, ay, ax, c, backward=True))


@pytest.mark.parametrize("size,out", [((2, 2), (9, 9)), ((2, 2), (10, 10)), ((3, 3), (12, 12)), ((1, 1), (1, 20))], ids=_sid)
def test_bilinear_backward_at_the_edge_of_the_gather_window(K, size, out):
    """gd_bilinear_bwd forms its ratio from the sizes, so sizes and ratio cannot disagree; what remains is the edge of
    the window: x4 fits, x4.5 sits on the guard (2 / rs + 5 = 14 up to rounding), x5 and a 1 -> 20 column do not.
    For the same reason the widening of the last column's window to Wo - 1 in linear_window cannot be observed: with
    rs = Wi / Wo its unwidened end ceil((Wi + 0.5) / rs - 0.5) + 1 >= Wo + 1 already lies beyond the last output."""
    (Hi, Wi), (Ho, Wo) = size, out
    dy = seeded((1, 2, Ho, Wo), 342)
    ay, ax = RU.linear_axis(Hi, Ho), RU.linear_axis(Wi, Wo)
    _error_or_reference(K, lambda: K.bilinear_bwd(dy.to(DEV), Hi, Wi), "bilinear bwd, window edge",
                        f"bilinear_bwd {_sid(size)}->{_sid(out)}", RU.resize_bwd(dy, ay, ax),
                        RU.resize_bound(dy, ay, ax, C_BWD, backward=True))


# =====================================================================================================================
# 5. more than 65535 planes: the second launch of every sliced launcher
# =====================================================================================================================
def test_plane_slicing_second_launch(K):
    """B * C = 65535 + 4 planes of 2 x 2, every plane with its own seeded values, through the eight sliced launchers:
    a slice that read or wrote slice 0 again, or dropped the offset of one pointer, shows in the last four planes"""
    N = NPLANES
    x = seeded((N, 1, 2, 2), 351)
    xg = x.to(DEV)
    # bicubic forward and the fixed x2 backward
    ay, ax = _cubic_pair(2, 2, 4, 4, 0.5, 0.5)
    dy4 = seeded((N, 1, 4, 4), 352)
    _hold("bicubic x2 fwd", "sliced bicubic_fwd", K.bicubic_fwd(xg, 4, 4, 0.5, 0.5), RU.resize_fwd(x, ay, ax),
          RU.resize_bound(x, ay, ax, C_FWD_CUBIC))
    _hold("bicubic x2 bwd", "sliced bicubic_bwd (x2 route)", K.bicubic_bwd(dy4.to(DEV), 2, 2, 0.5, 0.5),
          RU.resize_bwd(dy4, ay, ax), RU.resize_bound(dy4, ay, ax, C_BWD, backward=True))
    # the gather route: 2 x 2 -> 3 x 3
    rs = RU.f32(2.0 / 3.0)
    by, bx = _cubic_pair(2, 2, 3, 3, rs, rs)
    dy3 = seeded((N, 1, 3, 3), 353)
    _hold("bicubic gather bwd", "sliced bicubic_bwd (gather route)", K.bicubic_bwd(dy3.to(DEV), 2, 2, rs, rs),
          RU.resize_bwd(dy3, by, bx), RU.resize_bound(dy3, by, bx, C_BWD, backward=True))
    # bilinear forward with res, and backward
    ly, lx = RU.linear_axis(2, 4), RU.linear_axis(2, 4)
    res = seeded((N, 1, 4, 4), 354)
    ref, bnd = RU.resize_fwd(x, ly, lx), RU.resize_bound(x, ly, lx, C_FWD_LINEAR)
    _hold("bilinear fwd + res", "sliced bilinear_fwd", K.bilinear_fwd(xg, 4, 4, res=res.to(DEV)), RU.f64(res) + ref,
          bnd + 1.01 * U * (np.abs(RU.f64(res)) + RU.abs_image(x, ly, lx) + bnd))
    _hold("bilinear bwd", "sliced bilinear_bwd", K.bilinear_bwd(dy4.to(DEV), 2, 2), RU.resize_bwd(dy4, ly, lx),
          RU.resize_bound(dy4, ly, lx, C_BWD, backward=True))
    # max-pool
    g = seeded((N, 1, 1, 1), 355)
    _exact("sliced maxpool2_fwd", K.maxpool2_fwd(xg), RU.maxpool2_fwd(x))
    _exact("sliced maxpool2_bwd", K.maxpool2_bwd(xg, g.to(DEV)), RU.maxpool2_bwd(x, g))


# =====================================================================================================================
# 6. the fused input preamble
# =====================================================================================================================
@pytest.mark.parametrize("out", [(5, 7), (3, 260)], ids=_sid)
def test_combine_inputs_odd_sources_and_channel_offsets(K, out):
    """B = 3, C1 = 2, C2 = 3: the plane index z -> (b, c) and the c - C1 offset count; odd source sizes where
    floor(H * s) drops a row or column: (2 Ho + 1, 2 Wo) and (4 Ho + 3, 4 Wo + 1).  Ratios 2 and 4: no coordinate part."""
    Ho, Wo = out
    lr, aux = seeded((3, 2, 2 * Ho + 1, 2 * Wo), 361), seeded((3, 3, 4 * Ho + 3, 4 * Wo + 1), 362, 2.0)
    ref, bound = RU.combine_inputs(lr, aux, 2.0, 4.0, Ho, Wo)
    got = K.combine_inputs(lr.to(DEV), aux.to(DEV), 0.5, 0.25)
    assert tuple(got.shape) == (3, 5, Ho, Wo)
    _hold("combine_inputs", f"combine_inputs {_sid(out)}", got, ref, bound)


def test_combine_inputs_refuses_sizes_that_do_not_meet(K):
    lr = seeded((3, 2, 11, 14), 363).to(DEV)
    for aux_shape in ((3, 3, 27, 29), (3, 3, 23, 33), (2, 3, 23, 29)):      # rows, columns, batch
        with pytest.raises(_err_type()):
            K.combine_inputs(lr, seeded(aux_shape, 364).to(DEV), 0.5, 0.25)


# =====================================================================================================================
# 7. the tap sum and its adjoint
# =====================================================================================================================
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 300), (2, 3, 257), (1, 5, 4)], ids=_sid)
def test_shift_sum9_forward_adjoint_and_bias_gradient(K, shape, with_bias):
    B, H, W = shape
    u, dy = seeded((B, 9, H, W), 371), seeded((B, 1, H, W), 372)
    bias = seeded((1,), 373) + 2.0 if with_bias else None
    ug = u.to(DEV).requires_grad_(True)
    bg = bias.to(DEV).requires_grad_(True) if with_bias else None
    y = _ops().ShiftSum9Fn.apply(ug, bg)
    y.backward(dy.to(DEV))
    what = f"shift_sum9 {_sid(shape)}"
    _hold("tap sum fwd", what + " y", y, RU.shift_sum9_fwd(u, bias), 10 * U * RU.shift_sum9_abs(u, bias))
    assert torch.equal(ug.grad.cpu(), torch.from_numpy(RU.shift_sum9_bwd(dy)).float()), what + ": adjoint is not the shifted copy"
    if with_bias:
        n = dy.numel()
        _hold("tap sum dbias", what + " dbias", bg.grad, RU.f64(dy).sum().reshape(1), n * U * np.abs(RU.f64(dy)).sum())
    # <fwd(u), dy> = <u, bwd(dy)> on the device outputs, in float64: the forward's ten roundings are all that separates them
    y0 = RU.f64(K.shift_sum9_fwd(u.to(DEV), None))
    du = RU.f64(K.shift_sum9_bwd(dy.to(DEV)))
    lhs, rhs = (y0 * RU.f64(dy)).sum(), (RU.f64(u) * du).sum()
    slack = (10 * U * RU.shift_sum9_abs(u) * np.abs(RU.f64(dy))).sum() + 1e-13 * abs(rhs)
    print(f"[resample] tap sum adjoint identity | {what}: err/bound {abs(lhs - rhs) / slack:.3e}")
    assert abs(lhs - rhs) <= slack, f"{what}: <fwd u, dy> = {lhs!r} but <u, bwd dy> = {rhs!r}"


# =====================================================================================================================
# 8. max-pool: ties, infinities, NaNs -- exact
# =====================================================================================================================
LEVELS = torch.tensor([0.0, 0.0, 1.7001, -1.2003, 0.3007, 2.5])


def _pool_plane(case):
    """(H, W) float32: the hand-built windows, or a plane quantised to five values so that ties are everywhere"""
    if case == "hand":
        return torch.from_numpy(RU.hand_plane()).float()
    H, W = case
    idx = torch.randint(0, len(LEVELS), (H, W), generator=torch.Generator().manual_seed(381 + W))
    return LEVELS[idx]


def _pool_tensor(case, C):
    """(2, C, H, W): channel c is the plane rolled by c windows, batch 1 is batch 0 upside down (other tie positions)"""
    p = _pool_plane(case)
    x0 = torch.stack([torch.roll(p, 2 * c, 1) for c in range(C)], 0)
    return torch.stack([x0, x0.flip(1)], 0).contiguous()


POOL_CASES = ["hand", (2, 2), (2, 514), (6, 4)]


def test_hand_windows_cover_the_issue_list():
    w = np.array(HAND_WINDOWS)
    pairs = {tuple(np.flatnonzero(r == 5.0)) for r in w if (r == 5.0).sum() == 2 and np.nanmax(r) == 5.0}
    assert pairs == {(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)}
    nan_at = {int(np.flatnonzero(np.isnan(r))[0]) for r in w if np.isnan(r).sum() == 1 and np.isfinite(r[~np.isnan(r)]).all()}
    assert nan_at == {0, 1, 2, 3}
    assert any((r == 0).all() and not np.signbit(r).any() for r in w) and any((r == -np.inf).all() for r in w)
    assert any((r == r[0]).all() and r[0] > 0 for r in w) and any((r == np.inf).sum() >= 2 for r in w)


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: c if isinstance(c, str) else _sid(c))
def test_maxpool2_nchw_ties_inf_nan(K, case):
    """float32 NCHW: the forward is the reference bit for bit (a window with a NaN gives NaN), the backward puts the
    gradient on the first maximum or on the NaN, as ATen does; (2, 514) runs a second x block"""
    x = _pool_tensor(case, 3)
    dy = seeded((2, 3, x.shape[2] // 2, x.shape[3] // 2), 382) + 3.0      # never zero: a misplaced gradient shows
    xg = x.to(DEV).requires_grad_(True)
    y = _ops().MaxPool2Fn.apply(xg)
    y.backward(dy.to(DEV))
    _exact(f"maxpool2 {case} y", y, RU.maxpool2_fwd(x))
    _exact(f"maxpool2 {case} dx", xg.grad, RU.maxpool2_bwd(x, dy))


def _to_nhwc(t, split):
    """(B, C, H, W) float32 -> the pixel-major bf16 device tensor and the logical float32 values it encodes.  split:
    [hi | lo | hi], hi = bf16(v), lo = bf16(v - hi); a non-finite v keeps lo = 0 (hi carries it: inf - inf has no lo)"""
    hi = bf16_round(t)
    if not split:
        return hi.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV), hi
    lo = torch.where(torch.isfinite(t), bf16_round(t - hi), torch.zeros_like(t))
    enc = torch.cat([hi, lo, hi], 1).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
    return enc, hi + lo


def _from_nhwc(t, split):
    """-> (hi plane, logical value) as (B, C, H, W) float32 on the CPU; split: both hi copies must agree bit for bit"""
    v = t.float().cpu().permute(0, 3, 1, 2).contiguous()
    if not split:
        return v, v
    C = v.shape[1] // 3
    assert torch.equal(v[:, :C].view(torch.int32), v[:, 2 * C:].view(torch.int32)), "the two hi copies differ"
    return v[:, :C], v[:, :C] + v[:, C:2 * C]


@pytest.mark.parametrize("relu_mask", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: c if isinstance(c, str) else _sid(c))
def test_maxpool2_pixel_major_ties_inf_nan(K, case, C, split, relu_mask):
    """bf16 and split pixel-major: forward bit for bit, backward on the first maximum (or the NaN), with relu_mask
    nothing where the maximum is not above 0 -- so the all-zero window passes nothing with the gate and passes its
    gradient to the FIRST element without it.  C = 24: three channel octets per pixel.  Split storage cannot hold an
    infinity in its lo part (inf - hi is a NaN): there the hi plane is checked and the logical value must be
    non-finite; everywhere else the logical value hi + lo is checked too."""
    x = _pool_tensor(case, C)
    if split:
        x = x * 1.0009765625 if case != "hand" else x           # values that need their lo part (1 + 2^-10)
    xe, xl = _to_nhwc(x, split)
    dy = seeded((2, C, x.shape[2] // 2, x.shape[3] // 2), 383) + 3.0
    de, dl = _to_nhwc(dy, split)
    what = f"nhwc maxpool2 {case} C={C} split={split} relu={relu_mask}"
    ref = RU.maxpool2_fwd(xl)
    hi, val = _from_nhwc(K.nhwc_maxpool2_fwd(xe, split=split), split)
    _exact(what + " y (hi plane)", hi, RU.f64(bf16_round(torch.from_numpy(ref).float())))
    fin = np.isfinite(ref)
    _exact(what + " y", np.where(fin, RU.f64(val), 0.0), np.where(fin, ref, 0.0))
    assert not np.isfinite(RU.f64(val))[~fin].any(), what + ": a non-finite maximum came out finite"
    assert np.isnan(RU.f64(val))[np.isnan(ref)].all(), what + ": a NaN in the window did not give NaN"
    _, dx = _from_nhwc(K.nhwc_maxpool2_bwd(xe, de, relu_mask, split=split), split)
    _exact(what + " dx", dx, RU.maxpool2_bwd(xl, dl, relu_mask=relu_mask))
