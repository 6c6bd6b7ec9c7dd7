"""GPU: the split weight gradients in their default form -- every split stores a partial slab, det_reduce.hip adds the
slabs in ascending order, no atomics and no zero-fill.

Per shape: (a) the host plan says the launch splits at least three ways and that its last split is partial, (b) against
an fp64 CPU weight gradient of the same 16-bit-rounded operands every element is within 4 K 2^-24 sum|terms| (K terms
per element accumulated in fp32: the a-priori bound, whatever the order of the additions; the products of two bf16
values are exact in fp32), (c) two default-mode calls are bit-equal, (d) the default and
set_deterministic(True, reduce="ordered") are bit-equal, (e) the destination is filled with NaN before the call and
comes back finite: it is neither zeroed by a separate launch nor read.

Shapes: the smallest that split >= 3 ways with a partial last split and channel counts that are no multiple of the
32-channel tile.  The 3x3 launcher gives split = ceil(tiles / min(1024 / workgroups per split, tiles)) tiles of 4 x 32
pixels, so a partial last split needs more than 1024 / workgroups tiles: 2 x 257 x 2 = 1028 tiles in 343 splits of 3 (the
last has 2) for 40 -> 24, 343 tiles in 172 splits of 2 (the last has 1) for 72 -> 40.  The D-trunk layer on 32 x 32 has
four tiles per image: 12 splits of one (partial: 16 of 32 columns) tile at B = 3; a partial last SPLIT there would need
B > 128.  The 1x1 gradient splits its 100 k-tiles of 32 pixels into 12 splits of 9 (the last has 1)."""
import contextlib
import ctypes as C

import pytest
import torch

from gpu_util import DEV, bf16_round, seeded

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def gd():
    import gan_danet_amd as g
    from gan_danet_amd import _lib
    _lib.load()
    return g


def _K():
    from gan_danet_amd import kern
    return kern


@contextlib.contextmanager
def _det_ordered(gd):
    gd.set_deterministic(True, reduce="ordered")
    try:
        yield
    finally:
        gd.set_deterministic(False, reduce="unsplit")


def _wgrad64(x, dy, stride, k, pad):
    return torch.nn.grad.conv2d_weight(x.double(), (dy.shape[1], x.shape[1], k, k), dy.double(), stride=stride, padding=pad)


def _bound_check(got, ref, mag, kterms, what):
    """|got - ref| <= 4 K 2^-24 sum|terms| on every element; prints the largest ratio of the error to K 2^-24 sum|terms|"""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite result"
    unit = kterms * EPS * mag
    ratio = ((got - ref).abs() / unit.clamp_min(1e-300)).max().item()
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"{what}: K = {kterms}, max |err| / (K 2^-24 sum|terms|) = {ratio:.3e} (bound 4), rel-L2 {rel:.3e}")
    assert ratio <= 4.0, f"{what}: error {ratio:.3e} x K 2^-24 sum|terms| exceeds 4"


def _same_bits(a, b, what):
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


def _properties(gd, run, ref, mag, kterms, what):
    """run(dst) fills dst; (b) .. (e) of the module docstring"""
    def call():
        dst = torch.full(ref.shape, float("nan"), device=DEV, dtype=torch.float32)
        run(dst)
        return dst
    d1, d2 = call(), call()
    with _det_ordered(gd):
        o = call()
    _bound_check(d1, ref, mag, kterms, what)
    _same_bits(d1, d2, f"{what}: two default-mode calls")
    _same_bits(d1, o, f"{what}: default against reduce='ordered'")
    return d1


# name -> (B, Cin, H, W, Cout, stride, expected splits, tiles in the last split, tiles in the others)
CASES3 = {
    "40to24": (2, 40, 1027, 40, 24, 1, 343, 2, 3),
    "72to40": (1, 72, 1371, 30, 40, 1, 172, 1, 2),
    "trunk_s2_64to128": (3, 64, 32, 32, 128, 2, 12, 1, 1),
}


@pytest.fixture(scope="module")
def refs3():
    """operands and fp64 references of the 3x3 cases, computed once"""
    out = {}
    for i, (name, (B, Cin, H, W, Cout, stride, *_)) in enumerate(sorted(CASES3.items())):
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        x, dy = bf16_round(seeded((B, Cin, H, W), 801 + 2 * i)), bf16_round(seeded((B, Cout, Ho, Wo), 802 + 2 * i))
        out[name] = (x, dy, _wgrad64(x, dy, stride, 3, 1), _wgrad64(x.abs(), dy.abs(), stride, 3, 1))
    return out


@pytest.mark.parametrize("case", sorted(CASES3))
def test_conv3x3_wgrad_default_is_ordered(gd, refs3, case):
    K = _K()
    B, Cin, H, W, Cout, stride, want_splits, last, per = CASES3[case]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, dy, ref, mag = refs3[case]
    splits = K.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride)[0]
    ntiles = B * ((Wo + 31) // 32) * ((Ho + 3) // 4)
    assert splits == want_splits >= 3 and ntiles - (splits - 1) * per == last                                # (a)
    assert Cin % 32 != 0 or Cout % 32 != 0 or case.startswith("trunk")
    x16 = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)          # pixel-major, as the forward packs it
    if case.startswith("trunk"):
        # the D trunk's route: the pixel-major gradient goes channel-major in the pass that also sums the bias gradient
        g = dy.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
        dy16, db = K.nhwc_to_nchw16(g, True)
        db2 = K.nhwc_to_nchw16(g, True)[1]
        with _det_ordered(gd):
            dbo = K.nhwc_to_nchw16(g, True)[1]
        _bound_check(db, dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3)), B * Ho * Wo, f"{case} bias")
        _same_bits(db, db2, f"{case} bias: two default-mode calls")
        _same_bits(db, dbo, f"{case} bias: default against reduce='ordered'")
        dy16 = dy16.view(B, Cout, Ho * Wo)
    else:
        dy16 = dy.reshape(B, Cout, Ho * Wo).to(torch.bfloat16).to(DEV)

    def run(dw, accumulate=0):
        from gan_danet_amd import _lib as L
        L.check(K.lib().gd_conv3x3_wgrad_ws(None, 0, dy16.data_ptr(), None, 0, x16.data_ptr(), Cin, None, None, 0, B, Cout, Cin,
                                            H, W, stride, accumulate, dw.data_ptr(), K._stream(), *K.det_ws()), "gd_conv3x3_wgrad")
    d = _properties(gd, run, ref, mag, B * Ho * Wo, case)
    # accumulate: the sum kernel adds what dw held, in the same pass
    base = seeded(tuple(ref.shape), 899, 3.0)
    acc = base.to(DEV).clone()
    run(acc, 1)
    _same_bits(acc, base.to(DEV) + d, f"{case}: accumulate")


@pytest.fixture(scope="module")
def ref1():
    B, Cn, H, W = 2, 40, 40, 40
    x, dy = bf16_round(seeded((B, Cn, H, W), 811)), bf16_round(seeded((B, Cn, H, W), 812))
    return x, dy, _wgrad64(x, dy, 1, 1, 0), _wgrad64(x.abs(), dy.abs(), 1, 1, 0)


def test_conv1x1_wgrad_default_is_ordered(gd, ref1):
    from gan_danet_amd import _lib as L
    K = _K()
    x, dy, ref, mag = ref1
    B, Cn, H, W = x.shape
    splits = K.gemm_nt_plan(B=1, M=Cn, N=Cn, kseg=B, klen=H * W)[0]
    ktiles = B * H * W // 32
    per = -(-ktiles // 12)
    assert splits == 12 and 0 < ktiles - (splits - 1) * per < per                                            # (a)
    xg, dyg = x.to(DEV), dy.to(DEV)

    def run(dw):
        K._conv2d_wgrad(dyg, xg, 1, 1, 0, L.PREC_BF16, None, None, False, dw, Cn * H * W, Cn * H * W, B, Cn, Cn, H, W, H, W)
    _properties(gd, run, ref, mag, B * H * W, "1x1 40 -> 40")


def test_gemm_nt_accumulate_alpha_default_is_ordered(gd, ref1):
    """the accumulate + alpha form (the fp16-PAM s_inv scale, a second pass into one gradient): c += alpha dY X^T.  The bound
    gains one rounding for the product with alpha and one for the addition onto c: (K + 2) terms' worth on
    alpha sum|terms| + |c|"""
    from gan_danet_amd import _lib as L
    K = _K()
    x, dy, ref, mag = ref1
    B, Cn, H, W = x.shape
    N = H * W
    alpha = torch.tensor([0.37], device=DEV)
    al = float(alpha.double().item())
    c0 = seeded((Cn, Cn), 813, 50.0)
    want = c0.double() + al * ref.view(Cn, Cn)
    wmag = c0.double().abs() + abs(al) * mag.view(Cn, Cn)
    xg, dyg = x.to(DEV), dy.to(DEV)

    def call():
        c = c0.to(DEV).clone()
        K.gemm_nt(B=1, M=Cn, N=Cn, kseg=B, klen=N, a=dyg, a_bs=0, a_ss=Cn * N, lda=N, bm=xg, b_bs=0, b_ss=Cn * N, ldb=N, c=c,
                  c_bs=0, ldc=Cn, precision=L.PREC_BF16, alpha=alpha, accumulate=True)
        return c
    assert K.gemm_nt_plan(B=1, M=Cn, N=Cn, kseg=B, klen=N)[0] == 12
    d1, d2 = call(), call()
    with _det_ordered(gd):
        o = call()
    _bound_check(d1, want, wmag, B * N + 2, "1x1 accumulate + alpha")
    _same_bits(d1, d2, "accumulate + alpha: two default-mode calls")
    _same_bits(d1, o, "accumulate + alpha: default against reduce='ordered'")


def test_atomic_mode_stays_reachable(gd, ref1):
    """set_split_reduce("atomic") is the old default: same plan, no workspace, same bound"""
    from gan_danet_amd import _lib as L
    K = _K()
    x, dy, ref, mag = ref1
    B, Cn, H, W = x.shape
    xg, dyg = x.to(DEV), dy.to(DEV)
    K.set_split_reduce("atomic")
    try:
        assert K.lib().gd_get_split_reduce() == 1
        assert K.gemm_nt_plan(B=1, M=Cn, N=Cn, kseg=B, klen=H * W) == (12, 0)
        dw = K.conv2d_wgrad(dyg, xg, 1, 1, 0, L.PREC_BF16)
    finally:
        K.set_split_reduce("ordered")
    assert K.lib().gd_get_split_reduce() == 0
    _bound_check(dw, ref, mag, B * H * W, "1x1 atomic")
    with pytest.raises(L.GandanetError):
        K.set_split_reduce("nonsense")
    assert K.SPLIT_REDUCE == "ordered" and C.c_int(K.lib().gd_get_split_reduce()).value == 0
