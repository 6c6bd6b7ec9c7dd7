"""GPU: every convolution route on data for which the arithmetic is exact, compared with torch.equal (zero tolerance).

Operands are small integers (conv_exact_util.py), so every product is an exact integer in fp32 and every partial sum stays
below 2^24: fp32 accumulation is exact in any order, tiling, split-K and MFMA shape, with atomics or ordered slabs alike, and
the kernel must return the fp64 reference bit for bit.  One missing, doubled or mis-paired product -- the last channel of a
ragged 32-channel chunk, a patch column at a 32-pixel tile seam, a tap skipped for one parity class, one of the three
split-bf16 products of one fragment -- changes an integer and fails the test.  The split ("x3") routes run on hi + lo
operands against the three-term reference (hi hi + lo hi + hi lo; the kernels omit lo lo by design).  bf16- and
split-stored outputs are compared with the ONE deterministic rounding of the exact fp32 value.
tests/test_conv_exact_reference.py checks on the host that every row here meets these conditions.

The case tables (conv_exact_util.py) are derived from the launch code; each row names the branch it reaches, and the tests
assert the tile choice (and, where a host plan function exists, the plan) before they run the kernel."""
import contextlib

import pytest
import torch

import conv_exact_util as U
from conv_exact_util import assert_same
from gpu_util import DEV

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def gd():
    import gan_danet_amd as g
    from gan_danet_amd import _lib
    _lib.load()
    return g


def _KL():
    from gan_danet_amd import _lib, kern
    return kern, _lib


def _prec(L, p):
    return {"fp32": L.PREC_FP32, "bf16": L.PREC_BF16, "x3": L.PREC_X3}[p]


def _d(t):
    return None if t is None else t.to(DEV)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _slab(t, lead=4, trail=4):
    """t as the channel slice [lead : lead + C] of a NaN-filled slab -> (slab, view)"""
    B, Cn = t.shape[:2]
    s = _nan(B, lead + Cn + trail, *t.shape[2:])
    v = s[:, lead:lead + Cn]
    v.copy_(t.to(DEV))
    return s, v


def _neighbours_are_nan(slab, Cn, what, lead=4):
    assert slab[:, :lead].isnan().all() and slab[:, lead + Cn:].isnan().all(), f"{what}: wrote outside its channel slice"


@contextlib.contextmanager
def _generic_only(K):
    old = K.USE_CONV3X3_FAST
    K.USE_CONV3X3_FAST = False
    try:
        yield
    finally:
        K.USE_CONV3X3_FAST = old


def _conv_nn_fwd(K, x, w, stride, pad, prec, y, y_bs, **kw):
    """forward gather through K.conv_nn with the whole descriptor in reach (res, alpha, Mstore, out_layout, ...)"""
    B, Cin, Hi, Wi = x.shape
    Cout, _, k, _ = w.shape
    Ho, Wo = K.conv_out_size(Hi, k, stride, pad), K.conv_out_size(Wi, k, stride, pad)
    K.conv_nn(B=B, M=Cout, Ck=Cin, ks=k, stride=stride, pad=pad, transposed=False, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, a=w, a_bs=0,
              a_sm=Cin * k * k, a_sc=k * k, a_st=1, x=x, x_bs=K._bview(x), y=y, y_bs=y_bs, precision=prec, **kw)


# ---- a. halo / patch kernel ------------------------------------------------------------------------------------------
def _halo_eligible(K, L, B, M, Ck, Hi, Wi, Ho, Wo, stride, transposed):
    import ctypes as C
    d = L.ConvDesc()
    d.B, d.M, d.Mstore, d.Ck, d.ks, d.stride, d.pad, d.transposed = B, M, M, Ck, 3, stride, 1, int(transposed)
    d.Hi, d.Wi, d.Ho, d.Wo, d.precision = Hi, Wi, Ho, Wo, L.PREC_BF16
    return bool(K.lib().gd_conv3x3_eligible(C.byref(d)))


@pytest.mark.parametrize("name", sorted(U.HALO))
def test_halo_patch_kernel(gd, name):
    """gd_conv3x3 = conv3x3_halo_kernel<64|128, 8|4, 1|2> through K.conv2d_fwd / K.conv2d_dgrad with PREC_BF16: prologue +
    bias + ReLU from a channel slice of a NaN-filled slab into a channel slice of another (the neighbours stay NaN),
    accumulate, and the data gradient (transposed) over a NaN-filled output"""
    K, L = _KL()
    B, Cin, H, W, Cout, stride, fbm, dbm = U.HALO[name]
    e = U.halo_expect(name)
    o = e.ops
    Ho, Wo = o["Ho"], o["Wo"]
    assert K.USE_CONV3X3_FAST and U.pick_bm(Cout, Cin) == fbm
    assert _halo_eligible(K, L, B, Cout, Cin, H, W, Ho, Wo, stride, False)
    w, bias, sc, sh = _d(o["w"]), _d(o["bias"]), _d(o["sc"]), _d(o["sh"])
    xs, x = _slab(o["x"])
    ys, y = _slab(torch.full((B, Cout, Ho, Wo), NAN))
    K.conv2d_fwd(x, w, bias, stride, 1, L.PREC_BF16, act=L.ACT_RELU, out=y, in_scale=sc, in_shift=sh, in_relu=True)
    assert_same(y, e.stored("prologue_bias_relu"), f"{name}: prologue + bias + ReLU, slab to slab")
    _neighbours_are_nan(ys, Cout, name)
    acc = _d(o["base"]).clone()
    K.conv2d_fwd(x, w, None, stride, 1, L.PREC_BF16, out=acc, accumulate=True)
    assert_same(acc, e.stored("accumulate"), f"{name}: accumulate")
    if dbm is not None:
        assert U.pick_bm(Cin, Cout) == dbm and _halo_eligible(K, L, B, Cin, Cout, H, W, H, W, 1, True)
        dxs, dx = _slab(torch.full((B, Cin, H, W), NAN))
        K.conv2d_dgrad(_d(o["dy"]), w, (H, W), 1, 1, L.PREC_BF16, out=dx)
        assert_same(dx, e.stored("dgrad"), f"{name}: data gradient")
        _neighbours_are_nan(dxs, Cin, name + " dgrad")


def test_conv3x3_shift_property_small(gd):
    """the one-hot-tap shift of test_gpu_modules.test_conv3x3_full_size_shift_property at a size with ragged tiles"""
    K, L = _KL()
    x = U.ints((1, 2, 17, 65), 91, U.BIAS_VALS)
    w = torch.zeros(2, 2, 3, 3)
    w[0, 1, 0, 2] = 1.0
    w[1, 0, 2, 1] = 1.0
    y = K.conv2d_fwd(_d(x), _d(w), None, 1, 1, L.PREC_BF16)
    assert_same(y, U.to_store(U.conv(x, w, 1, 1), "f32", U.conv(x.abs(), w.abs(), 1, 1)), "one-hot taps")


# ---- b. generic implicit-GEMM kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", U.PRECS)
@pytest.mark.parametrize("name", sorted(U.GENERIC))
def test_generic_conv(gd, name, prec):
    """gd_conv2d = conv_nn_kernel<32|64|128, F32|BF16|X3> with the patch kernel switched off: forward with prologue + bias +
    ReLU and with bias + the baked-in LeakyReLU(0.2) (one fp32 multiply), the data gradient over NaN (a strided one runs as
    one launch per output parity class with tap skipping; classes without a live tap must come back exactly 0), and the
    data gradient with a device alpha = 2 and accumulate.  X3 runs on hi + lo operands."""
    K, L = _KL()
    B, Cin, H, W, Cout, ks, stride, pad, fbm, dbm = U.GENERIC[name]
    assert U.generic_bm(Cout) == fbm and U.generic_bm(Cin) == dbm
    e = U.generic_expect(name, prec)
    o = e.ops
    p = _prec(L, prec)
    x, w, dy, bias = _d(o["x"]), _d(o["w"]), _d(o["dy"]), _d(o["bias"])
    with _generic_only(K):
        y = K.conv2d_fwd(x, w, bias, stride, pad, p, act=L.ACT_RELU, in_scale=_d(o["sc"]), in_shift=_d(o["sh"]), in_relu=True,
                         out=_nan(B, Cout, o["Ho"], o["Wo"]))
        assert_same(y, e.stored("prologue_bias_relu"), f"{name} {prec}: prologue + bias + ReLU")
        y = K.conv2d_fwd(x, w, bias, stride, pad, p, act=L.ACT_LEAKY02, out=_nan(B, Cout, o["Ho"], o["Wo"]))
        assert_same(y, e.stored("bias_leaky02"), f"{name} {prec}: bias + LeakyReLU(0.2)")
        dx = K.conv2d_dgrad(dy, w, (H, W), stride, pad, p, out=_nan(B, Cin, H, W))
        assert_same(dx, e.stored("dgrad"), f"{name} {prec}: data gradient")
        if name == "k1s2p0":
            assert (dx[..., 1::2, :] == 0).all() and (dx[..., :, 1::2] == 0).all(), "a class without a live tap is not 0"
        acc = _d(o["dres"]).clone()
        K.conv2d_dgrad(dy, w, (H, W), stride, pad, p, out=acc, accumulate=True, alpha=torch.tensor([2.0], device=DEV))
        assert_same(acc, e.stored("dgrad_alpha_accumulate"), f"{name} {prec}: data gradient, alpha = 2, accumulate")


@pytest.mark.parametrize("prec", U.PRECS)
def test_generic_conv_descriptor_features(gd, prec):
    """the descriptor features of gd_conv2d that only K.conv_nn reaches: out_layout = 1 (pixel-major rows of ldo > Mstore
    elements), out_bf16, Mstore > M (padding rows exactly act(0) = 0, nothing written beyond Mstore / ldo), res, a device
    alpha (a power of two) and accumulate"""
    K, L = _KL()
    B, Ck, H, W, M, Mstore, ldo = U.DESC
    HW = H * W
    assert U.generic_bm(Mstore) == 64 and ldo > Mstore > M
    e = U.desc_expect(prec)
    o = e.ops
    p = _prec(L, prec)
    alpha = torch.tensor([2.0], device=DEV)

    def from_rows(y):       # (B, HW, ldo) -> (B, Mstore, H, W); the columns beyond Mstore must be untouched
        assert y[:, :, Mstore:].isnan().all(), "wrote beyond Mstore"
        return y[:, :, :Mstore].permute(0, 2, 1).reshape(B, Mstore, H, W).contiguous()
    y = _nan(B, HW, ldo, dtype=torch.bfloat16)
    _conv_nn_fwd(K, _d(o["x_int"]), _d(o["w_int"]), 1, 1, p, y, HW * ldo, Mstore=Mstore, out_layout=1, out_bf16=True, ldo=ldo,
                 bias=_d(o["bias"]), act=L.ACT_RELU)
    assert_same(from_rows(y), e.stored("layout1_bf16_bias_relu")[0], f"{prec}: out_layout 1, bf16, bias + ReLU")
    x, w, res = _d(o["x"]), _d(o["w"]), _d(o["res"])
    y = _nan(B, HW, ldo)
    _conv_nn_fwd(K, x, w, 1, 1, p, y, HW * ldo, Mstore=Mstore, out_layout=1, ldo=ldo, res=res, res_bs=M * HW, alpha=alpha)
    assert_same(from_rows(y), e.stored("layout1_res_alpha"), f"{prec}: out_layout 1, res, alpha = 2")
    y = _d(o["base48"]).clone()
    _conv_nn_fwd(K, x, w, 1, 1, p, y, Mstore * HW, Mstore=Mstore, res=res, res_bs=M * HW, alpha=alpha, accumulate=True)
    assert_same(y, e.stored("layout0_res_alpha_accumulate"), f"{prec}: Mstore > M, res, alpha = 2, accumulate")


# ---- c. 1x1 transpose-read kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "x3"])
@pytest.mark.parametrize("name", sorted(U.ONE))
def test_conv1x1_transpose_read(gd, name, prec):
    """conv1x1_tr_plain_kernel<32|64|128, X3?> (H W % 4 == 0) and, at H W = 35, the generic kernel it falls back to:
    prologue + bias + ReLU, res + accumulate, and the data gradient; x3 on hi + lo operands"""
    K, L = _KL()
    B, Cin, H, W, Cout, fbm, dbm, fast = U.ONE[name]
    assert U.generic_bm(Cout) == fbm and U.generic_bm(Cin) == dbm and ((H * W) % 4 == 0) == fast
    e = U.one_expect(name, prec)
    o = e.ops
    p = _prec(L, prec)
    x, w = _d(o["x"]), _d(o["w"])
    assert x.data_ptr() % 16 == 0
    y = K.conv2d_fwd(x, w, _d(o["bias"]), 1, 0, p, act=L.ACT_RELU, in_scale=_d(o["sc"]), in_shift=_d(o["sh"]), in_relu=True,
                     out=_nan(B, Cout, H, W))
    assert_same(y, e.stored("prologue_bias_relu"), f"{name} {prec}: prologue + bias + ReLU")
    acc = _d(o["base"]).clone()
    _conv_nn_fwd(K, x, w, 1, 0, p, acc, Cout * H * W, res=_d(o["res"]), res_bs=Cout * H * W, accumulate=True)
    assert_same(acc, e.stored("res_accumulate"), f"{name} {prec}: res + accumulate")
    dx = K.conv2d_dgrad(_d(o["dy"]), w, (H, W), 1, 0, p, out=_nan(B, Cin, H, W))
    assert_same(dx, e.stored("dgrad"), f"{name} {prec}: data gradient")


# ---- d. pixel-major kernels ------------------------------------------------------------------------------------------
def _nhwc(t):
    """packed by hand: (B, C, H, W) fp32 host -> (B, H, W, C) bf16 device"""
    return t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)


def _nhwc_split(t):
    """packed by hand: -> (B, H, W, 3 C) bf16 device, [hi | lo | hi]"""
    hi, lo = U.split(t)
    return torch.cat([hi, lo, hi], 1).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)


def _pack(K, t, split):
    """packed by the project's own packers, checked against the hand-built copy so that a pack bug and a conv bug can be
    told apart"""
    B, Cn, H, W = t.shape
    if split and (H * W) % 8 != 0:          # gd_pack_16_split needs H W % 8 == 0: such rows run on the hand-built copy alone
        hand = _nhwc_split(t)
        return hand, hand
    if split:
        p = K.pack_split(_d(t))[1].view(B, H, W, 3 * Cn)
        hand = _nhwc_split(t)
    else:
        p = K.pack_bf16(_d(t), Cn, H * W, t_shape=(H * W, Cn))[1].view(B, H, W, Cn)
        hand = _nhwc(t)
    assert_same(p, hand.cpu(), "packer against the hand-built pixel-major copy")
    return p, hand


def _check_pm(y, e, key, split, what):
    """a pixel-major result (B, H, W, [3] M) against the stored form of expectation ``key``"""
    v = y.cpu().permute(0, 3, 1, 2).contiguous()
    if not split:
        return assert_same(v, e.stored(key)[0], what)
    M = v.shape[1] // 3
    hi, lo = e.stored(key)
    assert_same(v[:, :M].contiguous(), hi, what + ": hi plane")
    assert_same(v[:, M:2 * M].contiguous(), lo, what + ": lo plane")
    assert_same(v[:, 2 * M:].contiguous(), hi, what + ": second hi plane")


NHWC_S1_ROWS = [(n, False) for n in sorted(U.NHWC_S1)] + [(n, True) for n in U.NHWC_S1_SPLIT]


@pytest.mark.parametrize("name,split", NHWC_S1_ROWS, ids=[f"{n}-{'split' if s else 'plain'}" for n, s in NHWC_S1_ROWS])
def test_conv3x3_nhwc_stride1(gd, name, split):
    """conv3x3_nhwc_kernel<64|128, 1, EPI = 1> through K.conv3x3_nhwc: forward with bias + ReLU on the packers' output, the
    data-gradient operator with mask and res on hand-packed operands; <64|128, 1, EPI = 0> through K.conv3x3_nhwc_f32out
    into a channel slice of a NaN-filled slab (y_bs > M H W)"""
    K, L = _KL()
    B, Cin, H, W, Cout = U.NHWC_S1[name]
    ph = 3 if split else 1
    e = U.nhwc_s1_expect(name, split)
    o = e.ops
    w = _d(o["w"])
    xp, xhand = _pack(K, o["x"], split)
    y = K.conv3x3_nhwc(xp, K.conv3x3_operator(w, "fwd", split), _d(o["bias"]), Cout, relu=True, split=split)
    _check_pm(y, e, "fwd_bias_relu", split, f"{name}: forward, bias + ReLU (BM {U.pick_bm(Cout, ph * Cin)})")
    pk = _nhwc_split if split else _nhwc
    dx = K.conv3x3_nhwc(pk(o["dy"]), K.conv3x3_operator(w, "dgrad", split), None, Cin, mask=pk(o["mask"]), res=pk(o["dres"]),
                        split=split)
    _check_pm(dx, e, "dgrad_mask_res", split, f"{name}: data gradient, mask + res (BM {U.pick_bm(Cin, ph * Cout)})")
    if "f32out" in e.wants:
        ys, out = _slab(torch.full((B, Cout, H, W), NAN))
        K.conv3x3_nhwc_f32out(xhand.view(B, H * W, Cin), K.conv3x3_operator(w, "fwd"), _d(o["bias"]), Cout, H, W, relu=True, out=out)
        assert_same(out, e.stored("f32out"), f"{name}: fp32 NCHW epilogue into a slab slice")
        _neighbours_are_nan(ys, Cout, name + " f32out")


NHWC_S2_ROWS = [(n, False) for n in sorted(U.NHWC_S2)] + [(n, True) for n in U.NHWC_S2_SPLIT]


@pytest.mark.parametrize("name,split", NHWC_S2_ROWS, ids=[f"{n}-{'split' if s else 'plain'}" for n, s in NHWC_S2_ROWS])
def test_conv3x3_nhwc_stride2(gd, name, split):
    """conv3x3_nhwc_kernel<64|128, 2, 1> (act 0 / 1 / 2 with slope 0.25), conv3x3_nhwc_dgrad2_kernel by input parity with the
    LeakyReLU mask (slope 0.25) at odd H and W, and K.conv3x3_wgrad_nhwc with its bias sums (one launch, or the three
    accumulating launches of the split form)"""
    K, L = _KL()
    B, Cin, H, W, Cout, act = U.NHWC_S2[name]
    assert H % 2 == 1 and W % 2 == 1
    e = U.nhwc_s2_expect(name, split)
    o = e.ops
    w = _d(o["w"])
    xp, _ = _pack(K, o["x"], split)
    code = {None: 0, "relu": 1, "leaky": 2}[act]
    y = K.conv3x3_nhwc_s2(xp, K.conv3x3_operator(w, "fwd", split), _d(o["bias"]), Cout, code, U.SLOPE, split=split)
    _check_pm(y, e, "fwd", split, f"{name}: stride-2 forward, act {act}")
    pk = _nhwc_split if split else _nhwc
    dyp = pk(o["dy"])
    dx = K.conv3x3_nhwc_s2_dgrad(dyp, K.conv3x3_operator(w, "dgrad_s2", split), pk(o["mask"]), U.SLOPE, split=split)
    _check_pm(dx, e, "dgrad_leaky", split, f"{name}: stride-2 data gradient by parity, LeakyReLU mask")
    dw, db = K.conv3x3_wgrad_nhwc(dyp, xp, 2, True, split=split)
    assert_same(dw, e.stored("wgrad_nhwc"), f"{name}: weight gradient from pixel-major operands")
    assert_same(db, e.stored("bias_sums"), f"{name}: bias sums")


@pytest.mark.parametrize("route", ["wide", "x3"])
def test_ops_packed_routes(gd, route):
    """ops._wide3x3 (16-bit mode) and ops._x3_eligible (operand mode "x3", hi + lo operands) through
    ops.conv2d(...).backward: y, dx, dw, db"""
    from gan_danet_amd import ops
    e = U.ops_expect(route)
    o = e.ops
    xg, wg, bg = (_d(o[k]).requires_grad_(True) for k in ("x", "w", "bias"))
    assert ops.CONV_WIDE_NHWC
    if route == "wide":
        ctx = [gd.precision("bf16")]
    else:
        ctx = [gd.precision("fp32"), gd.layer_override(other="x3")]
    with contextlib.ExitStack() as st:
        for c in ctx:
            st.enter_context(c)
        if route == "wide":
            assert ops._wide3x3(xg, wg, 1, 1, ops.ACT_RELU, ops._prec("other"))
        else:
            assert ops._x3("other") and ops._x3_eligible(xg, wg, 1, 1, ops.ACT_RELU)
        y = ops.conv2d(xg, wg, bg, 1, 1, ops.ACT_RELU)
        y.backward(_d(o["dy"]))
    for key, t in (("y", y), ("dx", xg.grad), ("dw", wg.grad), ("db", bg.grad)):
        assert_same(t, e.stored(key), f"{route}: {key}")


# ---- e. weight gradients ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _mode(gd, K, mode):
    if mode == "atomic":
        K.set_split_reduce("atomic")
    elif mode != "default":
        gd.set_deterministic(True, reduce=mode)
    try:
        yield
    finally:
        K.set_split_reduce("ordered")
        gd.set_deterministic(False, reduce="unsplit")


MODES = ("default", "atomic", "ordered", "unsplit")


def _wgrad3_branch(Cout, Cin, stride, form):
    """the launch branch of gd_conv3x3_wgrad_ws, restated: (NW, CS, PIPED)"""
    nw = min((2, 4, 6), key=lambda n: (-(-Cout // (32 * n)) * 32 * n, -n))
    chunks = -(-Cin // 32)
    cs = Cout <= 32 and stride == 1 and chunks >= 3
    if cs:
        groups = (chunks + 3) // 4
        return -(-chunks // groups), True, form == "16"
    piped = form == "16" and (nw >= 4 if stride == 1 else nw == 4)
    return nw, False, piped


WGRAD3_BRANCH = {"cs3_piped": (3, True, True), "cs4_piped": (4, True, True), "cs3_f32": (3, True, False),
                 "cs4_f32": (4, True, False), "nw4_piped": (4, False, True), "nw6_piped": (6, False, True),
                 "nw2_s1": (2, False, False), "nw4_s1": (4, False, False), "nw6_s1": (6, False, False),
                 "nw4_s2_piped": (4, False, True), "nw2_s2": (2, False, False), "nw4_s2": (4, False, False),
                 "nw6_s2": (6, False, False)}


@pytest.mark.parametrize("name", sorted(U.WGRAD3))
def test_conv3x3_wgrad_every_branch_every_reduce_mode(gd, name):
    """gd_conv3x3_wgrad_ws = conv3x3_wgrad_kernel<NW, S, CS, PIPED, ORD>: every launch branch under the default slab mode,
    set_split_reduce("atomic"), and set_deterministic(True, reduce = "ordered" / "unsplit").  All four must give the same
    exact integers; accumulate adds onto what dw held."""
    K, L = _KL()
    B, Cin, H, W, Cout, stride, form, pro = U.WGRAD3[name]
    assert _wgrad3_branch(Cout, Cin, stride, form) == WGRAD3_BRANCH[name]
    e = U.wgrad3_expect(name)
    o = e.ops
    Ho, Wo = o["Ho"], o["Wo"]
    sc, sh = (_d(o["sc"]), _d(o["sh"])) if pro else (None, None)
    if form == "16":
        dy16 = o["dy"].reshape(B, Cout, Ho * Wo).to(torch.bfloat16).to(DEV)
        x16 = o["x"].permute(0, 2, 3, 1).reshape(B, H * W, Cin).contiguous().to(torch.bfloat16).to(DEV)
        args = (None, 0, dy16.data_ptr(), None, 0, x16.data_ptr(), Cin, None, None, 0)
    else:
        dy, x = _d(o["dy"]), _d(o["x"])
        args = (dy.data_ptr(), Cout * Ho * Wo, None, x.data_ptr(), Cin * H * W, None, 0, K._ptr(sc), K._ptr(sh), int(pro))

    def run(dw, accumulate):
        L.check(K.lib().gd_conv3x3_wgrad_ws(*args, B, Cout, Cin, H, W, stride, accumulate, dw.data_ptr(), K._stream(),
                                            *K.det_ws()), "gd_conv3x3_wgrad")
    for mode in MODES:
        with _mode(gd, K, mode):
            splits = K.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride)[0]
            assert (splits == 1) if mode == "unsplit" else (splits > 1), f"{name} {mode}: {splits} splits"
            dw = _nan(Cout, Cin, 3, 3)
            run(dw, 0)
            assert_same(dw, e.stored("dw"), f"{name} {mode}: dw")
            acc = _d(o["dw0"]).clone()
            run(acc, 1)
            assert_same(acc, e.stored("accumulate"), f"{name} {mode}: accumulate")


def test_conv3x3_wgrad_split_three_launches(gd):
    """K.conv3x3_wgrad16(split = True): dy_hi x_hi + dy_lo x_hi + dy_hi x_lo as three accumulating launches on the packers'
    hi + lo operands"""
    K, L = _KL()
    B, Cin, H, W, Cout = U.WGRAD3_SPLIT
    e = U.wgrad3_split_expect()
    o = e.ops
    dyp = K.pack_split(_d(o["dy"]), want_plain=True, want_tr=False)[0]
    hi, lo = U.split(o["dy"])
    assert_same(dyp.float(), torch.stack([hi, lo]).reshape(2, B, Cout, H * W), "pack_split plain [hi, lo]")
    xp, _ = _pack(K, o["x"], True)
    for mode in MODES:
        with _mode(gd, K, mode):
            dw = K.conv3x3_wgrad16(dyp.view(2, B, Cout, H * W), xp.view(B, H * W, 3 * Cin), H, W, 1, split=True)
            assert_same(dw, e.stored("dw"), f"split weight gradient, {mode}")


@pytest.mark.parametrize("prec", U.PRECS)
@pytest.mark.parametrize("name", sorted(U.WGRAD1))
def test_conv1x1_wgrad_gemm_nt(gd, name, prec):
    """the 1x1 weight gradient = gemm_nt_kernel<32|64|128, F32|BF16|X3, VEC?> with two k-splits (asserted from the plan), in
    the default slab mode and with atomics"""
    K, L = _KL()
    B, Cin, H, W, Cout, bm, vec = U.WGRAD1[name]
    assert U.generic_bm(Cout) == bm and ((H * W) % 32 == 0) == vec
    e = U.wgrad1_expect(name, prec)
    o = e.ops
    p = _prec(L, prec)
    dy, x = _d(o["dy"]), _d(o["x"])
    for mode in ("default", "atomic"):
        with _mode(gd, K, mode):
            assert K.gemm_nt_plan(B=1, M=Cout, N=Cin, kseg=B, klen=H * W, precision=p)[0] == 2
            assert_same(K.conv2d_wgrad(dy, x, 1, 1, 0, p), e.stored("dw"), f"{name} {prec} {mode}: 1x1 dw")


@pytest.mark.parametrize("prec", U.PRECS)
def test_conv4x4_stride2_wgrad_im2col(gd, prec):
    """the 4x4 / stride 2 / pad 1 weight gradient: gemm_nt with the im2col B operand and the fused prologue, two k-splits"""
    K, L = _KL()
    B, Cin, H, W, Cout, ks, stride, pad = U.WGRAD_IM2COL
    e = U.im2col_expect(prec)
    o = e.ops
    p = _prec(L, prec)
    for mode in ("default", "atomic"):
        with _mode(gd, K, mode):
            assert K.gemm_nt_plan(B=1, M=Cout, N=Cin * ks * ks, kseg=B, klen=o["Ho"] * o["Wo"], precision=p)[0] == 2
            dw = K.conv2d_wgrad(_d(o["dy"]), _d(o["x"]), ks, stride, pad, p, in_scale=_d(o["sc"]), in_shift=_d(o["sh"]), in_relu=True)
            assert_same(dw, e.stored("dw_prologue"), f"{prec} {mode}: 4x4 / stride 2 dw with prologue")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_linear_exact(gd, prec):
    """ops.linear at (5, 777, 130): the forward is a split-K gemm_nt (three k-splits), the backward two generic-kernel calls"""
    from gan_danet_amd import ops
    K, L = _KL()
    Bn, Kin, Nout = U.LINEAR
    e = U.linear_expect()
    o = e.ops
    xg, wg, bg = (_d(o[k]).requires_grad_(True) for k in ("x", "w", "bias"))
    with gd.precision(prec):
        assert K.gemm_nt_plan(B=1, M=Bn, N=Nout, kseg=1, klen=Kin, precision=ops._prec("disc"))[0] == 3
        y = ops.linear(xg, wg, bg)
        y.backward(_d(o["dy"]))
    for key, t in (("y", y), ("dx", xg.grad), ("dw", wg.grad), ("db", bg.grad)):
        assert_same(t, e.stored(key), f"linear {prec}: {key}")


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("ci", [1, 3])
def test_disc_stem_exact(gd, ci, split):
    """gd_disc_stem_fwd / _dgrad / _wgrad (fp32 FMAs from the fp32 image) at odd H and W: LeakyReLU(0.25) forward stored as
    bf16 or [hi | lo | hi], data gradient, weight and bias gradient in every reduce mode; split: the gradient is hi + lo"""
    K, L = _KL()
    B, H, W, Co = U.STEM
    e = U.stem_expect(ci, split)
    o = e.ops
    img, w = _d(o["x"]), _d(o["w"])
    a = K.disc_stem_fwd(img, w, _d(o["bias"]), U.SLOPE, split=split)
    _check_pm(a, e, "fwd", split, f"stem ci {ci}: forward")
    g = (_nhwc_split if split else _nhwc)(o["dy"])
    assert_same(K.disc_stem_dgrad(g, w, H, W, split=split), e.stored("dgrad"), f"stem ci {ci}: data gradient")
    for mode in MODES:
        with _mode(gd, K, mode):
            dw, db = K.disc_stem_wgrad(g, img, True, split=split)
            assert_same(dw, e.stored("dw"), f"stem ci {ci} {mode}: dw")
            assert_same(db, e.stored("db"), f"stem ci {ci} {mode}: db")
