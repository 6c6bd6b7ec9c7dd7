"""GPU: the channel attention (ops._cam_forward / ops._cam_backward), the PAM product chain (ops._pam_chain_fwd /
ops._pam_chain_bwd) and the batched, strided GEMM use of gd_conv2d (K.conv_nn with Hi = 1, one A matrix per image, read
row-major or transposed, alpha + residual + accumulate, operands and outputs as channel slices of wider slabs) -- called
directly, against the float64 closed forms of tests/cam_util.py, at shapes with ragged M, k and pixel tiles, on inputs
whose softmax is not saturated (tests/test_cam_reference.py asserts their conditioning and the fp32 margins on the CPU).

Bounds: FP32_TOL and BF16_TOL of tests/test_gpu_kernels.py, 1e-4 of test_conv2d_generic_split_bf16_vs_fp64."""
import functools

import pytest
import torch

import cam_util as CU
from gpu_util import DEV, bf16_round, relmax, seeded

pytestmark = pytest.mark.gpu

FP32_TOL = 2e-5
BF16_TOL = 2e-2
X3_TOL = 1e-4
GAMMA = 2.0
ALPHA = 0.37


@pytest.fixture(scope="module")
def gd():
    import gan_danet_amd as g
    from gan_danet_amd import _lib
    _lib.load()
    return g


def _mods():
    from gan_danet_amd import _lib, kern, ops
    return ops, kern, _lib


def _prec(name):
    _, _, L = _mods()
    return {"fp32": L.PREC_FP32, "x3": L.PREC_X3, "bf16": L.PREC_BF16}[name]


def _report(what, errs):
    """every figure, before anything is asserted"""
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))


def _rows_cols_rell2(got, ref):
    """the largest rel-L2 error over the (image, channel) rows and over the (image, pixel) columns of a (B, C, N) result:
    one wrong row of C, or one wrong pixel strip, cannot hide in a global norm"""
    d = got - ref
    rows = (d.norm(dim=2) / ref.norm(dim=2)).max().item()
    cols = (d.norm(dim=1) / ref.norm(dim=1)).max().item()
    return rows, cols


# ---- (a) CAM ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cam_problem(shape):
    """inputs and the float64 reference of one shape: computed once, shared by its six cases, never modified"""
    B, C, H, W = shape
    x, dout = CU.cam_inputs(B, C, H, W, CU.CAM_SEED), seeded((B, C, H * W), CU.CAM_DOUT_SEED)
    return x, dout, CU.cam_reference(x, GAMMA, dout)


_CAM_SPLIT = {(1, 200, 45, 22), (2, 136, 32, 32)}       # the Gram products long enough to be k-split


@pytest.mark.parametrize("slab", [False, True], ids=["dense", "slab"])
@pytest.mark.parametrize("prec", ["fp32", "x3", "bf16"])
@pytest.mark.parametrize("shape", CU.CAM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cam_kernels_vs_fp64(gd, shape, prec, slab):
    """ops._cam_forward and ops._cam_backward as CamFn / DualAttentionFn call them (dx prefilled with dOut; slab: out3 and
    d_cam are the upper channel halves of (B, 2C, H, W) buffers whose lower halves must come back bit-identical), gamma =
    2, the residual removed in fp64 on the host before anything is compared.  The shapes are cam_util.CAM_SHAPES (what
    each reaches is noted there); gd_gemm_nt_plan confirms which Gram products are k-split.
    att, dgamma: always fp32.  apply and dx: fp32 and x3 against fp64 on the unrounded operands; bf16 forward against
    fp64 on the operands as the kernel saw them (the returned att and x, rounded to bf16); bf16 backward against fp64 on
    the unrounded operands, rel-L2 per row and per column.
    measured (largest over shapes and slab / dense; margin to the bound):
      att 2.3e-6 (8.7x inside 2e-5), dgamma 1.8e-8 of the sum of |terms| (1100x);
      fp32: apply 2.2e-6 (9.1x), dx 1.6e-6 (12.8x); x3: apply 1.06e-5 (9.4x inside 1e-4), dx 1.01e-5 (9.9x);
      bf16: apply 3.0e-7 (330x inside 1e-4), dx rel-L2 rows 3.8e-3, columns 4.9e-3 (4.1x inside 2e-2)"""
    ops, K, L = _mods()
    B, C, H, W = shape
    N = H * W
    x, dout, ref = _cam_problem(shape)
    splits, _ = K.gemm_nt_plan(B=B, M=C, N=C, kseg=1, klen=N)
    assert (splits > 1) == (shape in _CAM_SPLIT), f"Gram k-splits {splits}"
    p = _prec(prec)
    gamma = torch.tensor([GAMMA], device=DEV)
    xd = x.to(DEV).view(B, C, H, W)
    if slab:
        feats, dfeat = seeded((B, 2 * C, H, W), 7).to(DEV), seeded((B, 2 * C, H, W), 8).to(DEV)
        dfeat[:, C:] = dout.view(B, C, H, W).to(DEV)
        feats0, dfeat0 = feats.clone(), dfeat.clone()
        out3, d_cam = ops._as3(feats[:, C:]), ops._as3(dfeat[:, C:])
    else:
        out3, d_cam = torch.full((B, C, N), float("nan"), device=DEV), dout.to(DEV)
    att = ops._cam_forward(xd, gamma, out3, p)
    dx = dout.to(DEV).clone()
    dgamma = ops._cam_backward(att, xd, gamma, d_cam, dx, p)
    torch.cuda.synchronize()
    if slab:
        assert torch.equal(feats[:, :C], feats0[:, :C]), "the forward wrote outside its half of the slab"
        assert torch.equal(dfeat, dfeat0), "the backward wrote into dOut's slab"
    att_c, y, dxc = att.double().cpu(), out3.double().cpu(), dx.double().cpu()
    assert torch.isfinite(y).all() and torch.isfinite(dxc).all() and torch.isfinite(att_c).all()
    apply_got = (y - x.double()) / GAMMA
    dx_got = (dxc - dout.double()) / GAMMA
    dx_ref = ref["dx_att"] + ref["dx_sym"]
    errs = {"att": relmax(att_c, ref["att"]),
            "dgamma": abs(dgamma.item() - ref["dgamma"].item()) / ref["dgamma_abs"].item()}
    if prec == "bf16":
        apply_ref = bf16_round(att.cpu()).double() @ bf16_round(x).double()
        errs["apply"] = relmax(apply_got, apply_ref)
        errs["dx_rows"], errs["dx_cols"] = _rows_cols_rell2(dx_got, dx_ref)
    else:
        errs["apply"] = relmax(apply_got, ref["apply"])
        errs["dx"] = relmax(dx_got, dx_ref)
    # which of the two backward products is off, should dx fail: got minus one reference term against the other term
    hint = {"dx-dx_sym vs dx_att": relmax(dx_got - ref["dx_sym"], ref["dx_att"]),
            "dx-dx_att vs dx_sym": relmax(dx_got - ref["dx_att"], ref["dx_sym"])}
    _report(f"cam_kernels {shape} {prec} {'slab' if slab else 'dense'}", errs)
    assert errs["att"] <= FP32_TOL, errs
    assert errs["dgamma"] <= FP32_TOL, errs
    assert errs["apply"] <= (FP32_TOL if prec == "fp32" else X3_TOL), errs
    if prec == "bf16":
        assert max(errs["dx_rows"], errs["dx_cols"]) <= BF16_TOL, (errs, hint)
    else:
        assert errs["dx"] <= (FP32_TOL if prec == "fp32" else X3_TOL), (errs, hint)


# ---- (b) K.conv_nn as a batched, strided GEMM ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemm_problem(shape):
    M, Ck, P = shape
    t = CU.gemm_inputs(M, Ck, P, 40 + M)
    prod = {"plain": CU.gemm_reference(t["a"], t["x"]), "bf16": CU.gemm_reference(bf16_round(t["a"]), bf16_round(t["x"]))}
    return t, prod


def _conv_nn(K, prec, a, a_t, x, y, B, M, Ck, P, fused, res=None, alpha=None):
    """y (B, M, P) (+)= [alpha] A X [+ res] with one A per image: a_t False = a is (B, M, Ck) row-major, True = a is
    (B, Ck, M), read transposed; x, y, res may be channel slices (their batch strides are taken from the views)"""
    a_sm, a_sc = (1, M) if a_t else (Ck, 1)
    K.conv_nn(B=B, M=M, Ck=Ck, ks=1, stride=1, pad=0, transposed=False, Hi=1, Wi=P, Ho=1, Wo=P, a=a, a_bs=M * Ck,
              a_sm=a_sm, a_sc=a_sc, a_st=0, x=x, x_bs=K._bview(x), y=y, y_bs=K._bview(y), precision=prec,
              alpha=alpha if fused else None, res=res if fused else None, res_bs=K._bview(res) if fused else 0,
              accumulate=fused)


@pytest.mark.parametrize("prec", ["fp32", "x3", "bf16"])
@pytest.mark.parametrize("shape", CU.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batched_strided_conv_nn_vs_fp64(gd, shape, prec):
    """K.conv_nn with ks = 1, Hi = Ho = 1, Wi = Wo = P, B = 3 and a different A per image, in the operand forms of
    ops._cam_forward / _cam_backward / _pam_chain_bwd / LinearFn.backward: A row-major or transposed, each plain and with
    alpha (a device scalar, 0.37) + res + accumulate into a prefilled y; the two fused forms once more with x, y and res
    as channel slices of wider slabs, everything outside the written slice bit-identical afterwards.  y0 and res have the
    product's own scale (Ck^-1/2), so the whole result is compared: none of the three terms hides another.
    (M, Ck, P): (35, 35, 4) the chain's dQt at N = 35, r = 4 -- one pixel quad, the smallest transpose-read launch;
    (990, 990, 23) gather kernel, 128-row tiles with the last at 94 rows, 31 k tiles with the last at 30; (40, 200, 480);
    (184, 184, 1024); (136, 35, 96).
    fp32: FP32_TOL relmax; x3: 1e-4 on the unrounded operands, and more than 10x closer than plain bf16 on the same
    operands when Ck >= 64 (the lo plane is live); bf16: 1e-4 on bf16-rounded operands (exact products: accumulation and
    addressing are what is left).
    measured (largest over shapes and forms; margin to the bound):
      fp32 1.15e-6 (17x inside 2e-5), x3 6.0e-6 (16.7x inside 1e-4), bf16 3.8e-7 (260x inside 1e-4);
      plain bf16 / x3 error ratio at Ck >= 64: 523 .. 576 (bound 10)"""
    _, K, L = _mods()
    M, Ck, P = shape
    B = CU.GEMM_B
    t, prod = _gemm_problem(shape)
    p = _prec(prec)
    rnd = bf16_round if prec == "bf16" else (lambda v: v)
    a, x = rnd(t["a"]), rnd(t["x"])
    product = prod["bf16" if prec == "bf16" else "plain"]
    fused_ref = t["y0"].double() + ALPHA * product + t["res"].double()
    tol = FP32_TOL if prec == "fp32" else X3_TOL
    a_rm, a_tr = a.to(DEV), a.transpose(1, 2).contiguous().to(DEV)
    xd, y0, res = x.to(DEV), t["y0"].to(DEV), t["res"].to(DEV)
    alpha = torch.tensor([ALPHA], device=DEV)
    errs, ratios = {}, {}
    for a_t in (False, True):
        for fused in (False, True):
            name = ("transposed" if a_t else "row-major") + (" fused" if fused else "")
            want = fused_ref if fused else product
            y = y0.clone() if fused else torch.full((B, M, P), float("nan"), device=DEV)
            _conv_nn(K, p, a_tr if a_t else a_rm, a_t, xd, y, B, M, Ck, P, fused, res, alpha)
            errs[name] = relmax(y, want)
            if prec == "x3" and Ck >= 64:
                yb = y0.clone() if fused else torch.full((B, M, P), float("nan"), device=DEV)
                _conv_nn(K, L.PREC_BF16, a_tr if a_t else a_rm, a_t, xd, yb, B, M, Ck, P, fused, res, alpha)
                ratios[name] = relmax(yb, want) / max(errs[name], 1e-30)
        # the fused form on slab slices: x = channels 2.. of (B, Ck + 3, P), y = the upper half of (B, 2M, P) as in
        # DualAttentionFn, res = channels 3.. of (B, M + 5, P)
        xs, ys, rs = seeded((B, Ck + 3, P), 61).to(DEV), seeded((B, 2 * M, P), 62).to(DEV), seeded((B, M + 5, P), 63).to(DEV)
        xs[:, 2:2 + Ck], ys[:, M:], rs[:, 3:3 + M] = xd, y0, res
        xs0, ys0, rs0 = xs.clone(), ys.clone(), rs.clone()
        _conv_nn(K, p, a_tr if a_t else a_rm, a_t, xs[:, 2:2 + Ck], ys[:, M:], B, M, Ck, P, True, rs[:, 3:3 + M], alpha)
        name = ("transposed" if a_t else "row-major") + " fused slab"
        errs[name] = relmax(ys[:, M:], fused_ref)
        assert torch.equal(ys[:, :M], ys0[:, :M]), f"{name}: wrote outside the output slice"
        assert torch.equal(xs, xs0) and torch.equal(rs, rs0), f"{name}: wrote into an operand slab"
    torch.cuda.synchronize()
    _report(f"batched_conv_nn {shape} {prec}", errs)
    if ratios:
        _report(f"batched_conv_nn {shape} bf16/x3 error ratio", ratios)
    for name, err in errs.items():
        assert err <= tol, f"{name}: rel err {err:.3e} > {tol:.0e}"
    for name, ratio in ratios.items():
        assert ratio > 10, f"{name}: plain bf16 is only {ratio:.1f}x further from fp64 than x3"


# ---- (c) the PAM product chain -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain_problem(shape):
    B, r, C, N = shape
    t = CU.chain_inputs(B, r, C, N, 300 + N)
    return t, CU.pam_chain_reference(*t[:4], GAMMA, t[4])


@pytest.mark.parametrize("slab", [False, True], ids=["dense", "slab"])
@pytest.mark.parametrize("shape", CU.CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pam_chain_vs_fp64(gd, shape, slab):
    """ops._pam_chain_fwd and ops._pam_chain_bwd in exact fp32 (the default PAM route of the fp32 mode): two gd_gemm_nt
    products, the row softmax and its backward, and four batched conv_nn products with ragged N (35, 480, 990) and r (4,
    23, 5).  slab: out3 is the lower channel half of a (B, 2C, N) buffer and dOut the lower half of another, as in
    DualAttentionFn; with B = 2 that takes the per-image loop of ops._axpy_dev3.  The residual is removed in fp64 before
    out is compared; dgamma is bounded against the sum of its |terms|.
    measured (largest over shapes and slab / dense; margin to the bound):
      p 1.7e-7, o_attn 1.06e-6, out 1.14e-6, dq 7.2e-7, dk 7.5e-7, dv 1.58e-6 (the largest: 12.7x inside 2e-5),
      dgamma 5.0e-9 of the sum of |terms|"""
    ops, K, L = _mods()
    B, r, C, N = shape
    (q, k, v, x, dout), ref = _chain_problem(shape)
    gamma = torch.tensor([GAMMA], device=DEV)
    qd, kd, vd, xd = (t.to(DEV) for t in (q, k, v, x))
    if slab:
        feats, dfeat = seeded((B, 2 * C, N), 7).to(DEV), seeded((B, 2 * C, N), 8).to(DEV)
        dfeat[:, :C] = dout.to(DEV)
        feats0, dfeat0 = feats.clone(), dfeat.clone()
        out3, d_pam = feats[:, :C], dfeat[:, :C]
    else:
        out3, d_pam = torch.full((B, C, N), float("nan"), device=DEV), dout.to(DEV)
    saved = ops._pam_chain_fwd(qd, kd, vd, xd, gamma, out3, L.PREC_FP32)
    dq, dk, dv, dgamma = ops._pam_chain_bwd(saved, gamma, d_pam, L.PREC_FP32)
    torch.cuda.synchronize()
    if slab:
        assert torch.equal(feats[:, C:], feats0[:, C:]), "the forward wrote outside its half of the slab"
        assert torch.equal(dfeat, dfeat0), "the backward wrote into dOut's slab"
    out = out3.double().cpu()
    assert torch.isfinite(out).all()
    got = {"p": saved[3], "o_attn": saved[4], "dq": dq, "dk": dk, "dv": dv}
    errs = {n: relmax(got[n], ref[n]) for n in got}
    errs["out"] = relmax((out - x.double()) / GAMMA, ref["o_attn"])
    errs["dgamma"] = abs(dgamma.item() - ref["dgamma"].item()) / ref["dgamma_abs"].item()
    _report(f"pam_chain {shape} {'slab' if slab else 'dense'}", errs)
    for n in got:
        assert got[n].shape == ref[n].shape, (n, got[n].shape)
    for name, err in errs.items():
        assert err <= FP32_TOL, f"{name}: rel err {err:.3e} > {FP32_TOL:.0e}"
