"""Tensor-level wrappers of the C ABI (no autograd here).

torch is used for device memory and streams only: every function takes CUDA
(ROCm) fp32 tensors, checks layout on the host, allocates outputs/workspaces
with ``torch.empty`` and enqueues the HIP kernels on torch's current stream.
CPU tensors are rejected -- there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L

Tensor = torch.Tensor


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: Tensor, name: str = "tensor", dtype=torch.float32) -> None:
    if not t.is_cuda:
        raise L.GandanetError(f"{name}: expected a GPU tensor (there is no CPU fallback in the product path)")
    if t.dtype != dtype:
        raise L.GandanetError(f"{name}: expected {dtype}, got {t.dtype}")


def _dense(t: Tensor, name: str = "tensor", dtype=torch.float32) -> Tensor:
    _chk(t, name, dtype)
    if not t.is_contiguous():
        raise L.GandanetError(f"{name}: expected a contiguous tensor, got strides {t.stride()}")
    return t


def _bview(t: Tensor, name: str = "tensor") -> int:
    """Validate a (B, C, H, W) or (B, C, N) tensor whose per-image block is dense (a channel slice of a
    wider slab is fine) and return its batch stride in elements."""
    _chk(t, name)
    if t.dim() == 4:
        b, c, h, w = t.shape
        ok = t.stride(3) == 1 and t.stride(2) == w and t.stride(1) == h * w
        inner = c * h * w
    elif t.dim() == 3:
        b, c, n = t.shape
        ok = t.stride(2) == 1 and t.stride(1) == n
        inner = c * n
    else:
        raise L.GandanetError(f"{name}: expected a 3-D or 4-D tensor")
    if not ok:
        raise L.GandanetError(f"{name}: per-image block must be dense, got strides {t.stride()}")
    bs = t.stride(0) if b > 1 else inner
    if b > 1 and bs < inner:
        raise L.GandanetError(f"{name}: overlapping batch stride")
    return bs


def lib():
    return L.load()


USE_CONV3X3_FAST = True   # route eligible 3x3/s1/p1 bf16 convs to the LDS-patch kernel (tests flip it to A/B)


# ---- optional HIP-event brackets around the hot kernels (bench.py's live roofline measurement) -------------
PROFILE_ON = False
PROFILE_CONV = os.environ.get("GD_PROFILE_CONV", "0") == "1"     # also bracket every conv call, keyed by its shape
PROFILE: list = []   # (name, start_event, end_event, algorithmic_flops, algorithmic_bytes)


class _Bracket:
    """records a start/end event pair on the stream the kernel is enqueued on (torch's current stream)"""

    def __init__(self, name: str, flops: float, nbytes: float = 0.0):
        self.name, self.flops, self.nbytes = name, flops, nbytes

    def __enter__(self):
        if PROFILE_ON:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if PROFILE_ON:
            self.e1.record()
            PROFILE.append((self.name, self.e0, self.e1, self.flops, self.nbytes))
        return False


class _ConvBracket(_Bracket):
    """opt-in (GD_PROFILE_CONV=1) per-shape bracket of a convolution call: name = kind k s Cin->Cout @HoxWo"""

    def __init__(self, kind, k, stride, cin, cout, ho, wo, b):
        super().__init__(f"conv_{kind}_k{k}s{stride}_{cin}->{cout}@{ho}x{wo}", 2.0 * k * k * cin * cout * ho * wo * b)

    def __enter__(self):
        return super().__enter__() if PROFILE_CONV else self

    def __exit__(self, *exc):
        return super().__exit__(*exc) if PROFILE_CONV else False


def profile_summary():
    """name -> (launches, avg ms, algorithmic flop per launch, algorithmic bytes per launch)"""
    torch.cuda.synchronize()
    agg = {}
    for name, e0, e1, fl, nb in PROFILE:
        a = agg.setdefault(name, [0, 0.0, 0.0, 0.0])
        a[0] += 1
        a[1] += e0.elapsed_time(e1)
        a[2] += fl
        a[3] += nb
    return {k: (v[0], v[1] / v[0], v[2] / v[0], v[3] / v[0]) for k, v in agg.items()}


# ------------------------------------------------------------------------------------------------
# implicit-GEMM "NN" kernel
# ------------------------------------------------------------------------------------------------
def conv_nn(*, B: int, M: int, Ck: int, ks: int, stride: int, pad: int, transposed: bool, Hi: int, Wi: int,
            Ho: int, Wo: int, a: Tensor, a_bs: int, a_sm: int, a_sc: int, a_st: int, x: Tensor, x_bs: int,
            y: Tensor, y_bs: int, precision: int, Mstore: int = 0, in_scale: Optional[Tensor] = None,
            in_shift: Optional[Tensor] = None, in_relu: bool = False, out_layout: int = 0, out_bf16: bool = False,
            ldo: int = 0, alpha: Optional[Tensor] = None, bias: Optional[Tensor] = None,
            res: Optional[Tensor] = None, res_bs: int = 0, act: int = 0, accumulate: bool = False) -> None:
    d = L.ConvDesc()
    d.B, d.M, d.Mstore, d.Ck, d.ks, d.stride, d.pad = B, M, max(M, Mstore), Ck, ks, stride, pad
    d.transposed = int(transposed)
    d.Hi, d.Wi, d.Ho, d.Wo = Hi, Wi, Ho, Wo
    d.a, d.a_bs, d.a_sm, d.a_sc, d.a_st = _ptr(a), a_bs, a_sm, a_sc, a_st
    d.x, d.x_bs = _ptr(x), x_bs
    d.in_scale, d.in_shift, d.in_relu = _ptr(in_scale), _ptr(in_shift), int(in_relu)
    d.y, d.y_bs = _ptr(y), y_bs
    d.out_layout, d.out_bf16, d.ldo = out_layout, int(out_bf16), ldo
    d.alpha, d.bias, d.res, d.res_bs = _ptr(alpha), _ptr(bias), _ptr(res), res_bs
    d.act, d.accumulate, d.precision = act, int(accumulate), precision
    if USE_CONV3X3_FAST and lib().gd_conv3x3_eligible(C.byref(d)):
        nbytes = int(lib().gd_conv3x3_ws_bytes(M, Ck))
        ws = torch.empty(nbytes // 2, device=x.device, dtype=torch.bfloat16)   # packed bf16 weights
        L.check(lib().gd_conv3x3(C.byref(d), _ptr(ws), nbytes, _stream()), "gd_conv3x3")
        return
    L.check(lib().gd_conv2d(C.byref(d), _stream()), "gd_conv2d")


def conv_out_size(h: int, k: int, stride: int, pad: int) -> int:
    return (h + 2 * pad - k) // stride + 1


def conv2d_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor], stride: int, pad: int, precision: int, *,
               act: int = 0, out: Optional[Tensor] = None, in_scale=None, in_shift=None, in_relu=False,
               accumulate: bool = False) -> Tensor:
    """nn.Conv2d forward, optional fused input affine+ReLU, bias, activation; ``out`` may be a channel slice."""
    xbs = _bview(x, "conv input")
    _dense(w, "conv weight")
    B, Cin, Hi, Wi = x.shape
    Cout, Cin_w, k, k2 = w.shape
    if Cin_w != Cin or k != k2:
        raise L.GandanetError(f"conv2d: weight {tuple(w.shape)} does not match input {tuple(x.shape)}")
    Ho, Wo = conv_out_size(Hi, k, stride, pad), conv_out_size(Wi, k, stride, pad)
    if out is None:
        out = torch.empty(B, Cout, Ho, Wo, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, Cout, Ho, Wo):
        raise L.GandanetError("conv2d: bad out shape")
    with _ConvBracket("fwd", k, stride, Cin, Cout, Ho, Wo, B):
        conv_nn(B=B, M=Cout, Ck=Cin, ks=k, stride=stride, pad=pad, transposed=False, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo,
                a=w, a_bs=0, a_sm=Cin * k * k, a_sc=k * k, a_st=1, x=x, x_bs=xbs, y=out, y_bs=_bview(out, "conv out"),
                precision=precision, in_scale=in_scale, in_shift=in_shift, in_relu=in_relu, bias=bias, act=act,
                accumulate=accumulate)
    return out


def conv2d_dgrad(dy: Tensor, w: Tensor, in_hw: Tuple[int, int], stride: int, pad: int, precision: int, *,
                 out: Optional[Tensor] = None, accumulate: bool = False, alpha: Optional[Tensor] = None) -> Tensor:
    """Gradient of nn.Conv2d w.r.t. its input: transposed gather of dy with the same OIHW weights."""
    dbs = _bview(dy, "conv dy")
    B, Cout, Ho, Wo = dy.shape
    Cout_w, Cin, k, _ = w.shape
    Hi, Wi = in_hw
    if Cout_w != Cout:
        raise L.GandanetError("conv2d_dgrad: weight/out-channel mismatch")
    if out is None:
        out = torch.empty(B, Cin, Hi, Wi, device=dy.device, dtype=torch.float32)
    with _ConvBracket("dgrad", k, stride, Cin, Cout, Ho, Wo, B):
        conv_nn(B=B, M=Cin, Ck=Cout, ks=k, stride=stride, pad=pad, transposed=True, Hi=Ho, Wi=Wo, Ho=Hi, Wo=Wi,
                a=w, a_bs=0, a_sm=k * k, a_sc=Cin * k * k, a_st=1, x=dy, x_bs=dbs, y=out, y_bs=_bview(out, "conv dx"),
                precision=precision, accumulate=accumulate, alpha=alpha)
    return out


def gemm_nt(*, B: int, M: int, N: int, kseg: int, klen: int, a: Tensor, a_bs: int, a_ss: int, lda: int,
            bm: Tensor, b_bs: int, b_ss: int, ldb: int, c: Tensor, c_bs: int, ldc: int, precision: int,
            im2col=None, in_scale=None, in_shift=None, in_relu=False, alpha=None, bias=None,
            accumulate: bool = False, splits: int = 0) -> None:
    d = L.GemmNTDesc()
    d.B, d.M, d.N, d.kseg, d.klen = B, M, N, kseg, klen
    d.a, d.a_bs, d.a_ss, d.lda = _ptr(a), a_bs, a_ss, lda
    d.bm, d.b_bs, d.b_ss, d.ldb = _ptr(bm), b_bs, b_ss, ldb
    if im2col is not None:
        d.im2col = 1
        d.ks, d.stride, d.pad, d.Hi, d.Wi, d.Ho, d.Wo = im2col
    d.in_scale, d.in_shift, d.in_relu = _ptr(in_scale), _ptr(in_shift), int(in_relu)
    d.c, d.c_bs, d.ldc = _ptr(c), c_bs, ldc
    d.alpha, d.bias = _ptr(alpha), _ptr(bias)
    d.accumulate, d.splits, d.precision = int(accumulate), splits, precision
    L.check(lib().gd_gemm_nt_ws(C.byref(d), _stream(), *det_ws()), "gd_gemm_nt")


def conv2d_wgrad(dy: Tensor, x: Tensor, k: int, stride: int, pad: int, precision: int, *, in_scale=None,
                 in_shift=None, in_relu=False, alpha: Optional[Tensor] = None, splits: int = 0) -> Tensor:
    """Gradient of nn.Conv2d w.r.t. its OIHW weight: dW[co][ci,kh,kw] = sum_{b,p} dy[b,co,p] x~[b,ci,p(+)tap].
    ``alpha`` (1x1 convs only): device scalar multiplying the result; ``splits`` (1x1 convs only): k-splits of the GEMM
    (0 = chosen by the kernel and combined as set_split_reduce says, 1 = unsplit)."""
    if alpha is not None and not (k == 1 and stride == 1 and pad == 0):
        raise L.GandanetError("conv2d_wgrad: alpha is supported for 1x1 convs only")
    dbs, xbs = _bview(dy, "wgrad dy"), _bview(x, "wgrad x")
    B, Cout, Ho, Wo = dy.shape
    _, Cin, Hi, Wi = x.shape
    dw = torch.empty(Cout, Cin, k, k, device=dy.device, dtype=torch.float32)
    with _ConvBracket("wgrad", k, stride, Cin, Cout, Ho, Wo, B):
        return _conv2d_wgrad(dy, x, k, stride, pad, precision, in_scale, in_shift, in_relu, dw, dbs, xbs, B, Cout, Cin, Hi,
                             Wi, Ho, Wo, alpha, splits)


def _conv2d_wgrad(dy, x, k, stride, pad, precision, in_scale, in_shift, in_relu, dw, dbs, xbs, B, Cout, Cin, Hi, Wi, Ho, Wo,
                  alpha=None, splits=0):
    if USE_CONV3X3_FAST and k == 3 and stride in (1, 2) and pad == 1 and precision == L.PREC_BF16:
        dy16 = x16 = None
        x_ld = 0
        if Cout > 32 and Cin >= 4 * 32:
            # every 32-channel chunk of ci re-reads each dY tile: hand the kernel a bf16 copy made once
            dy16, _ = pack_bf16(dy.view(B, Cout, Ho * Wo), Cout, Ho * Wo, plain_shape=(Cout, Ho * Wo))
            if in_scale is None and x.dim() == 4:
                # and a pixel-major bf16 copy of x: each of the Cout/BM m-blocks re-stages every patch, as 16-byte
                # copies instead of strided 4-byte gathers (the 2C -> C fuse convs: 12.4 -> 10.5 ms incl. the pack, bench shape)
                x_ld = (Cin + 7) // 8 * 8
                _, x16 = pack_bf16(x, Cin, Hi * Wi, t_shape=(Hi * Wi, x_ld))
        L.check(lib().gd_conv3x3_wgrad_ws(_ptr(dy), dbs, _ptr(dy16), _ptr(x), xbs, _ptr(x16), x_ld, _ptr(in_scale),
                                       _ptr(in_shift), int(in_relu), B, Cout, Cin, Hi, Wi, stride, 0, _ptr(dw), _stream(),
                                          *det_ws()), "gd_conv3x3_wgrad")
        return dw
    if k == 1 and stride == 1 and pad == 0:
        # 1x1: dW = dY X~^T with both operands pixel-contiguous -> plain NT GEMM (float4-staged when aligned); a fused
        # BN affine (+ReLU) of the input is a per-row transform of the B operand
        gemm_nt(B=1, M=Cout, N=Cin, kseg=B, klen=Ho * Wo, a=dy, a_bs=0, a_ss=dbs, lda=Ho * Wo, bm=x, b_bs=0, b_ss=xbs,
                ldb=Hi * Wi, c=dw, c_bs=0, ldc=Cin, precision=precision, in_scale=in_scale, in_shift=in_shift,
                in_relu=in_relu, alpha=alpha, splits=splits)
        return dw
    gemm_nt(B=1, M=Cout, N=Cin * k * k, kseg=B, klen=Ho * Wo, a=dy, a_bs=0, a_ss=dbs, lda=Ho * Wo, bm=x, b_bs=0,
            b_ss=xbs, ldb=0, c=dw, c_bs=0, ldc=Cin * k * k, precision=precision,
            im2col=(k, stride, pad, Hi, Wi, Ho, Wo), in_scale=in_scale, in_shift=in_shift, in_relu=in_relu)
    return dw


def bn_ws(B: int, Cn: int, HW: int, device) -> Tensor:
    n = lib().gd_bn_stats_ws_floats(B, Cn, HW)
    return torch.empty(max(int(n), 1), device=device, dtype=torch.float32)


def channel_sum(x: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    bs = _bview(x, "channel_sum input")
    B, Cn = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    if out is None:
        out = torch.empty(Cn, device=x.device, dtype=torch.float32)
    L.check(lib().gd_channel_sum(_ptr(x), bs, B, Cn, HW, _ptr(out), int(accumulate), _ptr(bn_ws(B, Cn, HW, x.device)),
                                 _stream()), "gd_channel_sum")
    return out


# ------------------------------------------------------------------------------------------------
# batch norm
# ------------------------------------------------------------------------------------------------
def bn_stats(x: Tensor, eps: float, momentum: float, running_mean: Optional[Tensor],
             running_var: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    bs = _bview(x, "bn input")
    B, Cn = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    mean = torch.empty(Cn, device=x.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    L.check(lib().gd_bn_stats(_ptr(x), bs, B, Cn, HW, eps, momentum, _ptr(mean), _ptr(invstd), _ptr(running_mean),
                              _ptr(running_var), _ptr(bn_ws(B, Cn, HW, x.device)), _stream()), "gd_bn_stats")
    return mean, invstd


def bn_stats_local(x: Tensor) -> Tensor:
    """SyncBN, local half: (C, 3) = (count, mean, M2) of this rank's shard per channel (gd_bn_stats_local)"""
    bs = _bview(x, "bn input")
    B, Cn = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    stats = torch.empty(Cn, 3, device=x.device, dtype=torch.float32)
    L.check(lib().gd_bn_stats_local(_ptr(x), bs, B, Cn, HW, _ptr(stats), _ptr(bn_ws(B, Cn, HW, x.device)), _stream()),
            "gd_bn_stats_local")
    return stats


def bn_stats_merge(stats_all: Tensor, eps: float, momentum: float, running_mean: Optional[Tensor],
                   running_var: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """SyncBN: (world, C, 3) all-gathered records -> mean, invstd of the global batch (+ running statistics)"""
    _dense(stats_all, "gathered BN records")
    world, Cn, _ = stats_all.shape
    mean = torch.empty(Cn, device=stats_all.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    L.check(lib().gd_bn_stats_merge(_ptr(stats_all), world, Cn, eps, momentum, _ptr(mean), _ptr(invstd), _ptr(running_mean),
                                    _ptr(running_var), _stream()), "gd_bn_stats_merge")
    return mean, invstd


def bn_act_bwd_dx(dy: Tensor, x: Tensor, scale: Tensor, shift: Tensor, mean: Tensor, invstd: Tensor, dgamma_sum: Tensor,
                  dbeta_sum: Tensor, inv_n: float, act: int, dx: Optional[Tensor] = None, accumulate_dx: bool = False) -> Tensor:
    """SyncBN: dx from the all-reduced per-channel sums (gd_bn_act_bwd_dx)"""
    dbs, xbs = _bview(dy, "bn dy"), _bview(x, "bn x")
    B, Cn = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    if dx is None:
        dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        accumulate_dx = False
    L.check(lib().gd_bn_act_bwd_dx(_ptr(dy), dbs, _ptr(x), xbs, _ptr(scale), _ptr(shift), _ptr(mean), _ptr(invstd),
                                   _ptr(dgamma_sum), _ptr(dbeta_sum), float(inv_n), B, Cn, HW, act, _ptr(dx), _bview(dx),
                                   int(accumulate_dx), _stream()), "gd_bn_act_bwd_dx")
    return dx


def bn_fold(gamma: Tensor, beta: Tensor, mean: Tensor, invstd: Tensor) -> Tuple[Tensor, Tensor]:
    scale, shift = torch.empty_like(gamma), torch.empty_like(gamma)
    L.check(lib().gd_bn_fold(_ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), gamma.numel(), _ptr(scale),
                             _ptr(shift), _stream()), "gd_bn_fold")
    return scale, shift


def bn_fold_eval(gamma: Tensor, beta: Tensor, running_mean: Tensor, running_var: Tensor, eps: float):
    scale, shift, invstd = torch.empty_like(gamma), torch.empty_like(gamma), torch.empty_like(gamma)
    L.check(lib().gd_bn_fold_eval(_ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), eps,
                                  gamma.numel(), _ptr(scale), _ptr(shift), _ptr(invstd), _stream()), "gd_bn_fold_eval")
    return scale, shift, invstd


def affine_act(x: Tensor, scale: Optional[Tensor], shift: Optional[Tensor], act: int,
               out: Optional[Tensor] = None) -> Tensor:
    bs = _bview(x, "affine input")
    B, Cn = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    L.check(lib().gd_affine_act(_ptr(x), bs, _ptr(scale), _ptr(shift), B, Cn, HW, act, _ptr(out), _bview(out),
                                _stream()), "gd_affine_act")
    return out


def bn_act_bwd(dy: Tensor, x: Tensor, scale: Tensor, shift: Tensor, mean: Tensor, invstd: Tensor, act: int,
               train: bool, dx: Optional[Tensor] = None, accumulate_dx: bool = False, want_dx: bool = True,
               sums_out: Optional[Tensor] = None):
    """``sums_out`` (2, C): dgamma / dbeta are written into its rows (SyncBN all-reduces that one buffer)"""
    dbs, xbs = _bview(dy, "bn dy"), _bview(x, "bn x")
    B, Cn = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    if sums_out is not None:
        dgamma, dbeta = _dense(sums_out)[0], sums_out[1]
    else:
        dgamma = torch.empty(Cn, device=x.device, dtype=torch.float32)
        dbeta = torch.empty_like(dgamma)
    if want_dx and dx is None:
        dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    L.check(lib().gd_bn_act_bwd(_ptr(dy), dbs, _ptr(x), xbs, _ptr(scale), _ptr(shift), _ptr(mean), _ptr(invstd), None,
                                B, Cn, HW, act, int(train), _ptr(dgamma), _ptr(dbeta), _ptr(dx) if want_dx else None,
                                _bview(dx) if want_dx else 0, int(accumulate_dx), _ptr(bn_ws(B, Cn, HW, x.device)),
                                _stream()), "gd_bn_act_bwd")
    return dgamma, dbeta, dx


# ------------------------------------------------------------------------------------------------
# resampling
# ------------------------------------------------------------------------------------------------
def bicubic_fwd(x: Tensor, Ho: int, Wo: int, rsh: float, rsw: float) -> Tensor:
    _dense(x, "bicubic input")
    B, Cn, Hi, Wi = x.shape
    y = torch.empty(B, Cn, Ho, Wo, device=x.device, dtype=torch.float32)
    L.check(lib().gd_bicubic_fwd(_ptr(x), B * Cn, Hi, Wi, _ptr(y), Ho, Wo, rsh, rsw, _stream()), "gd_bicubic_fwd")
    return y


def shift_sum9_fwd(u: Tensor, bias: Optional[Tensor]) -> Tensor:
    _dense(u, "tap planes")
    B, nine, H, W = u.shape
    if nine != 9:
        raise L.GandanetError(f"shift_sum9: expected (B, 9, H, W) tap planes, got {tuple(u.shape)}")
    y = torch.empty(B, 1, H, W, device=u.device, dtype=torch.float32)
    L.check(lib().gd_shift_sum9_fwd(_ptr(u), _ptr(bias), _ptr(y), B, H, W, _stream()), "gd_shift_sum9_fwd")
    return y


def shift_sum9_bwd(dy: Tensor) -> Tensor:
    _dense(dy, "dy")
    B, _, H, W = dy.shape
    du = torch.empty(B, 9, H, W, device=dy.device, dtype=torch.float32)
    L.check(lib().gd_shift_sum9_bwd(_ptr(dy), _ptr(du), B, H, W, _stream()), "gd_shift_sum9_bwd")
    return du


def combine_inputs(lr: Tensor, aux: Tensor, s1: float = 0.5, s2: float = 0.25) -> Tensor:
    """cat([bicubic(lr, scale_factor=s1), bicubic(aux, scale_factor=s2)], 1) in one launch
    (GAN_DANet_train.ipynb:L218-224; output size floor(in * scale) like F.interpolate)"""
    _dense(lr, "lr_grace_05"), _dense(aux, "hr_aux")
    B, C1, H1, W1 = lr.shape
    B2, C2, H2, W2 = aux.shape
    Ho, Wo = int(math.floor(H1 * s1)), int(math.floor(W1 * s1))
    if B2 != B or (int(math.floor(H2 * s2)), int(math.floor(W2 * s2))) != (Ho, Wo):
        raise L.GandanetError(f"combine_inputs: {tuple(lr.shape)} x{s1} and {tuple(aux.shape)} x{s2} do not meet")
    out = torch.empty(B, C1 + C2, Ho, Wo, device=lr.device, dtype=torch.float32)
    L.check(lib().gd_combine_inputs(_ptr(lr), C1, H1, W1, 1.0 / s1, _ptr(aux), C2, H2, W2, 1.0 / s2, _ptr(out), B, Ho,
                                    Wo, _stream()), "gd_combine_inputs")
    return out


def _hist_match(be, src, ref, weight: float):
    """one body for the device / host twins of gd_hist_match (``be``: _DEV or _HOST, below)"""
    if be.host:                                           # _Host.dense converts; the device refuses anything but float32
        src, ref = np.asarray(src), np.asarray(ref)
        if src.dtype != np.float32 or ref.dtype != np.float32:
            raise L.GandanetError(f"hist_match: expected float32 arrays, got {src.dtype} / {ref.dtype}")
    src, ref = be.dense(src, "histogram source", be.f32), be.dense(ref, "histogram reference", be.f32)
    if src.ndim < 1 or ref.ndim < 1 or ref.shape[0] != src.shape[0]:
        raise L.GandanetError("hist_match: batch sizes differ")
    B = src.shape[0]
    ns, nt = math.prod(src.shape[1:]), math.prod(ref.shape[1:])
    out = be.empty(src.shape, be.f64, src)
    ws = () if be.host else be.ws(None, lib().gd_hist_match_ws_bytes(ns, nt), src, "hist_match")
    be.call("gd_hist_match", be.ptr(src), be.ptr(ref), B, ns, nt, float(weight), be.ptr(out), *ws)
    return out


def hist_match(src: Tensor, ref: Tensor, weight: float) -> Tensor:
    """per-sample mild histogram matching (test.ipynb c1:69-85); src (B, ...), ref (B, ...) fp32 -> fp64 like src.
    GPU tensors run gd_hist_match on the current stream; CPU tensors go to its host twin gd_hist_match_host (plain C++ over
    the same per-element code, csrc/histmatch_core.h), and both give the same bits.

    A NaN in ``src`` propagates to its own position only: it gives NaN there and, sorted last whatever its sign bit (as
    numpy sorts), ranks above every number for the other elements.  Non-finite values in ``ref`` are outside the contract
    (np.interp's own rules for them differ between numpy versions) and are not tested."""
    if isinstance(src, Tensor) and isinstance(ref, Tensor) and not src.is_cuda and not ref.is_cuda:
        return torch.from_numpy(_hist_match(_HOST, src.numpy(), ref.numpy(), weight))
    return _hist_match(_DEV, src, ref, weight)


def hist_match_host(src, ref, weight: float):
    """``hist_match`` on HOST numpy float32 arrays (gd_hist_match_host); a new float64 array shaped like ``src``"""
    return _hist_match(_HOST, src, ref, weight)


def blend_region(gen: Tensor, grace: Tensor, mask: Tensor, region) -> Tensor:
    """in place on ``gen``: gen[.., sr:er, sc:ec] = gen * (1 - mask) + grace * mask"""
    _dense(gen, "blend target"), _dense(grace, "blend source"), _dense(mask, "blend mask")
    sr, er, sc, ec = (int(v) for v in region)
    if gen.shape != grace.shape or tuple(mask.shape) != (er - sr, ec - sc):
        raise L.GandanetError(f"blend_region: shapes {tuple(gen.shape)} / {tuple(grace.shape)} / mask {tuple(mask.shape)}")
    B, Cn, H, W = gen.shape
    L.check(lib().gd_blend_region(_ptr(gen), _ptr(grace), _ptr(mask), B * Cn, H, W, sr, er, sc, ec, _stream()),
            "gd_blend_region")
    return gen


def bicubic_bwd(dy: Tensor, Hi: int, Wi: int, rsh: float, rsw: float) -> Tensor:
    _dense(dy, "bicubic dy")
    B, Cn, Ho, Wo = dy.shape
    dx = torch.empty(B, Cn, Hi, Wi, device=dy.device, dtype=torch.float32)
    L.check(lib().gd_bicubic_bwd(_ptr(dy), B * Cn, Hi, Wi, _ptr(dx), Ho, Wo, rsh, rsw, _stream()), "gd_bicubic_bwd")
    return dx


def bilinear_fwd(x: Tensor, Ho: int, Wo: int, out: Optional[Tensor] = None, accumulate: bool = False,
                 res: Optional[Tensor] = None) -> Tensor:
    """out = bilinear(x) [+ out if accumulate] [or res + bilinear(x) when ``res`` is given]"""
    _dense(x, "bilinear input")
    B, Cn, Hi, Wi = x.shape
    if out is None:
        out = torch.empty(B, Cn, Ho, Wo, device=x.device, dtype=torch.float32)
        accumulate = False
    _dense(out, "bilinear out")
    if res is not None:
        _dense(res, "bilinear residual")
        if res.shape != out.shape:
            raise L.GandanetError("bilinear_fwd: residual shape mismatch")
    L.check(lib().gd_bilinear_fwd(_ptr(x), B * Cn, Hi, Wi, _ptr(out), Ho, Wo, int(accumulate), _ptr(res), _stream()),
            "gd_bilinear_fwd")
    return out


def bilinear_bwd(dy: Tensor, Hi: int, Wi: int) -> Tensor:
    _dense(dy, "bilinear dy")
    B, Cn, Ho, Wo = dy.shape
    dx = torch.empty(B, Cn, Hi, Wi, device=dy.device, dtype=torch.float32)
    L.check(lib().gd_bilinear_bwd(_ptr(dy), B * Cn, Hi, Wi, _ptr(dx), Ho, Wo, _stream()), "gd_bilinear_bwd")
    return dx


def maxpool2_fwd(x: Tensor) -> Tensor:
    _dense(x, "maxpool input")
    B, Cn, Hi, Wi = x.shape
    y = torch.empty(B, Cn, Hi // 2, Wi // 2, device=x.device, dtype=torch.float32)
    L.check(lib().gd_maxpool2_fwd(_ptr(x), B * Cn, Hi, Wi, _ptr(y), _stream()), "gd_maxpool2_fwd")
    return y


def maxpool2_bwd(x: Tensor, dy: Tensor) -> Tensor:
    _dense(x), _dense(dy)
    B, Cn, Hi, Wi = x.shape
    dx = torch.empty_like(x)
    L.check(lib().gd_maxpool2_bwd(_ptr(x), _ptr(dy), B * Cn, Hi, Wi, _ptr(dx), _stream()), "gd_maxpool2_bwd")
    return dx


# ------------------------------------------------------------------------------------------------
# pointwise / reductions
# ------------------------------------------------------------------------------------------------
def act_fwd(x: Tensor, act: int, out: Optional[Tensor] = None) -> Tensor:
    _dense(x)
    out = torch.empty_like(x) if out is None else out
    L.check(lib().gd_act_fwd(_ptr(x), _ptr(out), x.numel(), act, _stream()), "gd_act_fwd")
    return out


def act_bwd(y: Tensor, dy: Tensor, act: int) -> Tensor:
    _dense(y), _dense(dy)
    dx = torch.empty_like(dy)
    L.check(lib().gd_act_bwd(_ptr(y), _ptr(dy), _ptr(dx), y.numel(), act, _stream()), "gd_act_bwd")
    return dx


def axpby(x: Tensor, a: float, y: Tensor, b: float) -> Tensor:
    """y = a*x + b*y (in place on y)"""
    _dense(x), _dense(y)
    L.check(lib().gd_axpby(_ptr(x), a, _ptr(y), b, x.numel(), _stream()), "gd_axpby")
    return y


def scale_dev(x: Tensor, s: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out (+)= s * x with s a 1-element device tensor"""
    _dense(x)
    if out is None:
        out = torch.empty_like(x)
        accumulate = False
    L.check(lib().gd_scale_dev(_ptr(x), _ptr(s), _ptr(out), x.numel(), int(accumulate), _stream()), "gd_scale_dev")
    return out


def copy_slab(src: Tensor, dst: Tensor, accumulate: bool = False) -> Tensor:
    sbs, dbs = _bview(src, "copy src"), _bview(dst, "copy dst")
    if src.shape != dst.shape:
        raise L.GandanetError("copy_slab: shape mismatch")
    L.check(lib().gd_copy_slab(_ptr(src), sbs, _ptr(dst), dbs, src.shape[0], src[0].numel(), int(accumulate),
                               _stream()), "gd_copy_slab")
    return dst


def softmax_rows(x: Tensor, sign: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    _dense(x)
    out = torch.empty_like(x) if out is None else out
    cols = x.shape[-1]
    L.check(lib().gd_softmax_rows(_ptr(x), _ptr(out), x.numel() // cols, cols, sign, _stream()), "gd_softmax_rows")
    return out


def softmax_rows_bwd(p: Tensor, dp: Tensor, sign: float = 1.0) -> Tensor:
    _dense(p), _dense(dp)
    dx = torch.empty_like(p)
    cols = p.shape[-1]
    L.check(lib().gd_softmax_rows_bwd(_ptr(p), _ptr(dp), _ptr(dx), p.numel() // cols, cols, sign, _stream()),
            "gd_softmax_rows_bwd")
    return dx


def _red_ws(device) -> Tensor:
    return torch.empty(2048, device=device, dtype=torch.float32)


def dot(a: Tensor, b: Optional[Tensor], out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    _dense(a)
    if b is not None:
        _dense(b)
    if out is None:
        out = torch.empty(1, device=a.device, dtype=torch.float32)
        accumulate = False
    L.check(lib().gd_dot(_ptr(a), _ptr(b), a.numel(), _ptr(out), int(accumulate), _ptr(_red_ws(a.device)), _stream()),
            "gd_dot")
    return out


def transpose(s: Tensor) -> Tensor:
    """(B, R, C) -> (B, C, R)"""
    _dense(s)
    B, R, Cc = s.shape
    t = torch.empty(B, Cc, R, device=s.device, dtype=torch.float32)
    L.check(lib().gd_transpose(_ptr(s), _ptr(t), B, R, Cc, _stream()), "gd_transpose")
    return t


def add_transpose(a: Tensor) -> Tensor:
    _dense(a)
    B, n, _ = a.shape
    out = torch.empty_like(a)
    L.check(lib().gd_add_transpose(_ptr(a), _ptr(out), B, n, _stream()), "gd_add_transpose")
    return out


def copy_rows(src: Tensor, s_bs: int, s_ld: int, dst: Tensor, d_bs: int, d_ld: int, B: int, R: int, Cc: int):
    L.check(lib().gd_copy_rows(_ptr(src), s_bs, s_ld, _ptr(dst), d_bs, d_ld, B, R, Cc, _stream()), "gd_copy_rows")
    return dst


# ---- losses ---------------------------------------------------------------------------------------
def bce_logits(z: Tensor, label: float, want_grad: bool):
    _dense(z)
    out = torch.empty(1, device=z.device, dtype=torch.float32)
    dz = torch.empty_like(z) if want_grad else None
    L.check(lib().gd_bce_logits(_ptr(z), z.numel(), label, _ptr(out), _ptr(dz), _ptr(_red_ws(z.device)), _stream()),
            "gd_bce_logits")
    return out, dz


def bce_logits_target(z: Tensor, t: Tensor, want_dz: bool, want_dt: bool):
    _dense(z), _dense(t)
    out = torch.empty(1, device=z.device, dtype=torch.float32)
    dz = torch.empty_like(z) if want_dz else None
    dt = torch.empty_like(t) if want_dt else None
    L.check(lib().gd_bce_logits_target(_ptr(z), _ptr(t), z.numel(), _ptr(out), _ptr(dz), _ptr(dt),
                                       _ptr(_red_ws(z.device)), _stream()), "gd_bce_logits_target")
    return out, dz, dt


def leaky_fwd(x: Tensor, slope: float) -> Tensor:
    _dense(x)
    y = torch.empty_like(x)
    L.check(lib().gd_leaky_fwd(_ptr(x), _ptr(y), x.numel(), float(slope), _stream()), "gd_leaky_fwd")
    return y


def leaky_bwd(x: Tensor, dy: Tensor, slope: float) -> Tensor:
    _dense(x), _dense(dy)
    dx = torch.empty_like(x)
    L.check(lib().gd_leaky_bwd(_ptr(x), _ptr(dy), _ptr(dx), x.numel(), float(slope), _stream()), "gd_leaky_bwd")
    return dx


def diff_loss(kind: str, a: Tensor, b: Tensor, want_grad: bool):
    _dense(a), _dense(b)
    if a.shape != b.shape:
        raise L.GandanetError(f"{kind}: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    out = torch.empty(1, device=a.device, dtype=torch.float32)
    da = torch.empty_like(a) if want_grad else None
    fn = lib().gd_mse if kind == "mse" else lib().gd_l1
    L.check(fn(_ptr(a), _ptr(b), a.numel(), _ptr(out), _ptr(da), _ptr(_red_ws(a.device)), _stream()), f"gd_{kind}")
    return out, da


def tv(x: Tensor, weight: float, want_grad: bool):
    _dense(x)
    B, Cn, H, W = x.shape
    out = torch.empty(1, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x) if want_grad else None
    L.check(lib().gd_tv(_ptr(x), B, Cn, H, W, weight, _ptr(out), _ptr(dx), _ptr(_red_ws(x.device)), _stream()), "gd_tv")
    return out, dx


def ssim(a: Tensor, b: Tensor, window: int) -> Tensor:
    _dense(a), _dense(b)
    B, Cn, H, W = a.shape
    out = torch.empty(1, device=a.device, dtype=torch.float32)
    L.check(lib().gd_ssim(_ptr(a), _ptr(b), B * Cn, H, W, window, _ptr(out), _ptr(_red_ws(a.device)), _stream()),
            "gd_ssim")
    return out


def ssim_samples(a: Tensor, b: Tensor, window: int) -> Tensor:
    """per-sample SSIM means (B,)"""
    _dense(a), _dense(b)
    B, Cn, H, W = a.shape
    out = torch.empty(B, device=a.device, dtype=torch.float32)
    L.check(lib().gd_ssim_samples(_ptr(a), _ptr(b), B, Cn, H, W, window, _ptr(out), _ptr(_red_ws(a.device)), _stream()),
            "gd_ssim_samples")
    return out


def ssim_bwd(a: Tensor, b: Tensor, gscale: Tensor, window: int, need_a: bool = True, need_b: bool = True):
    """gradients of sum_s gscale[s] * sum_pixels ssim_map[s] w.r.t. a and b"""
    _dense(a), _dense(b), _dense(gscale)
    B, Cn, H, W = a.shape
    coef = torch.empty(4 * a.numel(), device=a.device, dtype=torch.float32)
    da = torch.empty_like(a) if need_a else None
    db = torch.empty_like(b) if need_b else None
    L.check(lib().gd_ssim_bwd(_ptr(a), _ptr(b), _ptr(gscale), B, Cn, H, W, window, _ptr(coef), _ptr(da), _ptr(db),
                              _stream()), "gd_ssim_bwd")
    return da, db


def adamw(p: Tensor, g: Tensor, m: Tensor, v: Tensor, step: int, lr: float, beta1: float, beta2: float, eps: float,
          weight_decay: float, grad_scale: float = 1.0) -> None:
    for t in (p, g, m, v):
        _dense(t, "adamw tensor")
    L.check(lib().gd_adamw(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), step, lr, beta1, beta2, eps, weight_decay,
                           grad_scale, _stream()), "gd_adamw")


# ---- PAM helpers ------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634    # gd_pam_flash_* take q pre-scaled by log2(e) (include/gandanet.h)


def pack_bf16(s: Tensor, R: int, Cc: int, *, scale: Optional[Tensor] = None, scale_imm: float = 1.0, plain_shape=None,
              t_shape=None, perm16: bool = False, ones_row: int = -1, f16: bool = False):
    """s: (B, R, Cc)-like fp32 block (per-image dense).  Returns (plain, transposed) 16-bit tensors (or None):
    bf16, or IEEE fp16 with ``f16`` (the fused PAM kernels' fp16 operand mode)."""
    sbs = _bview(s, "pack input")
    B = s.shape[0]
    plain = tr = None
    rp = ldp = ccp = ldt = 0
    dt = torch.float16 if f16 else torch.bfloat16
    if plain_shape is not None:
        rp, ldp = plain_shape
        plain = torch.empty(B, rp, ldp, device=s.device, dtype=dt)
    if t_shape is not None:
        ccp, ldt = t_shape
        tr = torch.empty(B, ccp, ldt, device=s.device, dtype=dt)
    L.check(lib().gd_pack_16(_ptr(s), sbs, B, R, Cc, _ptr(scale), float(scale_imm), _ptr(plain), rp, ldp, _ptr(tr),
                             ccp, ldt, int(perm16), int(ones_row), int(f16), _stream()), "gd_pack_16")
    return plain, tr


def pack_nhwc16_affine(x: Tensor, scale: Optional[Tensor], shift: Optional[Tensor], relu: bool) -> Tensor:
    """(B, C, H, W) fp32 (per-image dense, possibly a channel slice of a slab) -> (B, H*W, C) bf16 pixel-major copy of
    max(0, scale[c] x + shift[c]) (the BatchNorm + ReLU prologue of a dense layer); C % 8 == 0, H*W % 4 == 0"""
    sbs = _bview(x, "pack input")
    B, Cn, H, W = x.shape
    out = torch.empty(B, H * W, Cn, device=x.device, dtype=torch.bfloat16)
    L.check(lib().gd_pack_16_affine(_ptr(x), sbs, B, Cn, H * W, _ptr(scale), _ptr(shift), int(relu), None, 0, 0, _ptr(out),
                                    H * W, Cn, 0, _stream()), "gd_pack_16_affine")
    return out


def augment_d4(x: Tensor, ops: Tensor, noise: Optional[Tensor] = None, noise_scale: float = 0.05) -> Tensor:
    """per-sample flip / flip / rot90 (+ noise) of a (B, C, H, W) batch; ``ops`` int32 (B,) op words (gandanet.h)"""
    _dense(x, "augment input")
    _chk(ops, "augment ops", torch.int32)
    B, Cn, H, W = x.shape
    if ops.numel() != B or (noise is not None and _dense(noise, "noise").shape != x.shape):
        raise L.GandanetError("augment_d4: ops must hold one word per sample and noise must match the batch")
    y = torch.empty_like(x)
    L.check(lib().gd_augment_d4(_ptr(x), _ptr(y), B, Cn, H, W, _ptr(ops), _ptr(noise), float(noise_scale), _stream()),
            "gd_augment_d4")
    return y


def bcast_mul(x: Tensor, att: Tensor, mode: int) -> Tensor:
    """x (B, C, H, W) dense times a channel gate att (B, C) [mode 0] or a spatial gate att (B, H*W) [mode 1]"""
    _dense(x), _dense(att)
    B, Cn = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    if att.numel() != (B * Cn if mode == 0 else B * HW):
        raise L.GandanetError(f"bcast_mul: gate of {att.numel()} elements does not match x {tuple(x.shape)} (mode {mode})")
    y = torch.empty_like(x)
    L.check(lib().gd_bcast_mul(_ptr(x), _ptr(att), _ptr(y), B, Cn, HW, mode, _stream()), "gd_bcast_mul")
    return y


def row_dot(a: Tensor, b: Tensor, rows: int) -> Tensor:
    _dense(a), _dense(b)
    n = a.numel() // rows
    out = torch.empty(rows, device=a.device, dtype=torch.float32)
    L.check(lib().gd_row_dot(_ptr(a), _ptr(b), _ptr(out), rows, n, _stream()), "gd_row_dot")
    return out


def chan_maxmean_fwd(x: Tensor):
    _dense(x)
    B, Cn, H, W = x.shape
    y = torch.empty(B, 2, H, W, device=x.device, dtype=torch.float32)
    idx = torch.empty(B, H * W, device=x.device, dtype=torch.int32)
    L.check(lib().gd_chan_maxmean_fwd(_ptr(x), _ptr(y), _ptr(idx), B, Cn, H * W, _stream()), "gd_chan_maxmean_fwd")
    return y, idx


def chan_maxmean_bwd(dy: Tensor, idx: Tensor, Cn: int) -> Tensor:
    _dense(dy)
    B, _, H, W = dy.shape
    dx = torch.empty(B, Cn, H, W, device=dy.device, dtype=torch.float32)
    L.check(lib().gd_chan_maxmean_bwd(_ptr(dy), _ptr(idx), _ptr(dx), B, Cn, H * W, _stream()), "gd_chan_maxmean_bwd")
    return dx


def chan_dot(a: Tensor, o: Tensor, gamma: Tensor):
    abs_, obs = _bview(a), _bview(o)
    B, Cn = a.shape[0], a.shape[1]
    N = a[0, 0].numel()
    d_raw = torch.empty(B, N, device=a.device, dtype=torch.float32)
    delta = torch.empty_like(d_raw)
    L.check(lib().gd_chan_dot(_ptr(a), abs_, _ptr(o), obs, B, Cn, N, _ptr(gamma), _ptr(d_raw), _ptr(delta), _stream()),
            "gd_chan_dot")
    return d_raw, delta


def pam_f16_scale(dout: Tensor, gamma: Tensor, delta: Tensor) -> Tensor:
    """power-of-two scale of the fp16 PAM backward (gd_pam_f16_scale): returns scales = [gamma * 2^k, 2^-k]; ``delta`` is
    multiplied by 2^k in place"""
    bs = _bview(dout, "dOut")
    B, Cn = dout.shape[0], dout.shape[1]
    N = dout[0, 0].numel()
    scales = torch.empty(2, device=dout.device, dtype=torch.float32)
    L.check(lib().gd_pam_f16_scale(_ptr(dout), bs, B, Cn, N, _ptr(gamma), _ptr(_dense(delta)), _ptr(scales),
                                   _ptr(_red_ws(dout.device)), _stream()), "gd_pam_f16_scale")
    return scales


def pam_key_sqnorm_max(kt: Tensor, N: int, f16: bool = False) -> Tensor:
    """max_j |k_j|^2 per image of the packed keys kt (B, Npad, 32) (gd_pam_key_sqnorm_max)"""
    B, Npad = kt.shape[0], kt.shape[1]
    out = torch.empty(B, device=kt.device, dtype=torch.float32)
    L.check(lib().gd_pam_key_sqnorm_max(_ptr(kt), B, N, Npad, int(f16), _ptr(out), _stream()), "gd_pam_key_sqnorm_max")
    return out


def pam_flash_fwd(qt, kt, v, B, N, Npad, Cn, Cp, gamma, x, out, o_attn, lse, r_alg: int = 32, v_ones: bool = False,
                  f16: bool = False, k_sqmax: Optional[Tensor] = None):
    # algorithmic (unpadded) work: 2 N^2 (r + C) per image
    with _Bracket("pam_flash_fwd", 2.0 * N * N * (r_alg + Cn) * B):
        L.check(lib().gd_pam_flash_fwd(_ptr(qt), _ptr(kt), _ptr(v), B, N, Npad, Cn, Cp, int(v_ones), int(f16),
                                       _ptr(gamma), _ptr(x), _bview(x), _ptr(out), _bview(out), _ptr(o_attn), _ptr(lse),
                                       _ptr(k_sqmax), _stream()), "gd_pam_flash_fwd")


PAM_SHIFT = os.environ.get("GD_PAM_SHIFT", "0") != "0"       # bf16 forward: sampled per-query shift + max-free sweep (opt-in: see DESIGN 5.2)
PAM_SHIFT_SAMPLES = int(os.environ.get("GD_PAM_SHIFT_SAMPLES", "256"))


def pam_flash_fwd_shift(qt, kt, v, B, N, Npad, Cn, Cp, gamma, x, out, o_attn, lse, r_alg: int = 32, v_ones: bool = False,
                        nsample: Optional[int] = None, return_flags: bool = False):
    """gd_pam_flash_fwd_shift: bf16 forward with the sampled-shift max-free sweep + fallback pass for flagged workgroups"""
    _bf(qt, "qt"), _bf(kt, "kt")
    nbytes = int(lib().gd_pam_fwd_shift_ws_bytes(B, Npad))
    ws = torch.empty(nbytes // 4, device=qt.device, dtype=torch.int32)
    with _Bracket("pam_flash_fwd", 2.0 * N * N * (r_alg + Cn) * B):
        L.check(lib().gd_pam_flash_fwd_shift(_ptr(qt), _ptr(kt), _ptr(v), B, N, Npad, Cn, Cp, int(v_ones), _ptr(gamma), _ptr(x),
                                             _bview(x), _ptr(out), _bview(out), _ptr(o_attn), _ptr(lse),
                                             int(nsample or PAM_SHIFT_SAMPLES), _ptr(ws), nbytes, _stream()),
                "gd_pam_flash_fwd_shift")
    if return_flags:
        return ws[B * Npad:].clone()           # 1 = the workgroup (256 queries) was redone with the running maximum
    return None


PAM_SCRATCH_CAP = 40 << 30                                         # scratch of one call: at most 40 GiB
DETERMINISTIC = False
DET_REDUCE = "unsplit"            # how deterministic mode reduces over splits: "unsplit" or "ordered" (gd_set_det_reduce)
_DET_REDUCE_MODES = {"unsplit": 0, "ordered": 1}
DET_WS_BYTES: Optional[int] = None   # size of the ordered mode's workspace; None = GD_DET_WS_MB MiB (default 256)
_DET_WS: dict = {}                # (device index, stream handle) -> uint8 workspace tensor


def set_deterministic(on: bool, reduce: Optional[str] = None) -> None:
    """bitwise-reproducible kernels wherever a faster order-dependent form exists: PAM dQ through bf16 parts instead of
    fp32 atomics (gd_set_deterministic), and the split reductions (split-K GEMMs, 3x3 weight gradients, Discriminator1's
    stem gradient and bias sums) in the form ``reduce`` names: "unsplit" -- one adder per output element, the initial
    setting -- or "ordered" -- the default mode's splits, each writing a partial slab that a reduce kernel sums in
    ascending order (gd_set_det_reduce).  ``reduce=None`` keeps the current setting."""
    global DETERMINISTIC, DET_REDUCE
    if reduce is not None and reduce not in _DET_REDUCE_MODES:
        raise L.GandanetError(f"set_deterministic: reduce must be one of {sorted(_DET_REDUCE_MODES)}, got {reduce!r}")
    DETERMINISTIC = bool(on)
    lib().gd_set_deterministic(int(DETERMINISTIC))
    if reduce is not None:
        L.check(lib().gd_set_det_reduce(_DET_REDUCE_MODES[reduce]), "gd_set_det_reduce")
        DET_REDUCE = reduce


SPLIT_REDUCE = "ordered"          # how a split reduction combines its parts outside deterministic mode (gd_set_split_reduce)
_SPLIT_REDUCE_MODES = {"ordered": 0, "atomic": 1}


def set_split_reduce(mode: str) -> None:
    """how the split reductions outside PAM (3x3 and 1x1 weight gradients, split-K GEMMs, the D trunk's bias sums) combine
    their parts when deterministic mode is off: "ordered" -- the default: every split stores a partial slab into a
    workspace the library owns and a sum kernel adds the slabs in ascending order, bitwise reproducible, the output neither
    zeroed nor read -- or "atomic": fp32 atomics onto the zeroed output."""
    global SPLIT_REDUCE
    if mode not in _SPLIT_REDUCE_MODES:
        raise L.GandanetError(f"set_split_reduce: mode must be one of {sorted(_SPLIT_REDUCE_MODES)}, got {mode!r}")
    L.check(lib().gd_set_split_reduce(_SPLIT_REDUCE_MODES[mode]), "gd_set_split_reduce")
    SPLIT_REDUCE = mode


def split_ws_bytes() -> int:
    """bytes of partial-slab workspace the library holds for the default mode (hipMalloc: not in torch's statistics)"""
    return int(lib().gd_split_ws_bytes())


def det_ws_bytes() -> int:
    return int(DET_WS_BYTES) if DET_WS_BYTES is not None else int(os.environ.get("GD_DET_WS_MB", "256")) << 20


def det_ws() -> Tuple[Optional[int], int]:
    """(pointer, bytes) of the ordered mode's partial-slab workspace, (None, 0) outside that mode.  One tensor per
    (device, stream), allocated on first use.  Consecutive calls on one stream may share it because every use is
    stream-ordered: a split kernel and its reduce kernel are enqueued back to back, and the next call's kernels run
    after them.  Two streams never share one."""
    if not (DETERMINISTIC and DET_REDUCE == "ordered"):
        return None, 0
    nbytes = det_ws_bytes()
    if nbytes <= 0:
        return None, 0
    key = (torch.cuda.current_device(), _stream())
    t = _DET_WS.get(key)
    if t is None or t.numel() != nbytes:
        t = _DET_WS[key] = torch.empty(nbytes, device=torch.device("cuda", key[0]), dtype=torch.uint8)
    return t.data_ptr(), nbytes


def conv3x3_wgrad_plan(B: int, Cout: int, Cin: int, H: int, W: int, stride: int = 1, ws_bytes: Optional[int] = None):
    """(pixel splits, workspace bytes used) of a 3x3 weight gradient under the current modes; host only"""
    sp, need = C.c_int(0), C.c_size_t(0)
    nb = det_ws_bytes() if ws_bytes is None else ws_bytes
    L.check(lib().gd_conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride, nb, C.byref(sp), C.byref(need)), "gd_conv3x3_wgrad_plan")
    return sp.value, need.value


def gemm_nt_plan(*, B: int, M: int, N: int, kseg: int, klen: int, splits: int = 0, precision: int = L.PREC_FP32,
                 ws_bytes: Optional[int] = None):
    """(k-splits, workspace bytes used) of an NT GEMM of these sizes under the current modes; host only"""
    d = L.GemmNTDesc()
    d.B, d.M, d.N, d.kseg, d.klen, d.splits, d.precision = B, M, N, kseg, klen, splits, precision
    sp, need = C.c_int(0), C.c_size_t(0)
    nb = det_ws_bytes() if ws_bytes is None else ws_bytes
    L.check(lib().gd_gemm_nt_plan(C.byref(d), nb, C.byref(sp), C.byref(need)), "gd_gemm_nt_plan")
    return sp.value, need.value


def pam_bwd_form() -> int:
    """the backward form (gandanet.h GD_PAM_BWD_*) that pam_flash_bwd takes without an explicit ``form``: K64 with fp32
    atomics for dQ, or under set_deterministic(True) K64 with bf16 parts (bitwise reproducible).  Form 3 (two kernels without scratch, the
    reference the K64 forms are tested against) is reached through ``form`` only."""
    return L.PAM_BWD_K64_PARTS if DETERMINISTIC else L.PAM_BWD_K64_ATOMIC


def pam_flash_bwd(qt, kt, kn, vt, dot_, lse, delta, B, N, Npad, Cp, dqn, dkn, dv, r_alg: int = 32, c_alg: int = 0,
                  f16: bool = False, form: Optional[int] = None, out_bs: int = 0):
    """out_bs != 0 (form 0 only): dqn / dkn / dv are row blocks of one (B, rows, Npad) buffer with that batch stride"""
    form = pam_bwd_form() if form is None else form
    scratch, scratch_bytes = None, 0
    per_image = int(lib().gd_pam_bwd_scratch_bytes(Npad, form))
    if per_image:
        nslices = -(-(B * per_image) // PAM_SCRATCH_CAP)              # even slices of the batch that fit the cap
        images = max(1, -(-B // nslices))
        scratch_bytes = per_image * images
        scratch = torch.empty(scratch_bytes, device=dqn.device, dtype=torch.uint8)
    # algorithmic work of the backward = 2x forward: 4 N^2 (r + C) per image
    with _Bracket("pam_flash_bwd", 4.0 * N * N * (r_alg + (c_alg or Cp)) * B):
        L.check(lib().gd_pam_flash_bwd(_ptr(qt), _ptr(kt), _ptr(kn), _ptr(vt), _ptr(dot_), _ptr(lse), _ptr(delta), B,
                                       N, Npad, Cp, int(f16), int(form), _ptr(dqn), _ptr(dkn), _ptr(dv), int(out_bs),
                                       _ptr(scratch), scratch_bytes, _stream()), "gd_pam_flash_bwd")


# wide attention blocks (192 < C <= 511, gd_pam_wide_*)
def pam_wide_slots(r: int) -> int:
    """q / k slots of the wide kernels: 32 while the spare slot for the running maximum fits (r <= 31), else 64"""
    return 32 if r <= 31 else 64


def pam_wide_fwd(qt, kt, v, B, N, Npad, Cn, Cp, D, gamma, x, out, o_attn, lse, r_alg: int, f16: bool = False):
    with _Bracket("pam_wide_fwd", 2.0 * N * N * (r_alg + Cn) * B):
        L.check(lib().gd_pam_wide_fwd(_ptr(qt), _ptr(kt), _ptr(v), B, N, Npad, Cn, Cp, D, int(f16), _ptr(gamma), _ptr(x),
                                      _bview(x), _ptr(out), _bview(out), _ptr(o_attn), _ptr(lse), _stream()),
                "gd_pam_wide_fwd")


def pam_wide_bwd(qt, kt, kn, vt, dot_, lse, delta, B, N, Npad, Cp, D, dqn, dkn, dv, r_alg: int, c_alg: int,
                 f16: bool = False, deterministic: Optional[bool] = None):
    """dQ through fp32 atomics, or (set_deterministic / ``deterministic``) bf16 parts per key block + a reduction pass"""
    det = DETERMINISTIC if deterministic is None else bool(deterministic)
    scratch, scratch_bytes = None, 0
    per_image = int(lib().gd_pam_wide_scratch_bytes(Npad, D, int(det)))
    if per_image:
        nslices = -(-(B * per_image) // PAM_SCRATCH_CAP)
        scratch_bytes = per_image * max(1, -(-B // nslices))
        scratch = torch.empty(scratch_bytes, device=dqn.device, dtype=torch.uint8)
    with _Bracket("pam_wide_bwd", 4.0 * N * N * (r_alg + c_alg) * B):
        L.check(lib().gd_pam_wide_bwd(_ptr(qt), _ptr(kt), _ptr(kn), _ptr(vt), _ptr(dot_), _ptr(lse), _ptr(delta), B, N,
                                      Npad, Cp, D, int(f16), int(det), _ptr(dqn), _ptr(dkn), _ptr(dv), _ptr(scratch),
                                      scratch_bytes, _stream()), "gd_pam_wide_bwd")


# exact-operand PAM (operand mode "exact": set_precision("fp32"), layer_override(pam="exact")) through the fused fp32
# kernels (gd_pam_f32_*) instead of the product chain.  GD_PAM_F32_FLASH=1 always (C <= 511), 0 never, unset = auto: only
# where one of the chain's N x N matrices would pass PAM_F32_AUTO_ELEMS elements (B N^2 > 2^31 = 8 GiB)
_f32_flash = os.environ.get("GD_PAM_F32_FLASH", "")
PAM_F32_FLASH: Optional[bool] = True if _f32_flash == "1" else False if _f32_flash == "0" else None
PAM_F32_AUTO_ELEMS = 1 << 31


def _plane_bs(t: Tensor, name: str) -> int:
    """(B, R, Npad) fp32 plane whose rows are dense; returns its batch stride"""
    _chk(t, name)
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(1) != t.shape[2]:
        raise L.GandanetError(f"{name}: expected (B, rows, Npad) with dense rows, got strides {t.stride()}")
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2]


def pam_f32_fwd(q, k, v, B, N, Npad, Cn, r, gamma, x, out, o_attn, lse):
    """q, k (B, r, Npad), v (B, Cn, Npad) fp32 planes (zero columns past N); see gd_pam_f32_fwd"""
    with _Bracket("pam_f32_fwd", 2.0 * N * N * (r + Cn) * B):
        L.check(lib().gd_pam_f32_fwd(_ptr(q), _plane_bs(q, "q"), _ptr(k), _plane_bs(k, "k"), _ptr(v), _plane_bs(v, "v"), B, N,
                                     Npad, Cn, r, _ptr(gamma), _ptr(x), _bview(x), _ptr(out), _bview(out), _ptr(_dense(o_attn)),
                                     _ptr(_dense(lse)), _stream()), "gd_pam_f32_fwd")


def pam_f32_bwd(q, k, v, gdo, lse, delta, B, N, Npad, Cn, r, dq, dk, dv):
    """gdo (B, Cn, Npad) = gamma * dOut; dq, dk (B, r, N), dv (B, Cn, N) dense; see gd_pam_f32_bwd"""
    with _Bracket("pam_f32_bwd", 4.0 * N * N * (r + Cn) * B):
        L.check(lib().gd_pam_f32_bwd(_ptr(q), _plane_bs(q, "q"), _ptr(k), _plane_bs(k, "k"), _ptr(v), _plane_bs(v, "v"),
                                     _ptr(gdo), _plane_bs(gdo, "gdo"), _ptr(_dense(lse)), _ptr(_dense(delta)), B, N, Npad, Cn, r,
                                     _ptr(_dense(dq)), _ptr(_dense(dk)), _ptr(_dense(dv)), _stream()), "gd_pam_f32_bwd")


# ---- PAM attention probe (gd_pam_attn_*): the attention of q, k (B, r, Npad) fp32 planes without the N x N matrix ----------
def pam_attn_stats(q, k, B, N, Npad, r, lse, entropy=None, peak=None, logit_scale: float = 1.0):
    """(B, N) maps lse, entropy (nats), peak = max_j P_ij of softmax_j(logit_scale q_i . k_j); see gd_pam_attn_stats"""
    with _Bracket("pam_attn_stats", 2.0 * N * N * r * B):
        L.check(lib().gd_pam_attn_stats(_ptr(q), _plane_bs(q, "q"), _ptr(k), _plane_bs(k, "k"), B, N, Npad, r, float(logit_scale),
                                        _ptr(_dense(lse)), _ptr(None if entropy is None else _dense(entropy)),
                                        _ptr(None if peak is None else _dense(peak)), _stream()), "gd_pam_attn_stats")


def pam_attn_received(q, k, lse, B, N, Npad, r, received, logit_scale: float = 1.0):
    """received (B, N): sum over the queries of P_ij, from the lse of pam_attn_stats; see gd_pam_attn_received"""
    with _Bracket("pam_attn_received", 2.0 * N * N * r * B):
        L.check(lib().gd_pam_attn_received(_ptr(q), _plane_bs(q, "q"), _ptr(k), _plane_bs(k, "k"), _ptr(_dense(lse)), B, N, Npad,
                                           r, float(logit_scale), _ptr(_dense(received)), _stream()), "gd_pam_attn_received")


def pam_attn_rows(q, k, idx, B, N, Npad, r, rows, lse_rows=None, logit_scale: float = 1.0):
    """rows (B, S, N): the attention rows of the queries ``idx`` (int32, S values in [0, N)); see gd_pam_attn_rows"""
    _chk(idx, "idx", torch.int32)
    S = idx.numel()
    if idx.dim() != 1 or not idx.is_contiguous():
        raise L.GandanetError("idx: expected a contiguous 1-D int32 tensor")
    with _Bracket("pam_attn_rows", 4.0 * N * S * r * B):
        L.check(lib().gd_pam_attn_rows(_ptr(q), _plane_bs(q, "q"), _ptr(k), _plane_bs(k, "k"), _ptr(idx), S, B, N, Npad, r,
                                       float(logit_scale), _ptr(_dense(rows)),
                                       _ptr(None if lse_rows is None else _dense(lse_rows)), _stream()), "gd_pam_attn_rows")


def round_to_16(x: Tensor, scale: float = 1.0, f16: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """float(rne16(x * scale)) elementwise, bf16 or (``f16``) IEEE fp16: the rounding pack_bf16 applies; see gd_round_to_16"""
    _dense(x, "round_to_16 input")
    out = torch.empty_like(x) if out is None else _dense(out, "round_to_16 output")
    L.check(lib().gd_round_to_16(_ptr(x), _ptr(out), x.numel(), float(scale), int(f16), _stream()), "gd_round_to_16")
    return out


# =====================================================================================================
# NHWC bf16 kernels (frozen VGG19 feature stack of PerceptualLoss)
# =====================================================================================================
def _bf(t: Tensor, name: str = "tensor") -> Tensor:
    _chk(t, name, torch.bfloat16)
    if not t.is_contiguous():
        raise L.GandanetError(f"{name}: expected a contiguous tensor, got strides {t.stride()}")
    return t


def _nphys(split: bool) -> int:
    """physical bf16 channels per logical channel of a pixel-major tensor: 3 when split ([hi | lo | hi]), else 1"""
    return 3 if split else 1


def conv3x3_nhwc_pack(w: Tensor, transposed: bool) -> Tensor:
    """w (Cout, Cin, 3, 3) fp32 -> packed bf16 operator (transposed: 0 forward, 1 stride-1 data gradient, 2 stride-2
    data gradient)"""
    _dense(w, "conv weight")
    Cout, Cin = w.shape[0], w.shape[1]
    M, Kc = (Cin, Cout) if transposed else (Cout, Cin)
    nbytes = int(lib().gd_conv3x3_ws_bytes(M, Kc))
    ws = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    L.check(lib().gd_conv3x3_nhwc_pack(_ptr(w), Cout, Cin, int(transposed), _ptr(ws), nbytes, _stream()),
            "gd_conv3x3_nhwc_pack")
    return ws


def conv3x3_nhwc(x: Tensor, wpack: Tensor, bias: Optional[Tensor], M: int, relu: bool = False,
                 mask: Optional[Tensor] = None, res: Optional[Tensor] = None, split: bool = False) -> Tensor:
    """x (B, H, W, K) bf16 -> (B, H, W, M) bf16: [mask > 0] * act(conv3x3(x) + bias) + res; split: K = 3 Cin physical
    channels, wpack from split weights, y / mask / res with 3 M channels ([hi | lo | hi])"""
    _bf(x, "nhwc conv input")
    B, H, W, Kc = x.shape
    y = torch.empty(B, H, W, _nphys(split) * M, device=x.device, dtype=torch.bfloat16)
    for t, nm in ((mask, "mask"), (res, "res")):
        if t is not None and (_bf(t, nm).shape != y.shape):
            raise L.GandanetError(f"conv3x3_nhwc: {nm} {tuple(t.shape)} does not match the output {tuple(y.shape)}")
    with _Bracket("conv3x3_nhwc", 2.0 * 9 * Kc * M * H * W * B):
        L.check(lib().gd_conv3x3_nhwc(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(mask), _ptr(res), _ptr(y), B, H, W, Kc, M,
                                      int(relu), int(split), _stream()), "gd_conv3x3_nhwc")
    return y


def conv3x3_nhwc_f32out(x16: Tensor, wpack: Tensor, bias: Optional[Tensor], M: int, H: int, W: int, relu: bool = False,
                        out: Optional[Tensor] = None) -> Tensor:
    """x16 (B, H*W, K) pixel-major bf16 (pack_bf16 transposed output) -> conv3x3 s1 p1 (+bias, ReLU) as (B, M, H, W) fp32"""
    _bf(x16, "nhwc conv input")
    B, HW, Kc = x16.shape
    if HW != H * W:
        raise L.GandanetError(f"conv3x3_nhwc_f32out: input {tuple(x16.shape)} is not a {H} x {W} image")
    if out is None:
        out = torch.empty(B, M, H, W, device=x16.device, dtype=torch.float32)
    with _ConvBracket("nhwc_f32out", 3, 1, Kc, M, H, W, B):
        L.check(lib().gd_conv3x3_nhwc_f32out(_ptr(x16), _ptr(wpack), _ptr(bias), _ptr(out), _bview(out, "conv out"), B, H, W, Kc,
                                             M, int(relu), _stream()), "gd_conv3x3_nhwc_f32out")
    return out


# ---- split-bf16 ("x3") operands: set_precision("mixed") -------------------------------------------------------------
HLH, HL, H_ONLY = 0b010, 0b10, 0b0      # copy patterns of pack_split: bit j set = copy j holds the lo part


def pack_split(x: Tensor, *, scale: Optional[Tensor] = None, shift: Optional[Tensor] = None, relu: bool = False,
               want_plain: bool = False, want_tr: bool = True, mask: Optional[Tensor] = None):
    """(B, C, H, W) / (B, C, N) fp32 (per-image dense) -> split-bf16 copies (gd_pack_16_split):
    tr    (B, N, 3 C) pixel-major [hi | lo | hi]: the forward / data-gradient operand against gd_split3_weights
    plain (2, B, C, N) channel-major, [0] hi and [1] lo: the dY operand of the weight gradient's three launches
    mask: a ReLU output of x's shape -- the ReLU backward fused into the pack (x packed as zero where mask <= 0)"""
    sbs = _bview(x, "pack input")
    if mask is not None and tuple(mask.shape[:2]) + (mask[0, 0].numel(),) != tuple(x.shape[:2]) + (x[0, 0].numel(),):
        raise L.GandanetError(f"pack_split: mask {tuple(mask.shape)} does not match {tuple(x.shape)}")
    B, Cn = x.shape[0], x.shape[1]
    N = x[0, 0].numel()
    plain = torch.empty(2, B, Cn, N, device=x.device, dtype=torch.bfloat16) if want_plain else None
    tr = torch.empty(B, N, 3 * Cn, device=x.device, dtype=torch.bfloat16) if want_tr else None
    L.check(lib().gd_pack_16_split_masked(_ptr(x), sbs, B, Cn, N, _ptr(scale), _ptr(shift), int(relu),
                                          _ptr(plain), Cn * N, N, B * Cn * N, 2, HL,
                                          _ptr(tr), N * 3 * Cn, 3 * Cn, Cn, 3, HLH,
                                          _ptr(mask), 0 if mask is None else _bview(mask, "pack mask"), _stream()),
            "gd_pack_16_split")
    return plain, tr


def split3_weights(w: Tensor, axis: int) -> Tensor:
    """(Cout, Cin, k, k) fp32 -> [hi ; hi ; lo] along ``axis`` (1: input channels, forward; 0: output channels, the
    data gradient's contraction axis)"""
    _dense(w, "conv weight")
    Cout, Cin = w.shape[0], w.shape[1]
    taps = w[0, 0].numel()
    if axis == 1:
        out = torch.empty(Cout, 3 * Cin, *w.shape[2:], device=w.device, dtype=torch.float32)
        L.check(lib().gd_split3_weights(_ptr(w), Cout, Cin, taps, _ptr(out), _stream()), "gd_split3_weights")
    else:
        out = torch.empty(3 * Cout, Cin, *w.shape[2:], device=w.device, dtype=torch.float32)
        L.check(lib().gd_split3_weights(_ptr(w), 1, Cout, Cin * taps, _ptr(out), _stream()), "gd_split3_weights")
    return out


# the split weight gradient dW = dy_hi (x) x_hi + dy_lo (x) x_hi + dy_hi (x) x_lo, one launch per row:
# (part of dy16 [hi, lo], column block of x16 [hi | lo | hi], accumulate); the plain one is the first row alone
_WGRAD16_SPLIT = ((0, 0, 0), (1, 0, 1), (0, 1, 1))


def conv3x3_wgrad16(dy16: Tensor, x16: Tensor, H: int, W: int, stride: int = 1, split: bool = False,
                    tag: str = "wgrad_packed") -> Tensor:
    """weight gradient of a 3x3 / pad 1 conv from 16-bit copies of both operands (one launch):
    dy16 (B, Cout, Ho*Wo) channel-major, x16 (B, H*W, Cin) pixel-major (the forward's own pack).
    split: dy16 (2, B, Cout, Ho*Wo) [hi, lo], x16 (B, H*W, 3 Cin) [hi | lo | hi]; three launches adding into one dW"""
    _bf(dy16, "dy16"), _bf(x16, "x16")
    parts = dy16 if split else dy16[None]
    _, B, Cout, _ = parts.shape
    x_ld = x16.shape[2]
    Cin = x_ld // _nphys(split)
    dw = torch.empty(Cout, Cin, 3, 3, device=dy16.device, dtype=torch.float32)
    with _ConvBracket(tag, 3, stride, Cin, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1, B):
        for part, xblk, acc in _WGRAD16_SPLIT if split else _WGRAD16_SPLIT[:1]:
            L.check(lib().gd_conv3x3_wgrad_ws(None, 0, parts[part].data_ptr(), None, 0, x16.data_ptr() + 2 * xblk * Cin, x_ld,
                                              None, None, 0, B, Cout, Cin, H, W, stride, acc, _ptr(dw), _stream(), *det_ws()),
                    "gd_conv3x3_wgrad")
    return dw


_CONV3X3_ROLES = {"fwd": (1, 0), "dgrad": (0, 1), "dgrad_s2": (0, 2)}     # role -> (split3_weights axis, transposed)


def conv3x3_operator(w: Tensor, role: str, split: bool = False) -> Tensor:
    """the packed operator of w (Cout, Cin, 3, 3) for the pixel-major kernels: "fwd" the forward, "dgrad" / "dgrad_s2" the
    stride-1 / stride-2 data gradient; split: of the weights split [hi ; hi ; lo] along that role's contraction axis"""
    axis, transposed = _CONV3X3_ROLES[role]
    return conv3x3_nhwc_pack(split3_weights(w, axis) if split else w, transposed)


# ---- Discriminator1 on pixel-major bf16 (discriminator.py:57-77) ------------------------------------------------------
def _half_up(n: int) -> int:
    return (n - 1) // 2 + 1


def _stem_fwd(name: str, img: Tensor, w: Tensor, bias: Optional[Tensor], stride: int, act, split: bool) -> Tensor:
    """gd_<name>: fp32 NCHW image -> act(conv3x3 p1 + bias) at ``stride``, pixel-major bf16; act = its ReLU flag / LeakyReLU slope"""
    _dense(img, "stem image"), _dense(w, "stem weight")
    B, Ci, H, W = img.shape
    Co = w.shape[0]
    if w.shape[1] != Ci:
        raise L.GandanetError(f"{name}: weight {tuple(w.shape)} does not match image {tuple(img.shape)}")
    y = torch.empty(B, (H - 1) // stride + 1, (W - 1) // stride + 1, _nphys(split) * Co, device=img.device, dtype=torch.bfloat16)
    L.check(getattr(lib(), "gd_" + name)(_ptr(img), B, Ci, H, W, _ptr(w), _ptr(bias), Co, act, _ptr(y), int(split), _stream()),
            "gd_" + name)
    return y


def _stem_dgrad(name: str, g: Tensor, w: Tensor, H: int, W: int, stride: int, split: bool) -> Tensor:
    """gd_<name>: pixel-major bf16 gradient of a stem's pre-activation -> fp32 gradient (B, Ci, H, W) of its image"""
    _bf(g, "stem gradient"), _dense(w, "stem weight")
    B, Ho, Wo, Co = g.shape
    if (Ho, Wo) != ((H - 1) // stride + 1, (W - 1) // stride + 1):
        raise L.GandanetError(f"{name}: gradient {tuple(g.shape)} does not match a {H} x {W} image")
    dimg = torch.empty(B, w.shape[1], H, W, device=g.device, dtype=torch.float32)
    L.check(getattr(lib(), "gd_" + name)(_ptr(g), B, w.shape[1], H, W, _ptr(w), Co // _nphys(split), _ptr(dimg), int(split),
                                         _stream()), "gd_" + name)
    return dimg


def disc_stem_fwd(img: Tensor, w: Tensor, bias: Optional[Tensor], slope: float, split: bool = False) -> Tensor:
    """conv1: fp32 NCHW image -> LeakyReLU(conv3x3 s2 p1 + bias) as (B, Ho, Wo, Co) bf16; ``split`` (here and in the
    functions below): pixel-major tensors carry 3 C channels per pixel, the values split [hi | lo | hi] (operand mode "x3")"""
    return _stem_fwd("disc_stem_fwd", img, w, bias, 2, float(slope), split)


def disc_stem_wgrad(g: Tensor, img: Tensor, want_bias: bool = True, split: bool = False):
    """(dw (Co, Ci, 3, 3), db (Co) or None) of conv1 from the pre-activation gradient g (B, Ho, Wo, Co) bf16"""
    _bf(g, "stem gradient"), _dense(img, "stem image")
    B, Ci, H, W = img.shape
    Co = g.shape[3] // _nphys(split)
    if g.shape[:3] != (B, _half_up(H), _half_up(W)):
        raise L.GandanetError(f"disc_stem_wgrad: gradient {tuple(g.shape)} does not match image {tuple(img.shape)}")
    dw = torch.empty(Co, Ci, 3, 3, device=g.device, dtype=torch.float32)
    db = torch.empty(Co, device=g.device, dtype=torch.float32) if want_bias else None
    L.check(lib().gd_disc_stem_wgrad_ws(_ptr(g), _ptr(img), B, Ci, H, W, Co, _ptr(dw), _ptr(db), int(split), _stream(),
                                        *det_ws()), "gd_disc_stem_wgrad")
    return dw, db


def disc_stem_dgrad(g: Tensor, w: Tensor, H: int, W: int, split: bool = False) -> Tensor:
    return _stem_dgrad("disc_stem_dgrad", g, w, H, W, 2, split)


def conv3x3_nhwc_s2(x: Tensor, wpack: Tensor, bias: Optional[Tensor], M: int, act: int, slope: float = 0.2,
                    split: bool = False) -> Tensor:
    """x (B, H, W, K) bf16 -> act(conv3x3 s2 p1 + bias) (B, Ho, Wo, M) bf16; act 0 none / 1 ReLU / 2 LeakyReLU(slope);
    split: K = 3 Cin physical channels in, 3 M out, wpack from split3_weights(w, 1)"""
    _bf(x, "nhwc conv input")
    B, H, W, Kc = x.shape
    y = torch.empty(B, _half_up(H), _half_up(W), _nphys(split) * M, device=x.device, dtype=torch.bfloat16)
    with _Bracket("conv3x3_nhwc_s2", 2.0 * 9 * Kc * M * y.shape[1] * y.shape[2] * B):
        L.check(lib().gd_conv3x3_nhwc_s2(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(y), B, H, W, Kc, M, int(act), float(slope),
                                         int(split), _stream()), "gd_conv3x3_nhwc_s2")
    return y


def conv3x3_nhwc_s2_dgrad(dy: Tensor, wpack_t: Tensor, act_out: Tensor, slope: float = 0.2, split: bool = False) -> Tensor:
    """dy (B, Ho, Wo, M) bf16 -> dx (B, H, W, K) bf16 = convT(dy) * LeakyReLU'(act_out); shape taken from act_out;
    split: dy carries M = 3 Cout physical channels, act_out and dx 3 K, wpack_t from split3_weights(w, 0)"""
    _bf(dy, "nhwc conv gradient"), _bf(act_out, "activation output")
    B, H, W, Kc = act_out.shape
    Kc //= _nphys(split)
    M = dy.shape[3]
    if dy.shape[:3] != (B, _half_up(H), _half_up(W)):
        raise L.GandanetError(f"conv3x3_nhwc_s2_dgrad: dy {tuple(dy.shape)} does not match input {tuple(act_out.shape)}")
    dx = torch.empty_like(act_out)
    with _Bracket("conv3x3_nhwc_s2_dgrad", 2.0 * 9 * Kc * M * dy.shape[1] * dy.shape[2] * B):
        L.check(lib().gd_conv3x3_nhwc_s2_dgrad(_ptr(dy), _ptr(wpack_t), _ptr(act_out), float(slope), _ptr(dx), B, H, W, Kc, M,
                                               int(split), _stream()), "gd_conv3x3_nhwc_s2_dgrad")
    return dx


def nhwc_flatten_fwd(y: Tensor, split: bool = False) -> Tensor:
    """(B, h, w, C) bf16 -> (B, C*h*w) fp32 in the (c, h, w) order of NCHW .flatten(1)"""
    _bf(y, "flatten input")
    B, H, W, Cc = y.shape
    Cc //= _nphys(split)
    f = torch.empty(B, Cc * H * W, device=y.device, dtype=torch.float32)
    L.check(lib().gd_nhwc_flatten_fwd(_ptr(y), B, H * W, Cc, _ptr(f), int(split), _stream()), "gd_nhwc_flatten_fwd")
    return f


def nhwc_flatten_bwd(df: Tensor, y: Tensor, slope: float, split: bool = False) -> Tensor:
    _bf(y, "flatten input"), _dense(df, "flatten gradient")
    B, H, W, Cc = y.shape
    Cc //= _nphys(split)
    if df.numel() * _nphys(split) != y.numel():
        raise L.GandanetError(f"nhwc_flatten_bwd: gradient {tuple(df.shape)} does not match {tuple(y.shape)}")
    g = torch.empty_like(y)
    L.check(lib().gd_nhwc_flatten_bwd(_ptr(df), _ptr(y), float(slope), B, H * W, Cc, _ptr(g), int(split), _stream()),
            "gd_nhwc_flatten_bwd")
    return g


def nhwc_to_nchw16(g: Tensor, want_sum: bool, split: bool = False):
    """(B, h, w, C) bf16 -> ((B, C, h, w) bf16, per-channel sums (C) fp32 or None); split: g carries 3 C channels
    [hi | lo | hi] and the result is (2, B, C, h, w), hi then lo, with the sums of hi + lo"""
    _bf(g, "nhwc gradient")
    B, H, W, Cc = g.shape
    Cc //= _nphys(split)
    gt = torch.empty((2, B, Cc, H, W) if split else (B, Cc, H, W), device=g.device, dtype=torch.bfloat16)
    cs = torch.empty(Cc, device=g.device, dtype=torch.float32) if want_sum else None
    L.check(lib().gd_nhwc_to_nchw16_ws(_ptr(g), B, H * W, Cc, _ptr(gt), _ptr(cs), int(split), _stream(), *det_ws()),
            "gd_nhwc_to_nchw16")
    return gt, cs


def conv3x3_wgrad_nhwc(g: Tensor, x: Tensor, stride: int, want_bias: bool, split: bool = False):
    """Weight (and bias) gradient of a 3x3 / pad 1 conv whose input x (B, H, W, Cin) and output gradient g
    (B, Ho, Wo, Cout) are pixel-major bf16: g goes channel-major once (fused with the bias sums), x is staged as is.
    split: both carry [hi | lo | hi] (conv3x3_wgrad16)"""
    _bf(g, "nhwc gradient"), _bf(x, "nhwc input")
    B, H, W, Kc = x.shape
    gt, db = nhwc_to_nchw16(g, want_bias, split)
    return conv3x3_wgrad16(gt.flatten(-2), x.view(B, H * W, Kc), H, W, stride, split,
                           "wgrad_nhwc_x3" if split else "wgrad_nhwc"), db


def nhwc_stem_fwd(img: Tensor, w: Tensor, bias: Optional[Tensor], relu: bool, split: bool = False) -> Tensor:
    """``split`` (here and in the nhwc_* functions below): the pixel-major tensors carry 3 C channels per pixel, the values
    split [hi | lo | hi] (operand mode "x3")"""
    return _stem_fwd("nhwc_stem_fwd", img, w, bias, 1, int(relu), split)


def nhwc_stem_bwd(g: Tensor, w: Tensor, split: bool = False) -> Tensor:
    return _stem_dgrad("nhwc_stem_bwd", g, w, g.shape[1], g.shape[2], 1, split)


def nhwc_maxpool2_fwd(x: Tensor, split: bool = False) -> Tensor:
    _bf(x, "pool input")
    B, H, W, Cn = x.shape
    y = torch.empty(B, H // 2, W // 2, Cn, device=x.device, dtype=torch.bfloat16)
    L.check(lib().gd_nhwc_maxpool2_fwd(_ptr(x), B, H, W, Cn // _nphys(split), _ptr(y), int(split), _stream()),
            "gd_nhwc_maxpool2_fwd")
    return y


def nhwc_maxpool2_bwd(x: Tensor, dy: Tensor, relu_mask: bool, split: bool = False) -> Tensor:
    _bf(x, "pool input"), _bf(dy, "pool dy")
    B, H, W, Cn = x.shape
    dx = torch.empty_like(x)
    L.check(lib().gd_nhwc_maxpool2_bwd(_ptr(x), _ptr(dy), B, H, W, Cn // _nphys(split), int(relu_mask), _ptr(dx), int(split),
                                       _stream()), "gd_nhwc_maxpool2_bwd")
    return dx


def nhwc_l1(a: Tensor, b: Tensor, out: Tensor, accumulate: bool, split: bool = False) -> None:
    """out[0] (+)= mean |a - b| over bf16 tensors of equal shape (split: (..., 3 C) tensors of hi + lo values)"""
    _bf(a, "l1 a"), _bf(b, "l1 b")
    ws = torch.empty(1024, device=a.device, dtype=torch.float32)
    sc = a.shape[-1] // 3 if split else 0
    L.check(lib().gd_nhwc_l1(_ptr(a), _ptr(b), a.numel() // _nphys(split), _ptr(out), int(accumulate), _ptr(ws), sc,
                             _stream()), "gd_nhwc_l1")


def nhwc_l1_grad(a: Tensor, b: Tensor, upstream: Tensor, relu_mask: bool, split: bool = False) -> Tensor:
    _bf(a, "l1 a"), _bf(b, "l1 b"), _dense(upstream, "upstream gradient")
    g = torch.empty_like(a)
    sc = a.shape[-1] // 3 if split else 0
    L.check(lib().gd_nhwc_l1_grad(_ptr(a), _ptr(b), a.numel() // _nphys(split), _ptr(upstream), int(relu_mask), _ptr(g), sc,
                                  _stream()), "gd_nhwc_l1_grad")
    return g


# ---- evaluation (evalstats.hip) ----------------------------------------------------------------------------------------
def _filter_dtype(t: Tensor, name: str, u8: bool = False) -> int:
    """fp32 -> GD_FILTER_F32, fp64 -> GD_FILTER_F64 (with ``u8``: uint8 -> GD_CCL_U8) for a dense GPU tensor; the tag of every
    analysis entry point"""
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise L.GandanetError(f"{name}: expected a GPU tensor (there is no CPU fallback in the product path)")
    if t.dtype not in (torch.float32, torch.float64) and not (u8 and t.dtype == torch.uint8):
        raise L.GandanetError(f"{name}: expected float32{', ' if u8 else ' or '}float64{' or uint8' if u8 else ''}, got {t.dtype}")
    if not t.is_contiguous():
        raise L.GandanetError(f"{name}: expected a contiguous tensor, got strides {t.stride()}")
    return _Dev.tags[t.dtype]


def _out_dtype(out_dtype, src: Tensor, fn: str):
    """the output dtype of ``fn``: fp32 or fp64, the dtype of ``src`` by default"""
    out_dtype = src.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise L.GandanetError(f"{fn}: expected float32 or float64 output, got {out_dtype}")
    return out_dtype


def _plane_chunks(planes: int):
    """(lo, k): the planes [lo, lo + k) of one launch, at most 65535 (the grid.y limit)"""
    for lo in range(0, planes, 65535):
        yield lo, min(65535, planes - lo)


def eval_stats(pred: Tensor, truth: Tensor, rec: Tensor, mask: Optional[Tensor] = None, affine=None,
               skip_nan: bool = False) -> Tensor:
    """the 8-double record of ``pred`` against ``truth`` (include/gandanet.h, "evaluation") written into ``rec`` (a view
    of 8 fp64 on the device); ``mask`` (uint8, one entry per element of the trailing dims it covers) is shared by all
    leading planes; ``affine`` = (a, b) reads both inputs as v * a + b.  No host sync."""
    f64 = _filter_dtype(pred, "pred")
    if _filter_dtype(truth, "truth") != f64 or pred.shape != truth.shape:
        raise L.GandanetError(f"eval_stats: pred {tuple(pred.shape)} {pred.dtype} vs truth {tuple(truth.shape)} {truth.dtype}")
    _chk(rec, "record", torch.float64)
    if rec.numel() != 8 or not rec.is_contiguous():
        raise L.GandanetError("eval_stats: the record is 8 contiguous float64")
    n = pred.numel()
    hw = n if mask is None else mask.numel()
    if hw <= 0 or n % hw:
        raise L.GandanetError(f"eval_stats: a mask of {hw} entries does not tile {tuple(pred.shape)}")
    mask = _DEV.vec(mask, hw, "mask", torch.uint8)
    a, b = (1.0, 0.0) if affine is None else (float(affine[0]), float(affine[1]))
    nbytes = int(lib().gd_eval_stats_ws_bytes(n))
    ws = torch.empty(nbytes, device=pred.device, dtype=torch.uint8)
    flags = (L.EVAL_F64 if f64 else 0) | (L.EVAL_SKIP_NAN if skip_nan else 0)
    L.check(lib().gd_eval_stats(_ptr(pred), _ptr(truth), n // hw, hw, _ptr(mask), a, b, flags, _ptr(rec), _ptr(ws), nbytes,
                                _stream()), "gd_eval_stats")
    return rec


def _plane_mean(x: Tensor, mask: Optional[Tensor], plane_dims: int, dtype) -> Tuple[Tensor, Tensor]:
    _dense(x, "planes", dtype)
    fn = "gd_masked_plane_mean" + ("_f64" if dtype == torch.float64 else "")
    launch, ws_bytes = getattr(lib(), fn), getattr(lib(), fn + "_ws_bytes")
    lead = tuple(x.shape[:x.dim() - plane_dims])
    hw = math.prod(x.shape[x.dim() - plane_dims:])
    mask = _DEV.vec(mask, hw, "mask", torch.uint8)
    mean = torch.empty(lead, device=x.device, dtype=torch.float64)
    count = torch.empty(lead, device=x.device, dtype=torch.int64)
    for lo, k in _plane_chunks(math.prod(lead)):
        nbytes = int(ws_bytes(k, hw))
        ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
        L.check(launch(x.data_ptr() + x.element_size() * lo * hw, k, hw, _ptr(mask), mean.data_ptr() + 8 * lo,
                       count.data_ptr() + 8 * lo, _ptr(ws), nbytes, _stream()), fn)
    return mean, count


def masked_plane_mean(x: Tensor, mask: Optional[Tensor] = None, plane_dims: int = 2) -> Tuple[Tensor, Tensor]:
    """np.nanmean over the last ``plane_dims`` dims of the fp32 ``x`` with the pixels where ``mask`` is 0 left out: (mean
    fp64, valid count int64), both shaped like the leading dims; a plane without a valid pixel gives NaN"""
    return _plane_mean(x, mask, plane_dims, torch.float32)


def masked_plane_mean_f64(x: Tensor, mask: Optional[Tensor] = None, plane_dims: int = 2) -> Tuple[Tensor, Tensor]:
    """``masked_plane_mean`` of an fp64 tensor; NaN pixels are left out as well, as np.nanmean leaves them out"""
    return _plane_mean(x, mask, plane_dims, torch.float64)


def ensemble_stats(x: Tensor, mean: Optional[Tensor] = None, std: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """mean and population std over dim 0 of ``x`` (M, ...) with 1 <= M <= 32: every member dense, members a constant
    stride apart (a slab with unused rows behind each member is fine); fp32 or fp64, outputs in the same dtype"""
    if not x.is_cuda or x.dtype not in (torch.float32, torch.float64):
        raise L.GandanetError(f"ensemble_stats: expected a float32 / float64 GPU tensor, got {x.dtype} on {x.device}")
    M = x.shape[0]
    if x.dim() < 2 or not x[0].is_contiguous():
        raise L.GandanetError(f"ensemble_stats: every member must be dense, got strides {x.stride()}")
    n = x[0].numel()
    stride = x.stride(0) if M > 1 else n
    mean = torch.empty(x.shape[1:], device=x.device, dtype=x.dtype) if mean is None else mean
    std = torch.empty(x.shape[1:], device=x.device, dtype=x.dtype) if std is None else std
    for o, nm in ((mean, "mean"), (std, "std")):
        if not o.is_cuda or o.dtype != x.dtype or o.numel() != n or not o.is_contiguous():
            raise L.GandanetError(f"ensemble_stats: {nm} must be a dense {x.dtype} GPU tensor of {n} elements")
    L.check(lib().gd_ensemble_stats(_ptr(x), M, stride, n, int(x.dtype == torch.float64), _ptr(mean), _ptr(std), _stream()),
            "gd_ensemble_stats")
    return mean, std


def eval_merge_host(records) -> Tuple[list, dict]:
    """merge (k, 8) host records in the given order (plain C++ on the host, no GPU): (merged record, metrics dict)"""
    recs = np.ascontiguousarray(np.asarray(records, dtype=np.float64).reshape(-1, 8))
    out, met = (C.c_double * 8)(), (C.c_double * 4)()
    ptr = recs.ctypes.data_as(C.POINTER(C.c_double)) if len(recs) else None
    L.check(lib().gd_eval_merge_host(ptr, len(recs), out, met), "gd_eval_merge_host")
    return list(out), {"n": out[0], "mse": met[0], "mae": met[1], "r2": met[2], "cc": met[3]}


# ---- guarded step (include/gandanet.h, "guarded step") --------------------------------------------------------------
def guard_record(device) -> Tensor:
    """a zeroed guard record: 6 fp64 on ``device`` (sqnorm, norm, coef, ok, applied_steps, skipped_steps)"""
    return torch.zeros(L.GUARD_RECORD, device=device, dtype=torch.float64)


def _guard_rec(rec: Tensor) -> Tensor:
    _chk(rec, "guard record", torch.float64)
    if rec.numel() != L.GUARD_RECORD or not rec.is_contiguous():
        raise L.GandanetError(f"guard record: expected {L.GUARD_RECORD} contiguous float64")
    return rec


def grad_sqnorm(grads, rec: Tensor, grad_scale: float = 1.0, accumulate: bool = False) -> Tensor:
    """rec[0] (+)= sum over the dense fp32 tensors ``grads`` of (g * grad_scale)^2, in fp64 and in a fixed order; the
    pointers travel in the kernel arguments, so nothing is copied to the device and nothing waits.  No host sync."""
    _guard_rec(rec)
    grads = list(grads)
    if not grads:
        raise L.GandanetError("grad_sqnorm: empty tensor list")
    for g in grads:
        _dense(g, "grad_sqnorm tensor")
    k = len(grads)
    ptrs = (L.c_fp * k)(*[g.data_ptr() for g in grads])
    ns = (C.c_long * k)(*[g.numel() for g in grads])
    nbytes = int(lib().gd_grad_sqnorm_ws_bytes(sum(-(-g.numel() // L.GUARD_CHUNK) for g in grads)))
    ws = torch.empty(max(nbytes, 8), device=rec.device, dtype=torch.uint8)
    L.check(lib().gd_grad_sqnorm(ptrs, ns, k, grad_scale, int(accumulate), _ptr(rec), _ptr(ws), nbytes, _stream()),
            "gd_grad_sqnorm")
    return rec


def guard_finalize(rec: Tensor, max_norm: Optional[float] = None, skip_nonfinite: bool = False) -> Tensor:
    """norm, clip factor and the apply / skip decision from rec[0]; advances applied_steps or skipped_steps"""
    _guard_rec(rec)
    L.check(lib().gd_guard_finalize(_ptr(rec), 0.0 if max_norm is None else float(max_norm), int(skip_nonfinite), _stream()),
            "gd_guard_finalize")
    return rec


def adamw_guarded(p: Tensor, g: Tensor, m: Tensor, v: Tensor, rec: Tensor, lr: float, beta1: float, beta2: float, eps: float,
                  weight_decay: float, grad_scale: float = 1.0, ema: Optional[Tensor] = None, ema_decay: float = 0.0) -> None:
    """``adamw`` under the decision in ``rec``: clipped by rec's coef, skipped when rec's ok is 0, bias-corrected by rec's
    applied_steps; ``ema`` (optional) is updated in the same launch"""
    _guard_rec(rec)
    for t in (p, g, m, v) + (() if ema is None else (ema,)):
        _dense(t, "adamw_guarded tensor")
        if t.numel() != p.numel():
            raise L.GandanetError("adamw_guarded: tensors of different sizes")
    L.check(lib().gd_adamw_guarded(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), p.numel(), _ptr(rec), lr, beta1, beta2, eps,
                                   weight_decay, grad_scale, ema_decay, _stream()), "gd_adamw_guarded")


# ---- filters (include/gandanet.h, "filters"; filters.hip) ------------------------------------------------------------
def _axis_view(t: Tensor, axis: int) -> Tuple[int, int, int]:
    """(outer, L, inner) of a dense tensor around ``axis``"""
    return math.prod(t.shape[:axis]), t.shape[axis], math.prod(t.shape[axis + 1:])


def gaussian_weights_host(sigma: float, truncate: float = 4.0):
    """scipy's Gaussian taps as a ctypes array of 2 * radius + 1 doubles, and the radius (plain C++ on the host, no GPU)"""
    cap = 2 * L.FILTER_MAX_RADIUS + 1
    w = (C.c_double * cap)()
    radius = lib().gd_gaussian_weights_host(float(sigma), float(truncate), w, cap)
    if radius < 0:
        raise L.GandanetError(f"gd_gaussian_weights_host failed (rc={radius}): {L.last_error()}")
    return w, radius


def correlate1d_axis(src: Tensor, dst: Tensor, axis: int, weights, radius: int, edge_mode: int = L.EDGE_REFLECT) -> Tensor:
    """``dst`` = ``src`` correlated with ``weights`` (2 * radius + 1 host doubles) along ``axis``; no host sync"""
    dt = _filter_dtype(src, "correlate1d src")
    if _filter_dtype(dst, "correlate1d dst") != dt or dst.shape != src.shape:
        raise L.GandanetError(f"correlate1d_axis: src {tuple(src.shape)} {src.dtype} vs dst {tuple(dst.shape)} {dst.dtype}")
    if not isinstance(weights, C.Array):
        weights = (C.c_double * len(weights))(*[float(v) for v in weights])
    if len(weights) < 2 * radius + 1:
        raise L.GandanetError(f"correlate1d_axis: {len(weights)} weights for radius {radius}")
    outer, n, inner = _axis_view(src, axis)
    L.check(lib().gd_correlate1d_axis(_ptr(src), _ptr(dst), dt, outer, n, inner, weights, radius, edge_mode, _stream()),
            "gd_correlate1d_axis")
    return dst


def savgol_edges_axis(src: Tensor, dst: Tensor, axis: int, edge: Tensor, window: int) -> Tensor:
    """the first and last ``window // 2`` positions of ``dst`` along ``axis`` from ``edge`` (2, window // 2, window) fp64"""
    dt = _filter_dtype(src, "savgol src")
    if _filter_dtype(dst, "savgol dst") != dt or dst.shape != src.shape:
        raise L.GandanetError(f"savgol_edges_axis: src {tuple(src.shape)} {src.dtype} vs dst {tuple(dst.shape)} {dst.dtype}")
    _chk(edge, "savgol edge matrices", torch.float64)
    if not edge.is_contiguous() or tuple(edge.shape) != (2, window // 2, window):
        raise L.GandanetError(f"savgol_edges_axis: edge matrices {tuple(edge.shape)}, expected {(2, window // 2, window)}")
    outer, n, inner = _axis_view(src, axis)
    L.check(lib().gd_savgol_edges_axis(_ptr(src), _ptr(dst), dt, outer, n, inner, _ptr(edge), window, _stream()),
            "gd_savgol_edges_axis")
    return dst


def median_nd(src: Tensor, shape4, size4) -> Tensor:
    """median over a ``size4`` box of ``src`` seen as the 4-D ``shape4`` ('reflect' edges); a new tensor shaped like src"""
    dt = _filter_dtype(src, "median src")
    if len(shape4) != 4 or len(size4) != 4 or math.prod(shape4) != src.numel():
        raise L.GandanetError(f"median_nd: {tuple(shape4)} / {tuple(size4)} is not a 4-D view of {tuple(src.shape)}")
    dst = torch.empty_like(src)
    L.check(lib().gd_median_nd(_ptr(src), _ptr(dst), dt, (C.c_int64 * 4)(*shape4), (C.c_int * 4)(*size4), _stream()),
            "gd_median_nd")
    return dst


def fill_prepare(x: Tensor, placeholder: float) -> Tuple[Tensor, Tensor]:
    """(x with the gaps ``x <= placeholder`` zeroed, the valid mask as 0 / 1 in x's dtype) in one pass"""
    dt = _filter_dtype(x, "fill input")
    vals, mask = torch.empty_like(x), torch.empty_like(x)
    L.check(lib().gd_fill_prepare(_ptr(x), float(placeholder), _ptr(vals), _ptr(mask), dt, x.numel(), _stream()),
            "gd_fill_prepare")
    return vals, mask


def fill_ratio(x: Tensor, num: Tensor, den: Tensor, placeholder: float) -> Tensor:
    """num / (den == 0 ? 1 : den) at the gaps of ``x``, ``x`` itself elsewhere; a new tensor"""
    dt = _filter_dtype(x, "fill input")
    for t, nm in ((num, "numerator"), (den, "denominator")):
        if _filter_dtype(t, nm) != dt or t.shape != x.shape:
            raise L.GandanetError(f"fill_ratio: {nm} {tuple(t.shape)} {t.dtype} vs x {tuple(x.shape)} {x.dtype}")
    dst = torch.empty_like(x)
    L.check(lib().gd_fill_ratio(_ptr(x), _ptr(num), _ptr(den), float(placeholder), _ptr(dst), dt, x.numel(), _stream()),
            "gd_fill_ratio")
    return dst


# ---- spline zoom (include/gandanet.h, "spline zoom"; spline.hip) -------------------------------------------------------
def zoom_axis(src: Tensor, axis: int, n_out: int, order: int, mode: int, out_dtype=None) -> Tensor:
    """``src`` zoomed to ``n_out`` samples along ``axis`` (scipy.ndimage.zoom's rule for one axis); a new tensor of
    ``out_dtype`` (default: the dtype of ``src``).  The order-3 coefficients live in a temporary.  No host sync."""
    sdt = _filter_dtype(src, "zoom src")
    out_dtype = _out_dtype(out_dtype, src, "zoom_axis")
    outer, n, inner = _axis_view(src, axis)
    shape = list(src.shape)
    shape[axis] = int(n_out)
    dst = torch.empty(shape, device=src.device, dtype=out_dtype)
    nbytes = int(lib().gd_zoom_axis_ws_bytes(outer, n, inner, order, mode))
    ws = torch.empty(nbytes, device=src.device, dtype=torch.uint8) if nbytes else None
    L.check(lib().gd_zoom_axis(_ptr(src), _ptr(dst), sdt, int(out_dtype == torch.float64), outer, n, int(n_out), inner, order,
                               mode, _ptr(ws), nbytes, _stream()), "gd_zoom_axis")
    return dst


def spline_prefilter_axis(src: Tensor, axis: int) -> Tensor:
    """the cubic B-spline coefficients of ``src`` along ``axis`` (mirror boundary) as a new fp64 tensor"""
    sdt = _filter_dtype(src, "spline_filter src")
    outer, n, inner = _axis_view(src, axis)
    dst = torch.empty(src.shape, device=src.device, dtype=torch.float64)
    L.check(lib().gd_spline_prefilter_axis(_ptr(src), _ptr(dst), sdt, outer, n, inner, _stream()), "gd_spline_prefilter_axis")
    return dst


def restore_units(x: Tensor, trend: Optional[Tensor], mask: Optional[Tensor], scale: float, mean: float, unit: float,
                  out: Tensor) -> Tensor:
    """``out`` = ((x + trend) * scale + mean) * unit in fp64, NaN where ``mask`` (uint8, one entry per element of the
    trailing dims it covers) is 0; ``out`` may be ``x`` itself when the dtypes match"""
    xdt = _filter_dtype(x, "restore_units x")
    odt = _filter_dtype(out, "restore_units out")
    if out.shape != x.shape:
        raise L.GandanetError(f"restore_units: out {tuple(out.shape)} vs x {tuple(x.shape)}")
    tdt = 0
    if trend is not None:
        tdt = _filter_dtype(trend, "restore_units trend")
        if trend.shape != x.shape:
            raise L.GandanetError(f"restore_units: trend {tuple(trend.shape)} vs x {tuple(x.shape)}")
    n = x.numel()
    hw = n
    if mask is not None:
        hw = mask.numel()
        _DEV.vec(mask, hw, "mask", torch.uint8)
        if hw == 0 or n % hw or tuple(x.shape[x.dim() - mask.dim():]) != tuple(mask.shape):
            raise L.GandanetError(f"restore_units: mask {tuple(mask.shape)} does not cover the trailing dims of {tuple(x.shape)}")
    L.check(lib().gd_restore_units(_ptr(x), xdt, _ptr(trend), tdt, _ptr(mask), n // hw, hw, float(scale), float(mean),
                                   float(unit), _ptr(out), odt, _stream()), "gd_restore_units")
    return out


# ---- dataset preparation (include/gandanet.h, "dataset preparation"; prepare.hip) ----------------------------------------
def channel_moments(x: Tensor, channels: int) -> Tensor:
    """(count, mean, M2) of every channel of the dense channel-last ``x`` seen as (numel / channels, channels): a new
    (channels, 3) fp64 device tensor.  No host sync."""
    dt = _filter_dtype(x, "channel_moments input")
    c = int(channels)
    if c <= 0 or x.numel() == 0 or x.numel() % c:
        raise L.GandanetError(f"channel_moments: {tuple(x.shape)} is not a non-empty array of rows of {c} channels")
    m = x.numel() // c
    rec = torch.empty(c, 3, device=x.device, dtype=torch.float64)
    nbytes = int(lib().gd_channel_moments_ws_bytes(m, c))
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    L.check(lib().gd_channel_moments(_ptr(x), dt, m, c, _ptr(rec), _ptr(ws), nbytes, _stream()), "gd_channel_moments")
    return rec


def scale_from_moments_host(rec):
    """sklearn's (mean_, var_, scale_) as fp64 numpy arrays from a (C, 3) HOST array of records (plain C++, no GPU)"""
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    if rec.ndim != 2 or rec.shape[1] != 3:
        raise L.GandanetError(f"scale_from_moments_host: expected (C, 3) records, got {rec.shape}")
    c = rec.shape[0]
    dp = C.POINTER(C.c_double)
    mean, var, scale = np.empty(c), np.empty(c), np.empty(c)
    L.check(lib().gd_scale_from_moments_host(rec.ctypes.data_as(dp), c, mean.ctypes.data_as(dp), var.ctypes.data_as(dp),
                                             scale.ctypes.data_as(dp)), "gd_scale_from_moments_host")
    return mean, var, scale


def channel_affine(src: Tensor, mean: Tensor, scale: Tensor, inverse: bool = False, out_dtype=None, to_nchw: bool = False) -> Tensor:
    """``(src - mean[c]) / scale[c]`` or, with ``inverse``, ``src * scale[c] + mean[c]`` over the last axis of the dense
    ``src`` (``mean``, ``scale``: C fp64 device values); with ``to_nchw`` a 4-D (N, H, W, C) input comes out as a dense
    (N, C, H, W) tensor.  A new tensor of ``out_dtype`` (default: the dtype of ``src``)."""
    sdt = _filter_dtype(src, "channel_affine input")
    out_dtype = _out_dtype(out_dtype, src, "channel_affine")
    _chk(mean, "channel_affine mean", torch.float64)
    _chk(scale, "channel_affine scale", torch.float64)
    c = mean.numel()
    if scale.numel() != c or not mean.is_contiguous() or not scale.is_contiguous():
        raise L.GandanetError("channel_affine: mean and scale must be dense and of one length")
    if c == 0 or src.numel() == 0 or src.numel() % c:
        raise L.GandanetError(f"channel_affine: {tuple(src.shape)} is not a non-empty array of rows of {c} channels")
    m = src.numel() // c
    n = hw = 0
    shape = src.shape
    if to_nchw:
        if src.dim() != 4 or src.shape[3] != c:
            raise L.GandanetError(f"channel_affine: to_nchw needs an (N, H, W, {c}) tensor, got {tuple(src.shape)}")
        n, hw = src.shape[0], src.shape[1] * src.shape[2]
        shape = (src.shape[0], c, src.shape[1], src.shape[2])
    dst = torch.empty(shape, device=src.device, dtype=out_dtype)
    L.check(lib().gd_channel_affine(_ptr(src), sdt, _ptr(dst), int(out_dtype == torch.float64), m, c, _ptr(mean), _ptr(scale),
                                    int(bool(inverse)), n, hw, _stream()), "gd_channel_affine")
    return dst


def freq_cos_table_host(n: int, k1: int):
    """the (k1, n) fp64 numpy table cos(2 pi ((k t) mod n) / n) / n (plain C++ on the host, no GPU)"""
    if n <= 0 or k1 < 1:
        raise L.GandanetError(f"freq_cos_table_host: L = {n}, K1 = {k1}")
    coef = np.empty((k1, n))
    L.check(lib().gd_freq_cos_table_host(int(n), int(k1), coef.ctypes.data_as(C.POINTER(C.c_double))), "gd_freq_cos_table_host")
    return coef


def freq_augment_axis(src: Tensor, dst: Tensor, axis: int, noise: Tensor, coef: Tensor) -> Tensor:
    """``dst`` = ``src`` + the cosine sum of ``noise`` (the shape of src with K1 entries along ``axis``, fp64) weighted by
    ``coef`` (K1, L) fp64 along ``axis``; ``dst`` may be a dense slab of a larger buffer.  No host sync."""
    dt = _filter_dtype(src, "freq_augment src")
    if _filter_dtype(dst, "freq_augment dst") != dt or dst.shape != src.shape:
        raise L.GandanetError(f"freq_augment_axis: src {tuple(src.shape)} {src.dtype} vs dst {tuple(dst.shape)} {dst.dtype}")
    _chk(noise, "freq_augment noise", torch.float64)
    _chk(coef, "freq_augment table", torch.float64)
    outer, n, inner = _axis_view(src, axis)
    k1 = coef.shape[0] if coef.dim() == 2 else -1
    want = tuple(src.shape[:axis]) + (k1,) + tuple(src.shape[axis + 1:])
    if k1 < 1 or coef.shape[1] != n or not coef.is_contiguous() or tuple(noise.shape) != want or not noise.is_contiguous():
        raise L.GandanetError(f"freq_augment_axis: table {tuple(coef.shape)} / noise {tuple(noise.shape)} for src "
                              f"{tuple(src.shape)} along axis {axis}")
    L.check(lib().gd_freq_augment_axis(_ptr(src), _ptr(dst), dt, outer, n, inner, _ptr(noise), k1, _ptr(coef), _stream()),
            "gd_freq_augment_axis")
    return dst


# ---- basin analysis (include/gandanet.h, "Basin analysis"; basins.hip) -------------------------------------------------------
def _zone_edges_host(edges, offsets):
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if edges.ndim != 2 or edges.shape[1] != 4 or offsets.ndim != 1 or offsets.size < 2:
        raise L.GandanetError(f"zone edges: expected (E, 4) edges and Z + 1 offsets, got {edges.shape} and {offsets.shape}")
    return edges, offsets


def zone_rasterize(edges: Tensor, offsets, xs: Tensor, ys: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """(H, W) uint32 words, bit z set where the grid point (xs[j], ys[i]) lies in zone z: ``edges`` (E, 4) fp64 on the
    device, ``offsets`` Z + 1 host integers (1 <= Z <= 32), ``xs`` (W) and ``ys`` (H) fp64 on the device.  Every word of
    ``out`` is written.  No host sync."""
    for t, nm in ((edges, "zone edges"), (xs, "zone grid xs"), (ys, "zone grid ys")):
        _dense(t, nm, torch.float64)
    if edges.dim() != 2 or edges.shape[1] != 4 or xs.dim() != 1 or ys.dim() != 1:
        raise L.GandanetError(f"zone_rasterize: edges {tuple(edges.shape)}, xs {tuple(xs.shape)}, ys {tuple(ys.shape)}")
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    h, w = ys.numel(), xs.numel()
    if out is None:
        out = torch.empty(h, w, device=xs.device, dtype=torch.uint32)
    _chk(out, "zone bits", torch.uint32)
    if tuple(out.shape) != (h, w) or not out.is_contiguous():
        raise L.GandanetError(f"zone bits: expected a dense ({h}, {w}) tensor, got {tuple(out.shape)}")
    L.check(lib().gd_zone_rasterize(_ptr(edges), edges.shape[0], off.ctypes.data_as(C.POINTER(C.c_long)), off.size - 1, _ptr(xs), w,
                                    _ptr(ys), h, _ptr(out), _stream()), "gd_zone_rasterize")
    return out


def zone_rasterize_host(edges, offsets, xs, ys):
    """``zone_rasterize`` on HOST arrays (plain C++ loops over the same predicate, no GPU): an (H, W) uint32 numpy array"""
    edges, off = _zone_edges_host(edges, offsets)
    xs = np.ascontiguousarray(xs, dtype=np.float64).reshape(-1)
    ys = np.ascontiguousarray(ys, dtype=np.float64).reshape(-1)
    out = np.empty((ys.size, xs.size), dtype=np.uint32)
    dp = C.POINTER(C.c_double)
    L.check(lib().gd_zone_rasterize_host(edges.ctypes.data_as(dp), edges.shape[0], off.ctypes.data_as(C.POINTER(C.c_long)),
                                         off.size - 1, xs.ctypes.data_as(dp), xs.size, ys.ctypes.data_as(dp), ys.size,
                                         out.ctypes.data_as(C.POINTER(C.c_uint32))), "gd_zone_rasterize_host")
    return out


def zone_mean(x: Tensor, bits: Tensor, zones: int, weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """means of ``x`` over ``zones`` (<= 32) zones at once: ``bits`` (uint32, bit z = zone z) covers the trailing dims of
    the dense fp32 / fp64 ``x`` and is shared by all leading planes; a pixel counts for zone z iff its bit is set and its
    value is not NaN; ``weights`` (fp64, the shape of ``bits``) or None = 1.  Returns (mean fp64, count int64), both shaped
    like the leading dims of ``x`` followed by ``zones``; a zone without a contributing pixel gives NaN and 0."""
    dt = _filter_dtype(x, "zone_mean input")
    _chk(bits, "zone bits", torch.uint32)
    hw = bits.numel()
    nd = x.dim() - bits.dim()
    if hw == 0 or nd < 0 or tuple(x.shape[nd:]) != tuple(bits.shape) or not bits.is_contiguous():
        raise L.GandanetError(f"zone_mean: bits {tuple(bits.shape)} do not cover the trailing dims of {tuple(x.shape)}")
    if weights is not None:
        _chk(weights, "zone weights", torch.float64)
        if weights.shape != bits.shape or not weights.is_contiguous():
            raise L.GandanetError(f"zone_mean: weights {tuple(weights.shape)} vs bits {tuple(bits.shape)}")
    z = int(zones)
    if not 1 <= z <= L.ZONE_MAX:
        raise L.GandanetError(f"zone_mean: {z} zones, expected 1..{L.ZONE_MAX}")
    lead = tuple(x.shape[:nd])
    planes = math.prod(lead)
    if planes == 0:
        raise L.GandanetError("zone_mean: empty tensor")
    mean = torch.empty(lead + (z,), device=x.device, dtype=torch.float64)
    count = torch.empty(lead + (z,), device=x.device, dtype=torch.int64)
    for lo, k in _plane_chunks(planes):
        nbytes = int(lib().gd_zone_mean_ws_bytes(k, hw, z))
        ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
        L.check(lib().gd_zone_mean(x.data_ptr() + x.element_size() * lo * hw, dt, k, hw, _ptr(bits), z, _ptr(weights), mean.data_ptr() + 8 * lo * z,
                                   count.data_ptr() + 8 * lo * z, _ptr(ws), nbytes, _stream()), "gd_zone_mean")
    return mean, count


# ---- the two argument backends of the analysis wrappers below (stl .. bias correction) -----------------------------------------
# Every wrapper below that has a host twin is written once, over one of these: _DEV for GPU tensors (enqueues on torch's
# current stream) and _HOST for numpy arrays (calls the gd_*_host twin, plain C++).  The device side refuses what is not a
# dense GPU tensor; the host side converts lists and strided arrays first.  Where a twin has never made a check that the
# other makes, the body says so with ``be.host``.
class _Dev:
    host = False
    f32, f64, u8, i32 = torch.float32, torch.float64, torch.uint8, torch.int32
    tags = {torch.float32: L.FILTER_F32, torch.float64: L.FILTER_F64, torch.uint8: L.CCL_U8}

    @staticmethod
    def array(x, name: str, ndim: Optional[int] = None, u8: bool = False):
        """(x, dtype tag) of the main array: a dense, non-empty fp32 / fp64 (``u8``: or uint8) GPU tensor of ``ndim`` dims"""
        tag = _filter_dtype(x, name, u8)
        if x.numel() == 0 or (ndim is not None and x.dim() != ndim):
            raise L.GandanetError(f"{name}: expected a dense, non-empty {'' if ndim is None else f'{ndim}-D '}tensor, got {tuple(x.shape)}")
        return x, tag

    @staticmethod
    def dense(x, name: str, dtype):
        return _dense(x, name, dtype)

    @staticmethod
    def vec(x, n: Optional[int], name: str, dtype=torch.float64):
        """an optional dense device vector of ``n`` entries (any shape; None: any number) of ``dtype``"""
        if x is None:
            return None
        _dense(x, name, dtype)
        if n is not None and x.numel() != n:
            raise L.GandanetError(f"{name}: expected {n} entries, got {tuple(x.shape)}")
        return x

    @staticmethod
    def empty(shape, dtype, like):
        return torch.empty(tuple(shape), device=like.device, dtype=dtype)

    @staticmethod
    def out(out, shape, dtype, like, name: str):
        """the dense output of ``shape`` and ``dtype``: ``out`` when one is given, else a new tensor on the device of ``like``"""
        if out is None:
            return torch.empty(tuple(shape), device=like.device, dtype=dtype)
        _dense(out, name, dtype)
        if tuple(out.shape) != tuple(shape):
            raise L.GandanetError(f"{name}: expected a dense {tuple(shape)} {dtype} tensor, got {tuple(out.shape)}")
        return out

    @staticmethod
    def ws(ws, nbytes: int, like, name: str):
        """the (pointer, bytes) arguments of the dense uint8 workspace: ``ws`` when one is given (the C entry checks its size),
        else a new one of ``nbytes``"""
        if ws is None:
            ws = torch.empty(max(int(nbytes), 8), device=like.device, dtype=torch.uint8)
        return _dense(ws, name + " workspace", torch.uint8).data_ptr(), ws.numel()

    ptr = staticmethod(_ptr)

    @staticmethod
    def call(fn: str, *args) -> None:
        L.check(getattr(lib(), fn)(*args, _stream()), fn)


class _Host:
    host = True
    f32, f64, u8, i32 = np.float32, np.float64, np.uint8, np.int32
    tags = {"float32": L.FILTER_F32, "float64": L.FILTER_F64, "uint8": L.CCL_U8}

    @staticmethod
    def array(x, name: str, ndim: Optional[int] = None, u8: bool = False):
        """(x, dtype tag) of the main array: a contiguous copy unless it is one, non-empty, fp32 / fp64 (``u8``: or uint8), of
        ``ndim`` dims"""
        x = np.asarray(x)
        if x.dtype.name not in _Host.tags or (x.dtype == np.uint8 and not u8) or x.size == 0 or (ndim is not None and x.ndim != ndim):
            raise L.GandanetError(f"{name}: expected a non-empty float32 / float64{' / uint8' if u8 else ''} array"
                                  f"{'' if ndim is None else f' of {ndim} dims'}, got {x.dtype} {x.shape}")
        return np.ascontiguousarray(x), _Host.tags[x.dtype.name]

    @staticmethod
    def dense(x, name: str, dtype):
        return np.ascontiguousarray(x, dtype=dtype)

    @staticmethod
    def vec(x, n: Optional[int], name: str, dtype=np.float64):
        """an optional flat HOST vector: None, or a contiguous 1-D ``dtype`` array, of ``n`` entries where ``n`` is given"""
        if x is None:
            return None
        x = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
        if n is not None and x.size != n:
            raise L.GandanetError(f"{name}: expected {n} entries, got {x.size}")
        return x

    @staticmethod
    def empty(shape, dtype, like=None):
        return np.empty(tuple(shape), dtype=dtype)

    @staticmethod
    def out(out, shape, dtype, like, name: str):
        """a new array; the host twins that take an ``out`` write into a C-contiguous array of ``shape`` and ``dtype``"""
        if out is None:
            return np.empty(tuple(shape), dtype=dtype)
        if not isinstance(out, np.ndarray) or out.dtype != dtype or out.shape != tuple(shape) or not out.flags["C_CONTIGUOUS"]:
            raise L.GandanetError(f"{name}: expected a contiguous {tuple(shape)} {np.dtype(dtype)} array")
        return out

    @staticmethod
    def ws(ws, nbytes: int, like, name: str):
        return ()                                                      # the host twins take no workspace

    @staticmethod
    def ptr(x):
        return None if x is None else x.ctypes.data

    @staticmethod
    def call(fn: str, *args) -> None:
        L.check(getattr(lib(), fn + "_host")(*args), fn + "_host")


_DEV, _HOST = _Dev, _Host


def _which(names, table, what: str) -> int:
    """the ``which`` bit set of an iterable of map ``names`` out of ``table``"""
    which = 0
    for name in names:
        if name not in table:
            raise L.GandanetError(f"unknown {what} map {name!r}: expected one of {table}")
        which |= 1 << table.index(name)
    if which == 0:
        raise L.GandanetError(f"no {what} map selected")
    return which


def _which_names(which: int, table) -> list:
    """the names of ``table`` that the bit set ``which`` selects, in the order of ``table``"""
    return [nm for k, nm in enumerate(table) if which >> k & 1]


# ---- STL decomposition (include/gandanet.h, "STL decomposition"; stl.hip) ------------------------------------------------------
def _stl_args(p: dict):
    return [int(p[k]) for k in ("period", "seasonal", "trend", "low_pass", "seasonal_deg", "trend_deg", "low_pass_deg", "inner_iter",
                                "outer_iter")]


def _stl_decompose(be, x, p: dict, want_weights: bool = True):
    """STL of the M series of a dense fp32 / fp64 ``x`` (T, M), series m at ``x[:, m]``; ``p`` holds period, seasonal, trend,
    low_pass, the three degrees, inner_iter and outer_iter.  New tensors (trend, seasonal, resid, weights or None) shaped
    like ``x``.  No host sync."""
    x, dt = be.array(x, "stl_decompose input", 2)
    outs = [be.empty(x.shape, x.dtype, x) if k < 3 or want_weights else None for k in range(4)]
    be.call("gd_stl_decompose", be.ptr(x), dt, x.shape[0], x.shape[1], *_stl_args(p), *[be.ptr(o) for o in outs])
    return tuple(outs)


stl_decompose = functools.partial(_stl_decompose, _DEV)
stl_decompose_host = functools.partial(_stl_decompose, _HOST)   # on a HOST array: plain C++ loops over the same arithmetic, no GPU


# ---- per-pixel time series (include/gandanet.h, "Per-pixel time series"; series.hip) -----------------------------------------
def skill_which(metrics) -> int:
    """the ``which`` bit set of gd_series_skill for an iterable of map names (L.SKILL_MAPS)"""
    return _which(metrics, L.SKILL_MAPS, "skill")


def _series_stats(be, pred, truth, rec, mask, skip_nan: bool, accumulate: bool):
    pred, dt = be.array(pred, "series_stats pred", 2)
    truth, dt2 = be.array(truth, "series_stats truth", 2)
    if dt2 != dt or truth.shape != pred.shape:
        raise L.GandanetError(f"series_stats: pred {tuple(pred.shape)} {pred.dtype} vs truth {tuple(truth.shape)} {truth.dtype}")
    T, M = pred.shape
    rec = be.out(rec, (8, M), be.f64, pred, "series records")
    mask = be.vec(mask, None if be.host else M, "series_stats mask", be.u8)      # the host twin takes the length on trust
    be.call("gd_series_stats", be.ptr(pred), be.ptr(truth), dt, T, M, be.ptr(mask), L.EVAL_SKIP_NAN if skip_nan else 0, be.ptr(rec),
            int(accumulate))
    return rec


def series_stats(pred: Tensor, truth: Tensor, rec: Tensor, mask: Optional[Tensor] = None, skip_nan: bool = True,
                 accumulate: bool = False) -> Tensor:
    """the records of the M series of ``pred`` against ``truth`` (dense fp32 / fp64 (T, M), series m at ``[:, m]``) into
    ``rec`` (8, M) fp64; ``mask``: M uint8, 0 = skip the series; ``accumulate`` continues from the records in ``rec``.  No
    host sync."""
    if rec is None:
        raise L.GandanetError("series_stats: the records are an (8, M) float64 GPU tensor, got None")
    return _series_stats(_DEV, pred, truth, rec, mask, skip_nan, accumulate)


def series_stats_host(pred, truth, mask=None, skip_nan: bool = True, rec=None):
    """``series_stats`` on HOST arrays (plain C++ loops over the same arithmetic, no GPU): the (8, M) records, continued
    from a copy of ``rec`` when one is given"""
    acc = rec is not None
    return _series_stats(_HOST, pred, truth, np.array(rec, dtype=np.float64, order="C") if acc else None, mask, skip_nan, acc)


def _series_skill(be, rec, metrics, ddof: int = 0):
    """the maps named by ``metrics`` from (8, M) fp64 records, in the order of L.SKILL_MAPS: on the device a new
    (len(set(metrics)), M) fp64 tensor, on the host a dict name -> (M) array"""
    rec = be.dense(rec, "series records", be.f64)
    if not be.host and (rec.ndim != 2 or rec.shape[0] != 8 or rec.shape[1] == 0):
        raise L.GandanetError(f"series_skill: the records are (8, M) float64, got {tuple(rec.shape)}")
    which = skill_which(metrics)
    names, M = _which_names(which, L.SKILL_MAPS), rec.shape[1]
    out = be.empty((len(names), M), be.f64, rec)
    be.call("gd_series_skill", be.ptr(rec), M, int(ddof), which, be.ptr(out))
    return dict(zip(names, out)) if be.host else out


series_skill = functools.partial(_series_skill, _DEV)
series_skill_host = functools.partial(_series_skill, _HOST)


def _series_lstsq(be, x, basis, want_rss: bool = True):
    """least squares of the M series of ``x`` (dense fp32 / fp64 (T, M)) against ``basis`` (T, P) fp64, NaN samples left
    out: new fp64 tensors (coef (P, M), rss (M) or None, n (M))"""
    x, dt = be.array(x, "series_lstsq input", 2)
    T, M = x.shape
    basis = be.dense(basis, "series_lstsq basis", be.f64)
    if not be.host and (basis.ndim != 2 or basis.shape[0] != T or not 1 <= basis.shape[1] <= L.LSTSQ_MAX_P):
        raise L.GandanetError(f"series_lstsq: the basis is ({T}, P) float64 with 1 <= P <= {L.LSTSQ_MAX_P}, got {tuple(basis.shape)}")
    P = basis.shape[1]
    coef, n = be.empty((P, M), be.f64, x), be.empty((M,), be.f64, x)
    rss = be.empty((M,), be.f64, x) if want_rss else None
    be.call("gd_series_lstsq", be.ptr(x), dt, T, M, be.ptr(basis), P, be.ptr(coef), be.ptr(rss), be.ptr(n))
    return coef, rss, n


series_lstsq = functools.partial(_series_lstsq, _DEV)
series_lstsq_host = functools.partial(_series_lstsq, _HOST)


def harmonic_finalize(coef: Tensor, K: int, has_trend: bool, tau_scale: float, rss: Optional[Tensor], n: Optional[Tensor]):
    """(amp (K, M), phase (K, M), slope (M) or None, rms (M) or None) from the coefficient planes (P, M) of a fit against
    1, [tau], cos, sin, ...; all fp64, new tensors"""
    _dense(coef, "harmonic coefficients", torch.float64)
    P, M = coef.shape
    dev = coef.device
    amp = torch.empty((K, M), device=dev, dtype=torch.float64)
    phase = torch.empty((K, M), device=dev, dtype=torch.float64)
    slope = torch.empty(M, device=dev, dtype=torch.float64) if has_trend else None
    rms = torch.empty(M, device=dev, dtype=torch.float64) if rss is not None else None
    L.check(lib().gd_harmonic_finalize(_ptr(coef), P, M, int(K), int(has_trend), float(tau_scale), _ptr(rss), _ptr(n),
                                       _ptr(amp) if K else None, _ptr(phase) if K else None, _ptr(slope), _ptr(rms), _stream()),
            "gd_harmonic_finalize")
    return amp, phase, slope, rms


def _block_mean(be, x, fy: int, fx: int, weights=None, min_count: int = 1):
    """NaN-aware mean of every ``fy`` x ``fx`` block of the last two dims of the dense fp32 / fp64 ``x`` (..., H, W);
    ``weights``: (H, W) fp64 or None.  Returns (mean in the dtype of ``x``, count int32), shaped (..., H / fy, W / fx)."""
    x, dt = be.array(x, "block_mean input")
    if x.ndim < 2:
        raise L.GandanetError(f"block_mean: expected a non-empty (..., H, W) array, got {tuple(x.shape)}")
    H, W = x.shape[-2:]
    if be.host:                                 # the host twin leaves the blocks to the C entry and the weights' length to the caller
        weights = be.vec(weights, None, "block_mean weights")
    else:
        fy, fx = int(fy), int(fx)
        if fy < 1 or fx < 1 or H % fy or W % fx:
            raise L.GandanetError(f"block_mean: blocks of {fy} x {fx} do not divide ({H}, {W})")
        if weights is not None and tuple(be.dense(weights, "block_mean weights", be.f64).shape) != (H, W):
            raise L.GandanetError(f"block_mean: weights {tuple(weights.shape)} vs planes ({H}, {W})")
    shape = tuple(x.shape[:-2]) + (H // max(fy, 1), W // max(fx, 1))
    out, count = be.empty(shape, x.dtype, x), be.empty(shape, be.i32, x)
    be.call("gd_block_mean", be.ptr(x), dt, math.prod(x.shape[:-2]), H, W, int(fy), int(fx), be.ptr(weights), int(min_count), be.ptr(out),
            be.ptr(count))
    return out, count


block_mean = functools.partial(_block_mean, _DEV)
block_mean_host = functools.partial(_block_mean, _HOST)


# ---- per-pixel trend tests (include/gandanet.h, "Per-pixel trend tests"; trend.hip) ------------------------------------------
def trend_flags(sen: bool, ci: bool, continuity: bool) -> int:
    return (L.TREND_SEN if sen else 0) | (L.TREND_CI if ci else 0) | (L.TREND_CONTINUITY if continuity else 0)


def _trend_test(be, x, times, period: int = 0, mask=None, flags: int = L.TREND_CONTINUITY, zq: float = 0.0, out=None):
    """Mann-Kendall / Theil-Sen of the M series of a dense fp32 / fp64 ``x`` (T, M) at the fp64 ``times`` (T), which the
    caller of the device entry has checked to be finite and increasing (the host twin looks itself); ``period`` 0 = not
    seasonal; ``mask``: M uint8.  The planes (L.TREND_MAPS) go into ``out`` (10, M) fp64, a new tensor unless one is given;
    those that ``flags`` does not ask for are left as they are.  No host sync."""
    x, dt = be.array(x, "trend_test input", 2)
    T, M = x.shape
    times = be.vec(times, T, "trend_test times")
    if not be.host and times.ndim != 1:
        raise L.GandanetError(f"trend_test: {tuple(times.shape)} times for {T} samples")
    out = be.out(out, (len(L.TREND_MAPS), M), be.f64, x, "trend_test output")
    mask = be.vec(mask, None if be.host else M, "trend_test mask", be.u8)        # the host twin takes the length on trust
    be.call("gd_trend_test", be.ptr(x), dt, T, M, be.ptr(times), int(period), be.ptr(mask), int(flags), float(zq), be.ptr(out))
    return out


trend_test = functools.partial(_trend_test, _DEV)
trend_test_host = functools.partial(_trend_test, _HOST)   # plain C++ over the same per-pair arithmetic; sorts the stored slopes


# ---- per-pixel change points (include/gandanet.h, "Per-pixel change points"; changepoint.hip) --------------------------------
def change_point_flags(pettitt: bool, cusum: bool, step: bool, trend: bool) -> int:
    return (L.CP_PETTITT if pettitt else 0) | (L.CP_CUSUM if cusum else 0) | (L.CP_STEP if step else 0) | (L.CP_TREND if trend else 0)


def _change_point(be, x, times, mask=None, window=None, min_seg: int = 5, flags: int = 15, out=None):
    """Pettitt / CUSUM / two-segment fits of the M series of a dense fp32 / fp64 ``x`` (T, M) at the fp64 ``times`` (T), which
    the caller of the device entry has checked to be finite and increasing (the host twin looks itself); ``mask``: M uint8;
    ``window``: (2, M) int32, begin then end of every series.  The planes (L.CP_MAPS) go into ``out`` (25, M) fp64, a new
    tensor unless one is given; those of families that ``flags`` does not ask for are left as they are.  No host sync."""
    x, dt = be.array(x, "change_point input", 2)
    T, M = x.shape
    times = be.vec(times, T, "change_point times")
    if not be.host and times.ndim != 1:
        raise L.GandanetError(f"change_point: {tuple(times.shape)} times for {T} samples")
    out = be.out(out, (len(L.CP_MAPS), M), be.f64, x, "change_point output")
    mask = be.vec(mask, None if be.host else M, "change_point mask", be.u8)      # the host twin takes the length on trust
    window = be.vec(window, 2 * M, "change_point window", be.i32)
    be.call("gd_change_point", be.ptr(x), dt, T, M, be.ptr(times), be.ptr(mask), be.ptr(window), int(min_seg), int(flags), be.ptr(out))
    return out


change_point = functools.partial(_change_point, _DEV)
change_point_host = functools.partial(_change_point, _HOST)   # plain C++ over the same per-sample functions, slot by slot


# ---- ensemble verification (include/gandanet.h, "Ensemble verification"; ensverify.hip) ------------------------------------
def ens_verify_flags(f64: bool, fair: bool) -> int:
    return (L.ENSV_F64 if f64 else 0) | (L.ENSV_FAIR if fair else 0)


def _ens_members(x, is_host: bool, fn: str):
    """(M, n, member stride in elements) of a stack of members (M, ...): every member dense, a constant stride apart"""
    M = x.shape[0] if x.ndim >= 2 else 0
    if not (1 <= M <= L.ENSV_MAX_M):
        raise L.GandanetError(f"{fn}: expected (M, ...) members with 1 <= M <= {L.ENSV_MAX_M}, got shape {tuple(x.shape)}")
    dense = x[0].flags["C_CONTIGUOUS"] if is_host else x[0].is_contiguous()
    n = int(x[0].size if is_host else x[0].numel())
    if not dense or n == 0:
        raise L.GandanetError(f"{fn}: every member must be dense and non-empty")
    stride = n if M == 1 else (x.strides[0] // x.itemsize if is_host else x.stride(0))
    if M > 1 and stride < n:
        raise L.GandanetError(f"{fn}: members {stride} elements apart overlap ({n} elements each)")
    return M, n, int(stride)


# The two twins of ens_verify stay apart: the members are read in place (a strided stack is not copied), the device entry
# writes into the caller's record and maps and takes a workspace, the host twin allocates all of them.
def ens_verify(x: Tensor, truth: Tensor, rec: Tensor, mask: Optional[Tensor] = None, scale: float = 1.0, fair: bool = False,
               crps_map: Optional[Tensor] = None, err_map: Optional[Tensor] = None, spread_map: Optional[Tensor] = None,
               rank_map: Optional[Tensor] = None) -> Tensor:
    """the verification record (L.ENSV_REC fp64) of the members ``x`` (M, ...) against ``truth`` (...) written into
    ``rec`` (a dense view on the device), and the per-element maps that are given (the float ones in the input dtype,
    ``rank_map`` uint8, each dense with as many elements as ``truth``).  ``mask`` (uint8) covers the trailing dims and is
    shared by all leading planes.  No host sync."""
    if not x.is_cuda or x.dtype not in (torch.float32, torch.float64):
        raise L.GandanetError(f"ens_verify: expected float32 / float64 GPU members, got {x.dtype} on {x.device}")
    M, n, stride = _ens_members(x, False, "ens_verify")
    _dense(truth, "ens_verify truth", x.dtype)
    if truth.numel() != n:
        raise L.GandanetError(f"ens_verify: members of {n} elements against a truth of {truth.numel()}")
    _dense(rec, "ens_verify record", torch.float64)
    if rec.numel() != L.ENSV_REC:
        raise L.GandanetError(f"ens_verify: the record is {L.ENSV_REC} contiguous float64")
    hw = n if mask is None else mask.numel()
    if hw <= 0 or n % hw:
        raise L.GandanetError(f"ens_verify: a mask of {hw} entries does not tile {tuple(truth.shape)}")
    _DEV.vec(mask, hw, "ens_verify mask", torch.uint8)
    for o, nm, dt in ((crps_map, "crps_map", x.dtype), (err_map, "err_map", x.dtype), (spread_map, "spread_map", x.dtype),
                      (rank_map, "rank_map", torch.uint8)):
        _DEV.vec(o, n, "ens_verify " + nm, dt)
    nbytes = int(lib().gd_ens_verify_ws_bytes(n))
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    _DEV.call("gd_ens_verify", _ptr(x), M, stride, _ptr(truth), n // hw, hw, _ptr(mask), float(scale),
              ens_verify_flags(x.dtype == torch.float64, fair), _ptr(rec), _ptr(crps_map), _ptr(err_map), _ptr(spread_map), _ptr(rank_map),
              _ptr(ws), nbytes)
    return rec


def ens_verify_host(x, truth, mask=None, scale: float = 1.0, fair: bool = False, maps: bool = True):
    """``ens_verify`` on HOST arrays (plain C++ over the same per-element core, walking the device's grid; no GPU):
    (record, maps) with maps = dict(crps, err, spread, rank) shaped like ``truth``, or None"""
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise L.GandanetError(f"ens_verify_host: expected float32 / float64 members, got {x.dtype}")
    M, n, stride = _ens_members(x, True, "ens_verify_host")
    truth = np.ascontiguousarray(truth, dtype=x.dtype)
    if truth.size != n:
        raise L.GandanetError(f"ens_verify_host: members of {n} elements against a truth of {truth.size}")
    mask = _HOST.vec(mask, None, "ens_verify_host mask", np.uint8)
    hw = n if mask is None else mask.size
    if hw <= 0 or n % hw:
        raise L.GandanetError(f"ens_verify_host: a mask of {hw} entries does not tile {truth.shape}")
    rec = np.empty(L.ENSV_REC)
    out = {k: np.empty(truth.shape, np.uint8 if k == "rank" else x.dtype) for k in ("crps", "err", "spread", "rank")} if maps else None
    _HOST.call("gd_ens_verify", x.ctypes.data, M, stride, truth.ctypes.data, n // hw, hw, _HOST.ptr(mask), float(scale),
               ens_verify_flags(x.dtype == np.float64, fair), rec.ctypes.data, *[out[k].ctypes.data if maps else None for k in
                                                                                  ("crps", "err", "spread", "rank")])
    return rec, out


def ens_verify_merge_host(records, M: int) -> Tuple[list, dict]:
    """add (k, L.ENSV_REC) host records in the given order (plain C++ on the host, no GPU): (merged record, metrics dict).
    ``coverage`` maps the nominal levels L.ENSV_LEVELS to the observed fractions; ``rank_hist`` holds M + 1 fractions"""
    recs = np.ascontiguousarray(np.asarray(records, dtype=np.float64).reshape(-1, L.ENSV_REC))
    out, met = (C.c_double * L.ENSV_REC)(), (C.c_double * L.ENSV_METRICS)()
    ptr = recs.ctypes.data_as(C.POINTER(C.c_double)) if len(recs) else None
    L.check(lib().gd_ens_verify_merge_host(ptr, len(recs), int(M), out, met), "gd_ens_verify_merge_host")
    d = {"n": out[0], "M": int(M)}
    d.update({nm: met[k] for k, nm in enumerate(L.ENSV_METRIC_NAMES)})
    d["coverage"] = {lv: met[L.ENSV_M_COVER + k] for k, lv in enumerate(L.ENSV_LEVELS)}
    d["reliability"] = met[L.ENSV_M_RELIABILITY]
    d["tied"] = met[L.ENSV_M_TIED]
    d["rank_hist"] = [met[L.ENSV_M_HIST + b] for b in range(int(M) + 1)]
    d["rank_counts"] = [out[L.ENSV_HIST + b] for b in range(int(M) + 1)]
    d["cover_counts"] = [out[L.ENSV_COVER + k] for k in range(4)]
    return list(out), d


# ---- EOF analysis (include/gandanet.h, "EOF analysis"; eof.hip) ---------------------------------------------------------------
def _eof_series(be, x, mean, valid, weight, fn: str):
    """(x, dtype tag, mean, valid, weight) of a (T, M) array with its M fp64 means, M uint8 flags and optional M fp64 weights"""
    x, dt = be.array(x, fn + " input", 2)
    M = x.shape[1]
    return x, dt, be.vec(mean, M, fn + " mean"), be.vec(valid, M, fn + " valid", be.u8), be.vec(weight, M, fn + " weight")


def _eof_prepare(be, x, mask=None, weight=None, center: bool = True, mean=None, valid=None):
    """(mean (M) fp64, valid (M) uint8) of the M series of a dense fp32 / fp64 ``x`` (T, M); ``mask``: M uint8; ``weight``:
    M fp64; ``mean`` and ``valid`` may be dense views to write into.  No host sync."""
    x, dt = be.array(x, "eof_prepare input", 2)
    T, M = x.shape
    n = None if be.host else M                                                   # the host twin takes the lengths on trust
    mask, weight = be.vec(mask, n, "eof_prepare mask", be.u8), be.vec(weight, n, "eof_prepare weight")
    mean = be.empty((M,), be.f64, x) if mean is None else be.vec(mean, M, "eof_prepare mean")
    valid = be.empty((M,), be.u8, x) if valid is None else be.vec(valid, M, "eof_prepare valid", be.u8)
    be.call("gd_eof_prepare", be.ptr(x), dt, T, M, be.ptr(mask), be.ptr(weight), int(bool(center)), be.ptr(mean), be.ptr(valid))
    return mean, valid


eof_prepare = functools.partial(_eof_prepare, _DEV)
eof_prepare_host = functools.partial(_eof_prepare, _HOST)


def eof_gram_ws_bytes(T: int, M: int) -> int:
    return int(lib().gd_eof_gram_ws_bytes(int(T), int(M)))


def _eof_gram(be, x, mean, valid, weight=None, out=None, ws=None):
    """the (T, T) fp64 Gram matrix of the weighted anomalies of the dense fp32 / fp64 ``x`` (T, M), 2 <= T <= L.EOF_MAX_T;
    ``out`` and the uint8 workspace ``ws`` (eof_gram_ws_bytes) are allocated unless given.  On the host every entry is summed
    over m in ascending order.  No host sync."""
    x, dt, mean, valid, weight = _eof_series(be, x, mean, valid, weight, "eof_gram")
    T, M = x.shape
    out = be.empty((T, T), be.f64, x) if out is None else be.vec(out, T * T, "eof_gram output")
    be.call("gd_eof_gram", be.ptr(x), dt, T, M, be.ptr(mean), be.ptr(valid), be.ptr(weight), be.ptr(out),
            *be.ws(ws, eof_gram_ws_bytes(T, M), x, "eof_gram"))
    return out


eof_gram = functools.partial(_eof_gram, _DEV)
eof_gram_host = functools.partial(_eof_gram, _HOST)


def _eof_project(be, x, mean, valid, coef, weight=None, use_weight: bool = False, out=None):
    """(K, M) fp64 planes out[k, m] = s_m sum_t coef[t, k] (x[t, m] - mean[m]) for ``coef`` (T, K) fp64, 1 <= K <=
    L.EOF_MAX_K; ``out`` may be a dense (K, M) view to write into.  No host sync."""
    x, dt, mean, valid, weight = _eof_series(be, x, mean, valid, weight, "eof_project")
    T, M = x.shape
    coef = be.dense(coef, "eof_project coefficients", be.f64)
    if not be.host and (coef.ndim != 2 or coef.shape[0] != T or not 1 <= coef.shape[1] <= L.EOF_MAX_K):
        raise L.GandanetError(f"eof_project: the coefficients are ({T}, K) float64 with 1 <= K <= {L.EOF_MAX_K}, got {tuple(coef.shape)}")
    K = coef.shape[1]
    out = be.out(out, (K, M), be.f64, x, "eof_project output")
    be.call("gd_eof_project", be.ptr(x), dt, T, M, be.ptr(mean), be.ptr(valid), be.ptr(weight), int(bool(use_weight)), be.ptr(coef), K,
            be.ptr(out))
    return out


eof_project = functools.partial(_eof_project, _DEV)
eof_project_host = functools.partial(_eof_project, _HOST)


def _eof_reconstruct(be, eofs, pcs, mean, valid, weight=None, dtype=None, out=None):
    """(T, M) in ``dtype`` (fp32 / fp64, fp64 unless given): mean[m] + (sum_k pcs[t, k] eofs[k, m]) / sqrt(weight[m]) for
    ``eofs`` (K, M) and ``pcs`` (T, K) fp64, 1 <= K <= L.EOF_MAX_K; ``out`` may be a dense (T, M) view of ``dtype`` to write
    into.  No host sync."""
    eofs, pcs = be.dense(eofs, "eof_reconstruct eofs", be.f64), be.dense(pcs, "eof_reconstruct pcs", be.f64)
    if not be.host and (eofs.ndim != 2 or pcs.ndim != 2 or pcs.shape[1] != eofs.shape[0] or not 1 <= eofs.shape[0] <= L.EOF_MAX_K):
        raise L.GandanetError(f"eof_reconstruct: eofs (K, M) and pcs (T, K) with 1 <= K <= {L.EOF_MAX_K}, got {tuple(eofs.shape)} and "
                              f"{tuple(pcs.shape)}")
    dtype = be.f64 if dtype is None else (np.dtype(dtype) if be.host else dtype)
    if dtype not in (be.f32, be.f64):
        raise L.GandanetError(f"eof_reconstruct: the output is float32 or float64, got {dtype}")
    (K, M), T = eofs.shape, pcs.shape[0]
    n = None if be.host else M                                                   # the host twin takes the lengths on trust
    mean, valid = be.vec(mean, n, "eof_reconstruct mean"), be.vec(valid, n, "eof_reconstruct valid", be.u8)
    weight = be.vec(weight, n, "eof_reconstruct weight")
    out = be.out(out, (T, M), dtype, eofs, "eof_reconstruct output")
    be.call("gd_eof_reconstruct", be.ptr(eofs), be.ptr(pcs), be.ptr(mean), be.ptr(valid), be.ptr(weight), T, M, K, be.ptr(out),
            int(dtype == be.f64))
    return out


eof_reconstruct = functools.partial(_eof_reconstruct, _DEV)
eof_reconstruct_host = functools.partial(_eof_reconstruct, _HOST)


# ---- Spatial spectra (include/gandanet.h, "Spatial spectra"; spectra.hip) -----------------------------------------------------
def spec_twiddle_host(N: int):
    """cos and sin of 2 pi r / N, r = 0 .. N - 1, as one HOST array of 2 N doubles (octant reduction, within 1 ulp)"""
    tw = np.empty(2 * int(N))
    L.check(lib().gd_spec_twiddle_host(int(N), tw.ctypes.data), "gd_spec_twiddle_host")
    return tw


def spec_default_bins(H: int, W: int, dy: float, dx: float) -> int:
    return int(lib().gd_spec_default_bins(int(H), int(W), float(dy), float(dx)))


def spec_bins_host(H: int, W: int, dy: float, dx: float, nbins: int, kmax: float = 0.0):
    """the HOST bin table of an (H, W) grid of spacing (dy, dx): (bin (H, W // 2 + 1) int32, kcentre (nbins), count (nbins))"""
    H, W, nbins = int(H), int(W), int(nbins)
    bins = np.empty((max(H, 0), max(W, 0) // 2 + 1), dtype=np.int32)
    kc, count = np.empty(max(nbins, 0)), np.empty(max(nbins, 0), dtype=np.int64)
    L.check(lib().gd_spec_bins_host(H, W, float(dy), float(dx), nbins, float(kmax), bins.ctypes.data, kc.ctypes.data, count.ctypes.data),
            "gd_spec_bins_host")
    return bins, kc, count


def _spec_cube(be, x, mask, wy, wx, fn: str):
    """(x, dtype tag, mask, wy, wx) of a (T, H, W) cube with its optional H W uint8 mask and fp64 tapers of H and W entries"""
    x, dt = be.array(x, fn + " input", 3)
    T, H, W = x.shape
    return x, dt, be.vec(mask, H * W, fn + " mask", be.u8), be.vec(wy, H, fn + " wy"), be.vec(wx, W, fn + " wx")


def _spec_prepare(be, x, mask=None, wy=None, wx=None, detrend: str = "mean", coef=None, S=None):
    """(coef (T, 3), S (T, 2)) fp64 of the fields of a dense fp32 / fp64 ``x`` (T, H, W): the detrend coefficients
    (a, b, c) about the field's centre, and (sum of wy^2 wx^2, count) over the valid pixels.  ``mask``: H * W uint8 shared
    by all fields; ``wy`` (H), ``wx`` (W): fp64 tapers.  No host sync."""
    x, dt, mask, wy, wx = _spec_cube(be, x, mask, wy, wx, "spec_prepare")
    if detrend not in L.SPEC_DETREND:
        raise L.GandanetError(f"spec_prepare: detrend is one of {sorted(L.SPEC_DETREND)}, got {detrend!r}")
    T, H, W = x.shape
    coef, S = be.out(coef, (T, 3), be.f64, x, "spec_prepare coef"), be.out(S, (T, 2), be.f64, x, "spec_prepare S")
    be.call("gd_spec_prepare", be.ptr(x), dt, T, H, W, be.ptr(mask), be.ptr(wy), be.ptr(wx), L.SPEC_DETREND[detrend], be.ptr(coef), be.ptr(S))
    return coef, S


spec_prepare = functools.partial(_spec_prepare, _DEV)
spec_prepare_host = functools.partial(_spec_prepare, _HOST)


def spec_power_ws_bytes(T: int, H: int, W: int, nbins: int) -> int:
    return int(lib().gd_spec_power_ws_bytes(int(T), int(H), int(W), int(nbins)))


def spec_cross_ws_bytes(T: int, H: int, W: int, nbins: int) -> int:
    return int(lib().gd_spec_cross_ws_bytes(int(T), int(H), int(W), int(nbins)))


def _spec_tables(be, x, twid_h, twid_w, bins, fn: str):
    """the twiddle tables of 2 H and 2 W doubles and the (H, W // 2 + 1) int32 bin table of the cube ``x``"""
    T, H, W = x.shape
    bins = be.dense(bins, fn + " bins", be.i32)
    if not be.host and tuple(bins.shape) != (H, W // 2 + 1):                     # the host twin takes the table's shape on trust
        raise L.GandanetError(f"{fn}: the bin table is ({H}, {W // 2 + 1}) int32, got {tuple(bins.shape)}")
    return be.vec(twid_h, 2 * H, fn + " twid_h"), be.vec(twid_w, 2 * W, fn + " twid_w"), bins


def _spec_power(be, x, coef, S, twid_h, twid_w, bins, nbins: int, mask=None, wy=None, wx=None, power=None, dropped=None, p2d=None,
                ws=None):
    x, dt, mask, wy, wx = _spec_cube(be, x, mask, wy, wx, "spec_power")
    T, H, W = x.shape
    twid_h, twid_w, bins = _spec_tables(be, x, twid_h, twid_w, bins, "spec_power")
    coef, S = be.vec(coef, None if be.host else 3 * T, "spec_power coef"), be.vec(S, None if be.host else 2 * T, "spec_power S")
    nbins = int(nbins)
    power = be.out(power, (T, max(nbins, 0)), be.f64, x, "spec_power power")
    dropped = be.out(dropped, (T,), be.f64, x, "spec_power dropped")
    if p2d is not None:
        be.out(p2d, (T, H, W // 2 + 1), be.f64, x, "spec_power p2d")
    be.call("gd_spec_power", be.ptr(x), dt, T, H, W, be.ptr(mask), be.ptr(wy), be.ptr(wx), be.ptr(coef), be.ptr(S), be.ptr(twid_h),
            be.ptr(twid_w), be.ptr(bins), nbins, be.ptr(power), be.ptr(dropped), be.ptr(p2d),
            *be.ws(ws, spec_power_ws_bytes(T, H, W, nbins), x, "spec_power"))
    return power, dropped


def spec_power(x: Tensor, coef: Tensor, S: Tensor, twid_h: Tensor, twid_w: Tensor, bins: Tensor, nbins: int,
               mask: Optional[Tensor] = None, wy: Optional[Tensor] = None, wx: Optional[Tensor] = None, power: Optional[Tensor] = None,
               dropped: Optional[Tensor] = None, p2d: Optional[Tensor] = None, ws: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(power (T, nbins), dropped (T)) fp64 of the fields of a dense fp32 / fp64 ``x`` (T, H, W) from the results of
    ``spec_prepare`` and the device copies of the twiddle and bin tables; ``p2d`` (T, H, W // 2 + 1) fp64, when given,
    receives the un-binned power.  Outputs and the uint8 workspace (spec_power_ws_bytes) are allocated unless given.  No
    host sync."""
    return _spec_power(_DEV, x, coef, S, twid_h, twid_w, bins, nbins, mask, wy, wx, power, dropped, p2d, ws)


def spec_power_host(x, coef, S, bins, nbins: int, mask=None, wy=None, wx=None, two_d: bool = False):
    """``spec_power`` on HOST arrays, with twiddle tables of its own: (power (T, nbins), dropped (T), p2d (T, H, W // 2 + 1)
    or None)"""
    T, H, W = _HOST.array(x, "spec_power input", 3)[0].shape
    p2d = np.empty((T, H, W // 2 + 1)) if two_d else None
    return (*_spec_power(_HOST, x, coef, S, spec_twiddle_host(H), spec_twiddle_host(W), bins, nbins, mask, wy, wx, p2d=p2d), p2d)


def _spec_cross(be, xa, xb, coef_a, S_a, coef_b, S_b, twid_h, twid_w, bins, nbins: int, mask=None, wy=None, wx=None, out=None,
                dropped=None, ws=None):
    xa, dt, mask, wy, wx = _spec_cube(be, xa, mask, wy, wx, "spec_cross")
    xb, dtb = be.array(xb, "spec_cross input b", 3)
    if dtb != dt or xa.shape != xb.shape:
        raise L.GandanetError(f"spec_cross: a {tuple(xa.shape)} {xa.dtype} vs b {tuple(xb.shape)} {xb.dtype}")
    T, H, W = xa.shape
    twid_h, twid_w, bins = _spec_tables(be, xa, twid_h, twid_w, bins, "spec_cross")
    coef_a, coef_b = (be.vec(c, None if be.host else 3 * T, "spec_cross coef") for c in (coef_a, coef_b))
    S_a, S_b = (be.vec(s, None if be.host else 2 * T, "spec_cross S") for s in (S_a, S_b))
    nbins = int(nbins)
    out = be.out(out, (4, T, max(nbins, 0)), be.f64, xa, "spec_cross out")
    dropped = be.out(dropped, (T, 4), be.f64, xa, "spec_cross dropped")
    be.call("gd_spec_cross", be.ptr(xa), be.ptr(xb), dt, T, H, W, be.ptr(mask), be.ptr(wy), be.ptr(wx), be.ptr(coef_a), be.ptr(S_a),
            be.ptr(coef_b), be.ptr(S_b), be.ptr(twid_h), be.ptr(twid_w), be.ptr(bins), nbins, be.ptr(out), be.ptr(dropped),
            *be.ws(ws, spec_cross_ws_bytes(T, H, W, nbins), xa, "spec_cross"))
    return out, dropped


spec_cross = functools.partial(_spec_cross, _DEV)   # (out (4, T, nbins), dropped (T, 4)) fp64: the bin sums of P_aa, P_bb, co and quad


def spec_cross_host(xa, xb, coef_a, S_a, coef_b, S_b, bins, nbins: int, mask=None, wy=None, wx=None):
    """``spec_cross`` on HOST arrays, with twiddle tables of its own: (out (4, T, nbins), dropped (T, 4))"""
    T, H, W = _HOST.array(xa, "spec_cross input", 3)[0].shape
    return _spec_cross(_HOST, xa, xb, coef_a, S_a, coef_b, S_b, spec_twiddle_host(H), spec_twiddle_host(W), bins, nbins, mask, wy, wx)


# ---- drought analysis (include/gandanet.h, "Drought analysis"; drought.hip) --------------------------------------------------
def drought_which(maps) -> int:
    """the ``which`` bit set of gd_drought_events for an iterable of map names (L.DROUGHT_EV_MAPS)"""
    return _which(maps, L.DROUGHT_EV_MAPS, "drought event")


def _drought_series(be, x, mask, fn: str):
    """(x, dtype tag, mask) of a (T, M) array with its optional M uint8 mask"""
    x, dt = be.array(x, fn + " input", 2)
    return x, dt, be.vec(mask, x.shape[1], fn + " mask", be.u8)


def _drought_clim(be, x, period: int = 12, phase: int = 0, b0: int = 0, b1: Optional[int] = None, mask=None, out=None):
    """the (3, period, M) fp64 record (n, mean, M2 per slot) of the M series of a dense fp32 / fp64 ``x`` (T, M) over the
    baseline steps [b0, b1); ``mask``: M uint8.  A new tensor unless ``out`` is given.  No host sync."""
    x, dt, mask = _drought_series(be, x, mask, "drought_clim")
    T, M = x.shape
    out = be.out(out, (3, max(int(period), 0), M), be.f64, x, "drought climatology")
    be.call("gd_drought_clim", be.ptr(x), dt, T, M, int(period), int(phase), int(b0), int(T if b1 is None else b1), be.ptr(mask), be.ptr(out))
    return out


drought_clim = functools.partial(_drought_clim, _DEV)
drought_clim_host = functools.partial(_drought_clim, _HOST)


def _drought_index(be, x, clim, phase: int = 0, kind: int = L.DROUGHT_STANDARDIZED, ddof: int = 0, mask=None, out=None):
    """the anomaly or standardised index of a dense fp32 / fp64 ``x`` (T, M) against ``clim`` (3, period, M) fp64, in the
    dtype of ``x``"""
    x, dt, mask = _drought_series(be, x, mask, "drought_index")
    T, M = x.shape
    clim = be.dense(clim, "drought climatology", be.f64)
    if clim.ndim != 3 or clim.shape[0] != 3 or clim.shape[2] != M:
        raise L.GandanetError(f"drought_index: the climatology is (3, period, {M}) float64, got {tuple(clim.shape)}")
    out = be.out(out, (T, M), x.dtype, x, "drought index")
    be.call("gd_drought_index", be.ptr(x), dt, T, M, be.ptr(clim), clim.shape[1], int(phase), int(kind), int(ddof), be.ptr(mask), be.ptr(out))
    return out


drought_index = functools.partial(_drought_index, _DEV)
drought_index_host = functools.partial(_drought_index, _HOST)


def _drought_rank(be, x, table, period: int = 12, phase: int = 0, b0: int = 0, b1: Optional[int] = None, mask=None, out=None):
    """the rank index of a dense fp32 / fp64 ``x`` (T, M) through ``table`` (nmax, nmax) or (nmax^2) fp64, in the dtype of
    ``x``"""
    x, dt, mask = _drought_series(be, x, mask, "drought_rank")
    T, M = x.shape
    table = be.vec(table, None, "drought rank table")
    nmax = math.isqrt(math.prod(table.shape))
    if nmax * nmax != math.prod(table.shape) or nmax == 0:
        raise L.GandanetError(f"drought_rank: the table holds nmax^2 doubles, got {math.prod(table.shape)}")
    out = be.out(out, (T, M), x.dtype, x, "drought rank index")
    be.call("gd_drought_rank", be.ptr(x), dt, T, M, int(period), int(phase), int(b0), int(T if b1 is None else b1), be.ptr(mask),
            be.ptr(table), nmax, be.ptr(out))
    return out


drought_rank = functools.partial(_drought_rank, _DEV)
drought_rank_host = functools.partial(_drought_rank, _HOST)


def _drought_events(be, index, threshold: float, min_duration: int = 3, maps=L.DROUGHT_EV_MAPS, mask=None, want_steps: bool = False,
                    out=None, in_event=None):
    """(maps, in_event (T, M) uint8 or None) of a dense fp32 / fp64 ``index`` (T, M); the maps in the order of
    L.DROUGHT_EV_MAPS: on the device (len(set(maps)), M) fp64, on the host a dict name -> (M) array"""
    x, dt, mask = _drought_series(be, index, mask, "drought_events")
    T, M = x.shape
    which = drought_which(maps)
    names = _which_names(which, L.DROUGHT_EV_MAPS)
    out = be.out(out, (len(names), M), be.f64, x, "drought event maps")
    if want_steps or in_event is not None:
        in_event = be.out(in_event, (T, M), be.u8, x, "drought in_event")
    be.call("gd_drought_events", be.ptr(x), dt, T, M, float(threshold), int(min_duration), which, be.ptr(mask), be.ptr(out),
            be.ptr(in_event))
    return (dict(zip(names, out)) if be.host else out), in_event


drought_events = functools.partial(_drought_events, _DEV)
drought_events_host = functools.partial(_drought_events, _HOST)


def _drought_exceed(be, index, threshold: float, out=None):
    """1 where ``index`` <= ``threshold``, 0 where not, NaN where NaN, in the dtype of the dense fp32 / fp64 ``index``"""
    x, dt = be.array(index, "drought_exceed input")
    out = be.out(out, x.shape, x.dtype, x, "drought indicator")
    be.call("gd_drought_exceed", be.ptr(x), dt, math.prod(x.shape), float(threshold), be.ptr(out))
    return out


drought_exceed = functools.partial(_drought_exceed, _DEV)
drought_exceed_host = functools.partial(_drought_exceed, _HOST)


# ---- connected components (include/gandanet.h, "Connected components"; ccl.hip) ------------------------------------------------
def _ccl_ints(be, t, shape, name: str):
    """a dense int32 array; the device side holds it to ``shape`` where one is given, the host twins take the shape on trust"""
    t = be.dense(t, name, be.i32)
    if shape is not None and not be.host and tuple(t.shape) != tuple(shape):
        raise L.GandanetError(f"{name}: expected a dense {tuple(shape)} int32 tensor, got {tuple(t.shape)}")
    return t


def _ccl_ws(be, ws, n: int, like, name: str):
    return be.ws(ws, lib().gd_ccl_ws_bytes(int(n)), like, name)


def _ccl_label(be, x, threshold: float = 0.0, structure: int = 0, mask=None, tiles: bool = True, out=None):
    """parent (T, H, W) int32 of a dense fp32 / fp64 / uint8 cube: the smallest raster index of every voxel's component, -1
    on background.  ``structure``: the 13-bit word of backward offsets; ``tiles=False`` skips the LDS tile stage.  The host
    twin is a sequential union-find over the same code."""
    x, dt = be.array(x, "ccl_label input", 3, u8=True)
    T, H, W = x.shape
    mask = be.vec(mask, H * W, "ccl_label mask", be.u8)
    out = be.out(out, (T, H, W), be.i32, x, "ccl parent")
    be.call("gd_ccl_label", be.ptr(x), dt, T, H, W, float(threshold), be.ptr(mask), int(structure), 0 if tiles else L.CCL_NO_TILES,
            be.ptr(out))
    return out


ccl_label = functools.partial(_ccl_label, _DEV)
ccl_label_host = functools.partial(_ccl_label, _HOST)


def _ccl_filter(be, parent, min_size: int, ws=None):
    """components of fewer than ``min_size`` voxels become background (-1): in place on the device, in a copy on the host"""
    parent = np.array(parent, dtype=np.int32, order="C") if be.host else _ccl_ints(be, parent, None, "ccl parent")
    n = math.prod(parent.shape)
    be.call("gd_ccl_filter", be.ptr(parent), n, int(min_size), *_ccl_ws(be, ws, n, parent, "ccl_filter"))
    return parent


ccl_filter = functools.partial(_ccl_filter, _DEV)
ccl_filter_host = functools.partial(_ccl_filter, _HOST)


def _ccl_relabel(be, parent, out=None, count=None, ws=None):
    """(labels int32 of the shape of ``parent``, count): 0 on background, 1 .. K in raster order of each component's first
    voxel; the count is a (1,) int32 tensor on the device, an int on the host.  ``out`` may be ``parent`` itself."""
    parent = _ccl_ints(be, parent, None, "ccl parent")
    n = math.prod(parent.shape)
    out = be.empty(parent.shape, be.i32, parent) if out is None else _ccl_ints(be, out, parent.shape, "ccl labels")
    count = be.empty((1,), be.i32, parent) if count is None else _ccl_ints(be, count, (1,), "ccl count")
    be.call("gd_ccl_relabel", be.ptr(parent), n, be.ptr(out), be.ptr(count), *_ccl_ws(be, ws, n, parent, "ccl_relabel"))
    return out, (int(count[0]) if be.host else count)


ccl_relabel = functools.partial(_ccl_relabel, _DEV)
ccl_relabel_host = functools.partial(_ccl_relabel, _HOST)


def _ccl_bounds(be, labels, K: int, out=None):
    """(K, 7) int32: n, t0, t1, h0, h1, w0, w1 of the labels 1 .. K of a dense (T, H, W) int32 cube"""
    labels = _ccl_ints(be, labels, None, "ccl labels")
    if labels.ndim != 3:
        raise L.GandanetError(f"ccl_bounds: expected a (T, H, W) label cube, got {tuple(labels.shape)}")
    T, H, W = labels.shape
    out = be.out(out, (max(int(K), 0), len(L.CCL_BOUNDS)), be.i32, labels, "ccl bounds")
    be.call("gd_ccl_bounds", be.ptr(labels), T, H, W, int(K), be.ptr(out))
    return out


ccl_bounds = functools.partial(_ccl_bounds, _DEV)
ccl_bounds_host = functools.partial(_ccl_bounds, _HOST)


def _ccl_offsets(be, bounds, out=None, ws=None):
    """(K + 1) int32: the exclusive prefix sum of the clusters' durations; the last entry is the number of track records"""
    bounds = _ccl_ints(be, bounds, None, "ccl bounds")
    K = bounds.shape[0]
    out = be.out(out, (K + 1,), be.i32, bounds, "ccl offsets")
    be.call("gd_ccl_offsets", be.ptr(bounds), K, be.ptr(out), *_ccl_ws(be, ws, K, bounds, "ccl_offsets"))
    return out


ccl_offsets = functools.partial(_ccl_offsets, _DEV)
ccl_offsets_host = functools.partial(_ccl_offsets, _HOST)


def _ccl_tracks(be, x, labels, bounds, offsets, R: int, threshold: float = 0.0, weights=None, severity: bool = True):
    """(tracks (R, 6) fp64, index (R, 2) int32) of the labelled clusters of the cube ``x`` (None or uint8: count and area only)"""
    labels = _ccl_ints(be, labels, None, "ccl labels")
    T, H, W = labels.shape
    dt = L.CCL_U8
    if x is not None:
        x, dt = be.array(x, "ccl_tracks input", 3, u8=True)
        if not be.host and tuple(x.shape) != (T, H, W):                          # the host twin takes the cube's shape on trust
            raise L.GandanetError(f"ccl_tracks: the cube is {tuple(x.shape)}, the labels {tuple(labels.shape)}")
    K = len(bounds)
    bounds, offsets = _ccl_ints(be, bounds, (K, len(L.CCL_BOUNDS)), "ccl bounds"), _ccl_ints(be, offsets, (K + 1,), "ccl offsets")
    weights = be.vec(weights, H * W, "ccl weights")
    tracks, index = be.empty((int(R), len(L.CCL_TRACK)), be.f64, labels), be.empty((int(R), 2), be.i32, labels)
    be.call("gd_ccl_tracks", be.ptr(x), dt, T, H, W, float(threshold), be.ptr(labels), be.ptr(bounds), be.ptr(offsets), K, int(R),
            be.ptr(weights), L.CCL_SEVERITY if severity else 0, be.ptr(tracks), be.ptr(index))
    return tracks, index


ccl_tracks = functools.partial(_ccl_tracks, _DEV)


def ccl_tracks_host(x, labels, bounds, offsets, threshold: float = 0.0, weights=None, severity: bool = True):
    """``ccl_tracks`` on HOST arrays: (tracks (R, 6), index (R, 2)), R = offsets[-1]"""
    return _ccl_tracks(_HOST, x, labels, bounds, offsets, int(np.asarray(offsets).reshape(-1)[-1]), threshold, weights, severity)


def _ccl_totals(be, tracks, bounds, offsets, out=None):
    """(K, 8) fp64: volume, severity, peak_area, peak_area_step, peak, centroid t, h, w of every cluster"""
    K = len(bounds)
    tracks = be.dense(tracks, "ccl tracks", be.f64)
    bounds, offsets = _ccl_ints(be, bounds, (K, len(L.CCL_BOUNDS)), "ccl bounds"), _ccl_ints(be, offsets, (K + 1,), "ccl offsets")
    out = be.out(out, (K, len(L.CCL_TOTALS)), be.f64, tracks, "ccl totals")
    be.call("gd_ccl_totals", be.ptr(tracks), be.ptr(bounds), be.ptr(offsets), K, be.ptr(out))
    return out


ccl_totals = functools.partial(_ccl_totals, _DEV)
ccl_totals_host = functools.partial(_ccl_totals, _HOST)


# ---- neighbourhood verification (include/gandanet.h, "Neighbourhood verification"; neighborhood.hip) ----------------------------
NBR_WS_BUDGET = 256 << 20   # bytes of tables and partials in flight when the caller gives no workspace


def _nbr_thresholds(thr, T: int, name: str):
    """the (T, K) fp64 HOST table of ``thr``: (K,) entries hold at every step"""
    a = np.asarray(thr.detach().cpu() if isinstance(thr, Tensor) else thr, dtype=np.float64)
    if a.ndim == 0:
        a = a.reshape(1)
    if a.ndim == 1:
        a = np.broadcast_to(a, (T, a.size))
    if a.ndim != 2 or a.shape[0] != T or a.shape[1] == 0:
        raise L.GandanetError(f"{name}: expected (K,) or ({T}, K) thresholds, got {a.shape}")
    return np.ascontiguousarray(a)


def _nbr_step_thresholds(thr, T: int, name: str):
    """the (T,) fp64 HOST vector of one threshold, or of one per step"""
    a = np.asarray(thr.detach().cpu() if isinstance(thr, Tensor) else thr, dtype=np.float64).reshape(-1)
    if a.size not in (1, T):
        raise L.GandanetError(f"{name}: one threshold, or one per step ({T}), got {a.size}")
    return np.ascontiguousarray(np.broadcast_to(a, (T,)))


def _nbr_scales(scales):
    seq = [scales] if isinstance(scales, (int, np.integer)) else list(scales)
    if any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n < 1 << 31 for n in seq):
        raise L.GandanetError(f"scales: expected integer window widths, got {scales!r}")
    return np.asarray(seq, dtype=np.int32).reshape(-1)


def _nbr_normalize(normalize) -> int:
    if normalize not in L.NBR_NORMALIZE:
        raise L.GandanetError(f"normalize is one of {tuple(L.NBR_NORMALIZE)}, got {normalize!r}")
    return L.NBR_NORMALIZE[normalize]


def nbr_ws_bytes(H: int, W: int, K: int, planes: int = 1) -> int:
    return int(lib().gd_nbr_ws_bytes(int(H), int(W), int(K), int(planes)))


def _nbr_ws(be, ws, like, T: int, H: int, W: int, K: int, planes: Optional[int], name: str):
    """the workspace arguments for ``planes`` steps in flight (default: NBR_WS_BUDGET bytes of them)"""
    one = nbr_ws_bytes(H, W, K, 1)
    if planes is None:
        planes = max(1, min(T, NBR_WS_BUDGET // max(one, 1)))
    return be.ws(ws, one * max(1, min(int(planes), T)), like, name)


def _nbr_fss(be, f, o, thr_f, thr_o, scales, below: bool = True, normalize: str = "window", maps: bool = False, mask=None, ws=None,
             planes: Optional[int] = None):
    """(sums (T, K, S, 3), base (T, K, 3), maps (K, S, H, W, 3) or None) of two dense fp32 / fp64 cubes (T, H, W) of one
    dtype: the unsigned 64-bit records (every value is below 2^61; int64 tensors on the device, uint64 arrays on the host), or
    fp64 ``sums`` and ``maps`` with ``normalize="valid"``.  ``thr_f``, ``thr_o``: (K,) or (T, K) thresholds on the HOST; ``scales``:
    odd widths; ``mask``: H W uint8.  ``planes`` steps in flight (default: NBR_WS_BUDGET bytes of them).  No host sync."""
    f, dt = be.array(f, "nbr_fss forecast", 3)
    o, dt2 = be.array(o, "nbr_fss observed", 3)
    if dt2 != dt or o.shape != f.shape:
        raise L.GandanetError(f"nbr_fss: forecast {tuple(f.shape)} {f.dtype} against observed {tuple(o.shape)} {o.dtype}")
    T, H, W = f.shape
    tf, to = _nbr_thresholds(thr_f, T, "nbr_fss thresholds"), _nbr_thresholds(thr_o, T, "nbr_fss observed thresholds")
    if tf.shape != to.shape:
        raise L.GandanetError(f"nbr_fss: thresholds {tf.shape} against observed thresholds {to.shape}")
    K, sc, mode = tf.shape[1], _nbr_scales(scales), _nbr_normalize(normalize)
    S, n_s = sc.size, T * K * sc.size * 3
    mask = be.vec(mask, H * W, "nbr_fss mask", be.u8)
    if be.host:
        kind = np.float64 if mode else np.uint64
        sums, base = np.empty((T, K, S, 3), dtype=kind), np.empty((T, K, 3), dtype=np.uint64)
        p_sums, p_base = sums.ctypes.data, base.ctypes.data
    else:                                                                        # one int64 buffer behind both records
        kind = torch.float64 if mode else torch.int64
        rec = torch.empty(n_s + T * K * 3, device=f.device, dtype=torch.int64)
        sums, base = rec[:n_s].view(kind).view(T, K, S, 3), rec[n_s:].view(T, K, 3)
        p_sums, p_base = rec.data_ptr(), rec.data_ptr() + 8 * n_s
    out = be.empty((K, S, H, W, 3), kind, f) if maps else None
    be.call("gd_nbr_fss", be.ptr(f), be.ptr(o), dt, T, H, W, be.ptr(mask), tf.ctypes.data, to.ctypes.data, K, int(bool(below)),
            sc.ctypes.data, S, mode, p_sums, p_base, be.ptr(out), *_nbr_ws(be, ws, f, T, H, W, K, planes, "nbr_fss"))
    return sums, base, out


nbr_fss = functools.partial(_nbr_fss, _DEV)
nbr_fss_host = functools.partial(_nbr_fss, _HOST)   # plain C++ over the same per-pixel code, in the device's order of sums


def _nbr_fraction(be, x, thr, scale: int, below: bool = True, normalize: str = "window", mask=None, out=None, ws=None,
                  planes: Optional[int] = None):
    """the (T, H, W) fp64 neighbourhood fraction of a dense fp32 / fp64 cube at the odd width ``scale``; ``thr``: one
    threshold or one per step, on the HOST"""
    x, dt = be.array(x, "nbr_fraction input", 3)
    T, H, W = x.shape
    th = _nbr_step_thresholds(thr, T, "nbr_fraction threshold")
    sc = _nbr_scales(scale)
    if not be.host and sc.size != 1:                                             # the host twin reads the first of several
        raise L.GandanetError(f"nbr_fraction: one scale, got {scale!r}")
    mask = be.vec(mask, H * W, "nbr_fraction mask", be.u8)
    out = be.out(out, (T, H, W), be.f64, x, "neighbourhood fraction")
    be.call("gd_nbr_fraction", be.ptr(x), dt, T, H, W, be.ptr(mask), th.ctypes.data, int(bool(below)), int(sc[0]), _nbr_normalize(normalize),
            be.ptr(out), *_nbr_ws(be, ws, x, T, H, W, 1, planes, "nbr_fraction"))
    return out


nbr_fraction = functools.partial(_nbr_fraction, _DEV)
nbr_fraction_host = functools.partial(_nbr_fraction, _HOST)


# ---- bias correction (include/gandanet.h, "Bias correction"; quantmap.hip) -----------------------------------------------------
def qm_probs(q, fn: str, qmin: int = 1):
    """the probabilities ``q`` (a number or a sequence, on the host) as a float64 numpy vector of ``qmin`` .. QM_MAX_Q entries
    in [0, 1]"""
    try:
        qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    except (TypeError, ValueError):
        raise L.GandanetError(f"{fn}: q is a sequence of numbers held on the host, got {type(q).__name__}") from None
    if qa.ndim != 1 or not qmin <= qa.size <= L.QM_MAX_Q:
        raise L.GandanetError(f"{fn}: q holds {qmin} .. {L.QM_MAX_Q} probabilities, got shape {qa.shape}")
    if not bool(np.all((qa >= 0.0) & (qa <= 1.0))):
        raise L.GandanetError(f"{fn}: every probability lies in [0, 1] (none is NaN), got {qa.tolist()}")
    return np.ascontiguousarray(qa)


def qm_nodes(n_quantiles: int):
    """the node probabilities j / (Q - 1) of a quantile map of Q = ``n_quantiles`` nodes, a float64 numpy vector"""
    if isinstance(n_quantiles, bool) or not isinstance(n_quantiles, (int, np.integer)) or not 2 <= n_quantiles <= L.QM_MAX_Q:
        raise L.GandanetError(f"quantile map: 2 <= n_quantiles <= {L.QM_MAX_Q}, got {n_quantiles!r}")
    return np.arange(int(n_quantiles), dtype=np.float64) / float(int(n_quantiles) - 1)


def _qm_calendar(fn: str, T: int, period, phase, b0, b1, min_samples) -> None:
    """the limits of gd_qm_quantiles, each with a message of its own"""
    if T > L.QM_MAX_T:
        raise L.GandanetError(f"{fn}: T <= {L.QM_MAX_T}, got T = {T}")
    if not 1 <= period <= L.QM_MAX_PERIOD:
        raise L.GandanetError(f"{fn}: 1 <= period <= {L.QM_MAX_PERIOD}, got {period}")
    if not 0 <= phase < period:
        raise L.GandanetError(f"{fn}: 0 <= phase < period, got phase = {phase}, period = {period}")
    if not 0 <= b0 < b1 <= T:
        raise L.GandanetError(f"{fn}: the baseline is a half-open step range inside [0, {T}], got [{b0}, {b1})")
    if -(-(b1 - b0) // period) > L.QM_MAX_N:
        raise L.GandanetError(f"{fn}: at most {L.QM_MAX_N} baseline steps per slot, got {-(-(b1 - b0) // period)}")
    if min_samples < 0:
        raise L.GandanetError(f"{fn}: min_samples >= 0, got {min_samples}")


def _qm_route(route) -> int:
    if route not in L.QM_ROUTES:
        raise L.GandanetError(f"quantile route: expected one of {tuple(L.QM_ROUTES)}, got {route!r}")
    return L.QM_ROUTES[route]


def _qm_quantiles(be, x, q, period: int = 1, phase: int = 0, b0: int = 0, b1: Optional[int] = None, mask=None, x2=None,
                  min_samples: int = 1, layout: int = L.QM_LAYOUT_QSM, _route: str = "auto"):
    """(nodes, n) of the M series of a dense fp32 / fp64 ``x`` (T, M): the quantiles at the probabilities ``q`` (a host
    sequence, checked here on the device side and by the C entry on the host side, or an fp64 device vector the caller vouches
    for) of every calendar slot's baseline sample, fp64, (Q, period, M) (QM_LAYOUT_QSM) or (period, Q, M) (QM_LAYOUT_SQM), and
    the sample sizes (period, M) int32.  ``x2``: a second cube of the shape and dtype of ``x`` whose NaNs leave a step out as
    well.  ``_route`` ("auto", "small", "long") forces one of the two sort kernels (for the tests: both give the same bits).
    New tensors.  No host sync beyond the upload of a host ``q``."""
    x, dt = be.array(x, "qm_quantiles input", 2)
    T, M = x.shape
    period, phase, b0, b1, min_samples = int(period), int(phase), int(b0), int(T if b1 is None else b1), int(min_samples)
    if x2 is not None:
        x2, dt2 = be.array(x2, "qm_quantiles second cube", 2)
        if dt2 != dt or x2.shape != x.shape:
            raise L.GandanetError(f"qm_quantiles: the second cube is {tuple(x.shape)} {x.dtype} like the first, got {tuple(x2.shape)} {x2.dtype}")
    route = _qm_route(_route)
    if be.host:                                 # the host twin leaves q, the calendar, the layout and the route's limit to the C entry
        qd = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
    else:
        _qm_calendar("qm_quantiles", T, period, phase, b0, b1, min_samples)
        if isinstance(q, Tensor):
            qd = _dense(q, "qm_quantiles q", torch.float64).reshape(-1)
            if not 1 <= qd.numel() <= L.QM_MAX_Q:
                raise L.GandanetError(f"qm_quantiles: q holds 1 .. {L.QM_MAX_Q} probabilities, got {qd.numel()}")
        else:
            qd = torch.from_numpy(qm_probs(q, "qm_quantiles")).to(x.device)
        if layout not in (L.QM_LAYOUT_QSM, L.QM_LAYOUT_SQM):
            raise L.GandanetError(f"qm_quantiles: unknown layout {layout!r}")
        if route == L.QM_ROUTES["small"] and -(-(b1 - b0) // period) > L.QM_SMALL_N:
            raise L.GandanetError(f"qm_quantiles: the register route takes at most {L.QM_SMALL_N} baseline steps per slot")
    Q, slots = math.prod(qd.shape), max(period, 0)
    mask = be.vec(mask, M, "qm_quantiles mask", be.u8)
    quant = be.empty((Q, slots, M) if layout == L.QM_LAYOUT_QSM else (slots, Q, M), be.f64, x)
    n = be.empty((slots, M), be.i32, x)
    be.call("gd_qm_quantiles", be.ptr(x), be.ptr(x2), dt, T, M, be.ptr(qd), Q, period, phase, b0, b1, be.ptr(mask), min_samples, int(layout),
            route, be.ptr(quant), be.ptr(n))
    return quant, n


qm_quantiles = functools.partial(_qm_quantiles, _DEV)
qm_quantiles_host = functools.partial(_qm_quantiles, _HOST)


def _qm_tables(model_q, obs_q, fn: str, dev: bool):
    for t, nm in ((model_q, "model_q"), (obs_q, "obs_q")):
        if dev:
            _dense(t, f"{fn} {nm}", torch.float64)
        if t.ndim != 4 or tuple(t.shape) != tuple(model_q.shape):
            raise L.GandanetError(f"{fn}: model_q and obs_q are (period, Q, H, W) float64 tables of one shape, got {nm} {tuple(t.shape)}")
    period, Q, H, W = (int(v) for v in model_q.shape)
    if not 1 <= period <= L.QM_MAX_PERIOD:
        raise L.GandanetError(f"{fn}: 1 <= period <= {L.QM_MAX_PERIOD}, got {period}")
    if not 2 <= Q <= L.QM_MAX_Q:
        raise L.GandanetError(f"{fn}: 2 <= Q <= {L.QM_MAX_Q}, got {Q}")
    if H == 0 or W == 0:
        raise L.GandanetError(f"{fn}: empty table grid {(H, W)}")
    return period, Q, H, W


def _qm_factor(shape, H: int, W: int, fn: str) -> int:
    """the integer 1 <= f <= QM_MAX_F with (Hx, Wx) = (f H, f W)"""
    if len(shape) != 3 or 0 in tuple(shape):
        raise L.GandanetError(f"{fn}: expected a non-empty (T, f H, f W) cube, got {tuple(shape)}")
    f = shape[1] // H
    if f < 1 or shape[1] != f * H or shape[2] != f * W:
        raise L.GandanetError(f"{fn}: the cube's grid {tuple(shape[1:])} is not an integer multiple f of the table grid {(H, W)} on both axes")
    if f > L.QM_MAX_F:
        raise L.GandanetError(f"{fn}: f <= {L.QM_MAX_F}, got f = {f}")
    return int(f)


def _qm_codes(kind, extrapolate, phase, period, fn: str):
    if kind not in L.QM_KINDS:
        raise L.GandanetError(f"{fn}: kind is one of {tuple(L.QM_KINDS)}, got {kind!r}")
    if extrapolate not in L.QM_EXTRAPOLATE:
        raise L.GandanetError(f"{fn}: extrapolate is one of {tuple(L.QM_EXTRAPOLATE)}, got {extrapolate!r}")
    if not 0 <= phase < period:
        raise L.GandanetError(f"{fn}: 0 <= phase < period, got phase = {phase}, period = {period}")
    return L.QM_KINDS[kind], L.QM_EXTRAPOLATE[extrapolate]


def _qm_apply(be, x, model_q, obs_q, kind: str = "eqm", extrapolate: str = "constant", phase: int = 0, own_q=None, p=None, out=None):
    """the dense fp32 / fp64 cube ``x`` (T, f H, f W) mapped through the (period, Q, H, W) fp64 tables, in the dtype of ``x``;
    step t uses slot (t + ``phase``) mod period.  ``"qdm"`` takes ``own_q`` (period, Q, f H, f W), the node table of ``x``
    itself, and ``p``, the Q node probabilities."""
    x, dt = be.array(x, "qm_apply input")
    model_q, obs_q = (be.dense(t, f"qm_apply {nm}", be.f64) for t, nm in ((model_q, "model_q"), (obs_q, "obs_q")))
    period, Q, H, W = _qm_tables(model_q, obs_q, "qm_apply", False)
    f = _qm_factor(x.shape, H, W, "qm_apply")
    k, e = _qm_codes(kind, extrapolate, int(phase), period, "qm_apply")
    if k == L.QM_KINDS["qdm"]:
        if own_q is None or p is None:
            raise L.GandanetError("qm_apply: 'qdm' needs own_q, the node table of x itself, and p, the node probabilities")
        own_q = be.dense(own_q, "qm_apply own_q", be.f64)
        if tuple(own_q.shape) != (period, Q) + tuple(x.shape[1:]):
            raise L.GandanetError(f"qm_apply: own_q is {(period, Q) + tuple(x.shape[1:])}, got {tuple(own_q.shape)}")
        p = be.vec(p, Q, "qm_apply p")
    else:
        own_q = p = None
    out = be.out(out, x.shape, x.dtype, x, "qm_apply output")
    be.call("gd_qm_apply", be.ptr(x), dt, x.shape[0], H, W, f, be.ptr(model_q), be.ptr(obs_q), be.ptr(own_q), be.ptr(p), Q, period,
            int(phase), k, e, be.ptr(out))
    return out


qm_apply = functools.partial(_qm_apply, _DEV)
qm_apply_host = functools.partial(_qm_apply, _HOST)


# ---- lagged correlation (include/gandanet.h, "Lagged correlation"; lagcorr.hip) -------------------------------------------------
def _lag_range(lag_lo, lag_hi, fn: str):
    ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (lag_lo, lag_hi))
    if not ok or not -L.LAG_MAX <= lag_lo <= lag_hi <= L.LAG_MAX:
        raise L.GandanetError(f"{fn}: the lags are integers with -{L.LAG_MAX} <= lo <= hi <= {L.LAG_MAX}, got ({lag_lo!r}, {lag_hi!r})")
    return int(lag_lo), int(lag_hi)


def _lag_corr(be, a, b, lag_lo: int, lag_hi: int, min_pairs: int = 3, select: str = "abs", mask=None, curve: bool = True, best: bool = True):
    """r of ``a[t]`` against ``b[t + l]`` for l = ``lag_lo`` .. ``lag_hi`` (l > 0: b follows a) and every series of the dense
    fp32 / fp64 ``b`` (T, M); ``a`` is (T, M), or one series (T,) / (T, 1) shared by all M, of the dtype of ``b``.  ``mask``: M
    uint8, 0 = leave the series out.  New arrays (r (NL, M) fp64, n (NL, M) int32, best (4, M) fp64 in the order of
    L.LAG_PLANES); r and n are None without ``curve``, best is None without ``best``.  No host sync."""
    b, dt = be.array(b, "lag_corr b", 2)
    a, dta = be.array(a, "lag_corr a")
    T, M = b.shape
    if dta != dt or a.shape[0] != T or tuple(a.shape[1:]) not in ((), (1,), (M,)):
        raise L.GandanetError(f"lag_corr: a is ({T},), ({T}, 1) or ({T}, {M}) of the dtype of b, got {tuple(a.shape)} {a.dtype} against "
                              f"{tuple(b.shape)} {b.dtype}")
    a_M = M if a.ndim == 2 and a.shape[1] == M else 1
    lo, hi = _lag_range(lag_lo, lag_hi, "lag_corr")
    if select not in L.LAG_SELECT:
        raise L.GandanetError(f"lag_corr: select is one of {tuple(L.LAG_SELECT)}, got {select!r}")
    if not (curve or best):
        raise L.GandanetError("lag_corr: neither the curve nor the best lag is asked for")
    mask = be.vec(mask, M, "lag_corr mask", be.u8)
    nl = hi - lo + 1
    r = be.empty((nl, M), be.f64, b) if curve else None
    n = be.empty((nl, M), be.i32, b) if curve else None
    planes = be.empty((len(L.LAG_PLANES), M), be.f64, b) if best else None
    be.call("gd_lag_corr", be.ptr(a), be.ptr(b), dt, T, M, a_M, lo, hi, int(min_pairs), L.LAG_SELECT[select], be.ptr(mask), be.ptr(r),
            be.ptr(n), be.ptr(planes))
    return r, n, planes


lag_corr = functools.partial(_lag_corr, _DEV)
lag_corr_host = functools.partial(_lag_corr, _HOST)   # plain C++ over the same per-pair arithmetic, one series and lag at a time


def _series_acf(be, x, K: int, kind: str = "standard", mask=None, min_pairs: int = 3):
    """the autocorrelation at the lags 0 .. ``K`` of every series of the dense fp32 / fp64 ``x`` (T, M): new arrays (acf
    (K + 1, M) fp64, n (K + 1, M) int32, the valid pairs of each lag); ``kind`` "standard" (Box-Jenkins, c_k / c_0) or
    "pearson" (r of the overlapping parts)"""
    x, dt = be.array(x, "series_acf input", 2)
    T, M = x.shape
    _, K = _lag_range(0, K, "series_acf")
    if kind not in L.ACF_KINDS:
        raise L.GandanetError(f"series_acf: kind is one of {tuple(L.ACF_KINDS)}, got {kind!r}")
    mask = be.vec(mask, M, "series_acf mask", be.u8)
    acf, n = be.empty((K + 1, M), be.f64, x), be.empty((K + 1, M), be.i32, x)
    be.call("gd_series_acf", be.ptr(x), dt, T, M, K, L.ACF_KINDS[kind], int(min_pairs), be.ptr(mask), be.ptr(acf), be.ptr(n))
    return acf, n


series_acf = functools.partial(_series_acf, _DEV)
series_acf_host = functools.partial(_series_acf, _HOST)


def corr_signif(r: Tensor, n: Tensor, r1a: Tensor, r1b: Tensor):
    """(n_eff, z, p) of the correlations ``r`` of ``n`` pairs between series whose lag-1 autocorrelations are ``r1a`` (one value,
    or one per entry) and ``r1b``: dense fp64 GPU tensors of one size, new tensors of the shape of ``r``.  Device only."""
    _dense(r, "corr_signif r", torch.float64)
    M = r.numel()
    if M == 0:
        raise L.GandanetError("corr_signif: empty map")
    n, r1b = _Dev.vec(n, M, "corr_signif n"), _Dev.vec(r1b, M, "corr_signif r1b")
    _dense(r1a, "corr_signif r1a", torch.float64)
    if r1a.numel() not in (1, M):
        raise L.GandanetError(f"corr_signif: r1a holds 1 or {M} values, got {tuple(r1a.shape)}")
    n_eff, z, p = (torch.empty_like(r) for _ in range(3))
    _Dev.call("gd_corr_signif", _ptr(r), _ptr(n), _ptr(r1a), r1a.numel(), _ptr(r1b), M, _ptr(n_eff), _ptr(z), _ptr(p))
    return n_eff, z, p


# ---- triple collocation (include/gandanet.h, "Triple collocation"; tcol.hip) ---------------------------------------------------
def _tc_cubes(be, x, y, z, fn: str):
    x, dt = be.array(x, f"{fn} x", 2)
    cubes = [x]
    for c, nm in ((y, "y"), (z, "z")):
        c, dtc = be.array(c, f"{fn} {nm}", 2)
        if dtc != dt or tuple(c.shape) != tuple(x.shape):
            raise L.GandanetError(f"{fn}: {nm} is {tuple(x.shape)} {x.dtype} like x, got {tuple(c.shape)} {c.dtype}")
        cubes.append(c)
    T, M = x.shape
    if not be.host and not 1 <= T <= L.TC_MAX_T:
        raise L.GandanetError(f"{fn}: 1 <= T <= {L.TC_MAX_T}, got T = {T}")
    return cubes, dt, int(T), int(M)


def _tc_min_samples(min_samples, fn: str, host: bool) -> int:
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or (not host and min_samples < 3):
        raise L.GandanetError(f"{fn}: min_samples is an integer >= 3, got {min_samples!r}")
    return int(min_samples)


def _tc_estimate(be, x, y, z, min_samples: int = 10, mask=None, cov: bool = True):
    """the triple collocation of three dense fp32 / fp64 cubes (T, M) of one dtype: new arrays (stats (8, M) fp64 in the order of
    L.TC_STATS, cov (6, M) fp64 in the order of L.TC_COVS or None, n (M,) int32, flags (M,) int32, the bits of L.TC_FLAGS).
    ``mask``: M uint8, 0 = leave the series out.  No host sync."""
    (x, y, z), dt, T, M = _tc_cubes(be, x, y, z, "tc_estimate")
    min_samples = _tc_min_samples(min_samples, "tc_estimate", be.host)
    mask = be.vec(mask, M, "tc_estimate mask", be.u8)
    stats = be.empty((len(L.TC_STATS), M), be.f64, x)
    cv = be.empty((len(L.TC_COVS), M), be.f64, x) if cov else None
    n, flags = be.empty((M,), be.i32, x), be.empty((M,), be.i32, x)
    be.call("gd_tc_estimate", be.ptr(x), be.ptr(y), be.ptr(z), dt, T, M, min_samples, be.ptr(mask), be.ptr(stats), be.ptr(cv), be.ptr(n),
            be.ptr(flags))
    return stats, cv, n, flags


tc_estimate = functools.partial(_tc_estimate, _DEV)
tc_estimate_host = functools.partial(_tc_estimate, _HOST)   # plain C++ over the same per-series body


def tc_bootstrap_workspace(T: int, M: int, B: int) -> int:
    """the bytes that hold the replicates of all M pixels at once (gd_tc_bootstrap_workspace)"""
    return int(lib().gd_tc_bootstrap_workspace(int(T), int(M), int(B)))


def tc_bootstrap_min_workspace(T: int, B: int) -> int:
    """the smallest legal workspace: the index-check word and one group of pixels"""
    return 8 + int(lib().gd_tc_group(int(T))) * len(L.TC_STATS) * int(B) * 8


def _tc_bootstrap(be, x, y, z, idx, q=(0.025, 0.5, 0.975), min_samples: int = 10, mask=None, replicates: bool = False, ws=None):
    """the bootstrap of ``tc_estimate`` over the (T, B) uint16 table ``idx`` of step numbers (``collocation.bootstrap_indices``;
    a device tensor on the device side): new arrays (summary (8, 2 + Q, M) fp64: mean, std (ddof 1) and the quantiles at the
    probabilities ``q`` (a host sequence of 1 .. L.TC_MAX_Q numbers in [0, 1]) of the replicates that are not NaN, n_ok (8, M)
    int32: their number, replicates (B, 8, M) fp64 or None).  ``ws``: a uint8 device workspace of at least
    tc_bootstrap_min_workspace(T, B) bytes (default: min(tc_bootstrap_workspace(T, M, B), 256 MiB, not below the minimum)); no
    result depends on its size.  The device side waits once for the stream (the check of the index table)."""
    (x, y, z), dt, T, M = _tc_cubes(be, x, y, z, "tc_bootstrap")
    min_samples = _tc_min_samples(min_samples, "tc_bootstrap", be.host)
    if be.host:
        idx = np.ascontiguousarray(idx)
        qd = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
        if idx.dtype != np.uint16:
            raise L.GandanetError(f"tc_bootstrap: idx is a uint16 array, got {idx.dtype}")
    else:
        _dense(idx, "tc_bootstrap idx", torch.uint16)
        try:
            qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
        except (TypeError, ValueError):
            raise L.GandanetError(f"tc_bootstrap: q is a sequence of numbers held on the host, got {type(q).__name__}") from None
        if qa.ndim != 1 or not 1 <= qa.size <= L.TC_MAX_Q or not bool(np.all((qa >= 0.0) & (qa <= 1.0))):
            raise L.GandanetError(f"tc_bootstrap: q holds 1 .. {L.TC_MAX_Q} probabilities in [0, 1], got {qa.tolist()}")
        qd = torch.from_numpy(np.ascontiguousarray(qa)).to(x.device)
    if idx.ndim != 2 or idx.shape[0] != T or not (be.host or 1 <= idx.shape[1] <= L.TC_MAX_B):
        raise L.GandanetError(f"tc_bootstrap: idx is ({T}, B) with 1 <= B <= {L.TC_MAX_B}, got {tuple(idx.shape)}")
    B, Q = int(idx.shape[1]), math.prod(qd.shape)
    mask = be.vec(mask, M, "tc_bootstrap mask", be.u8)
    summary = be.empty((len(L.TC_STATS), 2 + Q, M), be.f64, x)
    n_ok = be.empty((len(L.TC_STATS), M), be.i32, x)
    rep = be.empty((B, len(L.TC_STATS), M), be.f64, x) if replicates else None
    nbytes = 0 if be.host else max(min(tc_bootstrap_workspace(T, M, B), 1 << 28), tc_bootstrap_min_workspace(T, B))
    be.call("gd_tc_bootstrap", be.ptr(x), be.ptr(y), be.ptr(z), dt, T, M, be.ptr(idx), B, min_samples, be.ptr(qd), Q, be.ptr(mask),
            be.ptr(summary), be.ptr(n_ok), be.ptr(rep), *be.ws(ws, nbytes, x, "tc_bootstrap"))
    return summary, n_ok, rep


tc_bootstrap = functools.partial(_tc_bootstrap, _DEV)
tc_bootstrap_host = functools.partial(_tc_bootstrap, _HOST)   # plain C++ over the same per-step code, one pixel at a time


# ---- singular spectrum analysis (include/gandanet.h, "Singular spectrum analysis"; ssa.hip) ------------------------------------
def _ssa_args(be, x, window, rank, method, mask, fn: str):
    x, dt = be.array(x, f"{fn} input", 2)
    T, P = x.shape
    for v, nm in ((window, "window"), (rank, "rank")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise L.GandanetError(f"{fn}: {nm} is an integer, got {v!r}")
    if method not in L.SSA_METHODS:
        raise L.GandanetError(f"{fn}: method is one of {sorted(L.SSA_METHODS)}, got {method!r}")
    mask = be.vec(mask, None if be.host else P, f"{fn} mask", be.u8)             # the host twin takes the length on trust
    return x, dt, int(T), int(P), int(window), int(rank), L.SSA_METHODS[method], mask


def _ssa_decompose(be, x, window: int, rank: int, method: str = "bk", mask=None, components: bool = False, vectors: bool = False):
    """SSA of the P complete series of a dense fp32 / fp64 ``x`` (T, P): new fp64 arrays (eig (rank, P), maps (9, P) in the order
    of L.SSA_MAPS, rc (rank, T, P) or None), and with ``vectors`` a fourth, the eigenvectors (rank, window, P).  The C entry checks the ranges of T, window and rank.  No host sync."""
    x, dt, T, P, window, rank, method, mask = _ssa_args(be, x, window, rank, method, mask, "ssa_decompose")
    eig, maps = be.empty((max(rank, 1), P), be.f64, x), be.empty((len(L.SSA_MAPS), P), be.f64, x)
    rc = be.empty((max(rank, 1), T, P), be.f64, x) if components else None
    evec = be.empty((max(rank, 1), max(window, 1), P), be.f64, x) if vectors else None
    be.call("gd_ssa_decompose", be.ptr(x), dt, T, P, window, rank, method, be.ptr(mask), be.ptr(eig), be.ptr(maps), be.ptr(rc), be.ptr(evec))
    return (eig, maps, rc, evec) if vectors else (eig, maps, rc)


ssa_decompose = functools.partial(_ssa_decompose, _DEV)
ssa_decompose_host = functools.partial(_ssa_decompose, _HOST)   # the same per-series function with one lane, plain C++


def _ssa_fill(be, x, window: int, rank: int, method: str = "bk", mask=None, tol: float = 1e-3, max_iter: int = 20, min_valid=None):
    """the SSA gap filling of the P series of a dense fp32 / fp64 ``x`` (T, P), NaN = gap: new fp64 arrays (filled (T, P),
    eig (rank, P), maps (9, P)).  ``min_valid`` defaults to 2 * window.  No host sync."""
    x, dt, T, P, window, rank, method, mask = _ssa_args(be, x, window, rank, method, mask, "ssa_fill")
    min_valid = 2 * window if min_valid is None else min_valid
    for v, nm in ((max_iter, "max_iter"), (min_valid, "min_valid")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise L.GandanetError(f"ssa_fill: {nm} is an integer, got {v!r}")
    filled = be.empty((T, P), be.f64, x)
    eig, maps = be.empty((max(rank, 1), P), be.f64, x), be.empty((len(L.SSA_MAPS), P), be.f64, x)
    be.call("gd_ssa_fill", be.ptr(x), dt, T, P, window, rank, method, be.ptr(mask), float(tol), int(max_iter), int(min_valid), be.ptr(filled),
            be.ptr(eig), be.ptr(maps))
    return filled, eig, maps


ssa_fill = functools.partial(_ssa_fill, _DEV)
ssa_fill_host = functools.partial(_ssa_fill, _HOST)


# ---- regionalisation: k-means on pixel series (include/gandanet.h, "Regionalisation"; kmeans.hip) -----------------------------
def _km_cube(be, x, cent, fn: str):
    x, dt = be.array(x, f"{fn} x", 2)
    T, M = x.shape
    cent = be.dense(cent, f"{fn} cent", be.f64)
    if cent.ndim != 2 or cent.shape[1] != T or not 1 <= cent.shape[0] <= L.KM_MAX_K or not 1 <= T <= L.KM_MAX_T:
        raise L.GandanetError(f"{fn}: cent is (K, {T}) fp64 with 1 <= K <= {L.KM_MAX_K} and T <= {L.KM_MAX_T}, got {tuple(cent.shape)}")
    return x, dt, int(T), int(M), cent, int(cent.shape[0])


def _km_assign(be, x, cent, shift=None, scale=None, mask=None, second: bool = False):
    """the nearest of the K centroids ``cent`` (K, T) fp64 for the M series of a dense fp32 / fp64 ``x`` (T, M): new arrays
    (label (M,) int32, dist (M,) fp64, label2, dist2: the second nearest with ``second``, else None).  ``shift`` / ``scale``: M
    fp64 each, the sample is (x - shift) * scale; ``mask``: M uint8, 0 = leave the series out.  A masked or non-finite series
    gets -1 / NaN.  No host sync."""
    x, dt, T, M, cent, K = _km_cube(be, x, cent, "km_assign")
    shift, scale = be.vec(shift, M, "km_assign shift", be.f64), be.vec(scale, M, "km_assign scale", be.f64)
    mask = be.vec(mask, M, "km_assign mask", be.u8)
    label, dist = be.empty((M,), be.i32, x), be.empty((M,), be.f64, x)
    label2, dist2 = (be.empty((M,), be.i32, x), be.empty((M,), be.f64, x)) if second else (None, None)
    be.call("gd_km_assign", be.ptr(x), dt, T, M, be.ptr(cent), K, be.ptr(shift), be.ptr(scale), be.ptr(mask), be.ptr(label), be.ptr(dist),
            be.ptr(label2), be.ptr(dist2))
    return label, dist, label2, dist2


km_assign = functools.partial(_km_assign, _DEV)
km_assign_host = functools.partial(_km_assign, _HOST)   # plain C++ over the same per-element code


def km_update_workspace(T: int, M: int, K: int) -> int:
    """the bytes that hold the totals and every slab of gd_km_update at once (gd_km_update_ws_bytes)"""
    return int(lib().gd_km_update_ws_bytes(int(T), int(M), int(K)))


def km_update_min_workspace(T: int, K: int) -> int:
    """the smallest legal workspace: the totals and one slab (gd_km_update_min_ws_bytes)"""
    return int(lib().gd_km_update_min_ws_bytes(int(T), int(K)))


def _km_update(be, x, label, dist, cent, w=None, shift=None, scale=None, ws=None):
    """the centroid update of ``km_assign``'s ``label`` / ``dist``: new arrays (cent (K, T) fp64: the weighted member means, the
    row of ``cent`` where a cluster has no weight; wsum (K,) fp64; count (K,) int64; within (K,) fp64, the weighted sums of
    ``dist``).  ``w``: M fp64 pixel weights.  ``ws``: a uint8 device workspace of at least km_update_min_workspace(T, K) bytes
    (default: min(km_update_workspace(T, M, K), 256 MiB)); no result depends on its size.  No host sync."""
    x, dt, T, M, cent, K = _km_cube(be, x, cent, "km_update")
    label, dist = be.vec(label, M, "km_update label", be.i32), be.vec(dist, M, "km_update dist", be.f64)
    if label is None or dist is None:
        raise L.GandanetError("km_update: label and dist are the outputs of km_assign")
    w, shift, scale = (be.vec(v, M, f"km_update {nm}", be.f64) for v, nm in ((w, "w"), (shift, "shift"), (scale, "scale")))
    out = cent.copy() if be.host else cent.clone()
    wsum, within = be.empty((K,), be.f64, x), be.empty((K,), be.f64, x)
    count = be.empty((K,), np.int64 if be.host else torch.int64, x)
    nbytes = 0 if be.host else max(min(km_update_workspace(T, M, K), 1 << 28), km_update_min_workspace(T, K))
    be.call("gd_km_update", be.ptr(x), dt, T, M, be.ptr(label), be.ptr(dist), be.ptr(w), be.ptr(shift), be.ptr(scale), K, be.ptr(out),
            be.ptr(wsum), be.ptr(count), be.ptr(within), *be.ws(ws, nbytes, x, "km_update"))
    return out, wsum, count, within


km_update = functools.partial(_km_update, _DEV)
km_update_host = functools.partial(_km_update, _HOST)   # plain C++: the same slabs, added in the same order


def _km_farthest(be, d, exclude=None):
    """the index of the largest finite entry of the fp64 map ``d`` that is not in ``exclude`` (up to L.KM_MAX_K int32 indices),
    the lowest index on a tie, -1 if there is none: a new (1,) int32 array on the side of ``d``.  No host sync."""
    d = be.vec(d, None, "km_farthest d", be.f64)
    if d is None or math.prod(d.shape) == 0:
        raise L.GandanetError("km_farthest: d is a non-empty fp64 map")
    exclude = be.vec(exclude, None, "km_farthest exclude", be.i32)
    ne = 0 if exclude is None else math.prod(exclude.shape)
    if ne > L.KM_MAX_K:
        raise L.GandanetError(f"km_farthest: at most {L.KM_MAX_K} excluded indices, got {ne}")
    index = be.empty((1,), be.i32, d)
    be.call("gd_km_farthest", be.ptr(d), math.prod(d.shape), be.ptr(exclude) if ne else None, ne, be.ptr(index))
    return index


km_farthest = functools.partial(_km_farthest, _DEV)
km_farthest_host = functools.partial(_km_farthest, _HOST)
