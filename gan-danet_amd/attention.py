"""Looking at the attention the dual-attention blocks train, on the device and without the N x N matrix.

The reference's ``PAMModule.forward`` (generator.py:113-122) holds ``attention`` as an ordinary (B, N, N) tensor; the fused
PAM kernels never form it (one image's matrix is 17 GB at a 256 x 256 tile).  The probe kernels (``gd_pam_attn_*``,
csrc/pam_probe.hip) answer the three questions one asks of it with sweeps over q and k alone:

* which pixels does this pixel attend to?              ``pam_attention_rows``: softmax rows of chosen pixels, as images
* where is attention diffuse and where is it peaked?   ``pam_attention_stats``: ``entropy`` (nats) and ``peak`` = max_j P_ij
* which locations are attended to by everyone?         ``pam_attention_stats``: ``received`` = sum_i P_ij (its mean is 1)

``operands`` says WHICH attention: ``"exact"`` is the softmax of the fp32 projections as they are; ``"as_run"`` (the
default) is the one the configured precision mode really multiplies -- in the 16-bit modes the flash kernels take
q log2 e and k rounded to bf16 (fp16 in "fp16" / "mixed"), so the probe rounds its planes the same way (``gd_round_to_16``)
and scales the logits back by ln 2; in exact operand mode the two are the same thing.

``cam_attention`` gives the other half of the dual attention, the (B, C, C) channel attention, from the kernels ``CamFn``
already runs.  Everything here runs under ``torch.no_grad()`` and stays on the device; nothing here is differentiable.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib as L
from . import kern as K
from . import ops
from .config import operand_mode
from .evaluate import _eval_mode
from .generator import CAMModule, DANetAttention, PAMModule

OPERANDS = ("as_run", "exact")


def _pam_of(m: nn.Module) -> PAMModule:
    if isinstance(m, DANetAttention):
        return m.position_attention
    if isinstance(m, PAMModule):
        return m
    raise TypeError(f"expected a PAMModule or a DANetAttention, got {type(m).__name__}")


def _probe_planes(pam: nn.Module, x: torch.Tensor, operands: str):
    """(q, k (B, r, Npad) planes, N, Npad, r, logit_scale) of ``pam`` on ``x``: the module's own query / key 1x1 convs through
    the route and precision ``ops._pam_forward`` uses, zero-padded when N is ragged, rounded as the 16-bit routes round
    them when ``operands`` resolves to that"""
    if operands not in OPERANDS:
        raise ValueError(f"operands must be one of {OPERANDS}")
    pam = _pam_of(pam)
    x = ops._c(x)
    B, Cn, H, W = x.shape
    N, r = H * W, pam.query.weight.shape[0]
    if not 1 <= r <= 63:
        raise L.GandanetError(f"the attention probe serves 1 <= r <= 63 query / key channels, this block has {r}")
    Np = ops._npad(N)
    prec = ops._prec("conv1x1")
    q = K.conv2d_fwd(x, pam.query.weight, pam.query.bias, 1, 0, prec).view(B, r, N)
    k = K.conv2d_fwd(x, pam.key.weight, pam.key.bias, 1, 0, prec).view(B, r, N)
    q, k = ops._pad_plane(q, N, Np), ops._pad_plane(k, N, Np)
    if operands == "exact" or operand_mode("pam") == "exact":
        return q, k, N, Np, r, 1.0
    f16 = ops._pam_f16()
    return K.round_to_16(q, K.LOG2E, f16, out=q), K.round_to_16(k, 1.0, f16, out=k), N, Np, r, math.log(2.0)


@torch.no_grad()
def pam_attention_stats(pam: nn.Module, x: torch.Tensor, operands: str = "as_run") -> Dict[str, torch.Tensor]:
    """Maps of the position attention P (B, N, N) of ``pam`` (a ``PAMModule``, or a ``DANetAttention`` whose
    ``position_attention`` is used) on the input ``x`` (B, C, H, W), each (B, H, W) fp32 on the device:

    ``lse``       log sum_j e^(q_i . k_j), nats
    ``entropy``   -sum_j P_ij ln P_ij, nats: 0 = one key takes everything, ln(H W) = uniform
    ``peak``      max_j P_ij
    ``received``  sum_i P_ij: the attention pixel j receives from all pixels (mean 1)

    Not differentiable."""
    q, k, N, Np, r, scale = _probe_planes(pam, x, operands)
    B, H, W = x.shape[0], x.shape[2], x.shape[3]
    out = {n: torch.empty(B, H, W, device=x.device, dtype=torch.float32) for n in ("lse", "entropy", "peak", "received")}
    K.pam_attn_stats(q, k, B, N, Np, r, out["lse"], out["entropy"], out["peak"], logit_scale=scale)
    K.pam_attn_received(q, k, out["lse"], B, N, Np, r, out["received"], logit_scale=scale)
    return out


def _point_index(points: Sequence[Tuple[int, int]], H: int, W: int, device) -> torch.Tensor:
    idx = []
    for p in points:
        row, col = int(p[0]), int(p[1])
        if not (0 <= row < H and 0 <= col < W):
            raise ValueError(f"point {(row, col)} is outside the {H} x {W} map")
        idx.append(row * W + col)
    if not 1 <= len(idx) <= 256:
        raise ValueError(f"between 1 and 256 points per call, got {len(idx)}")
    return torch.tensor(idx, dtype=torch.int32, device=device)


@torch.no_grad()
def pam_attention_rows(pam: nn.Module, x: torch.Tensor, points: Sequence[Tuple[int, int]],
                       operands: str = "as_run") -> torch.Tensor:
    """(B, S, H, W): for each of the S ``points`` (row, col) -- the same pixels in every image of the batch -- the image of
    how much that pixel attends to every pixel, softmax_j(q_point . k_j); each map sums to 1.  1 <= S <= 256.
    Not differentiable."""
    B, H, W = x.shape[0], x.shape[2], x.shape[3]
    idx = _point_index(points, H, W, x.device)
    q, k, N, Np, r, scale = _probe_planes(pam, x, operands)
    rows = torch.empty(B, idx.numel(), H, W, device=x.device, dtype=torch.float32)
    K.pam_attn_rows(q, k, idx, B, N, Np, r, rows, logit_scale=scale)
    return rows


@torch.no_grad()
def cam_attention(cam: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """(B, C, C) channel attention softmax(max(E) - E), E = X X^T (generator.py:133-136), of a ``CAMModule`` or a
    ``DANetAttention`` on the input ``x``: the fp32 Gram product and the row softmax ``CamFn`` runs (the module has no
    weights in this product).  Not differentiable."""
    if not isinstance(cam, (CAMModule, DANetAttention)):
        raise TypeError(f"expected a CAMModule or a DANetAttention, got {type(cam).__name__}")
    x = ops._c(x)
    B, Cn, H, W = x.shape
    N = H * W
    x3 = x.view(B, Cn, N)
    e = torch.empty(B, Cn, Cn, device=x.device, dtype=torch.float32)
    K.gemm_nt(B=B, M=Cn, N=Cn, kseg=1, klen=N, a=x3, a_bs=Cn * N, a_ss=0, lda=N, bm=x3, b_bs=Cn * N, b_ss=0,
              ldb=N, c=e, c_bs=Cn * Cn, ldc=Cn, precision=L.PREC_FP32)
    return K.softmax_rows(e, -1.0, out=e)   # softmax(rowmax(E) - E) == softmax(-E)


@torch.no_grad()
def attention_report(G: nn.Module, x: torch.Tensor, points: Sequence[Tuple[int, int]] = (), operands: str = "as_run",
                     input_attention: Optional[nn.Module] = None) -> Dict[str, Dict[str, torch.Tensor]]:
    """One eval-mode forward of ``G`` on ``x`` (through the gate ``input_attention`` first, if given), then the probe of
    every attention block on the input it saw: ``{module name: {lse, entropy, peak, received (B, H, W) [, rows (B, S, H, W)]
    [, channel (B, C, C)]}}`` for every ``DANetAttention`` (with ``channel``) and stand-alone ``PAMModule`` of ``G``, at that
    block's resolution.  ``points`` (row, col) are pixel coordinates in EACH block's own map, so they must fit
    the smallest one; leave them empty for the maps alone.  The modules come back in the mode they were in and
    the hooks are removed, also on error.  Not differentiable."""
    seen: Dict[str, Tuple[nn.Module, torch.Tensor]] = {}
    hooks = []

    def watch(name, mod):
        def pre(_, args):
            seen[name] = (mod, args[0].detach())
        hooks.append(mod.register_forward_pre_hook(pre))

    try:
        for name, mod in G.named_modules():
            if isinstance(mod, (DANetAttention, PAMModule)):
                watch(name, mod)
        with _eval_mode([G, input_attention]):
            G(x if input_attention is None else input_attention(x))
    finally:
        for h in hooks:
            h.remove()
    report = {}
    for name, (mod, xin) in seen.items():
        entry = pam_attention_stats(mod, xin, operands)
        if len(points):
            entry["rows"] = pam_attention_rows(mod, xin, points, operands)
        if isinstance(mod, DANetAttention):
            entry["channel"] = cam_attention(mod, xin)
        report[name] = entry
    return report
