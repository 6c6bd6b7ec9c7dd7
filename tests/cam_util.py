"""The float64 references of the channel attention (CAM) and of the PAM product chain, in closed form (no autograd), and
the inputs on which the CAM tests run.  tests/test_cam_reference.py checks both references against float64 autograd on
the CPU; tests/test_gpu_cam.py compares the kernels with them.

Every function takes ``dtype``: float64 is the reference, float32 the CPU emulation of what exact-fp32 kernels can
reach (the margin that backs the GPU bounds)."""
import torch

from gpu_util import seeded

# the CAM shapes of tests/test_gpu_cam.py (B, C, H, W); test_cam_reference.py asserts the conditioning of each
CAM_SHAPES = [
    (2, 40, 5, 7),        # N = 35: scalar-staged Gram, HW % 4 != 0 (gather kernel in the 16-bit modes), 64-row tile with 40 rows
    (2, 33, 8, 12),       # odd C: odd ldc of the Gram, odd a_sc; one partial pixel tile of 96
    (3, 24, 16, 16),      # M <= 32 tile, B = 3
    (2, 72, 24, 20),      # N = 480: float4-staged Gram, transpose-read kernel; 128-row tile with 72 live rows
    (2, 184, 24, 20),     # the network's width: three 64-row tiles, the last with 56 rows; last k tile of 24
    (1, 200, 45, 22),     # N = 990: k-split Gram, scalar-staged, HW % 4 != 0; eight pixel tiles, the last with 94
    (2, 136, 32, 32),     # N = 1024: k-split and float4-staged; three 64-row tiles, the last with 8 rows
]
CAM_SEED = 1
# seed of the output gradient of the CAM tests.  (With seed 2 the float32 emulation of dx at (2, 184, 24, 20) came to
# 2.005e-6 relmax, 9.97x instead of 10x inside FP32_TOL; seeds 3 .. 7 give 0.9e-6 .. 1.65e-6 there.  What the emulation
# pays is the rounding of rowmax(E) - E, values near sqrt(N), to float32: half an ulp of 22 is 1e-6.)
CAM_DOUT_SEED = 3
# the (M, Ck, P) of the batched strided products of tests/test_gpu_cam.py, B = 3
GEMM_SHAPES = [(35, 35, 4), (990, 990, 23), (40, 200, 480), (184, 184, 1024), (136, 35, 96)]
GEMM_B = 3
# the (B, r, C, N) of the PAM product chain
CHAIN_SHAPES = [(2, 4, 40, 35), (1, 23, 184, 480), (1, 5, 40, 990)]


def cam_inputs(B, C, H, W, seed):
    """(B, C, N) features scaled by N^-1/4: the off-diagonal logits of E = X X^T are then ~N(0, 1) and the diagonal is
    ~sqrt(N), so the softmax is not saturated and every off-diagonal attention weight matters.  One generator for the
    whole batch: no two images share a value."""
    N = H * W
    return seeded((B, C, N), seed) * N ** -0.25


def cam_reference(x, gamma, dout, dtype=torch.float64):
    """CAM on x (B, C, N) with the gradient dout (B, C, N) of its output, every intermediate by name:
    att = softmax(rowmax(E) - E), apply = att X, y = gamma apply + X; da = dOut X^T (the gradient that reaches att, over
    gamma), dgamma = sum att . da, de = the softmax backward with sign -1 (the gradient that reaches E, over gamma),
    sym = de + de^T, dx_att = att^T dOut, dx_sym = sym X, dx = dOut + gamma (dx_att + dx_sym)"""
    x, dout = x.to(dtype), dout.to(dtype)
    e = x @ x.transpose(1, 2)
    z = e.max(-1, keepdim=True).values - e
    w = torch.exp(z - z.max(-1, keepdim=True).values)
    att = w / w.sum(-1, keepdim=True)
    apply = att @ x
    y = gamma * apply + x
    da = dout @ x.transpose(1, 2)
    terms = att * da
    dgamma = terms.sum()
    de = -att * (da - terms.sum(-1, keepdim=True))
    sym = de + de.transpose(1, 2)
    dx_att = att.transpose(1, 2) @ dout
    dx_sym = sym @ x
    return dict(e=e, att=att, apply=apply, y=y, da=da, dgamma=dgamma, dgamma_abs=terms.abs().sum(), de=de, sym=sym,
                dx_att=dx_att, dx_sym=dx_sym, dx=dout + gamma * (dx_att + dx_sym))


def chain_inputs(B, r, C, N, seed):
    """q, k (B, r, N) ~ N(0, 1) r^-1/2 (logits of O(1)), v, x, dout (B, C, N) ~ N(0, 1)"""
    q, k = seeded((B, r, N), seed, r ** -0.5), seeded((B, r, N), seed + 1, r ** -0.5)
    return q, k, seeded((B, C, N), seed + 2), seeded((B, C, N), seed + 3), seeded((B, C, N), seed + 4)


def pam_chain_reference(q, k, v, x, gamma, dout, dtype=torch.float64):
    """the PAM product chain on the projections q, k (B, r, N), v (B, C, N), channel-major as ops._pam_chain_fwd takes
    them: p = softmax(q^T k), o_attn = v p^T, out = gamma o_attn + x, and the gradients of q, k, v and gamma"""
    q, k, v, x, dout = (t.to(dtype) for t in (q, k, v, x, dout))
    s = q.transpose(1, 2) @ k                                   # (B, N, N): s[i][j] = sum_d q[d][i] k[d][j]
    w = torch.exp(s - s.max(-1, keepdim=True).values)
    p = w / w.sum(-1, keepdim=True)
    o_attn = v @ p.transpose(1, 2)                              # o[c][i] = sum_j v[c][j] p[i][j]
    terms = dout * o_attn
    do = gamma * dout
    dp = do.transpose(1, 2) @ v                                 # dp[i][j] = sum_c do[c][i] v[c][j]
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    return dict(p=p, o_attn=o_attn, out=gamma * o_attn + x, dq=k @ ds.transpose(1, 2), dk=q @ ds, dv=do @ p,
                dgamma=terms.sum(), dgamma_abs=terms.abs().sum())


def conditioning(att):
    """(the largest attention weight, the smallest exp(row entropy) / C) of att (B, C, C): 1 / C and 1 for uniform
    rows, 1 and 1 / C for one-hot rows"""
    att = att.double()
    ent = -(att * torch.log(att.clamp_min(1e-300))).sum(-1)
    return att.max().item(), (torch.exp(ent).min() / att.shape[-1]).item()


def gemm_inputs(M, Ck, P, seed, B=GEMM_B):
    """operands ~ N(0, 1) / sqrt(Ck): A row-major (B, M, Ck), X (B, Ck, P); y0 and res (B, M, P) at the product's own
    scale Ck^-1/2, so that a prefilled output and a residual neither hide the product nor are hidden by it"""
    s = Ck ** -0.5
    return dict(a=seeded((B, M, Ck), seed, s), x=seeded((B, Ck, P), seed + 1, s), y0=seeded((B, M, P), seed + 2, s),
                res=seeded((B, M, P), seed + 3, s))


def gemm_reference(a, x, dtype=torch.float64):
    return torch.einsum("bmc,bcp->bmp", a.to(dtype), x.to(dtype))
