"""The float64 reference of the flash PAM kernels (narrow, wide): position attention without the 1/sqrt(d) factor and its
closed-form gradients.  tests/test_pam_reference.py checks it against float64 autograd on the CPU."""
import torch


def reference(c, x, gamma=0.7):
    """fp64 restatement of generator.py:115-122 and its gradients on the packed operands: c holds q, k (B, N, r) and
    v, do (B, N, C) in float64, do = the gradient that reaches O (gamma * dOut); x (B, C, N) is the residual input"""
    e = c["q"] @ c["k"].transpose(1, 2)                        # (B, N, N) energies, no 1/sqrt(d)
    lse = torch.logsumexp(e, -1)
    p = torch.softmax(e, -1)
    o = p @ c["v"]                                             # (B, N, C)
    dp = c["do"] @ c["v"].transpose(1, 2)
    delta = (c["do"] * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    return dict(o=o.transpose(1, 2), out=gamma * o.transpose(1, 2) + x.double().cpu(), lse=lse,
                dq=(ds @ c["k"]).transpose(1, 2), dk=(ds.transpose(1, 2) @ c["q"]).transpose(1, 2),
                dv=(p.transpose(1, 2) @ c["do"]).transpose(1, 2))
