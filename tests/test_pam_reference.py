"""The float64 reference of the flash PAM kernels (tests/pam_util.py) against float64 autograd through
softmax(q k^T) v, on the CPU: the evidence that what tests/test_gpu_pam_narrow.py, test_gpu_pam_wide.py and
test_gpu_pam_f32.py compare the kernels with is right."""
import pytest
import torch

import pam_util as PU

TOL = 1e-12
GAMMA = 0.7


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("r,c,n", [(1, 8, 35), (23, 184, 480)])
def test_reference_matches_autograd(r, c, n):
    B = 2
    q, k = _randn((B, n, r), 1, 0.6).requires_grad_(True), _randn((B, n, r), 2, 0.6).requires_grad_(True)
    v = _randn((B, n, c), 3).requires_grad_(True)
    x, dout = _randn((B, c, n), 4), _randn((B, c, n), 5)
    e = q @ k.transpose(1, 2)
    o = torch.softmax(e, -1) @ v                               # (B, N, C)
    out = GAMMA * o.transpose(1, 2) + x
    out.backward(dout)

    # the kernels are handed the gradient that reaches O: gamma * dOut, pixel-major
    ops = dict(q=q.detach(), k=k.detach(), v=v.detach(), do=GAMMA * dout.transpose(1, 2))
    ref = PU.reference(ops, x, GAMMA)
    errs = {"out": _rel(ref["out"], out.detach()), "o": _rel(ref["o"], o.detach().transpose(1, 2)),
            "lse": _rel(ref["lse"], torch.logsumexp(e.detach(), -1)),
            "dq": _rel(ref["dq"], q.grad.transpose(1, 2)), "dk": _rel(ref["dk"], k.grad.transpose(1, 2)),
            "dv": _rel(ref["dv"], v.grad.transpose(1, 2))}
    for name, err in errs.items():
        assert err <= TOL, f"{name}: rel err {err:.3e} > {TOL:.0e}"
    assert ref["dq"].shape == (B, r, n) and ref["dk"].shape == (B, r, n) and ref["dv"].shape == (B, c, n)


def test_reference_lse_is_independent_of_the_softmax():
    """lse comes from logsumexp, the probabilities from softmax: exp(e - lse) must be those probabilities, which is how
    the backward kernels rebuild P"""
    q, k, v = _randn((2, 35, 3), 6, 2.0), _randn((2, 35, 3), 7, 2.0), _randn((2, 35, 8), 8)
    ref = PU.reference(dict(q=q, k=k, v=v, do=torch.zeros(2, 35, 8, dtype=torch.float64)), torch.zeros(2, 8, 35), GAMMA)
    e = q @ k.transpose(1, 2)
    p = torch.exp(e - ref["lse"][..., None])
    assert _rel((p @ v).transpose(1, 2), ref["o"]) <= TOL
    assert (p.sum(-1) - 1).abs().max().item() <= TOL
