"""The float64 reference of the batch-norm kernels (tests/norm_util.py) against torch.nn.BatchNorm2d and autograd in
float64, on the CPU: the evidence that what tests/test_gpu_norm.py compares the kernels with is right."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_util as NU

TOL = 1e-12
SHAPES = [(2, 3, 1, 5), (3, 2, 7, 9), (4, 5, 16, 16), (300, 2, 2, 2)]
ACTS = [NU.ACT_NONE, NU.ACT_RELU, NU.ACT_LEAKY02]
EPS, MOM = 1e-5, 0.1


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b.detach().numpy() if hasattr(b, "detach") else b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    err = np.abs(a - b).max() / max(1.0, np.abs(b).max())
    assert err <= TOL, f"{what}: err {err:.3e} > {TOL:.0e}"


def _torch_act(v, act):
    if act == NU.ACT_RELU:
        return F.relu(v)
    if act == NU.ACT_LEAKY02:
        return F.leaky_relu(v, 0.2)
    return v


def _case(shape, seed):
    C = shape[1]
    x = _randn(shape, seed) * 1.7 + _randn((1, C, 1, 1), seed + 1) * 3
    return (x, 1 + 0.3 * _randn((C,), seed + 2), 0.5 * _randn((C,), seed + 3), 0.2 * _randn((C,), seed + 4),
            1 + 0.5 * _randn((C,), seed + 5) ** 2, _randn(shape, seed + 6))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_matches_batchnorm2d_and_autograd(shape, train, act):
    x, gamma, beta, rm, rv, dy = _case(shape, 7 + shape[0])
    # eps and momentum as the float32 values the C ABI passes: the reference rounds them the same way
    eps, mom = NU.f32(EPS), NU.f32(MOM)
    bn = torch.nn.BatchNorm2d(shape[1], eps=eps, momentum=mom).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    bn.train(train)
    xr = x.clone().requires_grad_(True)
    yr = _torch_act(bn(xr), act)
    yr.backward(dy)

    if train:
        st = NU.channel_stats(x)
        mean, inv = st.mean, NU.invstd(st.var, EPS)
        scale, shift = NU.fold(gamma, beta, mean, inv)
        nrm, nrv = NU.running_update(rm, rv, st, MOM)
        _close(nrm, bn.running_mean, "running_mean")
        _close(nrv, bn.running_var, "running_var")
        _close(st.var, x.var(dim=(0, 2, 3), unbiased=False), "biased variance")
        _close(st.unb, x.var(dim=(0, 2, 3), unbiased=True), "unbiased variance")
        _close(st.n, np.full(shape[1], x.numel() / shape[1]), "count")
    else:
        mean = rm
        scale, shift, inv = NU.fold_eval(gamma, beta, rm, rv, EPS)
    _close(NU.affine_act(x, scale, shift, act), yr, "y")
    dg, db, dx = NU.bn_act_bwd(dy, x, scale, shift, mean, inv, act, train)
    _close(dg, bn.weight.grad, "dgamma")
    _close(db, bn.bias.grad, "dbeta")
    _close(dx, xr.grad, "dx")
    # the SyncBN form: dx from externally supplied sums and 1 / count is the same expression
    n = x.numel() / shape[1]
    _close(NU.bn_dx(dy, x, scale, shift, mean, inv, dg, db, 1.0 / n, act, train), xr.grad, "dx from sums")
    _close(NU.channel_sum(dy), dy.sum(dim=(0, 2, 3)), "channel sum")


def test_single_element_channel_uses_the_biased_variance():
    x = _randn((1, 3, 1, 1), 5)
    st = NU.channel_stats(x)
    assert (st.m2 == 0).all() and (st.var == 0).all() and (st.unb == 0).all() and (st.n == 1).all()
    rm, rv = NU.running_update(np.ones(3), np.full(3, 2.0), st, MOM)
    m = NU.f32(MOM)
    _close(rm, (1 - m) * 1.0 + m * x.reshape(3), "running_mean")
    _close(rv, np.full(3, (1 - m) * 2.0), "running_var")


@pytest.mark.parametrize("sizes", [(5,), (2, 3), (1, 7, 2), tuple(range(1, 41))])
def test_merge_of_unequal_shards_equals_the_full_batch(sizes):
    C = 4
    x = _randn((sum(sizes), C, 3, 5), 11) * 2 + _randn((1, C, 1, 1), 12) * 50
    recs, lo = [], 0
    for s in sizes:
        recs.append(NU.records(NU.channel_stats(x[lo:lo + s])))
        lo += s
    got, full = NU.merge(np.stack(recs, 0)), NU.channel_stats(x)
    for name in NU.Stats._fields:
        _close(getattr(got, name), getattr(full, name), f"merged {name}")


def test_activation_gradient_at_zero_is_the_oracles():
    """at a pre-activation of exactly zero the reference passes the gradient, as oracle.functional does under autograd"""
    from oracle import functional as OF
    for act, fn in ((NU.ACT_RELU, OF.relu), (NU.ACT_LEAKY02, OF.leaky_relu)):
        z = torch.zeros(4, dtype=torch.float64, requires_grad=True)
        dy = _randn((4,), 3)
        fn(z).backward(dy)
        _close(NU.act_grad(np.zeros(4), dy, act), z.grad, f"act {act} gradient at zero")
        _close(NU.act(np.zeros(4), act), fn(z), f"act {act} at zero")
