"""float64 reference of csrc/norm.hip: batch statistics and their running update, the SyncBN shard merge, the train
and eval folds, y = act(x * scale + shift), the backward of act(bn(x)) and the per-channel sum.  numpy only, no GPU.

Every function widens what it is given to float64 and does nothing else in a narrower type.  A GPU test hands it the
*float32* tensors the kernel received (inputs, and the float32 scale / shift / mean / invstd the kernel would be
given), so a difference measures the kernel's arithmetic and not the rounding of its inputs.  Scalars that the C ABI
takes as ``float`` (eps, momentum, inv_n) go through ``f32`` first for the same reason.

Layout: activations are (B, C, ...) with any number of trailing plane axes; per-channel vectors are (C,).
Activations: ``ACT_NONE``, ``ACT_RELU``, ``ACT_LEAKY02`` as in gan_danet_amd._lib.  At a pre-activation of exactly
zero both relu and leaky pass the gradient (factor 1): that is what oracle.functional does (clamp_min and
where(x >= 0, ...) under autograd)."""
from collections import namedtuple

import numpy as np

ACT_NONE, ACT_RELU, ACT_LEAKY02 = 0, 1, 2
U = 2.0 ** -24            # unit roundoff of float32
CHUNK = 16384             # elements of one channel plane per workgroup (norm.hip)
SUM_TERMS = CHUNK // 256 + 16   # fp32 additions on the longest path of one chunk's sum: 64 per thread, 6 + 4 in the block
                                # tree, rounded up generously; the cross-chunk stage runs in double

Stats = namedtuple("Stats", "n mean m2 var unb")


def f64(t):
    """torch tensor / array / scalar -> float64 ndarray (a copy)"""
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.array(t, dtype=np.float64)


def f32(v):
    """the double value of ``v`` rounded to float32: what a ``float`` argument of the C ABI holds"""
    return float(np.float32(v))


def _planes(x):
    """(B, C, ...) -> (C, B * HW) float64"""
    x = f64(x)
    return np.moveaxis(x.reshape(x.shape[0], x.shape[1], -1), 1, 0).reshape(x.shape[1], -1)


def _bc(v, x):
    """(C,) -> broadcastable against (B, C, ...)"""
    return f64(v).reshape((1, -1) + (1,) * (x.ndim - 2))


# ---- statistics ----------------------------------------------------------------------------------------------------
def channel_stats(x) -> Stats:
    """per-channel count, mean, M2 = sum (x - mean)^2, biased and unbiased variance.  One element: the kernel's
    ``unb = var`` branch (there is no n - 1 to divide by)."""
    p = _planes(x)
    n = float(p.shape[1])
    mean = p.sum(1) / n
    m2 = ((p - mean[:, None]) ** 2).sum(1)
    var = m2 / n
    unb = m2 / (n - 1) if n > 1 else var.copy()
    return Stats(np.full(p.shape[0], n), mean, m2, var, unb)


def invstd(var, eps):
    return 1.0 / np.sqrt(f64(var) + f32(eps))


def running_update(running_mean, running_var, st: Stats, momentum):
    """(1 - m) * running + m * batch, the batch variance being the unbiased one"""
    m = f32(momentum)
    return (1.0 - m) * f64(running_mean) + m * st.mean, (1.0 - m) * f64(running_var) + m * st.unb


def records(st: Stats):
    """(C, 3) (count, mean, M2): what gd_bn_stats_local writes"""
    return np.stack([st.n, st.mean, st.m2], 1)


def merge(recs) -> Stats:
    """Chan merge of (world, C, 3) (count, mean, M2) records into the statistics of the union"""
    r = f64(recs)
    cnt, mu, m2 = r[..., 0], r[..., 1], r[..., 2]
    n = cnt.sum(0)
    mean = (cnt * mu).sum(0) / n
    M2 = (m2 + cnt * (mu - mean[None]) ** 2).sum(0)
    var = M2 / n
    unb = np.where(n > 1, M2 / np.maximum(n - 1, 1), var)
    return Stats(n, mean, M2, var, unb)


# ---- fold ----------------------------------------------------------------------------------------------------------
def fold(gamma, beta, mean, inv):
    """train form: scale = gamma * invstd, shift = beta - mean * scale"""
    scale = f64(gamma) * f64(inv)
    return scale, f64(beta) - f64(mean) * scale


def fold_eval(gamma, beta, running_mean, running_var, eps):
    """eval form: invstd from the running variance; returns scale, shift, invstd"""
    inv = invstd(running_var, eps)
    scale, shift = fold(gamma, beta, running_mean, inv)
    return scale, shift, inv


# ---- forward -------------------------------------------------------------------------------------------------------
def preact(x, scale, shift):
    x = f64(x)
    v = x if scale is None else x * _bc(scale, x)
    return v if shift is None else v + _bc(shift, x)


def act(v, kind):
    if kind == ACT_RELU:
        return np.maximum(v, 0.0)
    if kind == ACT_LEAKY02:
        return np.where(v >= 0, v, 0.2 * v)
    return v


def affine_act(x, scale, shift, kind):
    return act(preact(x, scale, shift), kind)


def act_grad(pre, dy, kind):
    """dy times the activation's derivative at ``pre`` (1 at exactly zero for relu and leaky, see the module text)"""
    dy = f64(dy)
    if kind == ACT_RELU:
        return np.where(pre >= 0, dy, 0.0)
    if kind == ACT_LEAKY02:
        return np.where(pre >= 0, dy, 0.2 * dy)
    return dy


# ---- backward ------------------------------------------------------------------------------------------------------
def xhat(x, mean, inv):
    x = f64(x)
    return (x - _bc(mean, x)) * _bc(inv, x)


def bn_sums(dy, x, scale, shift, mean, inv, kind):
    """g = dy * act'(x * scale + shift); returns dgamma = sum g * xhat, dbeta = sum g (per channel) and g"""
    g = act_grad(preact(x, scale, shift), dy, kind)
    return _planes(g * xhat(x, mean, inv)).sum(1), _planes(g).sum(1), g


def bn_dx(dy, x, scale, shift, mean, inv, dgamma_sum, dbeta_sum, inv_n, kind, train=True):
    """dx from given per-channel sums: scale * (g - dbeta * inv_n - xhat * dgamma * inv_n); eval: scale * g"""
    g = act_grad(preact(x, scale, shift), dy, kind)
    sc = _bc(scale, g)
    if not train:
        return sc * g
    k = float(inv_n)
    return sc * (g - _bc(dbeta_sum, g) * k - xhat(x, mean, inv) * (_bc(dgamma_sum, g) * k))


def bn_act_bwd(dy, x, scale, shift, mean, inv, kind, train):
    """dgamma, dbeta, dx of y = act(x * scale + shift), scale = gamma * invstd.  train: the batch statistics depend on
    x (mean and variance terms in dx, 1 / n the element count per channel); eval: they are constants"""
    dg, db, _ = bn_sums(dy, x, scale, shift, mean, inv, kind)
    n = _planes(x).shape[1]
    return dg, db, bn_dx(dy, x, scale, shift, mean, inv, dg, db, 1.0 / n, kind, train)


def channel_sum(x):
    return _planes(x).sum(1)


def channel_abs_sum(x):
    return np.abs(_planes(x)).sum(1)
