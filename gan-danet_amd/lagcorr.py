"""How many months does storage run behind its drivers, and what is a correlation of two autocorrelated series worth?
Lagged cross-correlation of every pixel series against a driver cube or a single index, the lag of the strongest link, the
autocorrelation of every series, and the effective sample size, Fisher z and p-value of a correlation map (also of the
``cc`` of ``skill_maps``), on the device.

Definitions (``include/gandanet.h``, "Lagged correlation"): ``r(l)`` correlates ``a[t]`` with ``b[t + l]``, so ``l > 0`` means
that ``b`` follows ``a``; only pairs with both members not NaN count, per lag (pairwise deletion); the best lag is taken over
the lags whose ``r`` is not NaN and a tie goes to the smaller ``|l|``, then to the positive lag.  ``n_eff``, ``z`` and ``p``
follow Bretherton et al. (1999) with the lag-1 autocorrelations of both series and are NOT corrected for the selection of the
best among several lags: the ``p`` of ``best_r`` is optimistic by up to the number of lags tried.  ``fdr_threshold`` controls
the false discovery rate over the pixels of a p map (Wilks 2016), not over the lags.  A seasonal cycle correlates everything
with everything: remove it first (``drought_index(kind="anomaly")``, ``stl_decompose``); that is the caller's job.

The kernels are ``csrc/lagcorr.hip`` over ``csrc/lagcorr_core.h``: fp32 or fp64 CUDA tensors, time along axis 0, T <= 2048,
lags within +-64, all arithmetic fp64, both cubes read once however many lags are asked for.  There is no CPU path in this
module (``kern.lag_corr_host`` and ``kern.series_acf_host`` are the plain C++ twins the tests use); ``fdr_threshold`` is torch
plumbing and takes tensors of any device.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import kern as K
from .timeseries import _cube, _series_mask

Tensor = torch.Tensor
L = K.L


class LagCorrelation(NamedTuple):
    lags: Tensor
    best_lag: Tensor
    best_r: Tensor
    best_n: Tensor
    r0: Tensor
    r: Optional[Tensor]
    n: Optional[Tensor]
    n_eff: Optional[Tensor]
    z: Optional[Tensor]
    p: Optional[Tensor]


def _lags(max_lag, lags, fn: str) -> Tuple[int, int]:
    if lags is None:
        if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 0 <= max_lag <= L.LAG_MAX:
            raise L.GandanetError(f"{fn}: max_lag is an integer in 0 .. {L.LAG_MAX}, got {max_lag!r}")
        return -int(max_lag), int(max_lag)
    if not isinstance(lags, (tuple, list)) or len(lags) != 2:
        raise L.GandanetError(f"{fn}: lags is a pair (lo, hi), got {lags!r}")
    return K._lag_range(lags[0], lags[1], fn)


def _lag1(x: Tensor, mask) -> Tensor:
    """the lag-1 "standard" autocorrelation of every series of a dense (T, M) tensor"""
    return K.series_acf(x, 1, "standard", mask)[0][1]


def lag_correlation(a: Tensor, b: Tensor, max_lag: int = 12, *, lags=None, min_pairs: int = 3, select: str = "abs",
                    mask: Optional[Tensor] = None, curve: bool = False, significance: bool = True) -> LagCorrelation:
    """Pearson r of ``a[t]`` against ``b[t + l]`` for the lags -``max_lag`` .. ``max_lag`` (or ``lags=(lo, hi)``) and every
    series of ``b`` (T, H, W) or (T, M); ``a`` has the shape of ``b``, or is one series (T,) that every pixel is compared
    with.  ``l > 0``: b follows a.  A lag with fewer than ``min_pairs`` (>= 2) valid pairs, or with a constant overlap, gives
    NaN.  ``select``: "abs" (largest |r|), "max" or "min".  ``mask`` (bool or uint8, the shape of one time step, nonzero = use
    the pixel) leaves pixels out.

    Returns ``lags`` (NL int64), the fp64 maps ``best_lag`` (NaN when no lag is valid), ``best_r``, ``best_n`` and ``r0``
    (NaN when 0 is not among the lags); with ``curve`` also ``r`` (NL, ...) fp64 and ``n`` (NL, ...) int32; with
    ``significance`` also ``n_eff``, ``z`` and the two-sided ``p`` of ``best_r`` from the lag-1 "standard" autocorrelations of
    both series -- not corrected for the selection over the lags.  Fields not asked for are None."""
    b = _cube(b, "lag_correlation b")
    a = _cube(a, "lag_correlation a")
    if b.dim() < 2:
        raise L.GandanetError("lag_correlation: b is (T, H, W) or (T, M)")
    t_len, tail = b.shape[0], tuple(b.shape[1:])
    if a.dtype != b.dtype or (a.dim() != 1 and a.shape != b.shape) or a.shape[0] != t_len:
        raise L.GandanetError(f"lag_correlation: a is ({t_len},) or has the shape and dtype of b, got {tuple(a.shape)} {a.dtype} against "
                              f"{tuple(b.shape)} {b.dtype}")
    if not 1 <= t_len <= L.LAG_MAX_T:
        raise L.GandanetError(f"lag_correlation: 1 <= T <= {L.LAG_MAX_T}, got T = {t_len}")
    lo, hi = _lags(max_lag, lags, "lag_correlation")
    if isinstance(min_pairs, bool) or not isinstance(min_pairs, (int, np.integer)) or min_pairs < 2:
        raise L.GandanetError(f"lag_correlation: min_pairs is an integer >= 2, got {min_pairs!r}")
    m = _series_mask(mask, tail, b.device)
    a2, b2 = a.reshape(t_len, -1), b.reshape(t_len, -1)
    r, n, best = K.lag_corr(a2, b2, lo, hi, int(min_pairs), select, m, curve=curve)
    maps = [best[k].reshape(tail) for k in range(4)]
    n_eff = z = p = None
    if significance:
        n_eff, z, p = (v.reshape(tail) for v in K.corr_signif(best[1], best[2], _lag1(a2, m if a.dim() > 1 else None), _lag1(b2, m)))
    nl = hi - lo + 1
    return LagCorrelation(torch.arange(lo, hi + 1, device=b.device), *maps, r.reshape((nl,) + tail) if curve else None,
                          n.reshape((nl,) + tail) if curve else None, n_eff, z, p)


def autocorrelation(x: Tensor, max_lag: int = 12, kind: str = "standard", mask: Optional[Tensor] = None, *,
                    min_pairs: int = 3) -> Tuple[Tensor, Tensor]:
    """the autocorrelation of every series ``x[:, ...]`` at the lags 0 .. ``max_lag``: (``acf`` (max_lag + 1, ...) fp64, ``n``
    the valid pairs of each lag, int32).  ``kind="standard"`` is the Box-Jenkins estimate c_k / c_0 with the mean and the
    variance of the whole series (acf_0 = 1); ``"pearson"`` is r of the two overlapping parts.  NaN samples are left out pair
    by pair."""
    x = _cube(x, "autocorrelation")
    lo, hi = _lags(max_lag, None, "autocorrelation")
    t_len, tail = x.shape[0], tuple(x.shape[1:])
    if not 1 <= t_len <= L.LAG_MAX_T:
        raise L.GandanetError(f"autocorrelation: 1 <= T <= {L.LAG_MAX_T}, got T = {t_len}")
    acf, n = K.series_acf(x.reshape(t_len, -1), hi, kind, _series_mask(mask, tail, x.device), int(min_pairs))
    return acf.reshape((hi + 1,) + tail), n.reshape((hi + 1,) + tail)


def correlation_significance(r: Tensor, n: Tensor, x: Optional[Tensor] = None, y: Optional[Tensor] = None, *,
                             r1x=None, r1y=None) -> Tuple[Tensor, Tensor, Tensor]:
    """(``n_eff``, ``z``, ``p``) of a correlation map ``r`` of ``n`` pairs, for instance ``cc`` and ``n`` of ``skill_maps``:
    n_eff = n (1 - r1x r1y) / (1 + r1x r1y) clamped to [0, n], z = atanh(r) sqrt(n_eff - 3), p = erfc(|z| / sqrt 2); NaN where
    n_eff <= 3.  The lag-1 autocorrelations come from the series ``x`` and ``y`` ((T, ...) with the map's shape behind T; ``x``
    may be one series (T,)) or are given as ``r1x`` / ``r1y`` (a map, or a number for ``r1x``)."""
    if not isinstance(r, Tensor) or not r.is_cuda or not isinstance(n, Tensor) or not n.is_cuda:
        raise L.GandanetError("correlation_significance: expected GPU tensors (there is no CPU path)")
    if n.shape != r.shape or r.numel() == 0:
        raise L.GandanetError(f"correlation_significance: r {tuple(r.shape)} and n {tuple(n.shape)} are two maps of one shape")
    shape = tuple(r.shape)

    def lag1(series, given, name, one_ok):
        if (series is None) == (given is None):
            raise L.GandanetError(f"correlation_significance: give either the series {name} or r1{name}")
        if series is not None:
            s = _cube(series, f"correlation_significance {name}")
            if tuple(s.shape[1:]) != shape and not (one_ok and s.dim() == 1):
                raise L.GandanetError(f"correlation_significance: {name} is (T,{' ' if shape else ''}{', '.join(map(str, shape))}), got {tuple(s.shape)}")
            return _lag1(s.reshape(s.shape[0], -1), None)
        g = given if isinstance(given, Tensor) else torch.as_tensor(given, dtype=torch.float64)
        g = g.to(device=r.device, dtype=torch.float64).contiguous()
        if tuple(g.shape) != shape and not (one_ok and g.numel() == 1):
            raise L.GandanetError(f"correlation_significance: r1{name} has the shape of r, got {tuple(g.shape)}")
        return g.reshape(-1)

    r1a, r1b = lag1(x, r1x, "x", True), lag1(y, r1y, "y", False)
    out = K.corr_signif(r.to(torch.float64).contiguous().reshape(-1), n.to(torch.float64).contiguous().reshape(-1), r1a, r1b)
    return tuple(v.reshape(shape) for v in out)


def driver_lags(target: Tensor, aux: Tensor, max_lag: int = 12, channels=None, **kw) -> Tuple[Tensor, Tensor, Tensor]:
    """which lag behind each driver does ``target`` (T, H, W) follow?  One ``lag_correlation(aux[:, c], target, max_lag, **kw)``
    per channel c of ``aux`` (T, C, H, W) (``channels``: the ones wanted, default all): (``best_lag``, ``best_r``, ``p``), each
    (C, H, W) fp64.  A positive lag means that the target follows the driver.  The kernel takes dense (T, M) cubes, and a
    channel of ``aux`` is a strided view: each channel is copied once into a (T, H, W) buffer, one channel at a time; the cube
    as a whole is never copied."""
    if not isinstance(aux, Tensor) or not aux.is_cuda or aux.dim() != 4 or not isinstance(target, Tensor) or aux[:, 0].shape != target.shape:
        raise L.GandanetError("driver_lags: target is a (T, H, W) and aux a (T, C, H, W) GPU tensor")
    chans = list(range(aux.shape[1])) if channels is None else [int(c) for c in channels]
    if not chans or any(not 0 <= c < aux.shape[1] for c in chans):
        raise L.GandanetError(f"driver_lags: channels out of 0 .. {aux.shape[1] - 1}: {channels!r}")
    kw = dict(kw, curve=False, significance=True)
    out = torch.empty((3, len(chans)) + tuple(target.shape[1:]), device=target.device, dtype=torch.float64)
    for i, c in enumerate(chans):
        res = lag_correlation(aux[:, c].contiguous(), target, max_lag, **kw)
        out[0, i], out[1, i], out[2, i] = res.best_lag, res.best_r, res.p
    return out[0], out[1], out[2]


def fdr_threshold(p: Tensor, alpha: float = 0.05, mask: Optional[Tensor] = None) -> Tuple[float, Tensor]:
    """Benjamini-Hochberg over the pixels of a p map that are not NaN (and where ``mask`` is nonzero): with the m p-values in
    ascending order, the threshold is the largest p_(k) with p_(k) <= alpha k / m (0.0 when there is none), and
    ``significant`` is the bool map p <= threshold.  Controls the false discovery rate at ``alpha`` over the map (Wilks
    2016); works on the ``p`` of ``trend_test`` as well.  torch sort and one scalar to the host; any device."""
    if not isinstance(p, Tensor) or not p.is_floating_point() or p.numel() == 0:
        raise L.GandanetError("fdr_threshold: p is a non-empty floating-point tensor")
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise L.GandanetError(f"fdr_threshold: alpha must lie in (0, 1), got {alpha!r}")
    valid = ~torch.isnan(p)
    if mask is not None:
        if not isinstance(mask, Tensor) or mask.shape != p.shape:
            raise L.GandanetError("fdr_threshold: the mask has the shape of p")
        valid = valid & (mask != 0).to(p.device)
    pv = torch.sort(p[valid].to(torch.float64)).values
    m = pv.numel()
    if m == 0:
        return 0.0, torch.zeros_like(valid)
    line = alpha * torch.arange(1, m + 1, device=p.device, dtype=torch.float64) / m
    thr = torch.where(pv <= line, pv, torch.full_like(pv, -1.0)).max().item()
    if thr < 0.0:
        return 0.0, torch.zeros_like(valid)
    return thr, valid & (p.to(torch.float64) <= thr)
