"""Statistics along the time axis of every pixel, on the device: skill maps of one cube against another (bias, RMSE,
correlation, NSE, KGE ...), the trend and the annual / semi-annual amplitude and phase of every pixel, and the NaN-aware
block mean that takes the 0.05 degree product back to the 0.25 degree grid of GRACE.  The reference only gestures at these
(the map comparison of ``test.ipynb`` ``_plot_spatial_distribution``, ``pearsonr`` of two mean series,
``taylorDiagram.py:151-159``); without this module both cubes had to be copied to the host.

The kernels are ``csrc/series.hip`` over ``csrc/series_core.h`` (``include/gandanet.h``, "Per-pixel time series"): fp32 or
fp64 CUDA tensors, time along axis 0, all arithmetic fp64, one thread per series walking t in ascending order, no atomics
(the same bits on every run, whatever the number of series).  There is no CPU path in this module (``kern.series_*_host``
and ``kern.block_mean_host`` are the plain C++ twins the tests use).  torch allocates, views and copies; the arithmetic on
the maps happens in the kernels.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kern as K

Tensor = torch.Tensor
L = K.L

METRICS = L.SKILL_MAPS
DEFAULT_METRICS = ("n", "bias", "rmse", "cc", "nse", "kge")


def _cube(x, name: str) -> Tensor:
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise L.GandanetError(f"{name}: expected a GPU tensor (there is no CPU path)")
    if x.dtype not in (torch.float32, torch.float64):
        raise L.GandanetError(f"{name}: expected float32 or float64, got {x.dtype}")
    if x.dim() == 0 or x.numel() == 0:
        raise L.GandanetError(f"{name}: expected a non-empty (T,) or (T, ...) tensor")
    return x if x.is_contiguous() else x.contiguous()


def _series_mask(mask, shape, device) -> Optional[Tensor]:
    if mask is None:
        return None
    if not isinstance(mask, Tensor) or not mask.is_cuda:
        raise L.GandanetError("mask: expected a GPU tensor (there is no CPU path)")
    if tuple(mask.shape) != tuple(shape):
        raise L.GandanetError(f"mask: expected the shape of one time step {tuple(shape)}, got {tuple(mask.shape)}")
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    return mask.contiguous().reshape(-1)


class SeriesSkill:
    """Streaming skill of a prediction against its truth along time, per pixel.  ``shape`` is the shape of one time step;
    ``mask`` (bool or uint8 of that shape, nonzero = use the pixel) leaves pixels out (their maps are NaN, n = 0);
    ``skip_nan`` drops a pair with a NaN on either side.  ``update`` takes chunks of time steps in order: the per-pixel
    recurrence is sequential, so chunks give the same bits as one call."""

    def __init__(self, shape: Sequence[int], mask: Optional[Tensor] = None, skip_nan: bool = True):
        self.shape = tuple(int(s) for s in shape)
        self.m = math.prod(self.shape)
        if self.m <= 0:
            raise L.GandanetError(f"SeriesSkill: empty shape {self.shape}")
        self.mask_arg = mask
        self.skip_nan = bool(skip_nan)
        self.mask: Optional[Tensor] = None
        self.rec: Optional[Tensor] = None

    def update(self, pred: Tensor, truth: Tensor) -> "SeriesSkill":
        pred, truth = _cube(pred, "SeriesSkill.update pred"), _cube(truth, "SeriesSkill.update truth")
        if tuple(pred.shape[1:]) != self.shape or pred.shape != truth.shape or pred.dtype != truth.dtype:
            raise L.GandanetError(f"SeriesSkill.update: expected two (T, {', '.join(map(str, self.shape))}) tensors of one dtype, got "
                                  f"{tuple(pred.shape)} {pred.dtype} and {tuple(truth.shape)} {truth.dtype}")
        first = self.rec is None
        if first:
            self.mask = _series_mask(self.mask_arg, self.shape, pred.device)
            self.rec = torch.empty((8, self.m), device=pred.device, dtype=torch.float64)
        K.series_stats(pred.reshape(pred.shape[0], self.m), truth.reshape(pred.shape[0], self.m), self.rec, self.mask, self.skip_nan,
                       accumulate=not first)
        return self

    def records(self) -> Tensor:
        """the (8, *shape) fp64 records (``include/gandanet.h``, "Evaluation"), a view of the running state"""
        if self.rec is None:
            raise L.GandanetError("SeriesSkill.records: no update yet")
        return self.rec.reshape((8,) + self.shape)

    def compute(self, metrics: Sequence[str] = DEFAULT_METRICS, ddof: int = 0) -> Dict[str, Tensor]:
        """the maps named by ``metrics`` (any of ``METRICS``), each fp64 of ``shape``; ``ddof`` is that of std_p / std_t"""
        if self.rec is None:
            raise L.GandanetError("SeriesSkill.compute: no update yet")
        out = K.series_skill(self.rec, metrics, ddof)
        names = [nm for nm in METRICS if nm in set(metrics)]
        return {nm: out[i].reshape(self.shape) for i, nm in enumerate(names)}


def skill_maps(pred: Tensor, truth: Tensor, mask: Optional[Tensor] = None, metrics: Sequence[str] = DEFAULT_METRICS, ddof: int = 0,
               skip_nan: bool = True) -> Dict[str, Tensor]:
    """per-pixel maps over time of ``pred`` against ``truth``, both ``(T, ...)``: the one-shot form of ``SeriesSkill``"""
    pred = _cube(pred, "skill_maps pred")
    return SeriesSkill(pred.shape[1:], mask, skip_nan).update(pred, truth).compute(metrics, ddof)


class TaylorStats(NamedTuple):
    refstd: Tensor
    stddev: Tensor
    corrcoef: Tensor
    crmsd: Tensor


def taylor_stats(pred: Tensor, truth: Tensor, mask: Optional[Tensor] = None, affine=None) -> TaylorStats:
    """the numbers of ``taylorDiagram.py:151-159`` over all valid pairs of two tensors of one shape: ``refstd`` and
    ``stddev`` (ddof 1), ``corrcoef`` and the centred RMS difference, 0-d fp64 tensors on the device (no host sync);
    ``TaylorDiagram(refstd).add_sample(stddev, corrcoef)`` takes the first three.  One ``gd_eval_stats`` record: ``mask``
    (uint8) and ``affine`` as ``kern.eval_stats`` takes them; pairs with a NaN are dropped."""
    pred, truth = _cube(pred, "taylor_stats pred"), _cube(truth, "taylor_stats truth")
    rec = torch.empty(8, device=pred.device, dtype=torch.float64)
    K.eval_stats(pred, truth, rec, mask=mask, affine=affine, skip_nan=True)
    out = K.series_skill(rec.reshape(8, 1), ("std_t", "std_p", "cc", "crmsd"), ddof=1)   # rows in the order of METRICS
    return TaylorStats(refstd=out[1, 0], stddev=out[0, 0], corrcoef=out[2, 0], crmsd=out[3, 0])


def _basis_tensor(basis, t_len: int, device) -> Tensor:
    if isinstance(basis, Tensor):
        b = basis.to(device=device, dtype=torch.float64)
    else:
        b = torch.from_numpy(np.ascontiguousarray(np.asarray(basis, dtype=np.float64))).to(device)
    if b.dim() != 2 or b.shape[0] != t_len or not 1 <= b.shape[1] <= L.LSTSQ_MAX_P:
        raise L.GandanetError(f"lstsq_series: the basis is ({t_len}, P) with 1 <= P <= {L.LSTSQ_MAX_P}, got {tuple(b.shape)}")
    return b.contiguous()


def lstsq_series(x: Tensor, basis) -> Tuple[Tensor, Tensor, Tensor]:
    """least squares of every series ``x[:, ...]`` against the common design matrix ``basis`` (T, P), 1 <= P <= 8 (array or
    tensor), NaN samples left out of their series' fit: ``coef`` (P, ...), ``rss`` (...) and ``n`` (...), fp64.  A series
    with fewer valid samples than P, or a singular system, has NaN ``coef`` and ``rss``."""
    x = _cube(x, "lstsq_series")
    b = _basis_tensor(basis, x.shape[0], x.device)
    coef, rss, n = K.series_lstsq(x.reshape(x.shape[0], -1), b)
    tail = tuple(x.shape[1:])
    return coef.reshape((b.shape[1],) + tail), rss.reshape(tail), n.reshape(tail)


class HarmonicFit(NamedTuple):
    mean: Tensor
    slope: Optional[Tensor]
    amplitude: Tensor
    phase: Tensor
    rms_resid: Tensor
    n: Tensor


def harmonic_basis(times, period: float = 12.0, harmonics: int = 2, trend: bool = True) -> Tuple[np.ndarray, float]:
    """the (T, 1 + trend + 2 harmonics) fp64 design matrix on the host: 1, tau = (t - t_mid) / t_half in [-1, 1] (this keeps
    the normal equations well conditioned), then cos(2 pi k t / period), sin(2 pi k t / period) for k = 1 .. harmonics;
    and d tau / d t = 1 / t_half"""
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    k_max = int(harmonics)
    if not 0 <= k_max <= 3 or k_max != harmonics:
        raise L.GandanetError(f"harmonic_fit: harmonics must be 0 .. 3, got {harmonics!r}")
    if not period > 0 or t.size == 0 or not np.all(np.isfinite(t)):
        raise L.GandanetError("harmonic_fit: the period must be positive and the times finite")
    t_mid, t_half = 0.5 * (t.max() + t.min()), 0.5 * (t.max() - t.min())
    t_half = t_half if t_half > 0 else 1.0
    cols = [np.ones_like(t)]
    if trend:
        cols.append((t - t_mid) / t_half)
    for k in range(1, k_max + 1):
        w = 2.0 * np.pi * k / float(period)
        cols += [np.cos(w * t), np.sin(w * t)]
    return np.stack(cols, axis=1), 1.0 / t_half


def harmonic_fit(x: Tensor, times=None, period: float = 12.0, harmonics: int = 2, trend: bool = True) -> HarmonicFit:
    """the standard GRACE analysis of every series ``x[:, ...]``: y = mean + slope (t - t_mid) + sum_k A_k cos(2 pi k t /
    period - phi_k), fitted by least squares over the samples that are not NaN.  ``times`` (T values, default 0 .. T - 1)
    are in the unit of ``period``.  Returns ``mean`` (the level at the middle of the record), ``slope`` per unit of
    ``times`` (None without ``trend``), ``amplitude`` and ``phase`` (``harmonics``, ...), ``rms_resid`` = sqrt(rss / n)
    and ``n``, all fp64.  ``harmonics=0, trend=True`` is the per-pixel linear trend."""
    x = _cube(x, "harmonic_fit")
    t_len = x.shape[0]
    times = np.arange(t_len, dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64).reshape(-1)
    if times.size != t_len:
        raise L.GandanetError(f"harmonic_fit: {times.size} times for {t_len} samples")
    basis, tau_scale = harmonic_basis(times, period, harmonics, trend)
    b = _basis_tensor(basis, t_len, x.device)
    coef, rss, n = K.series_lstsq(x.reshape(t_len, -1), b)
    amp, phase, slope, rms = K.harmonic_finalize(coef, int(harmonics), bool(trend), tau_scale, rss, n)
    tail = tuple(x.shape[1:])
    kk = (int(harmonics),) + tail
    return HarmonicFit(mean=coef[0].reshape(tail), slope=None if slope is None else slope.reshape(tail), amplitude=amp.reshape(kk),
                       phase=phase.reshape(kk), rms_resid=rms.reshape(tail), n=n.reshape(tail))


def _factor(factor) -> Tuple[int, int]:
    pair = tuple(factor) if isinstance(factor, (tuple, list)) else (factor, factor)
    if len(pair) != 2 or any(isinstance(f, bool) or not isinstance(f, (int, np.integer)) or f < 1 for f in pair):
        raise L.GandanetError(f"coarsen: the factor is a positive integer or a pair of them, got {factor!r}")
    fy, fx = pair
    return int(fy), int(fx)


def coarsen(x: Tensor, factor, weights: Optional[Tensor] = None, min_count: int = 1, return_count: bool = False):
    """NaN-aware mean of every ``factor`` (int or (fy, fx)) block of the last two axes of ``x`` (..., H, W): the inverse of
    the notebook's ``np.repeat(np.repeat(bias, 4, 1), 4, 2)``.  ``weights`` (H, W), for instance cos(lat); a block with
    fewer than ``min_count`` values that are not NaN gives NaN.  The result has the dtype of ``x``."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise L.GandanetError("coarsen: expected a GPU tensor (there is no CPU path)")
    fy, fx = _factor(factor)
    if weights is not None:
        if not isinstance(weights, Tensor) or not weights.is_cuda:
            raise L.GandanetError("coarsen: the weights are a GPU tensor")
        weights = weights.to(torch.float64).contiguous()
    out, count = K.block_mean(x if x.is_contiguous() else x.contiguous(), fy, fx, weights, min_count)
    return (out, count) if return_count else out


def consistency(downscaled: Tensor, coarse: Tensor, factor, mask: Optional[Tensor] = None, metrics: Sequence[str] = DEFAULT_METRICS,
                ddof: int = 0, weights: Optional[Tensor] = None, min_count: int = 1) -> Dict[str, Tensor]:
    """does the downscaled product, averaged back to the coarse grid, reproduce the coarse field?
    ``skill_maps(coarsen(downscaled, factor), coarse)`` on (T, H, W) against (T, H / fy, W / fx)."""
    return skill_maps(coarsen(downscaled, factor, weights, min_count), coarse, mask, metrics, ddof)
