"""Is a pixel's trend significant, and what is its robust slope?  The Mann-Kendall test and the Theil-Sen slope with its
confidence interval for every pixel series of a cube, on the device, plain or in the seasonal form of Hirsch and Slack
(``period=12`` for monthly data: only pairs of the same calendar month count).  ``harmonic_fit(harmonics=0)`` gives the
least-squares slope alone; this module adds the p-value, Kendall's tau, and a slope that the outlier months of GRACE do not
move.  The quantities are those of ``scipy.stats.theilslopes`` (``method='separate'``) and ``scipy.stats.kendalltau`` in
scipy's own order of operations: slope, intercept, interval and tau equal scipy's bit for bit.

The kernel is ``csrc/trend.hip`` over ``csrc/trend_core.h`` (``include/gandanet.h``, "Per-pixel trend tests"): fp32 or fp64
CUDA tensors, time along axis 0, all arithmetic fp64; one wave per series, the O(T^2) pairs swept from LDS, the order
statistics by an exact radix select that stores no slope.  There is no CPU path in this module (``kern.trend_test_host`` is
the plain C++ twin the tests use).
"""
from __future__ import annotations

import statistics
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import kern as K
from .timeseries import _cube, _series_mask

Tensor = torch.Tensor
L = K.L

MAPS = L.TREND_MAPS


class TrendTest(NamedTuple):
    n: Tensor
    s: Tensor
    var_s: Tensor
    z: Tensor
    p: Tensor
    tau: Tensor
    slope: Optional[Tensor]
    intercept: Optional[Tensor]
    slope_lo: Optional[Tensor]
    slope_hi: Optional[Tensor]


def normal_quantile(p: float) -> float:
    """the quantile of the standard normal distribution at ``p`` in (0, 1), on the host"""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise L.GandanetError(f"normal_quantile: p must lie in (0, 1), got {p!r}")
    return statistics.NormalDist().inv_cdf(p)


def _times(times, t_len: int) -> np.ndarray:
    t = np.arange(t_len, dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64).reshape(-1)
    if t.size != t_len:
        raise L.GandanetError(f"trend_test: {t.size} times for {t_len} samples")
    if not np.all(np.isfinite(t)) or not np.all(np.diff(t) > 0):
        raise L.GandanetError("trend_test: the times must be finite and strictly increasing")
    return np.ascontiguousarray(t)


def trend_test(x: Tensor, times=None, period: Optional[int] = None, mask: Optional[Tensor] = None, alpha: float = 0.05,
               sen: bool = True, ci: bool = True, continuity: bool = True) -> TrendTest:
    """Mann-Kendall and Theil-Sen of every series ``x[:, ...]`` (2 <= T <= 2048 samples), NaN samples left out of their
    series.  ``times`` (T finite, strictly increasing values, default 0 .. T - 1) are the abscissae of the slope.
    ``period`` = p >= 2 selects the seasonal form: sample k belongs to season k mod p, only pairs inside a season count and
    the slopes of all seasons are pooled.  ``mask`` (bool or uint8, the shape of one time step, nonzero = use the pixel)
    leaves pixels out (n = 0, NaN elsewhere).

    Returns fp64 maps of the shape of one time step: ``n`` valid samples, the statistic ``s``, its variance ``var_s``
    (corrected for ties), ``z`` (with the continuity correction unless ``continuity=False``), the two-sided ``p``, Kendall's
    ``tau`` (tau-b); with ``sen`` the median ``slope`` per unit of ``times`` and ``intercept`` = median(y) - slope
    median(t); with ``ci`` the bounds ``slope_lo``, ``slope_hi`` of the 1 - ``alpha`` interval (``alpha > 0.5`` means
    1 - alpha, as in scipy).  Maps that were not asked for are None.  A series with fewer than two valid samples has its
    ``n``, ``s`` = 0 and NaN elsewhere."""
    x = _cube(x, "trend_test")
    t_len = x.shape[0]
    if not 2 <= t_len <= L.TREND_MAX_T:
        raise L.GandanetError(f"trend_test: 2 <= T <= {L.TREND_MAX_T}, got T = {t_len}")
    if period is None:
        period = 0
    elif isinstance(period, bool) or not isinstance(period, (int, np.integer)) or not 2 <= period <= t_len:
        raise L.GandanetError(f"trend_test: the period is None or an integer in 2 .. T, got {period!r}")
    if ci and not sen:
        raise L.GandanetError("trend_test: the interval (ci) needs the slope (sen)")
    zq = 0.0
    if ci:
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise L.GandanetError(f"trend_test: alpha must lie in (0, 1), got {alpha!r}")
        zq = normal_quantile((1.0 - alpha if alpha > 0.5 else alpha) / 2.0)
    tail = tuple(x.shape[1:])
    t_dev = torch.from_numpy(_times(times, t_len)).to(x.device)
    out = K.trend_test(x.reshape(t_len, -1), t_dev, int(period), _series_mask(mask, tail, x.device), K.trend_flags(sen, ci, continuity), zq)
    maps = [out[k].reshape(tail) for k in range(len(MAPS))]
    if not sen:
        maps[6] = maps[7] = None
    if not ci:
        maps[8] = maps[9] = None
    return TrendTest(*maps)


def mann_kendall(x: Tensor, times=None, period: Optional[int] = None, mask: Optional[Tensor] = None,
                 continuity: bool = True) -> TrendTest:
    """the test alone (the pair sweep without the selection): ``trend_test(..., sen=False, ci=False)``"""
    return trend_test(x, times, period, mask, sen=False, ci=False, continuity=continuity)


def sen_slope(x: Tensor, times=None, period: Optional[int] = None, mask: Optional[Tensor] = None, alpha: float = 0.05,
              ci: bool = True, continuity: bool = True) -> TrendTest:
    """the test with the Theil-Sen slope, and its interval unless ``ci=False``: ``trend_test(..., sen=True)``"""
    return trend_test(x, times, period, mask, alpha, sen=True, ci=ci, continuity=continuity)
