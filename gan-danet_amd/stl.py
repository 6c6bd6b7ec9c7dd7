"""STL decomposition on the device: the trend / seasonal split ``load_data()`` of the reference's ``datasets.py`` ends
with (``detrend_and_compare(lr_grace_05)``, ``detrend_and_compare(lr_grace_025)``: ``statsmodels.tsa.seasonal.STL(y,
seasonal=13, period=12).fit()`` in a Python double loop, one call per grid point), for every series of a ``(T, ...)`` tensor
in one launch.

The algorithm is Cleveland et al. 1990 as netlib's ``stl.f`` and statsmodels' port of it compute it, stated rule by rule in
``include/gandanet.h`` ("STL decomposition"); the kernel is ``csrc/stl.hip`` over ``csrc/stl_core.h``: fp32 or fp64 CUDA
tensors, all arithmetic fp64, one rounding to the output type, no atomics (the same bits on every run, whatever the number
of series).  There is no CPU path in this module (``kern.stl_decompose_host`` is the plain C++ twin the tests use).

Bit or tolerance agreement with statsmodels itself cannot be verified here: statsmodels is not installed and the
reference's ``cache/dataset_cache.npz`` holds no recorded trend.  Agreement rests on the algorithm text, on closed-form
cases (a line plus a zero-mean periodic term comes back exactly) and on an independent fp64 restatement in
``tests/stl_util.py``, not on a run of statsmodels.  Jumps other than 1 are not implemented.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import kern as K

Tensor = torch.Tensor
L = K.L


class STLResult(NamedTuple):
    trend: Tensor
    seasonal: Tensor
    resid: Tensor
    weights: Tensor


def default_windows(period: int, seasonal: int) -> Tuple[int, int]:
    """statsmodels' default (trend, low_pass): the smallest odd integer >= 1.5 period / (1 - 1.5 / seasonal) and the
    smallest odd integer > period"""
    trend = int(math.ceil(1.5 * period / (1.0 - 1.5 / seasonal)))
    trend += 1 if trend % 2 == 0 else 0
    low_pass = period + 1
    low_pass += 1 if low_pass % 2 == 0 else 0
    return trend, low_pass


def _int(v, name: str) -> int:
    if isinstance(v, bool) or int(v) != v:
        raise L.GandanetError(f"stl_decompose: {name} must be an integer, got {v!r}")
    return int(v)


def resolve(t_len: int, period=12, seasonal=13, trend=None, low_pass=None, seasonal_deg=1, trend_deg=1, low_pass_deg=1, robust=False,
            inner_iter=None, outer_iter=None) -> dict:
    """the explicit parameter set of a call on series of length ``t_len``, defaults filled in and every rule checked on the
    host (the C entry points check them again)"""
    period, seasonal = _int(period, "period"), _int(seasonal, "seasonal")
    if period < 2:
        raise L.GandanetError("stl_decompose: period must be >= 2")
    if seasonal < 3 or seasonal % 2 == 0:
        raise L.GandanetError("stl_decompose: seasonal must be an odd integer >= 3")
    d_trend, d_low = default_windows(period, seasonal)
    trend = d_trend if trend is None else _int(trend, "trend")
    low_pass = d_low if low_pass is None else _int(low_pass, "low_pass")
    for v, name in ((trend, "trend"), (low_pass, "low_pass")):
        if v < 3 or v % 2 == 0:
            raise L.GandanetError(f"stl_decompose: {name} must be an odd integer >= 3")
        if v <= period:
            raise L.GandanetError(f"stl_decompose: {name} must be larger than the period")
    degs = [_int(d, "a degree") for d in (seasonal_deg, trend_deg, low_pass_deg)]
    if any(d not in (0, 1) for d in degs):
        raise L.GandanetError("stl_decompose: degrees are 0 or 1")
    inner_iter = (2 if robust else 5) if inner_iter is None else _int(inner_iter, "inner_iter")
    outer_iter = (15 if robust else 0) if outer_iter is None else _int(outer_iter, "outer_iter")
    if inner_iter < 1 or outer_iter < 0:
        raise L.GandanetError("stl_decompose: inner_iter must be >= 1 and outer_iter >= 0")
    if t_len < 2 * period:
        raise L.GandanetError(f"stl_decompose: {t_len} samples are fewer than two periods of {period}")
    if t_len > L.STL_MAX_T:
        raise L.GandanetError(f"stl_decompose: {t_len} samples, more than {L.STL_MAX_T}")
    return dict(period=period, seasonal=seasonal, trend=trend, low_pass=low_pass, seasonal_deg=degs[0], trend_deg=degs[1],
                low_pass_deg=degs[2], inner_iter=inner_iter, outer_iter=outer_iter)


def _input(x, name: str) -> Tensor:
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise L.GandanetError(f"{name}: expected a GPU tensor (there is no CPU path)")
    if x.dtype not in (torch.float32, torch.float64):
        raise L.GandanetError(f"{name}: expected float32 or float64, got {x.dtype}")
    if x.dim() == 0 or x.numel() == 0:
        raise L.GandanetError(f"{name}: expected a non-empty (T,) or (T, ...) tensor")
    return x if x.is_contiguous() else x.contiguous()


def stl_decompose(x: Tensor, period: int = 12, seasonal: int = 13, trend: Optional[int] = None, low_pass: Optional[int] = None,
                  seasonal_deg: int = 1, trend_deg: int = 1, low_pass_deg: int = 1, robust: bool = False,
                  inner_iter: Optional[int] = None, outer_iter: Optional[int] = None) -> STLResult:
    """``STL(y, period=, seasonal=, trend=, low_pass=, seasonal_deg=, trend_deg=, low_pass_deg=, robust=).fit(inner_iter=,
    outer_iter=)`` for every series ``x[:, ...]`` of a ``(T,)`` or ``(T, ...)`` GPU tensor, time along axis 0.

    ``trend=None`` is the smallest odd integer >= 1.5 period / (1 - 1.5 / seasonal) (21 for 12 and 13), ``low_pass=None`` the
    smallest odd integer > period; ``inner_iter`` / ``outer_iter`` default to 5 / 0, or 2 / 15 with ``robust=True``.  A call
    runs ``outer_iter + 1`` outer passes and renews the robustness weights after each but the last.  Returns ``trend``,
    ``seasonal``, ``resid`` (= x - seasonal - trend) and ``weights`` (the last robustness weights; ones without an outer
    iteration), new tensors of the shape and dtype of ``x``.  No host sync.

    A series that holds a non-finite value has unspecified outputs; the other series of the call are not affected."""
    x = _input(x, "stl_decompose")
    p = resolve(x.shape[0], period, seasonal, trend, low_pass, seasonal_deg, trend_deg, low_pass_deg, robust, inner_iter, outer_iter)
    outs = K.stl_decompose(x.reshape(x.shape[0], -1), p)
    return STLResult(*[o.reshape(x.shape) for o in outs])


def detrend_and_compare(data: Tensor):
    """``detrend_and_compare(data)`` of ``datasets.py`` on a ``(time, space_x, space_y)`` GPU tensor: the STL trend of every
    grid point (``seasonal=13, period=12``), ``detrended = data - trend``, ``reconstructed = detrended + trend`` and
    ``max_difference = max |data - reconstructed|``, reduced on the device and copied once (the one host sync).  Returns
    ``(trend, detrended, reconstructed, max_difference)`` as the reference does, tensors for its arrays and a Python float
    for the maximum; nothing is printed."""
    data = _input(data, "detrend_and_compare")
    p = resolve(data.shape[0], 12, 13)
    trend = K.stl_decompose(data.reshape(data.shape[0], -1), p, want_weights=False)[0].reshape(data.shape)
    detrended = data - trend
    reconstructed = detrended + trend
    max_difference = (data - reconstructed).abs().max().item()
    return trend, detrended, reconstructed, max_difference
