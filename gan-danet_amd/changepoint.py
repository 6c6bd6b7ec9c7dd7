"""When did the behaviour of a pixel's series change?  ``trend_test`` says whether a series has a monotone trend; this
module says where it breaks: the Pettitt test (Pettitt 1979: a rank test for a shift at an unknown time), the CUSUM
statistics Q and R of Buishand (1982), and two least-squares two-segment fits -- a shift of the mean ("step") and two
separate lines ("trend") -- for every pixel series of a cube, on the device; and binary segmentation for several breaks.
Every "index" is the time step of the LAST SAMPLE BEFORE the change.  Seasonal data: remove the cycle first
(``drought_index(kind="anomaly")``, ``stl_decompose``); a seasonal cycle is otherwise read as a sequence of changes.

The kernel is ``csrc/changepoint.hip`` over ``csrc/changepoint_core.h`` (``include/gandanet.h``, "Per-pixel change points",
holds the definitions in full): fp32 or fp64 CUDA tensors, time along axis 0, all arithmetic fp64; one wave per series, the
O(T^2) candidate sweeps from LDS.  There is no CPU path in this module (``kern.change_point_host`` is the plain C++ twin
the tests use).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import kern as K
from .timeseries import _cube, _series_mask

Tensor = torch.Tensor
L = K.L

MAPS = L.CP_MAPS
MAX_BREAKS = 7
_FAMILY = {"pt": L.CP_PETTITT, "cs": L.CP_CUSUM, "st": L.CP_STEP, "tr": L.CP_TREND}
_METHODS = {"pettitt": (L.CP_PETTITT, "pt_index", "pt_p"), "step": (L.CP_STEP, "st_index", "st_f"), "trend": (L.CP_TREND, "tr_index", "tr_f")}

ChangePoint = NamedTuple("ChangePoint", [(name, Optional[Tensor]) for name in MAPS])


class ChangePoints(NamedTuple):
    count: Tensor
    index: Tensor


def _min_seg(min_seg) -> int:
    if isinstance(min_seg, bool) or not isinstance(min_seg, (int, np.integer)) or not 2 <= min_seg <= L.CP_MAX_T:
        raise L.GandanetError(f"change_point: min_seg is an integer in 2 .. {L.CP_MAX_T}, got {min_seg!r}")
    return int(min_seg)


def _input(x, name: str):
    x = _cube(x, name)
    t_len = x.shape[0]
    if not 2 <= t_len <= L.CP_MAX_T:
        raise L.GandanetError(f"{name}: 2 <= T <= {L.CP_MAX_T}, got T = {t_len}")
    return x, t_len, tuple(x.shape[1:])


def _times(times, t_len: int) -> np.ndarray:
    t = np.arange(t_len, dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64).reshape(-1)
    if t.size != t_len:
        raise L.GandanetError(f"change_point: {t.size} times for {t_len} samples")
    if not np.all(np.isfinite(t)) or not np.all(np.diff(t) > 0):
        raise L.GandanetError("change_point: the times must be finite and strictly increasing")
    return np.ascontiguousarray(t)


def _window(window, tail, device) -> Optional[Tensor]:
    if window is None:
        return None
    m = int(np.prod(tail, dtype=np.int64))
    if isinstance(window, Tensor):
        if not window.is_cuda or window.dtype != torch.int32 or tuple(window.shape) != (2,) + tuple(tail):
            raise L.GandanetError(f"change_point: window is an int32 GPU tensor of shape {(2,) + tuple(tail)} or a (begin, end) pair of ints")
        return window.contiguous().reshape(2, m)
    try:
        begin, end = window
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (begin, end))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise L.GandanetError(f"change_point: window is an int32 GPU tensor of shape {(2,) + tuple(tail)} or a (begin, end) pair of ints")
    w = torch.empty((2, m), device=device, dtype=torch.int32)
    w[0] = int(begin)
    w[1] = int(end)
    return w


def change_point(x: Tensor, times=None, mask: Optional[Tensor] = None, window=None, min_seg: int = 5, pettitt: bool = True,
                 cusum: bool = True, step: bool = True, trend: bool = True) -> ChangePoint:
    """The single most likely change of every series ``x[:, ...]`` (2 <= T <= 2048 samples), NaN samples left out of their
    series.  ``times`` (T finite, strictly increasing values, default 0 .. T - 1) are the abscissae of the two-line fit.
    ``mask`` (bool or uint8, the shape of one time step, nonzero = use the pixel) leaves pixels out (n = 0).  ``window``: an
    int32 ``(2, ...)`` tensor (begin, end of every pixel) or a ``(begin, end)`` pair of ints: only the steps begin <= t < end
    take part (clamped to 0 .. T).  ``min_seg`` in 2 .. 2048: the fewest valid samples on either side of a break of the
    fitted models.

    Returns fp64 maps of the shape of one time step; maps of families not asked for are None; undefined entries are NaN and
    -1 in the index maps.  ``n``: valid samples.
    ``pettitt``: ``pt_k`` = max |U_k|, ``pt_u`` the signed U there (positive: higher before the change), ``pt_index``,
    ``pt_p`` = min(1, 2 exp(-6 K^2 / (n^3 + n^2))) (Pettitt's approximation, good for p < 0.5).
    ``cusum``: Buishand's ``cs_q`` = max |S_k| / (sd sqrt n) and range ``cs_r``, ``cs_index`` at the first maximum of
    |S_k|, and ``cs_p`` of Q from the Brownian-bridge limit 2 sum (-1)^(j+1) exp(-2 j^2 q^2): ASYMPTOTIC in n and
    anti-conservative for short series (Buishand tabulates smaller critical values at n <= 50).
    ``step``: the least-squares shift of the mean: ``st_index``, ``st_mean_before``, ``st_mean_after``, ``st_shift``,
    ``st_rss0`` (no break), ``st_rss`` and ``st_f`` = (rss0 - rss) / (rss / (n - 2)).
    ``trend``: two separate least-squares lines: ``tr_index``, the slopes (per unit of ``times``) and intercepts before and
    after, ``tr_jump`` (line 2 minus line 1 half way between the two samples around the break), ``tr_rss0`` (one line),
    ``tr_rss`` and ``tr_f`` = ((rss0 - rss) / 2) / (rss / (n - 4)).
    NEITHER F STATISTIC IS CORRECTED FOR THE SELECTION of the break among the candidates: the maximum over k of an F is not
    F-distributed, so ``st_f`` and ``tr_f`` rank pixels and feed thresholds; they are not p-values in disguise."""
    x, t_len, tail = _input(x, "change_point")
    min_seg = _min_seg(min_seg)
    flags = K.change_point_flags(pettitt, cusum, step, trend)
    t_dev = torch.from_numpy(_times(times, t_len)).to(x.device)
    out = K.change_point(x.reshape(t_len, -1), t_dev, _series_mask(mask, tail, x.device), _window(window, tail, x.device), min_seg, flags)
    return ChangePoint(*[out[k].reshape(tail) if k == 0 or flags & _FAMILY[name[:2]] else None for k, name in enumerate(MAPS)])


def pettitt(x: Tensor, times=None, mask: Optional[Tensor] = None, window=None) -> ChangePoint:
    """the Pettitt test alone: ``change_point(..., cusum=False, step=False, trend=False)``"""
    return change_point(x, times, mask, window, pettitt=True, cusum=False, step=False, trend=False)


def cusum(x: Tensor, times=None, mask: Optional[Tensor] = None, window=None) -> ChangePoint:
    """Buishand's CUSUM statistics alone (``cs_p`` is asymptotic): ``change_point(..., pettitt=False, step=False, trend=False)``"""
    return change_point(x, times, mask, window, pettitt=False, cusum=True, step=False, trend=False)


def segmented_fit(x: Tensor, model: str = "step", times=None, mask: Optional[Tensor] = None, window=None, min_seg: int = 5) -> ChangePoint:
    """one fitted model alone, ``model`` = "step" (a shift of the mean) or "trend" (two separate lines); its F statistic is
    not corrected for the selection of the break"""
    if model not in ("step", "trend"):
        raise L.GandanetError(f"segmented_fit: model is 'step' or 'trend', got {model!r}")
    return change_point(x, times, mask, window, min_seg, pettitt=False, cusum=False, step=model == "step", trend=model == "trend")


def change_points(x: Tensor, max_breaks: int = 3, method: str = "pettitt", alpha: float = 0.05, min_f: Optional[float] = None,
                  min_seg: int = 5, times=None, mask: Optional[Tensor] = None) -> ChangePoints:
    """Several breaks per pixel by binary segmentation.  Level by level, every open segment of every pixel is tested in ONE
    kernel call (each through its own ``window``); a segment splits at its break where ``pt_p < alpha`` (``method``
    "pettitt") or where the F statistic is ``>= min_f`` ("step", "trend"; ``min_f`` is required and, F being uncorrected for
    the selection of the break, is a threshold of the user's choosing, not a quantile of F); its two halves are open at the
    next level, a segment that does not split is closed.  Where a level offers a pixel more splits than ``max_breaks``
    leaves room for, the strongest go first (smallest p, largest F; ties to the earlier segment).  It ends when no pixel
    splits, and after at most ``max_breaks`` (<= 7) levels.  ``min_seg`` bounds the segments of the fitted models only: it
    has no effect with ``method="pettitt"``, whose segments may shrink to two samples.

    Returns ``count`` (int64, the shape of one time step) and ``index`` (int64, ``(max_breaks, ...)``): the breaks of each
    pixel ascending in time, -1 padded; each is the step of the last sample before the change.  The bookkeeping is torch
    ops on the device; one scalar per level (did any pixel split?) goes to the host.  A level with s open segments per
    pixel runs on s copies of the cube side by side."""
    x, t_len, tail = _input(x, "change_points")
    min_seg = _min_seg(min_seg)
    if isinstance(max_breaks, bool) or not isinstance(max_breaks, (int, np.integer)) or not 1 <= max_breaks <= MAX_BREAKS:
        raise L.GandanetError(f"change_points: max_breaks is an integer in 1 .. {MAX_BREAKS}, got {max_breaks!r}")
    if method not in _METHODS:
        raise L.GandanetError(f"change_points: method is one of {sorted(_METHODS)}, got {method!r}")
    flags, index_map, stat_map = _METHODS[method]
    if method == "pettitt":
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise L.GandanetError(f"change_points: alpha must lie in (0, 1), got {alpha!r}")
    else:
        if min_f is None or not float(min_f) > 0.0:
            raise L.GandanetError(f"change_points: method {method!r} needs min_f > 0, got {min_f!r}")
        min_f = float(min_f)
    x2 = x.reshape(t_len, -1)
    t_dev = torch.from_numpy(_times(times, t_len)).to(x.device)
    mask = _series_mask(mask, tail, x.device)
    count, index = _segmentation(lambda xs, ms, win: K.change_point(xs, t_dev, ms, win, min_seg, flags), x2, mask, int(max_breaks), method,
                                 alpha, min_f)
    return ChangePoints(count.reshape(tail), index.reshape((int(max_breaks),) + tail))


def _segmentation(run, x2: Tensor, mask: Optional[Tensor], max_breaks: int, method: str, alpha, min_f):
    """the levels of ``change_points`` over ``run(x (T, s M), mask (s M) or None, window (2, s M)) -> (25, s M)`` planes:
    (count (M), index (max_breaks, M)).  Torch ops on the device of ``x2`` throughout."""
    _, index_map, stat_map = _METHODS[method]
    dev = x2.device
    t_len, m = x2.shape
    ki, ks = MAPS.index(index_map), MAPS.index(stat_map)
    begin = torch.zeros((1, m), device=dev, dtype=torch.int32)        # the open segments [begin, end) of every pixel,
    end = torch.full((1, m), t_len, device=dev, dtype=torch.int32)     # closed ones are empty (0, 0)
    count = torch.zeros(m, device=dev, dtype=torch.int64)
    found = []                                                         # per level: the accepted breaks, t_len elsewhere
    for _ in range(int(max_breaks)):
        s = begin.shape[0]
        window = torch.stack((begin.reshape(-1), end.reshape(-1)))
        out = run(x2 if s == 1 else x2.repeat(1, s), None if mask is None else mask.repeat(s), window)
        idx = out[ki].reshape(s, m).to(torch.int64)
        stat = out[ks].reshape(s, m)
        if method == "pettitt":
            split, score = (stat < alpha) & (idx >= 0), -stat
        else:
            split, score = (stat >= min_f) & (idx >= 0), stat
        score = torch.where(split, score, torch.full_like(score, -float("inf")))
        order = torch.argsort(score, dim=0, descending=True, stable=True)
        rank = torch.empty_like(order).scatter_(0, order, torch.arange(s, device=dev).unsqueeze(1).expand(s, m))
        take = split & (rank < (int(max_breaks) - count).unsqueeze(0))
        if not bool(take.any()):
            break
        count += take.sum(0)
        found.append(torch.where(take, idx, torch.full_like(idx, t_len)))
        cut = (idx + 1).to(torch.int32)
        zero = torch.zeros_like(begin)
        kids_b = torch.stack((torch.where(take, begin, zero), torch.where(take, cut, zero)), 1).reshape(2 * s, m)
        kids_e = torch.stack((torch.where(take, cut, zero), torch.where(take, end, zero)), 1).reshape(2 * s, m)
        keep = min(2 * s, int(max_breaks) + 1)                         # a pixel never has more open segments than that
        front = torch.argsort((kids_e <= kids_b).to(torch.int8), dim=0, stable=True)[:keep]
        begin, end = torch.gather(kids_b, 0, front), torch.gather(kids_e, 0, front)
    if found:
        allb = torch.sort(torch.cat(found, 0), dim=0).values
        pad = max(0, int(max_breaks) - allb.shape[0])
        if pad:
            allb = torch.cat((allb, torch.full((pad, m), t_len, device=dev, dtype=torch.int64)), 0)
        index = allb[:int(max_breaks)]
        index = torch.where(index >= t_len, torch.full_like(index, -1), index)
    else:
        index = torch.full((int(max_breaks), m), -1, device=dev, dtype=torch.int64)
    return count, index
