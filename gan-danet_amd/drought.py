"""Where, when, how long and how severe were the droughts, and does the downscaled product see the same ones as GRACE?
The drought and water-storage-deficit analysis of a TWSA cube, on the device:

* ``climatology``: the calendar climatology (n, mean, M2 per month and pixel) over a baseline period;
* ``drought_index``: the water storage deficit ``x - mean`` of Thomas et al. 2014 (``"anomaly"``), the standardised
  GRACE-DSI of Zhao et al. 2017 (``"standardized"``), and two non-parametric indices from the midrank of a sample among the
  baseline samples of its calendar month: the Gringorten probability (``"percentile"``) and its normal quantile
  (``"empirical"``, the SPI-style standardised index);
* ``drought_events``: the events of run theory (runs of at least ``min_duration`` steps at or below a threshold) and their
  maps -- number, duration, severity, peak, start of the longest and of the worst, the run still open at the end;
* ``drought_area``: the (area-weighted) share of every zone's valid pixels in drought at every step, per threshold
  (``DSI_CLASSES`` are the D0 .. D4 classes of Zhao et al.);
* ``compare_events``: per-pixel hits, misses and false alarms of two products' event steps.

The kernels are ``csrc/drought.hip`` over ``csrc/drought_core.h`` (``include/gandanet.h``, "Drought analysis"): fp32 or fp64
CUDA tensors, time along axis 0 (T <= 2048), all arithmetic fp64, one thread per series walking t in ascending order, no
atomics (the same bits on every run, whatever the number of series).  Nothing transcendental runs on the device: the rank
indices read a table built here on the host.  There is no CPU path in this module (``kern.drought_*_host`` are the plain
C++ twins the tests use).  torch allocates, views and copies.
"""
from __future__ import annotations

import functools
import statistics
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kern as K
from .basins import ZoneMap
from .basins import zone_mean as _zone_mean
from .timeseries import _cube, _series_mask

Tensor = torch.Tensor
L = K.L

MAPS = L.DROUGHT_EV_MAPS
DSI_CLASSES = (-0.5, -0.8, -1.3, -1.6, -2.0)     # D0 .. D4 of Zhao et al. 2017: drought where DSI <= the class threshold
KINDS = ("standardized", "anomaly", "percentile", "empirical")


def _calendar(fn: str, t_len: int, period, phase, baseline) -> Tuple[int, int, int, int]:
    for v, nm in ((period, "period"), (phase, "phase")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise L.GandanetError(f"{fn}: {nm} must be an integer, got {v!r}")
    if not 1 <= period <= L.DROUGHT_MAX_PERIOD or not 0 <= phase < period:
        raise L.GandanetError(f"{fn}: 1 <= period <= {L.DROUGHT_MAX_PERIOD} and 0 <= phase < period, got {period}, {phase}")
    if t_len > L.DROUGHT_MAX_T:
        raise L.GandanetError(f"{fn}: T <= {L.DROUGHT_MAX_T}, got T = {t_len}")
    b0, b1 = (0, t_len) if baseline is None else (int(baseline[0]), int(baseline[1]))
    if not 0 <= b0 < b1 <= t_len:
        raise L.GandanetError(f"{fn}: the baseline is a half-open step range inside [0, {t_len}], got {baseline!r}")
    return int(period), int(phase), b0, b1


class DroughtClimatology:
    """n, mean and M2 (the sum of squared deviations) of every calendar slot and pixel over the baseline: ``rec`` is the
    (3, period, ...) fp64 record of ``gd_drought_clim``; slot of step t = (t + ``phase``) mod ``period``; ``baseline`` is
    the half-open step range it was taken over."""

    def __init__(self, rec: Tensor, period: int, phase: int, baseline: Tuple[int, int]):
        self.rec, self.period, self.phase, self.baseline = rec, int(period), int(phase), (int(baseline[0]), int(baseline[1]))

    @property
    def n(self) -> Tensor:
        return self.rec[0]

    @property
    def mean(self) -> Tensor:
        return self.rec[1]

    def std(self, ddof: int = 0) -> Tensor:
        """sqrt(M2 / (n - ddof)) per slot and pixel, NaN where n - ddof <= 0"""
        dof = self.rec[0] - float(ddof)
        return torch.where(dof > 0, torch.sqrt(self.rec[2] / dof), torch.full_like(dof, float("nan")))


def climatology(x: Tensor, period: int = 12, phase: int = 0, baseline: Optional[Tuple[int, int]] = None,
                mask: Optional[Tensor] = None) -> DroughtClimatology:
    """the calendar climatology of every series ``x[:, ...]``: step t belongs to slot (t + ``phase``) mod ``period``;
    ``baseline`` = (b0, b1) restricts it to the steps b0 <= t < b1 (default: the whole record); NaN samples are left out.
    ``mask`` (bool or uint8, the shape of one time step, nonzero = use the pixel) leaves pixels out (n = 0, NaN)."""
    x = _cube(x, "climatology")
    t_len, tail = x.shape[0], tuple(x.shape[1:])
    period, phase, b0, b1 = _calendar("climatology", t_len, period, phase, baseline)
    rec = K.drought_clim(x.reshape(t_len, -1), period, phase, b0, b1, _series_mask(mask, tail, x.device))
    return DroughtClimatology(rec.reshape((3, period) + tail), period, phase, (b0, b1))


@functools.lru_cache(maxsize=8)
def rank_table(kind: str, nmax: int) -> np.ndarray:
    """the (nmax, nmax) flattened table of ``gd_drought_rank``: entry (n - 1)^2 + (k - 1), 1 <= k <= 2 n - 1, is the
    Gringorten plotting position p = ((k + 1) / 2 - 0.44) / (n + 0.12) of the midrank (k + 1) / 2 among n samples
    (``"percentile"``) or the standard normal quantile of p (``"empirical"``)"""
    if kind not in ("percentile", "empirical"):
        raise L.GandanetError(f"rank_table: kind is 'percentile' or 'empirical', got {kind!r}")
    if not 1 <= nmax <= L.DROUGHT_MAX_N:
        raise L.GandanetError(f"rank_table: 1 <= nmax <= {L.DROUGHT_MAX_N}, got {nmax}")
    inv = statistics.NormalDist().inv_cdf
    table = np.empty(nmax * nmax)
    for n in range(1, nmax + 1):
        for k in range(1, 2 * n):
            p = ((k + 1) / 2 - 0.44) / (n + 0.12)
            table[(n - 1) ** 2 + (k - 1)] = p if kind == "percentile" else inv(p)
    table.setflags(write=False)
    return table


def drought_index(x: Tensor, kind: str = "standardized", clim: Optional[DroughtClimatology] = None, period: int = 12, phase: int = 0,
                  baseline: Optional[Tuple[int, int]] = None, ddof: int = 0, mask: Optional[Tensor] = None) -> Tensor:
    """a drought index of every series ``x[:, ...]``, a cube of the shape and dtype of ``x``.

    ``"anomaly"``: x - mean of the sample's calendar slot (the water storage deficit where negative);
    ``"standardized"``: that over the slot's standard deviation sqrt(M2 / (n - ``ddof``)) -- the GRACE-DSI; NaN for a slot
    with n - ddof <= 0 or without variance.  Both take ``clim`` (a ``DroughtClimatology``, for instance GRACE's own baseline)
    or compute it from ``x`` with ``period``, ``phase``, ``baseline``, ``mask``.
    ``"percentile"``: the Gringorten probability ((k + 1) / 2 - 0.44) / (n + 0.12) of the sample's midrank (k + 1) / 2
    among the n baseline samples of its slot (the sample itself joins them when it lies outside the baseline);
    ``"empirical"``: the standard normal quantile of that probability.  Both need at most 256 baseline samples per slot.
    A NaN sample, an empty slot and a masked pixel give NaN."""
    x = _cube(x, "drought_index")
    if kind not in KINDS:
        raise L.GandanetError(f"drought_index: kind is one of {KINDS}, got {kind!r}")
    t_len, tail = x.shape[0], tuple(x.shape[1:])
    m = _series_mask(mask, tail, x.device)
    x2 = x.reshape(t_len, -1)
    if kind in ("percentile", "empirical"):
        if clim is not None:
            raise L.GandanetError(f"drought_index: kind {kind!r} ranks against the samples themselves and takes no climatology")
        period, phase, b0, b1 = _calendar("drought_index", t_len, period, phase, baseline)
        nmax = -(-(b1 - b0) // period) + 1
        if nmax > L.DROUGHT_MAX_N:
            raise L.GandanetError(f"drought_index: {nmax - 1} baseline steps per slot, the rank indices take at most {L.DROUGHT_MAX_N - 1}")
        table = torch.from_numpy(rank_table(kind, nmax).copy()).to(x.device)
        return K.drought_rank(x2, table, period, phase, b0, b1, m).reshape(x.shape)
    if ddof not in (0, 1):
        raise L.GandanetError(f"drought_index: ddof is 0 or 1, got {ddof!r}")
    if clim is None:
        clim = climatology(x, period, phase, baseline, mask)
    elif not isinstance(clim, DroughtClimatology) or tuple(clim.rec.shape[2:]) != tail:
        raise L.GandanetError(f"drought_index: clim is a DroughtClimatology of pixels {tail}")
    rec = clim.rec.reshape(3, clim.period, -1)
    code = L.DROUGHT_ANOMALY if kind == "anomaly" else L.DROUGHT_STANDARDIZED
    return K.drought_index(x2, rec if rec.is_contiguous() else rec.contiguous(), clim.phase, code, int(ddof), m).reshape(x.shape)


class DroughtEvents:
    """the maps of ``drought_events``: ``maps`` (name -> fp64 tensor of the shape of one time step), also as attributes
    (``ev.n_events``; a map that was not asked for is None); ``in_event`` (T, ...) uint8 or None; ``threshold``,
    ``min_duration``"""

    def __init__(self, maps: Dict[str, Tensor], in_event: Optional[Tensor], threshold: float, min_duration: int):
        self.maps, self.in_event, self.threshold, self.min_duration = maps, in_event, float(threshold), int(min_duration)

    def __getattr__(self, name: str):
        if name in MAPS:
            return self.__dict__["maps"].get(name)
        raise AttributeError(name)

    def __getitem__(self, name: str) -> Tensor:
        return self.maps[name]


def drought_events(index: Tensor, threshold: float = -0.8, min_duration: int = 3, maps: Sequence[str] = MAPS,
                   return_steps: bool = False, mask: Optional[Tensor] = None) -> DroughtEvents:
    """run theory on every series ``index[:, ...]``: a step is dry when its value is <= ``threshold`` (a NaN step is not,
    and ends a run); an event is a maximal run of at least ``min_duration`` consecutive dry steps (3 after Thomas et al.
    2014); its severity is the sum of ``threshold`` - value over its steps.  ``maps`` names any of ``MAPS``: n_valid, n_dry,
    n_events, event_steps, max_duration, mean_duration, max_severity, total_severity, peak (the smallest value inside
    events), longest_start and worst_start (step numbers, -1 without events), last_run (the length of the run still open at
    the last step, whatever ``min_duration``).  ``return_steps`` adds ``in_event``, a uint8 cube with 1 on the steps of
    events."""
    index = _cube(index, "drought_events")
    t_len, tail = index.shape[0], tuple(index.shape[1:])
    if t_len > L.DROUGHT_MAX_T:
        raise L.GandanetError(f"drought_events: T <= {L.DROUGHT_MAX_T}, got T = {t_len}")
    if isinstance(min_duration, bool) or not isinstance(min_duration, (int, np.integer)) or min_duration < 1:
        raise L.GandanetError(f"drought_events: min_duration is an integer >= 1, got {min_duration!r}")
    threshold = float(threshold)
    if threshold != threshold:
        raise L.GandanetError("drought_events: the threshold is NaN")
    out, steps = K.drought_events(index.reshape(t_len, -1), threshold, int(min_duration), maps, _series_mask(mask, tail, index.device),
                                  want_steps=return_steps)
    names = [nm for nm in MAPS if nm in set(maps)]
    return DroughtEvents({nm: out[i].reshape(tail) for i, nm in enumerate(names)}, None if steps is None else steps.reshape(index.shape),
                         threshold, min_duration)


def drought_area(index: Tensor, thresholds: Sequence[float] = DSI_CLASSES, zonemap: Optional[ZoneMap] = None,
                 weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``(fraction (T, Z, K) fp64, count (T, Z) int64)``: at every step, the share of each zone's valid (not NaN) pixels of
    ``index`` (T, H, W) whose value is <= ``thresholds[k]``, and the number of those valid pixels.  ``weights`` (H, W), for
    instance cos(lat), makes it the share of the area.  Without a ``zonemap`` the whole domain is the one zone (and
    ``index`` may be any (T, ...)).  One indicator pass (``gd_drought_exceed``) and one ``gd_zone_mean`` per threshold over
    one reused buffer; a zone without a valid pixel gives NaN and 0."""
    index = _cube(index, "drought_area")
    ks = [float(t) for t in (thresholds if isinstance(thresholds, (tuple, list, np.ndarray)) else (thresholds,))]
    if not ks or any(t != t for t in ks):
        raise L.GandanetError(f"drought_area: the thresholds are a non-empty sequence of numbers, got {thresholds!r}")
    if index.dim() == 1:
        index = index.reshape(-1, 1)
    if weights is not None:
        if not isinstance(weights, Tensor) or not weights.is_cuda:
            raise L.GandanetError("drought_area: weights must be a GPU tensor (there is no CPU path)")
        weights = weights.to(torch.float64).contiguous()
    if zonemap is None:
        bits = torch.ones(index.shape[1:], device=index.device, dtype=torch.int32).view(torch.uint32)
        if weights is not None and weights.shape != bits.shape:
            raise L.GandanetError(f"drought_area: weights {tuple(weights.shape)} for pixels {tuple(bits.shape)}")
    buf = torch.empty_like(index)
    fractions, count = [], None
    for thr in ks:
        K.drought_exceed(index, thr, out=buf)
        mean, count = K.zone_mean(buf, bits, 1, weights) if zonemap is None else _zone_mean(buf, zonemap, weights)
        fractions.append(mean)
    return torch.stack(fractions, dim=-1), count


class EventComparison(NamedTuple):
    hits: Tensor
    misses: Tensor
    false_alarms: Tensor


def compare_events(a: Tensor, b: Tensor) -> EventComparison:
    """two ``in_event`` cubes (T, ...) uint8 on one grid, ``a`` the reference (GRACE) and ``b`` the product: per pixel, the
    steps both have in an event (hits), those only ``a`` has (misses) and those only ``b`` has (false alarms), int64"""
    for t in (a, b):
        if not isinstance(t, Tensor) or not t.is_cuda:
            raise L.GandanetError("compare_events: expected GPU tensors (there is no CPU path)")
        if t.dtype != torch.uint8:
            raise L.GandanetError(f"compare_events: expected uint8 in_event cubes, got {t.dtype}")
    if a.shape != b.shape or a.dim() == 0:
        raise L.GandanetError(f"compare_events: two cubes of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    ea, eb = a != 0, b != 0
    return EventComparison((ea & eb).sum(dim=0), (ea & ~eb).sum(dim=0), (~ea & eb).sum(dim=0))
