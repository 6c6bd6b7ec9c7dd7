"""At which spatial scale does the downscaled field put its droughts where GRACE puts them?  Neighbourhood verification on
the device: the fractions skill score (FSS) of Roberts & Lean 2008 (Mon. Wea. Rev. 136).

Both fields are thresholded (``x <= thr`` by default, the drought convention), the *fraction* of event pixels in an n x n
window around every pixel is compared, and the smallest n from which the score stays above ``0.5 + f0 / 2`` (f0 the observed
base rate) is the scale at which the product is useful.  A sharp field with a feature displaced by a few pixels is not
punished twice, as it is by pointwise scores and by ``drought.compare_events``.

* ``fractions_skill_score``: the score per step, threshold and scale, pooled over time, with base rates, frequency bias, the
  random and uniform reference scores, ``useful_scale`` and, with ``maps=True``, local score maps;
* ``neighborhood_fraction``: the fraction field of one cube, for plotting;
* ``fss_cross_grid``: a coarse cube against a fine one, the coarse cube replicated onto the fine grid;
* ``drought_fss``: two drought-index cubes at the D0 .. D4 class thresholds of ``drought.DSI_CLASSES``.

Definitions.  A pixel is valid where the mask is nonzero and neither field is NaN; a NaN is never an event and removes the
pixel from both fields.  cf, co, cv are the counts of forecast events, observed events and valid pixels in the window, which
is clipped at the domain edge (positions outside count zero).  The sums run over the valid centre pixels.
``normalize="window"`` (Roberts & Lean's zero padding) uses the fractions c / n^2; the n^4 cancels, so the record is three
integers A = sum (cf - co)^2, B = sum cf^2, C = sum co^2 and FSS = 1 - A / (B + C) is formed from exact integers: the record
does not depend on the order of summation and equals an independent computation bit for bit.  ``normalize="valid"`` uses
cf / cv and co / cv, which removes the edge and mask bias, in fp64 sums of a fixed order.  Pooled scores are sums of
numerators over sums of denominators, not means of ratios.

The kernels are ``csrc/neighborhood.hip`` over ``csrc/neighborhood_core.h`` (``include/gandanet.h``, "Neighbourhood
verification"): one summed-area table per step and threshold whose 64-bit words pack the three counts, four corner loads per
window, no atomics.  fp32 or fp64 CUDA tensors; there is no CPU path in this module (``kern.nbr_*_host`` are the plain C++
twins the tests use); torch allocates, views and copies, and the records cross to the host once per call.

Out of scope: percentile thresholds computed inside the call (pass per-step threshold tables, ``(T, K)``, one per field);
continuous "upscaled" scores from fp64 tables of the values; periodic longitude; non-square or even windows; H W > 2^20.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import kern as K
from .drought import DSI_CLASSES
from .timeseries import _series_mask

Tensor = torch.Tensor
L = K.L

DEFAULT_SCALES = (1, 3, 5, 9, 17, 33, 65, 129)


def _ratio(num, den):
    """num / den, NaN where den = 0; integer records are divided as exact integers, one rounding each"""
    num, den = np.asarray(num), np.asarray(den)
    if num.dtype.kind in "ui" and den.dtype.kind in "ui":
        flat = [a / b if b else float("nan") for a, b in zip(num.reshape(-1).tolist(), den.reshape(-1).tolist())]
        return np.array(flat, dtype=np.float64).reshape(num.shape)
    num, den = num.astype(np.float64), den.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


class FSSResult:
    """the records of ``fractions_skill_score`` on the host and what follows from them.

    ``sums`` (T, K, S, 3): A, B, C per step, threshold and scale -- uint64 with ``normalize="window"``, fp64 with ``"valid"``;
    ``base`` (T, K, 3) uint64: the forecast events, the observed events and the valid pixels of every step; ``scales`` (S,);
    ``thresholds`` and ``thresholds_observed`` (T, K); ``maps`` (K, S, H, W, 3) on the device or None."""

    def __init__(self, sums, base, scales, thresholds, thresholds_observed, normalize: str, maps: Optional[Tensor]):
        self.sums, self.base, self.scales = sums, base, tuple(int(n) for n in scales)
        self.thresholds, self.thresholds_observed, self.normalize, self.maps = thresholds, thresholds_observed, normalize, maps

    @staticmethod
    def _score(rec):
        """1 - A / (B + C) along the last axis, NaN where B + C = 0; integer records are added exactly first"""
        return 1.0 - _ratio(rec[..., 0], rec[..., 1] + rec[..., 2])

    @property
    def fss(self):
        """(T, K, S)"""
        return self._score(self.sums)

    @property
    def pooled(self):
        """(K, S): the sums of numerators and of denominators over time"""
        return self._score(self.sums.sum(axis=0))

    @property
    def base_rate_forecast(self):
        """(K,): forecast events over valid pixels, pooled over time"""
        b = self.base.sum(axis=0)
        return _ratio(b[:, 0], b[:, 2])

    @property
    def base_rate_observed(self):
        b = self.base.sum(axis=0)
        return _ratio(b[:, 1], b[:, 2])

    @property
    def frequency_bias(self):
        """(K,): forecast events over observed events"""
        b = self.base.sum(axis=0)
        return _ratio(b[:, 0], b[:, 1])

    @property
    def fss_random(self):
        """(K,): the score of a random forecast with the observed base rate, f_o"""
        return self.base_rate_observed

    @property
    def fss_uniform(self):
        """(K,): 0.5 + f_o / 2, the score of a uniform forecast of the base rate: the target of a useful scale"""
        return 0.5 + self.base_rate_observed / 2.0

    def useful_scale(self, k: int) -> Optional[int]:
        """the first scale from which the pooled score of threshold ``k`` stays >= ``fss_uniform`` (the first sustained
        crossing, as ``spectra.effective_resolution`` reads its ratio), or None"""
        ok = self.pooled[k] >= self.fss_uniform[k]    # False for NaN
        first = None
        for s in range(len(self.scales) - 1, -1, -1):
            if not ok[s]:
                break
            first = self.scales[s]
        return first

    def fss_map(self, k: int, s: int) -> Tensor:
        """(H, W) fp64 on the device: the score of every centre pixel over time, NaN where B + C = 0"""
        if self.maps is None:
            raise L.GandanetError("fss_map: call fractions_skill_score with maps=True")
        m = self.maps[k, s]
        den = (m[..., 1] + m[..., 2]).to(torch.float64)
        return torch.where(den > 0, 1.0 - m[..., 0].to(torch.float64) / den, torch.full_like(den, float("nan")))


def _pair(fn: str, forecast, observed):
    for t, nm in ((forecast, "forecast"), (observed, "observed")):
        if not isinstance(t, Tensor) or not t.is_cuda:
            raise L.GandanetError(f"{fn}: {nm} must be a GPU tensor (there is no CPU path)")
        if t.dtype not in (torch.float32, torch.float64) or t.dim() != 3 or t.numel() == 0:
            raise L.GandanetError(f"{fn}: {nm} is a non-empty float32 / float64 (T, H, W) cube, got {t.dtype} {tuple(t.shape)}")
    if forecast.shape != observed.shape or forecast.dtype != observed.dtype:
        raise L.GandanetError(f"{fn}: forecast {tuple(forecast.shape)} {forecast.dtype} against observed "
                              f"{tuple(observed.shape)} {observed.dtype}: one grid and one dtype")
    return forecast.contiguous(), observed.contiguous()


def fractions_skill_score(forecast: Tensor, observed: Tensor, thresholds, scales: Sequence[int] = DEFAULT_SCALES, *,
                          thresholds_observed=None, below: bool = True, mask: Optional[Tensor] = None, normalize: str = "window",
                          maps: bool = False) -> FSSResult:
    """the fractions skill score of ``forecast`` against ``observed``, (T, H, W) cubes of one dtype on one grid.

    ``thresholds``: K <= 8 numbers, or a (T, K) table of per-step thresholds (how percentile thresholds are passed);
    ``thresholds_observed``: the same for the observed field (default: ``thresholds``).  ``scales``: S <= 32 odd window
    widths in pixels; a window wider than the domain is the whole domain.  ``below``: the event is ``x <= thr`` (else
    ``x >= thr``).  ``mask`` (H, W), nonzero = use the pixel.  ``normalize``: ``"window"`` or ``"valid"`` (module docstring).
    ``maps=True`` also accumulates the sums over time per centre pixel (``FSSResult.fss_map``)."""
    f, o = _pair("fractions_skill_score", forecast, observed)
    T, H, W = f.shape
    thr_f = K._nbr_thresholds(thresholds, T, "fractions_skill_score thresholds")
    thr_o = thr_f if thresholds_observed is None else K._nbr_thresholds(thresholds_observed, T, "fractions_skill_score thresholds_observed")
    sums, base, out = K.nbr_fss(f, o, thr_f, thr_o, scales, below, normalize, maps, _series_mask(mask, (H, W), f.device))
    rec = torch.cat([sums.reshape(-1).view(torch.int64), base.reshape(-1)]).cpu().numpy()     # the one crossing to the host
    n = sums.numel()
    host_sums = rec[:n].view(np.float64 if normalize == "valid" else np.uint64).reshape(tuple(sums.shape))
    return FSSResult(host_sums, rec[n:].view(np.uint64).reshape(tuple(base.shape)), K._nbr_scales(scales), thr_f, thr_o, normalize, out)


def neighborhood_fraction(x: Tensor, threshold, scale: int, below: bool = True, mask: Optional[Tensor] = None,
                          normalize: str = "window") -> Tensor:
    """the (T, H, W) fp64 field of the fraction of event pixels of ``x`` in the ``scale`` x ``scale`` window around every
    pixel: count / scale^2 (``"window"``) or count / valid pixels of the window (``"valid"``); NaN at an invalid centre (a
    NaN of ``x`` or a masked pixel).  ``threshold``: one number, or one per step."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise L.GandanetError("neighborhood_fraction: expected a GPU tensor (there is no CPU path)")
    if x.dim() != 3:
        raise L.GandanetError(f"neighborhood_fraction: expected a (T, H, W) cube, got {tuple(x.shape)}")
    x = x.contiguous()
    return K.nbr_fraction(x, threshold, scale, below, normalize, _series_mask(mask, tuple(x.shape[1:]), x.device))


def fss_cross_grid(hi: Tensor, lo: Tensor, factor: int, thresholds, scales: Sequence[int] = DEFAULT_SCALES, *, hi_is_forecast: bool = True,
                   **kwargs) -> FSSResult:
    """``hi`` (T, H, W) against the coarse ``lo`` (T, H / factor, W / factor): every coarse pixel is replicated onto its
    ``factor`` x ``factor`` fine pixels (``repeat_interleave``) and the score is taken on the fine grid, ``scales`` in fine
    pixels.  ``hi`` is the forecast unless ``hi_is_forecast=False``; the keywords are those of ``fractions_skill_score``."""
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or factor < 1:
        raise L.GandanetError(f"fss_cross_grid: factor is an integer >= 1, got {factor!r}")
    for t in (hi, lo):
        if not isinstance(t, Tensor) or not t.is_cuda or t.dim() != 3:
            raise L.GandanetError("fss_cross_grid: expected (T, H, W) GPU tensors (there is no CPU path)")
    if (lo.shape[0], lo.shape[1] * factor, lo.shape[2] * factor) != tuple(hi.shape):
        raise L.GandanetError(f"fss_cross_grid: {tuple(lo.shape)} times {factor} is not {tuple(hi.shape)}")
    fine = lo.repeat_interleave(int(factor), dim=1).repeat_interleave(int(factor), dim=2)
    a, b = (hi, fine) if hi_is_forecast else (fine, hi)
    return fractions_skill_score(a, b, thresholds, scales, **kwargs)


def drought_fss(index_a: Tensor, index_b: Tensor, classes: Sequence[float] = DSI_CLASSES, scales: Sequence[int] = DEFAULT_SCALES,
                **kwargs) -> FSSResult:
    """the score of the drought-index cube ``index_a`` (the product) against ``index_b`` (the reference, GRACE) at the class
    thresholds of ``drought.py``: drought where the index is <= the class threshold"""
    return fractions_skill_score(index_a, index_b, tuple(float(c) for c in classes), scales, below=True, **kwargs)
