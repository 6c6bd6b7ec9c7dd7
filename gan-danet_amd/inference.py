"""Forward-only consumer of the generator: the device side of ``test.ipynb``'s ``predict_and_plot`` loop body
(c1:123-171) -- SURVEY.md row f3.  File formats (HDF5 / NetCDF), masks, scalers and plots stay in the caller's
Python; what runs per batch on the GPU is here:

    xin  = cat([lr_grace_025, aux], 1)                                   c1:154   (torch.cat: a copy, plumbing)
    yhat = model(xin)                       eval-mode generator          c1:157   (180 x 88 tiles: PAM over 15 840 tokens)
    yhat = F.interpolate(yhat, scale_factor=1.25, mode='bicubic')        c1:158   -> ``bicubic_resize``
    yhat = apply_mild_histogram_matching(yhat, lr_grace_025, weight)     c1:161   -> ``mild_histogram_matching``
    hr_grace = F.interpolate(lr_grace_025, scale_factor=4, 'bicubic')    c1:164   -> ``bicubic_resize``
    yhat = smooth_blend(yhat, hr_grace, region)                          c1:165   -> ``smooth_blend``
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np
import torch

from . import kern as K
from . import ops


def bicubic_resize(x: torch.Tensor, scale_factor: float) -> torch.Tensor:
    """``F.interpolate(x, scale_factor=s, mode='bicubic', align_corners=False)``: output size floor(in * s), source
    coordinate (dst + 0.5) / s - 0.5, A = -0.75, border-clamped taps (differentiable: ``ops.BicubicFn``)"""
    Ho, Wo = int(math.floor(x.shape[2] * scale_factor)), int(math.floor(x.shape[3] * scale_factor))
    return ops.BicubicFn.apply(x, Ho, Wo, 1.0 / scale_factor, 1.0 / scale_factor)


def blend_mask(region: Sequence[int], sigma: int = 5) -> np.ndarray:
    """the feathered window of ``smooth_blend`` (c1:92-97): ramps of width ``sigma`` on the four edges, then a Gaussian
    filter -- a host-side constant of the region's size, built with the calls the notebook makes"""
    from scipy.ndimage import gaussian_filter
    sr, er, sc, ec = region
    mask = np.ones((er - sr, ec - sc), dtype=float)
    mask[0:sigma, :] = np.linspace(0, 1, sigma)[:, None]
    mask[-sigma:, :] = np.linspace(1, 0, sigma)[:, None]
    mask[:, 0:sigma] = np.maximum(mask[:, 0:sigma], np.linspace(0, 1, sigma)[None, :])
    mask[:, -sigma:] = np.maximum(mask[:, -sigma:], np.linspace(1, 0, sigma)[None, :])
    return gaussian_filter(mask, sigma=sigma)


@torch.no_grad()
def smooth_blend(hr_generated: torch.Tensor, hr_grace: torch.Tensor, region: Sequence[int], sigma: int = 5) -> torch.Tensor:
    """c1:87-101: feather ``hr_grace`` into ``hr_generated`` over ``region`` = (row0, row1, col0, col1), IN PLACE on
    ``hr_generated`` as the notebook does; one launch (``gd_blend_region``)"""
    mask = torch.from_numpy(blend_mask(region, sigma)).to(dtype=torch.float32, device=hr_generated.device).contiguous()
    return K.blend_region(hr_generated, hr_grace.contiguous(), mask, region)


def mild_histogram_matching(hr_generated: torch.Tensor, lr_grace_025: torch.Tensor, weight: float = 0.0) -> torch.Tensor:
    """c1:69-85 ``apply_mild_histogram_matching``: per sample, ``(1 - weight) * source + weight * matched`` where
    ``matched`` maps the sample's empirical CDF onto the reference field's (np.unique / np.interp semantics).  The
    notebook calls it with ``weight = 0.0`` (c1:161), where the result IS the source: that case returns the input
    untouched.  Otherwise one launch sequence per sample (``gd_hist_match``: radix sorts + a quantile-interpolation
    kernel); the result is float64, as the notebook's numpy code returns.  CPU tensors go to the host twin of that kernel
    and give the same bits.

    A NaN in ``hr_generated`` propagates to its own position only: the result is NaN there, and for the other elements it
    ranks above every number (all NaNs sort last whatever their sign bit, as numpy sorts them).  Non-finite values in
    ``lr_grace_025`` are outside the contract: np.interp's own rules for them differ between numpy versions, so they are
    not tested."""
    if weight == 0.0:
        return hr_generated
    return K.hist_match(hr_generated.contiguous(), lr_grace_025.contiguous(), weight)


@torch.no_grad()
def predict_batch(model: torch.nn.Module, lr_grace_025: torch.Tensor, aux: torch.Tensor,
                  region: Tuple[int, int, int, int] = (0, 90, 0, 44), upscale: float = 1.25, hist_weight: float = 0.0,
                  blend_with: float = 4.0) -> torch.Tensor:
    """one iteration of the loader loop of ``predict_and_plot`` (c1:149-167) on the device.  As in the notebook the blend
    target is the x4 bicubic of ``lr_grace_025`` and the blend happens on the x1.25 image, so ``region`` must lie inside
    both."""
    xin = torch.cat([lr_grace_025, aux], dim=1)                          # layout copy
    yhat = bicubic_resize(model(xin), upscale)
    yhat = mild_histogram_matching(yhat, lr_grace_025, hist_weight)
    if yhat.dtype != torch.float32:          # the notebook continues in float64 from here; the blend kernel is fp32
        yhat = yhat.float()
    hr_grace = bicubic_resize(lr_grace_025, blend_with)
    sr, er, sc, ec = region
    if yhat.shape == hr_grace.shape:
        return smooth_blend(yhat, hr_grace, region)
    # the notebook slices both images with the same indices (c1:90-91): images of different size share the corner
    mask = torch.from_numpy(blend_mask(region)).to(dtype=torch.float32, device=yhat.device).contiguous()
    patch = hr_grace[:, :, sr:er, sc:ec].contiguous()
    canvas = yhat[:, :, sr:er, sc:ec].contiguous()
    K.blend_region(canvas, patch, mask, (0, er - sr, 0, ec - sc))
    yhat[:, :, sr:er, sc:ec] = canvas                                     # slice copy (plumbing)
    return yhat


# ---- behind the loader loop: test.ipynb cell 3, after the `with torch.no_grad()` loop -----------------------------------
def _mask_u8(mask, shape) -> torch.Tensor:
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise K.L.GandanetError("mask: expected a GPU tensor (there is no CPU path)")
    if tuple(mask.shape) != tuple(shape):
        raise K.L.GandanetError(f"mask: expected the product's plane {tuple(shape)}, got {tuple(mask.shape)}")
    return (mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)).contiguous()


@torch.no_grad()
def restore_units(res: torch.Tensor, trend=None, scale: float = 1.0, mean: float = 0.0, unit: float = 1.0, mask=None,
                  out_dtype=torch.float64, out=None) -> torch.Tensor:
    """``((res + trend) * scale + mean) * unit`` in one launch (``gd_restore_units``): the notebook's ``res + trend_ups``,
    ``scaler025.inverse_transform`` (a StandardScaler with one feature: ``* scale_ + mean_``) and ``* 10.0``.  Evaluated
    in fp64 in that order, every operation rounded, so an fp64 result equals numpy's bit for bit.  ``mask`` (the shape of
    res's trailing dims; 0 = outside) gives NaN there.  ``out=res`` works in place when ``res`` already has
    ``out_dtype``."""
    for t, name in ((res, "res"), (trend, "trend")):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise K.L.GandanetError(f"restore_units: {name} must be a GPU tensor (there is no CPU path)")
    res = res if res.is_contiguous() else res.contiguous()
    if trend is not None and not trend.is_contiguous():
        trend = trend.contiguous()
    if mask is not None:
        mask = _mask_u8(mask, res.shape[res.dim() - mask.dim():])
    if out is None:
        out = torch.empty(res.shape, device=res.device, dtype=out_dtype)
    return K.restore_units(res, trend, mask, scale, mean, unit, out)


@torch.no_grad()
def zoom_mask(mask: torch.Tensor, factor) -> torch.Tensor:
    """``zoom(mask, factor, order=1) != 0`` as uint8: the notebooks' ``tpbh_hi = zoom(tpbh, (5, 5), order=1)`` and ``tpbl =
    zoom(tpbl, (2, 2), order=1)`` with the comparison they are used in"""
    from . import spline
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise K.L.GandanetError("zoom_mask: expected a GPU tensor (there is no CPU path)")
    m = mask if mask.dtype in (torch.float32, torch.float64) else mask.to(torch.float64)
    return (spline.zoom(m, factor, order=1) != 0).to(torch.uint8)


@torch.no_grad()
def assemble_product(res: torch.Tensor, trend25: torch.Tensor, scale: float, mean: float, *, trend_zoom=(1, 5, 5),
                     unit: float = 10.0, mask=None, bias=None, bias_zoom=(1, 1.25, 1.25), uncertainty=None,
                     uncertainty_zoom=(1, 5, 5), quantile_map=None, quantile_kind: str = "eqm") -> dict:
    """the post-loop chain of test.ipynb cell 3 on the device, from the stacked tiles ``res`` (T, H, W) to the product:

        trend_ups = zoom(trend25, trend_zoom, order=3)          res = res + trend_ups
        res_cm = scaler.inverse_transform(res) * unit           (scale, mean: the scaler's scale_ and mean_)
        res_cm = quantile_map.apply(res_cm, quantile_kind)      (quantile_map given: a biascorrect.QuantileMap; not in
                                                                 the notebook, whose only corrections are bias and the
                                                                 global histogram match)
        res_cm[:, mask == 0] = nan                              (mask: (H, W), at product resolution)
        series = np.nanmean(res_cm, axis=(1, 2))
        product = res_cm + zoom(bias, bias_zoom, order=3)       (bias given)
        unc = zoom(uncertainty, uncertainty_zoom, order=0, mode='nearest')

    Returns ``{"product": (T, H, W) fp64, "series": (T,) fp64, "uncertainty": fp64-or-input-dtype tensor or None}``.  The
    series is taken before the bias is added, as in the notebook; a time step without a valid pixel gives NaN."""
    from . import spline
    trend_ups = spline.zoom(trend25, trend_zoom, order=3)
    if trend_ups.shape != res.shape:
        raise K.L.GandanetError(f"assemble_product: zoomed trend {tuple(trend_ups.shape)} vs tiles {tuple(res.shape)}")
    mask_u8 = None if mask is None else _mask_u8(mask, res.shape[-2:])
    if quantile_map is None:
        product = restore_units(res, trend_ups, scale, mean, unit, mask_u8)
    else:
        product = restore_units(res, trend_ups, scale, mean, unit, None)
        quantile_map.apply(product, kind=quantile_kind, out=product)         # one thread per element: in place is safe
        if mask_u8 is not None:
            product.masked_fill_(mask_u8 == 0, float("nan"))                 # plumbing: one ATen fill
    series, _ = K.masked_plane_mean_f64(product, mask_u8)
    if bias is not None:
        bias_ups = spline.zoom(bias, bias_zoom, order=3)
        if bias_ups.shape != product.shape:
            raise K.L.GandanetError(f"assemble_product: zoomed bias {tuple(bias_ups.shape)} vs product {tuple(product.shape)}")
        product += bias_ups.to(product.dtype)                        # plumbing: one ATen add
    unc = None if uncertainty is None else spline.zoom(uncertainty, uncertainty_zoom, order=0, mode="nearest")
    return {"product": product, "series": series, "uncertainty": unc}
