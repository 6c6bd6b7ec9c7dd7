"""``scipy.ndimage.zoom`` at spline orders 0, 1 and 3 on tensors that are already on the device.

Everything the inference notebooks do behind the loader loop goes through ``zoom``: the cubic upsampling of the trend
stack (``zoom(trend25, (1, 5, 5), order=3)``), the masks (order 1), the bias field (order 3 at 1.25), the uncertainty
(order 0, ``mode='nearest'``), and ``datasets.py`` builds its auxiliary fields with ``zoom(..., order=3,
mode='nearest')``.  Here the same rules are HIP kernels (``csrc/spline.hip``) on fp32 or fp64 CUDA tensors; there is no
CPU path.  The axes are processed one at a time -- prefilter (order 3) and interpolation of one axis, then the next --
with fp64 between the axes and one rounding to the input dtype at the end; scipy prefilters every axis and then
interpolates every axis, the per-axis operators commute, and the two agree to rounding.
"""
from __future__ import annotations

from typing import Sequence, Tuple, Union

import numpy as np
import torch

from . import kern as K
from .filters import _axes, _input

Tensor = torch.Tensor
L = K.L

_MODES = {"constant": L.ZOOM_MIRROR, "mirror": L.ZOOM_MIRROR, "nearest": L.ZOOM_NEAREST}


def output_shape(shape: Sequence[int], zoom) -> Tuple[int, ...]:
    """scipy's rule: ``int(round(n * f))`` per axis with Python's ``round`` (halves go to even: 10 * 0.25 -> 2)"""
    if np.isscalar(zoom):
        zoom = [zoom] * len(shape)
    zoom = [float(f) for f in zoom]
    if len(zoom) != len(shape):
        raise ValueError("zoom must be a scalar or hold one factor per dimension")
    return tuple(int(round(n * f)) for n, f in zip(shape, zoom))


def _check(order, mode, cval, prefilter, grid_mode) -> int:
    if order not in (0, 1, 3):
        raise ValueError(f"spline order {order!r} is not supported (0, 1 and 3 are)")
    if mode not in _MODES:
        raise ValueError(f"mode {mode!r} is not supported ('constant', 'mirror' and 'nearest' are)")
    if cval != 0:
        raise ValueError("cval != 0 is not supported")
    if grid_mode:
        raise ValueError("grid_mode=True is not supported")
    if not prefilter:
        raise ValueError("prefilter=False is not supported")
    return _MODES[mode]


def zoom(x: Tensor, zoom: Union[float, Sequence[float]], order: int = 3, mode: str = "constant", cval: float = 0.0,
         prefilter: bool = True, grid_mode: bool = False) -> Tensor:
    """``scipy.ndimage.zoom(x, zoom, order=order, mode=mode)`` for orders 0, 1, 3 and modes 'constant', 'mirror',
    'nearest'; a new tensor of x's dtype.  ``zoom``: a scalar, or one factor per dimension.  With ``grid_mode=False`` the
    coordinates never leave the array, so 'constant' never produces ``cval`` and equals 'mirror' (scipy does return
    ``cval`` for the last sample of an axis where rounding lifts (n_out - 1) * ((n - 1) / (n_out - 1)) above n - 1, as at
    63 -> 315; this function interpolates it).  An axis with factor 1
    is skipped; the others run in ascending order of n_out / n_in, so the intermediates stay small.  ValueError for
    anything else scipy accepts (orders 2, 4, 5, 'reflect', 'wrap', 'grid-*', ``cval != 0``, ``grid_mode=True``,
    ``prefilter=False``)."""
    zmode = _check(order, mode, cval, prefilter, grid_mode)
    shape = tuple(x.shape) if isinstance(x, Tensor) else ()
    out_shape = output_shape(shape, zoom)
    x = _input(x, "zoom")
    if x.dim() == 0 or x.numel() == 0 or min(out_shape) < 1:
        raise ValueError(f"zoom: shape {shape} -> {out_shape} has an empty axis")
    factors = [zoom] * x.dim() if np.isscalar(zoom) else list(zoom)
    todo = [a for a in range(x.dim()) if float(factors[a]) != 1.0]
    todo.sort(key=lambda a: (out_shape[a] / shape[a], a))
    cur = x
    for k, a in enumerate(todo):
        last = k == len(todo) - 1
        cur = K.zoom_axis(cur, a, out_shape[a], order, zmode, x.dtype if last else torch.float64)
    return x.clone() if cur is x else cur


def spline_filter(x: Tensor, axes=None) -> Tensor:
    """``scipy.ndimage.spline_filter(x, order=3, mode='mirror', output=float64)`` over ``axes`` (default: all), one
    ``spline_filter1d`` per axis in ascending order: the cubic B-spline coefficients ``zoom`` interpolates in its
    'constant' and 'mirror' modes.  fp64 whatever the input dtype.  (The 'nearest' prefilter exists only inside
    ``zoom``, behind its 12-sample padding.)"""
    x = _input(x, "spline_filter")
    cur = x
    for a in sorted(_axes(x, axes)):
        if x.numel():
            cur = K.spline_prefilter_axis(cur, a)
    return x.double() if cur is x else cur
