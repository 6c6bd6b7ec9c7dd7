"""Smoothing and gap filling of fields that are already on the device, with scipy's semantics.

The notebook trainer takes ``smoothing_method=`` and applies it to the whole ``hr_aux`` array before the split
(GAN_DANet_train.ipynb: ``smooth_data_gaussian`` / ``smooth_data_median`` / ``smooth_data_savitzky_golay``), and
``datasets.py`` smooths every GLDAS plane with ``gaussian_filter(sigma=3)`` and repairs the -9999 gaps with a normalised
convolution (``fill_placeholder_with_nearest``).  Here the same filters are HIP kernels (``csrc/filters.hip``) on fp32 or
fp64 CUDA tensors; there is no CPU path.  Boundary mode is scipy's default ``reflect`` throughout; every sum is fp64 and
every pass is rounded to the storage type once, as ``scipy.ndimage.correlate1d`` does.  NaN inputs: the Gaussian and
Savitzky-Golay filters propagate them like any sum; the median of a window that holds a NaN is unspecified.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import kern as K

Tensor = torch.Tensor
L = K.L


def _input(x, name: str) -> Tensor:
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise L.GandanetError(f"{name}: expected a GPU tensor (there is no CPU path)")
    if x.dtype not in (torch.float32, torch.float64):
        raise L.GandanetError(f"{name}: expected float32 or float64, got {x.dtype}")
    return x if x.is_contiguous() else x.contiguous()


def _axes(x: Tensor, axes) -> Tuple[int, ...]:
    if axes is None:
        return tuple(range(x.dim()))
    axes = (axes,) if isinstance(axes, int) else tuple(axes)
    out = []
    for a in axes:
        if not -x.dim() <= a < x.dim():
            raise ValueError(f"axis {a} is out of range for a {x.dim()}-D tensor")
        out.append(a % x.dim())
    if len(set(out)) != len(out):
        raise ValueError("axes must be unique")
    return tuple(out)


def _per_axis(value, axes, name: str):
    if np.isscalar(value):
        return [value] * len(axes)
    value = list(value)
    if len(value) != len(axes):
        raise ValueError(f"{name} must be a scalar or hold one value per filtered axis")
    return value


def gaussian_filter(x: Tensor, sigma, axes=None, truncate: float = 4.0) -> Tensor:
    """``scipy.ndimage.gaussian_filter(x, sigma, axes=axes, truncate=truncate)`` (order 0, mode 'reflect').

    ``sigma``: a scalar, or one value per listed axis; axes with ``sigma <= 1e-15`` are skipped.  The passes run in the
    order ``axes`` lists them (default: every axis, ascending, as scipy), each rounded to the storage type, ping-ponging
    between two temporaries; the result is a new tensor and ``x`` is untouched.  ``gaussian_filter(t, 3, axes=(2, 3))`` on
    an (N, C, H, W) tensor is the per-plane sigma = 3 smoothing ``datasets.py`` applies to every GLDAS plane."""
    x = _input(x, "gaussian_filter")
    axes = _axes(x, axes)
    sigmas = [float(s) for s in _per_axis(sigma, axes, "sigma")]
    src, bufs = x, []
    for axis, s in zip(axes, sigmas):
        if s <= 1e-15 or x.numel() == 0:
            continue
        w, radius = K.gaussian_weights_host(s, truncate)
        if len(bufs) < 2:
            bufs.append(torch.empty_like(x))
        dst = bufs[0] if src is not bufs[0] else bufs[1]
        K.correlate1d_axis(src, dst, axis, w, radius, L.EDGE_REFLECT)
        src = dst
    return x.clone() if src is x else src


def _merge_for_median(shape, sizes):
    """collapse runs of unfiltered (size 1) dimensions, then pad to four dimensions in front"""
    mshape, msize = [], []
    for n, s in zip(shape, sizes):
        if s == 1 and msize and msize[-1] == 1:
            mshape[-1] *= n
        else:
            mshape.append(n)
            msize.append(s)
    if len(mshape) > 4:
        raise L.GandanetError(f"median_filter: shape {tuple(shape)} with window {tuple(sizes)} does not reduce to four dimensions")
    pad = 4 - len(mshape)
    return [1] * pad + mshape, [1] * pad + msize


def median_filter(x: Tensor, size=3, axes=None) -> Tensor:
    """``scipy.ndimage.median_filter(x, size=size, axes=axes)`` (mode 'reflect'): ``size`` is 1, 3 or 5 per filtered axis
    and the window holds 3, 5, 9, 25, 27 or 81 elements.  Exact: the median of an odd count is one of the inputs."""
    x = _input(x, "median_filter")
    axes = _axes(x, axes)
    sizes = [1] * x.dim()
    for a, s in zip(axes, _per_axis(size, axes, "size")):
        if int(s) != s:
            raise ValueError("size must be an integer")
        sizes[a] = int(s)
    if all(s == 1 for s in sizes) or x.numel() == 0:
        return x.clone()
    shape4, size4 = _merge_for_median(list(x.shape), sizes)
    return K.median_nd(x, shape4, size4)


def savgol_tables(window_length: int, polyorder: int):
    """(interior coefficients (window,), edge matrices (2, window // 2, window)) of ``savgol_filter(..., deriv=0,
    mode='interp')`` in fp64, from the hat matrix H = A (A^T A)^-1 A^T of the Vandermonde system A[j, p] = t_j^p on the
    window's sample positions: row h = window // 2 of H smooths the centre (``scipy.signal.savgol_coeffs``), rows 0 .. h-1
    give the polynomial fitted to the first ``window`` samples at the first h positions, rows window-h .. window-1 the
    same at the far end.

    The edge rows come from an orthonormal basis of A's columns (H = Q Q^T), exact to a few 1e-16.  The centre row is the
    minimum-norm least-squares solution of A^T c = e_0 -- the same row of H, computed the way ``savgol_coeffs`` computes
    it, so that the interior reproduces scipy's own coefficients rather than differing from them by scipy's rounding
    (1.1e-12 at window 33, order 4, where the exact row and scipy's disagree by that much)."""
    w, p = int(window_length), int(polyorder)
    if w < 1 or w % 2 == 0:
        raise ValueError("window_length must be a positive odd integer")
    if p < 0 or p >= w:
        raise ValueError("polyorder must be less than window_length")
    h = w // 2
    t = np.arange(w, dtype=np.float64) - h
    q, _ = np.linalg.qr(np.vander(t, p + 1, increasing=True))   # H = Q Q^T for any basis Q of the column space
    hat = q @ q.T
    e0 = np.zeros(p + 1)
    e0[0] = 1.0
    # savgol_coeffs orders its positions for a convolution (descending); flipped back these are correlation weights
    centre = np.linalg.lstsq(t[::-1] ** np.arange(p + 1).reshape(-1, 1), e0, rcond=None)[0][::-1].copy()
    return centre, np.stack([hat[:h], hat[w - h:]]) if h else np.zeros((2, 0, w))


def savgol_filter(x: Tensor, window_length: int, polyorder: int, axis: int = -1) -> Tensor:
    """``scipy.signal.savgol_filter(x, window_length, polyorder, axis=axis)`` (deriv 0, mode 'interp'): the interior is one
    correlation with the smoothing coefficients, the first and last ``window_length // 2`` positions are the polynomial
    fitted to the first / last ``window_length`` samples.  ValueError where scipy raises one."""
    coeffs, edges = savgol_tables(window_length, polyorder)
    x = _input(x, "savgol_filter")
    (axis,) = _axes(x, axis)
    w = int(window_length)
    if w > x.shape[axis]:
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    if w > L.SAVGOL_MAX_WINDOW:
        raise L.GandanetError(f"savgol_filter: window_length {w} exceeds {L.SAVGOL_MAX_WINDOW}")
    if x.numel() == 0:
        return x.clone()
    out = torch.empty_like(x)
    K.correlate1d_axis(x, out, axis, list(coeffs), w // 2, L.EDGE_INTERIOR)
    if w > 1:
        K.savgol_edges_axis(x, out, axis, torch.from_numpy(np.ascontiguousarray(edges)).to(x.device), w)
    return out


def fill_masked(x: Tensor, placeholder: float = -9999, sigma=3, axes=None) -> Tensor:
    """Fill the gaps ``x <= placeholder`` by normalised convolution: smoothed(values with the gaps zeroed) /
    smoothed(valid mask), the quotient taken only at the gaps (a smoothed mask of exactly 0 divides by 1); every other
    point is returned bit for bit.  With ``x`` of shape (T, H, W) and the default ``axes`` this is the body of
    ``fill_placeholder_with_nearest`` (datasets.py) for one variable."""
    x = _input(x, "fill_masked")
    if x.numel() == 0:
        return x.clone()
    vals, mask = K.fill_prepare(x, placeholder)
    num = gaussian_filter(vals, sigma, axes)
    den = gaussian_filter(mask, sigma, axes)
    return K.fill_ratio(x, num, den, placeholder)


# ---- the notebook's three smoothing methods on the dataset's stored (N, C, H, W) tensor ----------------------------------
def _stored(hr_aux, name: str) -> Tensor:
    hr_aux = _input(hr_aux, name)
    if hr_aux.dim() != 4:
        raise L.GandanetError(f"{name}: expected the stored (N, C, H, W) tensor, got {tuple(hr_aux.shape)}")
    return hr_aux


def smooth_data_gaussian(hr_aux: Tensor, sigma: float = 2) -> Tensor:
    """the notebook's ``smooth_data_gaussian``: ``gaussian_filter(data, sigma)`` over ALL FOUR axes of the (N, H, W, C)
    array, time and channel included.  On the stored (N, C, H, W) tensor the passes run over axes (0, 2, 3, 1) -- scipy's
    order N, H, W, C -- because every pass is rounded to the storage type."""
    return gaussian_filter(_stored(hr_aux, "smooth_data_gaussian"), sigma, axes=(0, 2, 3, 1))


def smooth_data_median(hr_aux: Tensor, size: int = 3) -> Tensor:
    """the notebook's ``smooth_data_median``: ``median_filter(data, size)`` over the size^4 box of all four axes"""
    return median_filter(_stored(hr_aux, "smooth_data_median"), size)


def smooth_data_savitzky_golay(hr_aux: Tensor, window_length: int = 5, polyorder: int = 2) -> Tensor:
    """the notebook's ``smooth_data_savitzky_golay``: ``savgol_filter`` along the array's last axis, the channels (stored
    axis 1)"""
    return savgol_filter(_stored(hr_aux, "smooth_data_savitzky_golay"), window_length, polyorder, axis=1)


SMOOTHING_METHODS = {"gaussian": smooth_data_gaussian, "median": smooth_data_median, "savgol": smooth_data_savitzky_golay}
