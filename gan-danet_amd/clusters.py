"""Which dry pixels belong to the same drought?  Contiguous dry regions of a (T, H, W) index cube, linked through time:
3-D connected components on the device, and for every cluster its life, bounding box, area series, severity and centroid
track -- the input of severity-area-duration analysis, and the way to ask whether the downscaled product breaks one GRACE
drought into several.

* ``label_components``: labels 1 .. K in raster order of each component's first voxel (the numbering of
  ``scipy.ndimage.label``) for any symmetric 3 x 3 x 3 structure;
* ``drought_clusters``: the labels and the per-cluster tables of a drought index at a threshold, optionally after the
  per-step patch filter of Andreadis et al. 2005 (``min_step_pixels``).

The kernels are ``csrc/ccl.hip`` over ``csrc/ccl_core.h`` (``include/gandanet.h``, "Connected components"): union-find in
LDS tiles, unions across tile borders in global memory, integer atomics only, so labels and tables are the same bits on
every run.  The cube stays on the device; two integers cross to the host, the number of clusters (to size the tables) and
the number of track records.  Only CUDA tensors are accepted and there is no CPU path (``kern.ccl_*_host`` are the plain
C++ twins the tests use).  torch allocates, views and copies.

Out of scope: periodic longitude (a cluster that crosses the date line is two), a minimum-overlap rule between steps (one
shared neighbour links two steps), and matching clusters across two grids.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import kern as K
from .timeseries import _series_mask

Tensor = torch.Tensor
L = K.L

PLANAR_BITS = 0x1E00     # the backward offsets inside a time step: (0, -1, -1), (0, -1, 0), (0, -1, 1), (0, 0, -1)
_NAMED = {"planar4": (1 << 10) | (1 << 12), "planar8": PLANAR_BITS}


def structure_word(structure) -> int:
    """the 13-bit word of ``gd_ccl_label`` for ``structure``: 1, 2 or 3 (``scipy.ndimage.generate_binary_structure(3, .)``:
    faces, + edges, + corners), ``"planar4"`` / ``"planar8"`` (4- / 8-connected in space, no link in time), or a symmetric
    3 x 3 x 3 array with its centre set"""
    if isinstance(structure, str):
        if structure not in _NAMED:
            raise L.GandanetError(f"structure: a name is one of {sorted(_NAMED)}, got {structure!r}")
        return _NAMED[structure]
    if isinstance(structure, (int, np.integer)) and not isinstance(structure, bool):
        if structure not in (1, 2, 3):
            raise L.GandanetError(f"structure: a connectivity is 1, 2 or 3, got {structure!r}")
        d = np.abs(np.indices((3, 3, 3)) - 1).sum(0)
        s = d <= structure
    else:
        s = np.asarray(structure.cpu() if isinstance(structure, Tensor) else structure) != 0
        if s.shape != (3, 3, 3):
            raise L.GandanetError(f"structure: expected 1, 2, 3, a name or a 3 x 3 x 3 array, got shape {s.shape}")
        if not s[1, 1, 1]:
            raise L.GandanetError("structure: the centre is not set")
        if not np.array_equal(s, s[::-1, ::-1, ::-1]):
            raise L.GandanetError("structure: not symmetric")
    flat = s.reshape(-1)
    return sum(1 << k for k in range(L.CCL_STRUCT_BITS) if flat[k])


def _input(x, fn: str) -> Tensor:
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise L.GandanetError(f"{fn}: expected a GPU tensor (there is no CPU path)")
    if x.dtype == torch.bool:
        x = x.to(torch.uint8)
    if x.dtype not in (torch.float32, torch.float64, torch.uint8):
        raise L.GandanetError(f"{fn}: expected float32, float64, uint8 or bool, got {x.dtype}")
    if x.dim() != 3 or x.numel() == 0:
        raise L.GandanetError(f"{fn}: expected a non-empty (T, H, W) cube, got {tuple(x.shape)}")
    if x.numel() >= 1 << 31:
        raise L.GandanetError(f"{fn}: {x.numel()} voxels, indices are int32")
    return x if x.is_contiguous() else x.contiguous()


def _min_size(v, name: str, lowest: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lowest:
        raise L.GandanetError(f"{name} is an integer >= {lowest}, got {v!r}")
    return int(v)


def _threshold(x: Tensor, threshold, fn: str) -> float:
    if x.dtype == torch.uint8:
        return 0.0
    if threshold is None or float(threshold) != float(threshold):
        raise L.GandanetError(f"{fn}: a float cube needs a threshold that is a number, got {threshold!r}")
    return float(threshold)


def _label(x: Tensor, thr: float, word: int, min_size: int, mask: Optional[Tensor]) -> Tuple[Tensor, int]:
    parent = K.ccl_label(x, thr, word, mask)
    ws = torch.empty(max(L.load().gd_ccl_ws_bytes(x.numel()), 8), device=x.device, dtype=torch.uint8)
    if min_size > 1:
        K.ccl_filter(parent, min_size, ws)
    labels, count = K.ccl_relabel(parent, out=parent, ws=ws)
    return labels, int(count.item())


def label_components(x: Tensor, threshold: Optional[float] = None, structure=1, min_size: int = 1,
                     mask: Optional[Tensor] = None) -> Tuple[Tensor, int]:
    """``(labels, K)``: the connected components of the foreground of the (T, H, W) cube ``x``, int32 labels of the shape of
    ``x``, 0 on background and 1 .. K in raster order of each component's first voxel.

    Foreground: ``x <= threshold`` for a float32 / float64 cube (never for NaN) on the pixels where ``mask`` (H, W; bool or
    uint8) is nonzero; nonzero for a uint8 or bool cube such as ``DroughtEvents.in_event`` (``threshold`` is not read, and
    ``mask`` is not applied).  ``structure``: see ``structure_word``.  Components of fewer than ``min_size`` voxels are
    dropped before the numbering."""
    x = _input(x, "label_components")
    word = structure_word(structure)
    thr = _threshold(x, threshold, "label_components")
    m = _series_mask(mask, tuple(x.shape[1:]), x.device)
    return _label(x, thr, word, _min_size(min_size, "label_components: min_size", 1), m)


class DroughtClusters:
    """the clusters of ``drought_clusters``: ``labels`` (T, H, W) int32, ``n`` clusters, and per cluster k (label k + 1):
    ``voxels``, ``start``, ``end`` (steps, inclusive), ``duration`` (int32); ``bbox`` (n, 6) int32 t0, t1, h0, h1, w0, w1;
    ``volume`` (the area summed over the steps), ``severity`` (the sum of area x (threshold - value)), ``peak_area`` and
    ``peak_area_step``, ``peak`` (the smallest value) and ``centroid`` (n, 3) (t, h, w), area-weighted, all fp64.  ``bounds``,
    ``offsets``, ``tracks``, ``index`` and ``totals`` are the raw tables of ``include/gandanet.h``."""

    def __init__(self, labels: Tensor, n: int, bounds: Tensor, offsets: Tensor, tracks: Tensor, index: Tensor, totals: Tensor,
                 threshold: float):
        self.labels, self.n, self.threshold = labels, int(n), float(threshold)
        self.bounds, self.offsets, self.tracks, self.index, self.totals = bounds, offsets, tracks, index, totals
        self.voxels, self.start, self.end = bounds[:, 0], bounds[:, 1], bounds[:, 2]
        self.duration = self.end - self.start + 1
        self.bbox = bounds[:, 1:]
        to = {nm: totals[:, k] for k, nm in enumerate(L.CCL_TOTALS)}
        self.volume, self.severity, self.peak_area, self.peak = to["volume"], to["severity"], to["peak_area"], to["peak"]
        self.peak_area_step = to["peak_area_step"]
        self.centroid = totals[:, 5:8]
        self._host_offsets = None

    def track(self, k: int) -> Dict[str, Tensor]:
        """cluster ``k`` (0-based) step by step: ``step``, ``count``, ``area``, ``severity``, ``centroid_h``, ``centroid_w``
        and ``min``, one entry per step of its life"""
        if not 0 <= k < self.n:
            raise L.GandanetError(f"track: 0 <= k < {self.n}, got {k!r}")
        if self._host_offsets is None:
            self._host_offsets = self.offsets.cpu().numpy()
        rec = self.tracks[int(self._host_offsets[k]):int(self._host_offsets[k + 1])]
        col = {nm: rec[:, j] for j, nm in enumerate(L.CCL_TRACK)}
        return {"step": self.index[int(self._host_offsets[k]):int(self._host_offsets[k + 1]), 1], "count": col["count"],
                "area": col["area"], "severity": col["severity"], "centroid_h": col["sum_h"] / col["area"],
                "centroid_w": col["sum_w"] / col["area"], "min": col["min"]}

    def area_series(self) -> Tensor:
        """(T, n) fp64: the area of every cluster at every step, zero outside its life"""
        out = torch.zeros((self.labels.shape[0], self.n), device=self.labels.device, dtype=torch.float64)
        if self.n:
            out[self.index[:, 1].long(), self.index[:, 0].long()] = self.tracks[:, 1]
        return out


def drought_clusters(index: Tensor, threshold: float = -0.8, structure=2, min_size: int = 1, min_step_pixels: int = 0,
                     weights: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> DroughtClusters:
    """the drought clusters of an index cube (T, H, W): connected regions of ``index <= threshold`` (the D1 class of the
    GRACE-DSI by default), linked in space and time by ``structure`` (see ``structure_word``; 2 = faces and edges).

    ``min_size`` drops clusters of fewer voxels.  ``min_step_pixels`` > 0 is the recipe of Andreadis et al. 2005: every step
    is labelled on its own with the spatial part of ``structure``, patches of fewer pixels are dropped, and what is left is
    linked in 3-D.  ``weights`` (H, W), for instance the cell areas or cos(lat), weigh area, severity and centroids (1
    without).  ``mask`` (H, W) leaves pixels out.  A uint8 / bool cube such as ``DroughtEvents.in_event`` is taken as the
    foreground itself: it has counts, areas and centroids, and NaN severity, peak and min.

    Not done here: periodic longitude, a minimum-overlap rule between steps, matching clusters across two grids."""
    x = _input(index, "drought_clusters")
    word = structure_word(structure)
    values = x.dtype != torch.uint8
    thr = _threshold(x, threshold, "drought_clusters")
    m = _series_mask(mask, tuple(x.shape[1:]), x.device)
    min_size = _min_size(min_size, "drought_clusters: min_size", 1)
    min_step_pixels = _min_size(min_step_pixels, "drought_clusters: min_step_pixels", 0)
    T, H, W = x.shape
    if weights is not None:
        if not isinstance(weights, Tensor) or not weights.is_cuda or tuple(weights.shape) != (H, W):
            raise L.GandanetError(f"drought_clusters: weights is a GPU tensor of shape {(H, W)} (there is no CPU path)")
        weights = weights.to(torch.float64).contiguous()
    if min_step_pixels > 1:
        planar, _ = _label(x, thr, word & PLANAR_BITS, min_step_pixels, m)
        labels, n = _label((planar > 0).to(torch.uint8), 0.0, word, min_size, None)
    else:
        labels, n = _label(x, thr, word, min_size, m)
    dev = x.device
    if n == 0:
        i32, f64 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float64)
        return DroughtClusters(labels, 0, torch.empty((0, len(L.CCL_BOUNDS)), **i32), torch.zeros(1, **i32),
                               torch.empty((0, len(L.CCL_TRACK)), **f64), torch.empty((0, 2), **i32),
                               torch.empty((0, len(L.CCL_TOTALS)), **f64), thr)
    bounds = K.ccl_bounds(labels, n)
    offsets = K.ccl_offsets(bounds)
    records = int(offsets[-1].item())
    tracks, rec_index = K.ccl_tracks(x if values else None, labels, bounds, offsets, records, thr, weights, severity=values)
    totals = K.ccl_totals(tracks, bounds, offsets)
    return DroughtClusters(labels, n, bounds, offsets, tracks, rec_index, totals, thr)
