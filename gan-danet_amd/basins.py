"""Basin analysis on the device: the loop body of the reference's ``Basin_TWSA_Comparison_GRACE_Downscaled.ipynb`` (cell 5).

For each of its 12 basins the notebook builds ``mask = [polygon.contains(Point(x, y)) for every grid point]`` on the 0.25
and on the 0.05 degree grid and takes ``np.nanmean(data[:, mask], axis=1)`` of both products.  Here

* ``pack_polygons`` turns polygons (ring lists, GeoJSON mappings, anything with ``__geo_interface__``) into one edge table
  on the host -- shapely is not needed;
* ``rasterize`` marks the grid points of all zones in one launch per 32 zones (``gd_zone_rasterize``) -> ``ZoneMap``;
* ``zone_mean`` averages a (T, H, W) or (T, C, H, W) tensor over all zones in one pass over the data (``gd_zone_mean``);
* ``basin_series`` is the notebook's loop: both series per basin plus their correlation and RMSE, one host copy at the end.

The containment rule is even-odd over all rings of a zone (outer rings and holes alike, any order, any orientation): a
point is inside iff an odd number of edges (x0, y0)-(x1, y1) have ``(y0 > py) != (y1 > py)`` and
``px < x0 + (py - y0) * (x1 - x0) / (y1 - y0)`` in fp64.  For a valid (Multi)Polygon that is shapely's ``contains`` at
every point that is not on a boundary; points exactly on a boundary are unspecified (shapely calls them outside).

The kernels are ``csrc/basins.hip``; no atomics in global memory, the same bits on every run.  There is no CPU path.
Reading shapefiles, plotting and the Excel export stay with the caller.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kern as K

Tensor = torch.Tensor
L = K.L


# ---- polygons -> edges (host) ---------------------------------------------------------------------------------------------
def _ring_edges(ring) -> np.ndarray:
    pts = np.asarray(ring, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] < 2:
        raise ValueError(f"a ring is an (n, 2) array of lon / lat, got shape {pts.shape}")
    pts = pts[:, :2]
    if not np.all(np.isfinite(pts)):
        raise ValueError("a ring holds a non-finite coordinate")
    if len(pts) and not np.array_equal(pts[0], pts[-1]):
        pts = np.concatenate([pts, pts[:1]])                      # close an open ring
    if len(np.unique(pts, axis=0)) < 3:
        raise ValueError("a ring needs at least 3 distinct vertices")
    edges = np.concatenate([pts[:-1], pts[1:]], axis=1)
    return edges[np.any(edges[:, :2] != edges[:, 2:], axis=1)]    # zero-length edges never count


def _rings_of(zone) -> list:
    geo = getattr(zone, "__geo_interface__", zone)
    if isinstance(geo, dict):
        kind, coords = geo.get("type"), geo.get("coordinates")
        if kind == "Polygon":
            return list(coords)
        if kind == "MultiPolygon":
            return [ring for part in coords for ring in part]
        raise ValueError(f"a zone is a Polygon or a MultiPolygon, got {kind!r}")
    return list(geo)


def pack_polygons(zones) -> Tuple[np.ndarray, np.ndarray]:
    """``(edges (E, 4) float64, offsets (Z + 1) int64)`` of Z zones: the edges (x0, y0, x1, y1) of zone z are the rows
    ``offsets[z]:offsets[z + 1]``.  A zone is a list of rings (each an (n, 2) array-like of lon / lat), a GeoJSON-style
    mapping of type ``Polygon`` or ``MultiPolygon``, or any object with ``__geo_interface__`` (a shapely geometry).  Rings
    are closed if open, zero-length edges are dropped, a ring with fewer than 3 distinct vertices raises ``ValueError``."""
    tables, offsets = [], [0]
    for zone in zones:
        rings = [_ring_edges(r) for r in _rings_of(zone)]
        if not rings:
            raise ValueError("a zone without rings")
        tables.extend(rings)
        offsets.append(offsets[-1] + sum(len(r) for r in rings))
    if not tables:
        raise ValueError("no zones")
    return np.ascontiguousarray(np.concatenate(tables)), np.asarray(offsets, dtype=np.int64)


# ---- the zone map ---------------------------------------------------------------------------------------------------------------
class ZoneMap:
    """Z rasterised zones on an (H, W) grid: ``bits`` (G, H, W) uint32 on the device, G = ceil(Z / 32), bit ``z % 32`` of
    group ``z // 32`` set where the point (lon[j], lat[i]) lies in zone z; ``names``, ``lon`` (W), ``lat`` (H); ``len()`` = Z."""

    def __init__(self, bits: Tensor, names: Sequence[str], lon: Tensor, lat: Tensor):
        self.bits, self.names, self.lon, self.lat = bits, list(names), lon, lat

    def __len__(self) -> int:
        return len(self.names)

    @property
    def shape(self) -> Tuple[int, int]:
        return tuple(self.bits.shape[1:])

    def mask(self, z: int) -> Tensor:
        """zone ``z`` as an (H, W) uint8 device tensor (1 = inside): a ``mask=`` of ``RegressionMetrics``,
        ``evaluate_ensemble`` and ``inference.restore_units``"""
        if isinstance(z, str):
            z = self.names.index(z)
        if not 0 <= z < len(self):
            raise IndexError(f"zone {z} of {len(self)}")
        word = self.bits[z // L.ZONE_MAX].view(torch.int32)
        return ((word >> (z % L.ZONE_MAX)) & 1).to(torch.uint8)

    def to(self, device) -> "ZoneMap":
        return ZoneMap(self.bits.to(device), self.names, self.lon.to(device), self.lat.to(device))


def _axis(v, name: str, device) -> Tensor:
    if isinstance(v, Tensor):
        if not v.is_cuda:
            raise L.GandanetError(f"{name}: expected a GPU tensor or a host sequence (there is no CPU path)")
        t = v.to(torch.float64)
    else:
        if device is None:
            if not torch.cuda.is_available():
                raise L.GandanetError(f"{name}: no GPU to put the grid on (there is no CPU path)")
            device = torch.device("cuda", torch.cuda.current_device())
        if torch.device(device).type != "cuda":
            raise L.GandanetError(f"{name}: device {device} is not a GPU (there is no CPU path)")
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(device)
    if t.dim() != 1 or t.numel() == 0:
        raise L.GandanetError(f"{name}: expected a non-empty 1-D axis, got {tuple(t.shape)}")
    return t.contiguous()


def rasterize(zones, lon, lat, names: Optional[Sequence[str]] = None, device=None) -> ZoneMap:
    """the notebook's ``mask = np.array([polygon.contains(pt) for pt in points]).reshape(lat_grid.shape)`` for all
    ``zones`` (see ``pack_polygons``) at once.  ``lon`` (W) and ``lat`` (H) are 1-D sequences or GPU tensors; the grid is
    rectilinear, need not be uniform and may run either way; grid point (i, j) is (lon[j], lat[i]).  Sequences go to
    ``device`` (default: the current GPU), tensors stay where they are.  One launch per 32 zones; no host sync."""
    for v, nm in ((lon, "lon"), (lat, "lat")):
        if isinstance(v, Tensor) and not v.is_cuda:
            raise L.GandanetError(f"rasterize: {nm} must be a GPU tensor or a host sequence (there is no CPU path)")
    if device is None:
        device = next((v.device for v in (lon, lat) if isinstance(v, Tensor)), None)
    xs, ys = _axis(lon, "rasterize lon", device), _axis(lat, "rasterize lat", device)
    if xs.device != ys.device:
        raise L.GandanetError(f"rasterize: lon on {xs.device}, lat on {ys.device}")
    edges, offsets = pack_polygons(zones)
    nz = len(offsets) - 1
    names = [f"zone{z}" for z in range(nz)] if names is None else [str(n) for n in names]
    if len(names) != nz or len(set(names)) != nz:
        raise ValueError(f"{nz} zones need {nz} distinct names, got {names}")
    edges_dev = torch.from_numpy(edges).to(xs.device)
    groups = (nz + L.ZONE_MAX - 1) // L.ZONE_MAX
    bits = torch.empty(groups, ys.numel(), xs.numel(), device=xs.device, dtype=torch.uint32)
    for g in range(groups):
        lo, hi = g * L.ZONE_MAX, min(nz, (g + 1) * L.ZONE_MAX)
        e0, e1 = int(offsets[lo]), int(offsets[hi])
        K.zone_rasterize(edges_dev[e0:e1], offsets[lo:hi + 1] - e0, xs, ys, out=bits[g])
    return ZoneMap(bits, names, xs, ys)


# ---- zonal means ------------------------------------------------------------------------------------------------------------
def zone_mean(x: Tensor, zonemap: ZoneMap, weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``np.nanmean(x[:, mask_z], axis=1)`` for every zone z of ``zonemap`` in one pass over ``x`` ((T, H, W) or
    (T, C, H, W), fp32 or fp64, on the device): ``(mean, count)`` with a trailing axis Z, mean fp64, count int64 (the
    pixels of the zone that are not NaN).  ``weights`` (H, W), for instance cos(lat) area weights, gives
    ``sum w x / sum w``; the notebook uses none.  A zone without a contributing pixel gives NaN and count 0."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise L.GandanetError("zone_mean: expected a GPU tensor (there is no CPU path)")
    if not isinstance(zonemap, ZoneMap) or not zonemap.bits.is_cuda:
        raise L.GandanetError("zone_mean: expected a ZoneMap on the GPU")
    if x.dim() < 3 or tuple(x.shape[-2:]) != zonemap.shape:
        raise L.GandanetError(f"zone_mean: a tensor of shape {tuple(x.shape)} on a zone map of {zonemap.shape}")
    if weights is not None:
        if not isinstance(weights, Tensor) or not weights.is_cuda:
            raise L.GandanetError("zone_mean: weights must be a GPU tensor (there is no CPU path)")
        weights = weights.to(torch.float64).contiguous()
    x = x if x.is_contiguous() else x.contiguous()
    means, counts = [], []
    for g in range(zonemap.bits.shape[0]):
        nz = min(L.ZONE_MAX, len(zonemap) - g * L.ZONE_MAX)
        m, c = K.zone_mean(x, zonemap.bits[g], nz, weights)
        means.append(m)
        counts.append(c)
    return (means[0], counts[0]) if len(means) == 1 else (torch.cat(means, dim=-1), torch.cat(counts, dim=-1))


def basin_series(grace025: Tensor, grid025, downscaled005: Tensor, grid005, zones, names: Optional[Sequence[str]] = None) -> Dict[str, dict]:
    """the notebook's loop over the basins: ``grace025`` (T, H, W) on ``grid025 = (lon, lat)`` and ``downscaled005``
    (T, H5, W5) on ``grid005``; every zone is rasterised on both grids and both mean series are taken.  Returns
    ``{name: {"grace": (T,), "downscaled": (T,), "count_grace": (T,), "count_downscaled": (T,), "cc": float, "rmse":
    float}}`` as host values: cc and rmse compare the two series over the time steps where both are numbers (the
    ``gd_eval_stats`` record with NaN skipping).  Everything is enqueued first; one copy to the host ends the call."""
    for t, nm in ((grace025, "grace025"), (downscaled005, "downscaled005")):
        if not isinstance(t, Tensor) or not t.is_cuda:
            raise L.GandanetError(f"basin_series: {nm} must be a GPU tensor (there is no CPU path)")
        if t.dim() != 3:
            raise L.GandanetError(f"basin_series: {nm} must be (T, H, W), got {tuple(t.shape)}")
    if grace025.shape[0] != downscaled005.shape[0]:
        raise L.GandanetError("basin_series: the two products differ in the number of time steps")
    zones = list(zones)
    dev = grace025.device
    zm25 = rasterize(zones, grid025[0], grid025[1], names, device=dev)
    zm05 = rasterize(zones, grid005[0], grid005[1], names, device=downscaled005.device)
    mg, cg = zone_mean(grace025, zm25)
    md, cd = zone_mean(downscaled005, zm05)
    sg, sd = mg.t().contiguous(), md.to(dev).t().contiguous()      # (Z, T): one dense series per basin
    nz, nt = sg.shape
    rec = torch.empty(nz, 8, device=dev, dtype=torch.float64)
    for z in range(nz):
        K.eval_stats(sd[z], sg[z], rec[z], skip_nan=True)
    host = torch.cat([sg, sd, cg.t().to(torch.float64), cd.to(dev).t().to(torch.float64), rec], dim=1).cpu().numpy()
    out = {}
    for z, name in enumerate(zm25.names):
        row = host[z]
        _, met = K.eval_merge_host(row[4 * nt:])
        out[name] = {"grace": row[:nt].copy(), "downscaled": row[nt:2 * nt].copy(),
                     "count_grace": row[2 * nt:3 * nt].astype(np.int64), "count_downscaled": row[3 * nt:4 * nt].astype(np.int64),
                     "cc": met["cc"], "rmse": math.sqrt(met["mse"]) if met["n"] > 0 else float("nan")}
    return out
