"""Which pixels behave alike?  Regionalisation of a (T, ...) cube by k-means (Lloyd's algorithm) on its pixel series, on the
device: the step between pixel maps and a table of regions, and the check that the downscaled product regionalises like GRACE
(``region_agreement``).  The regions come back as a ``Regions`` whose ``to_zonemap`` is a ``basins.ZoneMap``, so ``zone_mean``,
``basin_series``, ``drought_area`` and every ``mask=`` take data-driven regions unchanged.

Definitions (``include/gandanet.h``, "Regionalisation"): the sample of pixel m is ``v[t] = (x[t, m] - shift[m]) * scale[m]``
(``normalize``), its distance to centroid k is the sum over ascending t of ``(v[t] - c[k, t])**2`` (never the expanded form,
which cancels), its label is the nearest centroid with the lower index on a tie; a centroid is the weighted mean of its
members, summed in a fixed order (slabs of 1024 neighbouring pixels in ascending order).  All arithmetic is fp64, there are no
atomics and no (M, K) matrix: each Lloyd iteration is one ``gd_km_assign`` and one ``gd_km_update``, each reading the cube once.
The same inputs give the same bits on every run.

What is NOT claimed: Lloyd's algorithm finds a local optimum of the inertia, not the global one (use ``n_init`` with
``init="kmeans++"`` or ``"random"``, or compare with ``"maximin"``); ``silhouette`` is the simplified, centroid-based silhouette,
not the pairwise one; the series are treated as independent vectors, there is no spatial contiguity constraint, so a region may
be scattered; a shared seasonal cycle dominates the distances, so remove it first (``drought_index(kind="anomaly")``,
``stl_decompose``) if regions of anomaly behaviour are wanted.  A series with a NaN or inf is left out (label -1), listwise as
in ``eof_analysis``: fill gaps first (``ssa_fill``).

The kernels are ``csrc/kmeans.hip`` over ``csrc/kmeans_core.h``: fp32 or fp64 CUDA tensors, time along axis 0, T <= 2048,
k <= 64.  There is no CPU path in this module (``kern.km_assign_host``, ``kern.km_update_host`` and ``kern.km_farthest_host`` are
the plain C++ twins the tests use).
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import kern as K
from .basins import ZoneMap, _axis, zone_mean
from .timeseries import _cube, _series_mask

Tensor = torch.Tensor
L = K.L

INITS = ("maximin", "random", "kmeans++")
NORMALIZE = ("none", "center", "zscore")


def _normalizers(x2: Tensor, normalize: str) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """(shift, scale) fp64 (M,) of ``normalize``: torch reductions over time, 32 steps at a time so that no fp64 copy of an
    fp32 cube is made.  center: shift = the time mean.  zscore: also scale = 1 / sqrt(mean of (x - shift)**2); a constant
    series has scale inf, its samples are NaN and it is left out."""
    if normalize not in NORMALIZE:
        raise L.GandanetError(f"normalize is one of {NORMALIZE}, got {normalize!r}")
    if normalize == "none":
        return None, None
    t_len = x2.shape[0]
    shift = torch.mean(x2, dim=0, dtype=torch.float64)
    if normalize == "center":
        return shift, None
    ss = torch.zeros_like(shift)
    for t0 in range(0, t_len, 32):
        d = x2[t0:t0 + 32].to(torch.float64) - shift
        ss += (d * d).sum(dim=0)
    return shift, 1.0 / torch.sqrt(ss / t_len)


def _sample(x2: Tensor, idx: Tensor, shift, scale) -> Tensor:
    """the (n, T) fp64 samples of the pixels ``idx`` (int64 device tensor): (x - shift) * scale, two torch ops, each rounded on
    its own like the kernel's"""
    v = x2.index_select(1, idx).to(torch.float64)
    if shift is not None:
        v = v - shift.index_select(0, idx)
    if scale is not None:
        v = v * scale.index_select(0, idx)
    return v.t().contiguous()


def _ordered_sum(v: Tensor) -> Tensor:
    """the sum of a short fp64 vector in ascending order from its first entry (torch.sum does not promise an order)"""
    return functools.reduce(torch.add, v.unbind(0))


@dataclasses.dataclass
class Regions:
    """``labels`` (...) int32, -1 outside (masked or non-finite series); ``centroids`` (k, T) fp64, in the normalised units;
    ``counts`` (k) int64; ``weight`` (k) fp64, the sum of the pixel weights; ``within_ss`` (k) fp64, the weighted sums of the
    squared distances; ``inertia`` their sum over ascending k (0-d fp64 tensor); ``n_iter`` the centroid updates made;
    ``converged`` (None when the loop ran without looking, ``tol=None``); ``distance`` / ``second_distance`` (...) fp64 squared
    distances to the nearest / second nearest centroid and ``second_label`` (-1 / NaN when k = 1).  Labels, distances and the
    per-cluster sums all belong to ``centroids``: they come from one last assignment."""
    labels: Tensor
    centroids: Tensor
    counts: Tensor
    weight: Tensor
    within_ss: Tensor
    inertia: Tensor
    n_iter: int
    converged: Optional[bool]
    distance: Tensor
    second_label: Tensor
    second_distance: Tensor
    normalize: str = "none"
    pixel_weights: Optional[Tensor] = None

    @property
    def k(self) -> int:
        return int(self.centroids.shape[0])

    def silhouette(self) -> Tuple[Tensor, Tensor]:
        """``(map, mean)``: the SIMPLIFIED silhouette ``(b - a) / max(a, b)`` with a, b the Euclidean distances (square roots
        of ``distance``, ``second_distance``) to the own and to the nearest other CENTROID, not the pairwise silhouette over
        all members; 0 where a = b = 0, NaN outside and when k = 1.  ``mean`` is the pixel-weighted mean over the valid pixels."""
        a, b = torch.sqrt(self.distance), torch.sqrt(self.second_distance)
        top = torch.maximum(a, b)
        s = torch.where(top > 0.0, (b - a) / top, torch.where(top == 0.0, torch.zeros_like(top), top))
        ok = ~torch.isnan(s)
        w = torch.ones_like(s) if self.pixel_weights is None else self.pixel_weights.reshape(s.shape)
        w = torch.where(ok, w, torch.zeros_like(w))
        return s, (torch.where(ok, s, torch.zeros_like(s)) * w).sum() / w.sum()

    def predict(self, x2: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        """the labels of another (T, ...) cube of the same T against these centroids (for instance the coarsened product
        against centroids found on GRACE), normalised the way the fit was"""
        x2 = _cube(x2, "predict")
        if x2.shape[0] != self.centroids.shape[1]:
            raise L.GandanetError(f"predict: T = {self.centroids.shape[1]}, got a cube of {tuple(x2.shape)}")
        tail = tuple(x2.shape[1:])
        flat = x2.reshape(x2.shape[0], -1)
        shift, scale = _normalizers(flat, self.normalize)
        return K.km_assign(flat, self.centroids, shift, scale, _series_mask(mask, tail, x2.device))[0].reshape(tail)

    def reorder(self, by: str = "size") -> "Regions":
        """renumbered regions: ``by="size"`` the largest ``counts`` first, ``"centroid_mean"`` ascending time mean of the
        centroid; stable (ties keep their order).  One small copy to the host."""
        if by == "size":
            perm = np.argsort(-self.counts.cpu().numpy(), kind="stable")
        elif by == "centroid_mean":
            perm = np.argsort(self.centroids.mean(dim=1).cpu().numpy(), kind="stable")
        else:
            raise L.GandanetError(f"reorder: by is 'size' or 'centroid_mean', got {by!r}")
        dev = self.labels.device
        p = torch.from_numpy(perm.astype(np.int64)).to(dev)
        inv = torch.empty(self.k + 1, dtype=torch.int32, device=dev)
        inv[p] = torch.arange(self.k, dtype=torch.int32, device=dev)
        inv[self.k] = -1                                                  # where a label of -1 (index k after the shift below) lands

        def relabel(lab):
            return inv[torch.where(lab >= 0, lab, torch.full_like(lab, self.k)).to(torch.int64)]

        return dataclasses.replace(self, labels=relabel(self.labels), second_label=relabel(self.second_label), centroids=self.centroids[p],
                                   counts=self.counts[p], weight=self.weight[p], within_ss=self.within_ss[p])

    def to_zonemap(self, lon, lat, names: Optional[Sequence[str]] = None) -> ZoneMap:
        """the regions as a ``basins.ZoneMap`` on the (H, W) grid of ``labels``: ``bits`` (ceil(k / 32), H, W) uint32, one bit
        set per labelled pixel"""
        if self.labels.dim() != 2:
            raise L.GandanetError(f"to_zonemap: the regions live on {tuple(self.labels.shape)}, not on an (H, W) grid")
        dev = self.labels.device
        xs, ys = _axis(lon, "to_zonemap lon", dev), _axis(lat, "to_zonemap lat", dev)
        if (ys.numel(), xs.numel()) != tuple(self.labels.shape):
            raise L.GandanetError(f"to_zonemap: lat x lon is {ys.numel()} x {xs.numel()}, the labels are {tuple(self.labels.shape)}")
        names = [f"region{z}" for z in range(self.k)] if names is None else [str(n) for n in names]
        if len(names) != self.k or len(set(names)) != self.k:
            raise ValueError(f"{self.k} regions need {self.k} distinct names, got {names}")
        lab = self.labels.to(torch.int64)
        groups = (self.k + L.ZONE_MAX - 1) // L.ZONE_MAX
        word = torch.ones_like(lab) << (lab.clamp_min(0) % L.ZONE_MAX)
        bits = torch.stack([torch.where((lab >= 0) & (lab // L.ZONE_MAX == g), word, torch.zeros_like(word)) for g in range(groups)])
        return ZoneMap(bits.to(torch.int32).view(torch.uint32).contiguous(), names, xs, ys)

    def region_series(self, x: Tensor, weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """``zone_mean(x, self.to_zonemap(..), weights)``: the (T, k) mean series of ``x`` (in its own units) over the regions
        and the counts"""
        h, w = self.labels.shape if self.labels.dim() == 2 else (0, 0)
        return zone_mean(x, self.to_zonemap(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)), weights)


def _pixel_weights(weights, lat, tail, device) -> Optional[Tensor]:
    if weights is not None and lat is not None:
        raise L.GandanetError("kmeans_series: give weights or lat, not both")
    if lat is not None:
        if len(tail) != 2:
            raise L.GandanetError(f"kmeans_series: lat needs an (H, W) grid, got {tail}")
        ys = _axis(lat, "kmeans_series lat", device)
        if ys.numel() != tail[0]:
            raise L.GandanetError(f"kmeans_series: lat has {ys.numel()} entries for {tail[0]} rows")
        weights = torch.cos(torch.deg2rad(ys)).clamp_min(0.0)[:, None].expand(tail)
    if weights is None:
        return None
    if not isinstance(weights, Tensor) or not weights.is_cuda or tuple(weights.shape) != tuple(tail):
        raise L.GandanetError(f"kmeans_series: weights is a GPU tensor of the shape of one time step {tuple(tail)}")
    return weights.to(torch.float64).contiguous().reshape(-1)


class _Fit:
    """one cube with its normalisers, weights and mask: the calls of the loop in one place"""

    def __init__(self, x2, shift, scale, w, mask):
        self.x2, self.shift, self.scale, self.w, self.mask = x2, shift, scale, w, mask

    def assign(self, cent, second=False):
        return K.km_assign(self.x2, cent, self.shift, self.scale, self.mask, second)

    def update(self, label, dist, cent):
        return K.km_update(self.x2, label, dist, cent, self.w, self.shift, self.scale)

    def sample(self, idx):
        return _sample(self.x2, idx.to(torch.int64).reshape(-1), self.shift, self.scale)


def _init_maximin(f: _Fit, k: int) -> Tensor:
    t_len = f.x2.shape[0]
    zero = torch.zeros(1, t_len, dtype=torch.float64, device=f.x2.device)
    label, dist, _, _ = f.assign(zero)
    mean = f.update(label, dist, zero)[0]                                 # the weighted mean series of the valid pixels
    chosen = K.km_farthest(-f.assign(mean)[1])                            # the series nearest to it, the lowest index on a tie
    cent = f.sample(chosen)
    near = f.assign(cent)[1]
    for _ in range(1, k):
        nxt = K.km_farthest(near, chosen)
        chosen = torch.cat([chosen, nxt])
        c = f.sample(nxt)
        cent = torch.cat([cent, c])
        near = torch.minimum(near, f.assign(c)[1])                        # NaN (left-out pixels) stays NaN
    return cent


def _init_random(f: _Fit, k: int, valid: np.ndarray, rng) -> Tensor:
    pick = rng.choice(valid, size=k, replace=False)
    return f.sample(torch.from_numpy(np.ascontiguousarray(pick, dtype=np.int64)).to(f.x2.device))


def _init_pp(f: _Fit, k: int, valid: np.ndarray, rng) -> Tensor:
    dev = f.x2.device
    first = int(valid[int(rng.integers(0, valid.size))])
    cent = f.sample(torch.tensor([first], device=dev))
    near = f.assign(cent)[1]
    us = rng.random(k - 1)
    for j in range(1, k):
        p = torch.nan_to_num(near, nan=0.0) if f.w is None else torch.nan_to_num(near, nan=0.0) * f.w
        cs = torch.cumsum(p, dim=0)
        target = (cs[-1] * float(us[j - 1])).reshape(1)
        idx = torch.searchsorted(cs, target, right=True).clamp_max(cs.numel() - 1)
        # a pixel of zero mass (left out, or every remaining D is 0, or the target rounded up to cs[-1]) is never a centre:
        # the valid pixel farthest from its centre stands in (there are >= k valid pixels, so it exists)
        idx = torch.where(p.index_select(0, idx) > 0.0, idx, K.km_farthest(near).to(torch.int64))
        c = f.sample(idx)
        cent = torch.cat([cent, c])
        near = torch.minimum(near, f.assign(c)[1])
    return cent


def _lloyd(f: _Fit, cent: Tensor, max_iter: int, tol, relocate_empty: bool):
    """(cent, n_iter, converged): assign, stop if no label changed, update, re-seat; see ``kmeans_series``"""
    prev, prev_inertia, n_iter, converged = None, None, 0, (None if tol is None else False)
    for _ in range(max_iter):
        label, dist, _, _ = f.assign(cent)
        if tol is not None and prev is not None and not bool((label != prev).any()):       # the one copy of this iteration
            converged = True
            break
        cent, _, count, within = f.update(label, dist, cent)
        n_iter += 1
        prev = label
        if tol is None:
            continue
        if tol > 0.0 or relocate_empty:
            # .. or this one, with tol > 0 / re-seating: the inertia (in ascending k, so that n_iter is the same on every run),
            # the empty clusters and the pixels a re-seat can land on (those with a finite distance)
            rec = torch.stack([_ordered_sum(within) if tol > 0.0 else within.new_zeros(()), (count == 0).sum().to(torch.float64),
                               torch.isfinite(dist).sum().to(torch.float64)]).cpu()
            inertia, n_empty, n_seats = float(rec[0]), int(rec[1]), int(rec[2])
            if n_empty and relocate_empty:
                taken = None
                for kk in np.flatnonzero(count.cpu().numpy() == 0)[:n_seats]:   # never more re-seats than seats: no -1 pick
                    nxt = K.km_farthest(dist, taken)
                    taken = nxt if taken is None else torch.cat([taken, nxt])
                    cent[int(kk)] = f.sample(nxt)[0]
            elif tol > 0.0 and prev_inertia is not None and prev_inertia - inertia < tol * inertia:
                converged = True
                break
            prev_inertia = inertia
    return cent, n_iter, converged


def kmeans_series(x: Tensor, k: int, init: Union[str, Tensor] = "maximin", n_init: int = 1, max_iter: int = 100, tol: Optional[float] = 0.0,
                  normalize: str = "none", weights: Optional[Tensor] = None, lat=None, mask: Optional[Tensor] = None, seed: int = 0,
                  relocate_empty: bool = True) -> Regions:
    """k-means of the pixel series of ``x`` (T, ...) fp32 / fp64 on the device into ``k`` (<= 64) regions.

    ``init`` (default ``"maximin"``: it needs no random numbers, so the default call is a pure function of its inputs):
      ``"maximin"``   the first centre is the series nearest to the weighted mean series; every further one is the valid
                      series farthest from its nearest chosen centre (``gd_km_farthest``: the lowest pixel index on a tie).
      ``"random"``    ``numpy.random.default_rng(seed).choice(valid, size=k, replace=False)`` with ``valid`` the ascending
                      flat indices of the pixels that are neither masked nor non-finite.
      ``"kmeans++"``  D^2 sampling.  Recipe: ``rng = numpy.random.default_rng(seed)``; the first centre is
                      ``valid[rng.integers(0, len(valid))]``; then ``u = rng.random(k - 1)`` and for j = 1 .. k - 1: D = the
                      squared distance of every pixel to its nearest chosen centre (``gd_km_assign``; 0 where a pixel is
                      left out), ``cs = torch.cumsum(w * D)`` over ascending flat index, and centre j is the pixel
                      ``torch.searchsorted(cs, u[j - 1] * cs[-1], right=True)`` (clamped to the last pixel).
      a tensor (k, T) the starting centroids themselves, in the normalised units.
    With ``n_init > 1`` run i uses ``seed + i``; the run with the smallest inertia is kept, the first on a tie.
    ``normalize``: ``"none"``, ``"center"`` (each series minus its time mean) or ``"zscore"`` (also divided by its standard
    deviation; a constant series is left out); the maps are fp64 torch reductions made once and handed to the kernels, the
    cube is not copied.  ``weights`` (the shape of one step) or ``lat`` (H latitudes in degrees: cos lat) weigh the pixels in
    the centroid means and in the inertia.  ``mask``: nonzero = use the pixel.

    The loop: assign; stop if no label changed; update; ``relocate_empty`` re-seats each cluster left without a member, in
    ascending order, on the valid pixel farthest from its own centroid that is not already re-seated (``gd_km_farthest``), and
    the next assignment follows; with ``tol > 0`` the loop also stops when the inertia fell by less than ``tol`` x inertia.
    Each test costs one small copy to the host per iteration (the "changed" flag; with ``tol > 0`` or ``relocate_empty`` a
    second small record).  With ``tol=None`` the loop runs ``max_iter`` iterations without any host sync and without
    re-seating (which needs the counts on the host); ``converged`` is then None.  After the loop one more assign and update
    give the labels, both distance maps and the per-cluster sums that belong to the returned centroids.
    Fewer than ``k`` valid series (not masked, all samples finite) is an error, and so are explicit centroids with a NaN or
    an inf; both are checked once before the loop (one copy to the host), except for explicit centroids with ``tol=None``,
    which make no host sync at all and never pick a pixel.

    Lloyd's algorithm finds a local optimum; the series are independent vectors (no contiguity constraint); remove the
    seasonal cycle first if regions of anomaly behaviour are wanted; fill gaps first (``ssa_fill``)."""
    x = _cube(x, "kmeans_series")
    if x.dim() < 2:
        raise L.GandanetError(f"kmeans_series: x is a (T, ...) cube, got {tuple(x.shape)}")
    t_len, tail = int(x.shape[0]), tuple(x.shape[1:])
    for v, nm, lo in ((k, "k", 1), (n_init, "n_init", 1), (max_iter, "max_iter", 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise L.GandanetError(f"kmeans_series: {nm} is an integer >= {lo}, got {v!r}")
    if k > L.KM_MAX_K or t_len > L.KM_MAX_T:
        raise L.GandanetError(f"kmeans_series: k <= {L.KM_MAX_K} and T <= {L.KM_MAX_T}, got k = {k}, T = {t_len}")
    if tol is not None and not float(tol) >= 0.0:
        raise L.GandanetError(f"kmeans_series: tol is None or a number >= 0, got {tol!r}")
    x2 = x.reshape(t_len, -1)
    shift, scale = _normalizers(x2, normalize)
    w = _pixel_weights(weights, lat, tail, x.device)
    f = _Fit(x2, shift, scale, w, _series_mask(mask, tail, x.device))
    explicit = isinstance(init, Tensor)
    if explicit:
        if not init.is_cuda or tuple(init.shape) != (k, t_len):
            raise L.GandanetError(f"kmeans_series: init is a GPU tensor ({k}, {t_len}), got {tuple(init.shape)}")
        n_init = 1
    elif init not in INITS:
        raise L.GandanetError(f"kmeans_series: init is one of {INITS} or a (k, T) tensor, got {init!r}")
    # The valid series, counted once on the host: fewer than k cannot be clustered, and a re-seat or a named init would have
    # no pixel to land on.  Only explicit centroids with tol=None skip the count: that path promises no host sync, and it
    # neither picks pixels nor re-seats.
    if not explicit or tol is not None:
        zero = torch.zeros(1, t_len, dtype=torch.float64, device=x.device)
        valid = torch.nonzero(f.assign(zero)[0] >= 0).reshape(-1).cpu().numpy()
        if valid.size < k:
            raise L.GandanetError(f"kmeans_series: {valid.size} valid series for k = {k}")
        if explicit and not bool(torch.isfinite(init).all()):
            raise L.GandanetError("kmeans_series: init holds a NaN or an inf")
        if not explicit and init == "maximin":
            n_init = 1
    best = None
    for run in range(n_init):
        if explicit:
            cent = init.to(torch.float64).contiguous().clone()
        elif init == "maximin":
            cent = _init_maximin(f, k)
        else:
            rng = np.random.default_rng(seed + run)
            cent = (_init_random if init == "random" else _init_pp)(f, k, valid, rng)
        cent, n_iter, converged = _lloyd(f, cent, max_iter, None if tol is None else float(tol), relocate_empty)
        label, dist, label2, dist2 = f.assign(cent, second=True)
        _, wsum, count, within = f.update(label, dist, cent)
        res = Regions(label.reshape(tail), cent, count, wsum, within, _ordered_sum(within), n_iter, converged, dist.reshape(tail),
                      label2.reshape(tail), dist2.reshape(tail), normalize, w)
        if best is None or (n_init > 1 and float(res.inertia) < float(best.inertia)):
            best = res
    return best


def kmeans_scan(x: Tensor, ks: Sequence[int], **kw) -> Dict[str, list]:
    """the usual table for choosing k: ``{"k", "inertia", "silhouette", "calinski_harabasz", "regions"}``, one entry per k of
    ``ks``, from ``kmeans_series(x, k, **kw)``.  silhouette: the mean simplified silhouette (NaN at k = 1).  Calinski-Harabasz:
    ``(B / (k - 1)) / (W / (n - k))`` with W the inertia, B = (the inertia of the k = 1 fit of the same pixels) - W and n the
    number of valid pixels (NaN at k = 1).  With ``weights`` / ``lat`` W and B are weighted sums while n stays the plain pixel
    count, so the index is comparable between values of k on one cube but not with an unweighted fit.  Host floats."""
    out = {"k": [], "inertia": [], "silhouette": [], "calinski_harabasz": [], "regions": []}
    base = kmeans_series(x, 1, **{**kw, "init": "maximin"})
    total, n = float(base.inertia), int(base.counts.sum())
    for k in ks:
        r = base if k == 1 and not isinstance(kw.get("init"), Tensor) else kmeans_series(x, int(k), **kw)
        wss = float(r.inertia)
        out["k"].append(int(k))
        out["inertia"].append(wss)
        out["silhouette"].append(float(r.silhouette()[1]))
        out["calinski_harabasz"].append(((total - wss) / (k - 1)) / (wss / (n - k)) if 1 < k < n and wss > 0.0 else float("nan"))
        out["regions"].append(r)
    return out


def region_agreement(a: Tensor, b: Tensor, weights: Optional[Tensor] = None) -> Dict[str, object]:
    """do two label maps on one grid (int32, -1 = outside; ``Regions.labels``) cut the domain alike?  Over the pixels labelled
    in both: ``table`` (ka, kb) the contingency table (int64 counts from integer torch ops; with ``weights`` fp64 sums),
    ``ari`` the adjusted Rand index (Hubert & Arabie) from the count table, ``purity`` = sum over the rows of the row maximum /
    total, and ``matching``: a one-to-one list of (label of a, label of b) pairs chosen GREEDILY on the table (the largest
    remaining entry first, the lowest (row, column) on a tie): not the optimal assignment."""
    for t, nm in ((a, "a"), (b, "b")):
        if not isinstance(t, Tensor) or not t.is_cuda or t.dtype not in (torch.int32, torch.int64):
            raise L.GandanetError(f"region_agreement: {nm} is an integer GPU label map")
    if a.shape != b.shape:
        raise L.GandanetError(f"region_agreement: label maps of {tuple(a.shape)} and {tuple(b.shape)}")
    fa, fb = a.reshape(-1).to(torch.int64), b.reshape(-1).to(torch.int64)
    both = (fa >= 0) & (fb >= 0)
    fa, fb = fa[both], fb[both]
    if fa.numel() == 0:
        raise L.GandanetError("region_agreement: no pixel is labelled in both maps")
    ka, kb = int(fa.max()) + 1, int(fb.max()) + 1
    counts = torch.bincount(fa * kb + fb, minlength=ka * kb).reshape(ka, kb)
    n = counts.sum().cpu().numpy().astype(np.float64)
    c = counts.cpu().numpy().astype(np.float64)
    pairs = lambda v: (v * (v - 1.0) / 2.0).sum()
    s_ij, s_a, s_b, tot = pairs(c), pairs(c.sum(1)), pairs(c.sum(0)), n * (n - 1.0) / 2.0
    expected = s_a * s_b / tot if tot > 0 else 0.0
    denom = 0.5 * (s_a + s_b) - expected
    ari = 1.0 if denom == 0.0 else float((s_ij - expected) / denom)
    if weights is not None:
        if not isinstance(weights, Tensor) or not weights.is_cuda or weights.shape != a.shape:
            raise L.GandanetError("region_agreement: weights is a GPU tensor of the shape of the maps")
        table = torch.bincount(fa * kb + fb, weights=weights.reshape(-1).to(torch.float64)[both], minlength=ka * kb).reshape(ka, kb)
    else:
        table = counts
    t = table.cpu().numpy().astype(np.float64)
    purity = float(t.max(axis=1).sum() / t.sum())
    left, matching = t.copy(), []
    for _ in range(min(ka, kb)):
        i, j = np.unravel_index(int(np.argmax(left)), left.shape)         # first maximum in row-major order
        if left[i, j] < 0.0:
            break
        matching.append((int(i), int(j)))
        left[i, :], left[:, j] = -1.0, -1.0
    return {"table": table, "ari": ari, "purity": purity, "matching": matching}
