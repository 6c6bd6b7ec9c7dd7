"""How large is the random error of the downscaled product, next to GRACE and next to a land-surface model, when none of the
three is the truth?  Triple collocation (Stoffelen 1998; the covariance form and the squared correlation with the unknown truth
of McColl et al. 2014) of three collocated cubes per pixel, and a moving-block bootstrap over time that puts an interval on
every map, on the device.

Definitions (``include/gandanet.h``, "Triple collocation"): a step counts for a pixel only if all three cubes are not NaN there;
with the covariances Q of the counted steps, ``err_var_x = Qxx - Qxy Qxz / Qyz`` (y, z likewise), ``rho2_x = Qxy Qxz / (Qxx Qyz)``
is the squared correlation of x with the truth, and ``beta_y = Qyz / Qxz``, ``beta_z = Qyz / Qxy`` scale y and z against x
(``beta_x = 1``).  Everything is NaN below ``min_samples`` counted steps and where a cross-covariance is not positive (the
products do not agree in sign: collocation is undefined).  A negative error variance or a ``rho2 > 1`` is a legitimate sampling
outcome of a short record: it is returned as it is and flagged, never clipped.

The caller's job: (1) remove the seasonal cycle first (``drought_index(kind="anomaly")``, ``stl_decompose``) -- a cycle shared
by the three products is "truth" to the method and hides the errors; (2) bring the three cubes to one grid (``coarsen``), for
instance GRACE at 0.25 degrees, ``coarsen(product, (5, 5))`` and the GLDAS storage channel; (3) know that the method assumes
errors that are mutually independent and independent of the truth: two products that share a forcing or a retrieval share
errors, and the shared part is booked as truth.

The kernels are ``csrc/tcol.hip`` over ``csrc/tcol_core.h``: fp32 or fp64 CUDA tensors, time along axis 0, T <= 2048, B <= 2048,
all arithmetic fp64.  There is no CPU path in this module (``kern.tc_estimate_host`` and ``kern.tc_bootstrap_host`` are the
plain C++ twins the tests use); ``bootstrap_indices`` is numpy on the host.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kern as K
from .timeseries import _cube, _series_mask

Tensor = torch.Tensor
L = K.L

STATS = L.TC_STATS


class TripleCollocation(NamedTuple):
    """``err_var``, ``err_std`` (sqrt, NaN where negative), ``rho2``, ``rho`` and ``beta`` are dicts of fp64 maps keyed by the
    three ``names`` (``beta`` of the first is 1 where the pixel is valid); ``cov`` is keyed by the pairs ``(a, b)``; ``n``
    (int32) counts the steps used, ``flags`` (int32) holds the bits of ``FLAGS``, ``valid`` is the bool map of defined
    statistics; ``stats`` is the raw (8, ...) tensor in the order of ``STATS``."""
    names: Tuple[str, str, str]
    err_var: Dict[str, Tensor]
    err_std: Dict[str, Tensor]
    rho2: Dict[str, Tensor]
    rho: Dict[str, Tensor]
    beta: Dict[str, Tensor]
    cov: Dict[Tuple[str, str], Tensor]
    n: Tensor
    flags: Tensor
    valid: Tensor
    stats: Tensor

    def snr_db(self) -> Dict[str, Tensor]:
        """the signal-to-noise ratio of every product in decibels, 10 log10(rho2 / (1 - rho2)) (torch on the device; NaN where
        rho2 is outside (0, 1))"""
        out = {}
        for k, r2 in self.rho2.items():
            ok = (r2 > 0.0) & (r2 < 1.0)
            out[k] = torch.where(ok, 10.0 * torch.log10(r2 / (1.0 - r2)), torch.full_like(r2, float("nan")))
        return out

    def merge_weights(self) -> Dict[str, Tensor]:
        """the inverse-error-variance weights of a least-squares merge of the three products (each rescaled by its beta):
        w_k = (1 / err_var_k) / sum_j (1 / err_var_j) with the error variances on the scale of the first product (err_var_k /
        beta_k^2); they sum to 1 and are NaN where any error variance is <= 0"""
        scaled = [self.err_var[k] / (self.beta[k] * self.beta[k]) for k in self.names]
        ok = (scaled[0] > 0.0) & (scaled[1] > 0.0) & (scaled[2] > 0.0)
        inv = [1.0 / v for v in scaled]
        tot = inv[0] + inv[1] + inv[2]
        nan = torch.full_like(tot, float("nan"))
        return {k: torch.where(ok, i / tot, nan) for k, i in zip(self.names, inv)}


FLAGS = L.TC_FLAGS


class TripleCollocationBootstrap(NamedTuple):
    """``mean``, ``std`` (ddof 1) and ``quantiles`` (Q, ...) of every statistic over its replicates that are not NaN, dicts keyed
    by the names of ``STATS``; ``n_ok`` counts those replicates (int32); ``q`` are the probabilities; ``estimate`` is the point
    estimate; ``replicates`` is the (B, 8, ...) tensor with ``keep_replicates``, else None."""
    q: Tuple[float, ...]
    mean: Dict[str, Tensor]
    std: Dict[str, Tensor]
    quantiles: Dict[str, Tensor]
    n_ok: Dict[str, Tensor]
    estimate: TripleCollocation
    indices: np.ndarray
    replicates: Optional[Tensor]

    def interval(self, stat: str) -> Tuple[Tensor, Tensor]:
        """(lower, upper): the first and the last quantile of ``stat`` (one of ``STATS``), the 95 % percentile interval at the
        default ``q``"""
        if stat not in self.quantiles:
            raise L.GandanetError(f"interval: stat is one of {STATS}, got {stat!r}")
        if len(self.q) < 2:
            raise L.GandanetError("interval: needs two or more probabilities")
        qs = self.quantiles[stat]
        return qs[0], qs[-1]


def _three(x, y, z, fn: str):
    x, y, z = _cube(x, f"{fn} x"), _cube(y, f"{fn} y"), _cube(z, f"{fn} z")
    if x.dim() < 2 or y.shape != x.shape or z.shape != x.shape or y.dtype != x.dtype or z.dtype != x.dtype:
        raise L.GandanetError(f"{fn}: x, y and z are (T, ...) cubes of one shape and dtype, got {tuple(x.shape)} {x.dtype}, "
                              f"{tuple(y.shape)} {y.dtype}, {tuple(z.shape)} {z.dtype}")
    if not 1 <= x.shape[0] <= L.TC_MAX_T:
        raise L.GandanetError(f"{fn}: 1 <= T <= {L.TC_MAX_T}, got T = {x.shape[0]}")
    return x, y, z


def _names(names, fn: str) -> Tuple[str, str, str]:
    names = tuple(names)
    if len(names) != 3 or len(set(names)) != 3:
        raise L.GandanetError(f"{fn}: names are three different keys, got {names!r}")
    return names


def triple_collocation(x: Tensor, y: Tensor, z: Tensor, min_samples: int = 10, mask: Optional[Tensor] = None,
                       names: Sequence[str] = ("x", "y", "z")) -> TripleCollocation:
    """Triple collocation of three (T, ...) cubes of equal shape and dtype (fp32 or fp64 GPU tensors): per pixel the error
    variance of each cube, each cube's squared correlation with the unknown truth and the scale factors of the second and the
    third cube against the first.  ``min_samples`` (>= 3): fewer steps with all three values present give NaN.  ``mask`` (bool
    or uint8, the shape of one time step, nonzero = use the pixel) leaves pixels out.  ``names`` key the result's dicts.

    Before the call: remove the seasonal cycle (``drought_index(kind="anomaly")``, ``stl_decompose``), bring the cubes to one
    grid (``coarsen``), and make sure the three errors can be taken as mutually independent."""
    names = _names(names, "triple_collocation")
    x, y, z = _three(x, y, z, "triple_collocation")
    t_len, tail = x.shape[0], tuple(x.shape[1:])
    m = _series_mask(mask, tail, x.device)
    stats, cov, n, flags = K.tc_estimate(x.reshape(t_len, -1), y.reshape(t_len, -1), z.reshape(t_len, -1), min_samples, m)
    return _result(names, stats, cov, n, flags, tail)


def _result(names, stats, cov, n, flags, tail) -> TripleCollocation:
    st = stats.reshape((len(STATS),) + tail)
    valid = ~torch.isnan(st[6])
    nan = torch.full_like(st[0], float("nan"))
    err_var = {k: st[i] for i, k in enumerate(names)}
    rho2 = {k: st[3 + i] for i, k in enumerate(names)}
    beta = {names[0]: torch.where(valid, torch.ones_like(st[0]), nan), names[1]: st[6], names[2]: st[7]}
    err_std = {k: torch.where(v >= 0.0, torch.sqrt(v.clamp_min(0.0)), nan) for k, v in err_var.items()}
    rho = {k: torch.where(v >= 0.0, torch.sqrt(v.clamp_min(0.0)), nan) for k, v in rho2.items()}
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    cv = {(names[a], names[b]): cov[i].reshape(tail) for i, (a, b) in enumerate(pairs)}
    return TripleCollocation(names, err_var, err_std, rho2, rho, beta, cv, n.reshape(tail), flags.reshape(tail), valid, st)


def bootstrap_indices(T: int, B: int, block: int = 6, seed: int = 0, circular: bool = True) -> np.ndarray:
    """The (T, B) uint16 table of a moving-block bootstrap: column b lists the T steps of replicate b.  Recipe (so that a table
    can be rebuilt elsewhere): with ``nb = ceil(T / block)``, ``starts = np.random.default_rng(seed).integers(0, T, size=(B,
    nb))`` when ``circular`` (a block that runs past the end wraps to step 0, modulo T) or ``integers(0, T - block + 1, ...)``
    when not (``block <= T`` then); block k of replicate b is the steps ``starts[b, k] + 0 .. block - 1``; the nb blocks are
    laid end to end and cut to the first T steps.  ``block=1`` is the ordinary bootstrap; choose ``block`` near the
    decorrelation time of the series (``autocorrelation``)."""
    for v, nm in ((T, "T"), (B, "B"), (block, "block")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise L.GandanetError(f"bootstrap_indices: {nm} is a positive integer, got {v!r}")
    if T > L.TC_MAX_T or B > L.TC_MAX_B:
        raise L.GandanetError(f"bootstrap_indices: T <= {L.TC_MAX_T} and B <= {L.TC_MAX_B}, got T = {T}, B = {B}")
    if not circular and block > T:
        raise L.GandanetError(f"bootstrap_indices: without wrapping block <= T, got block = {block}, T = {T}")
    T, B, block = int(T), int(B), int(block)
    nb = -(-T // block)
    starts = np.random.default_rng(seed).integers(0, T if circular else T - block + 1, size=(B, nb))
    steps = (starts[:, :, None] + np.arange(block)[None, None, :]).reshape(B, nb * block)[:, :T]
    if circular:
        steps = steps % T
    return np.ascontiguousarray(steps.T.astype(np.uint16))


def triple_collocation_bootstrap(x: Tensor, y: Tensor, z: Tensor, B: int = 1000, block: int = 6,
                                 q: Sequence[float] = (0.025, 0.5, 0.975), seed: int = 0, indices=None, *, min_samples: int = 10,
                                 mask: Optional[Tensor] = None, names: Sequence[str] = ("x", "y", "z"), circular: bool = True,
                                 keep_replicates: bool = False, workspace: Optional[Tensor] = None) -> TripleCollocationBootstrap:
    """The moving-block bootstrap of ``triple_collocation`` over time: ``B`` replicates (<= 2048) of blocks of ``block`` steps
    from ``bootstrap_indices(T, B, block, seed, circular)``, or from ``indices``, a (T, B) uint16 table of your own (numpy or
    GPU tensor).  One table serves all pixels, so a replicate keeps its spatial structure.  Per statistic of ``STATS`` and
    pixel: ``mean``, ``std`` and the quantiles at ``q`` (1 .. 8 probabilities) over the replicates that are defined, and
    ``n_ok``, their number.  ``keep_replicates`` returns the (B, 8, ...) tensor as well; ``workspace`` is an optional uint8
    GPU tensor (the results do not depend on its size).  The point estimate comes with the result.  The caller's job is that
    of ``triple_collocation``."""
    names = _names(names, "triple_collocation_bootstrap")
    x, y, z = _three(x, y, z, "triple_collocation_bootstrap")
    t_len, tail = x.shape[0], tuple(x.shape[1:])
    if indices is None:
        indices = bootstrap_indices(t_len, B, block, seed, circular)
    if isinstance(indices, np.ndarray):
        if indices.dtype != np.uint16 or indices.ndim != 2 or indices.shape[0] != t_len:
            raise L.GandanetError(f"triple_collocation_bootstrap: indices is a ({t_len}, B) uint16 table, got {indices.dtype} {indices.shape}")
        table, idx_dev = indices, torch.from_numpy(np.ascontiguousarray(indices)).to(x.device)
    elif isinstance(indices, Tensor) and indices.is_cuda and indices.dtype == torch.uint16:
        idx_dev = indices.contiguous()
        table = idx_dev.cpu().numpy()
    else:
        raise L.GandanetError("triple_collocation_bootstrap: indices is a (T, B) uint16 numpy array or GPU tensor")
    m = _series_mask(mask, tail, x.device)
    x2, y2, z2 = x.reshape(t_len, -1), y.reshape(t_len, -1), z.reshape(t_len, -1)
    est = _result(names, *K.tc_estimate(x2, y2, z2, min_samples, m), tail)
    summary, n_ok, rep = K.tc_bootstrap(x2, y2, z2, idx_dev, q, min_samples, m, keep_replicates, workspace)
    nq = summary.shape[1] - 2
    s = summary.reshape((len(STATS), 2 + nq) + tail)
    return TripleCollocationBootstrap(tuple(float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64))),
                                      {k: s[i, 0] for i, k in enumerate(STATS)}, {k: s[i, 1] for i, k in enumerate(STATS)},
                                      {k: s[i, 2:] for i, k in enumerate(STATS)},
                                      {k: n_ok[i].reshape(tail) for i, k in enumerate(STATS)}, est, table,
                                      rep.reshape((rep.shape[0], len(STATS)) + tail) if rep is not None else None)
