"""Singular spectrum analysis of every pixel series of a cube, on the device: the data-adaptive counterpart of
``harmonic_fit`` and ``stl_decompose`` (a trend and oscillatory pairs whose amplitude may change over the record), and the
standard repair of gaps in TIME of the GRACE literature (Kondrashov & Ghil 2006; Yi & Sneeuw 2021 for the eleven months
between GRACE and GRACE-FO).  ``filters.fill_masked`` repairs gaps in space within one plane; ``ssa_fill`` repairs a series
along time, after which the pixels that ``eof_analysis`` drops for a single gap can take part.

The kernel is ``csrc/ssa.hip`` over ``csrc/ssa_core.h`` (``include/gandanet.h``, "Singular spectrum analysis", holds the
definitions in full): fp32 or fp64 CUDA tensors, time along axis 0, all arithmetic fp64; one wave per series, the lag
covariance, a cyclic Jacobi eigen-solver and the diagonal averaging from LDS.  There is no CPU path in this module
(``kern.ssa_decompose_host`` and ``kern.ssa_fill_host`` are the plain C++ twins the tests use).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import kern as K
from .timeseries import _cube, _series_mask

Tensor = torch.Tensor
L = K.L

MAPS = L.SSA_MAPS
FLAGS = L.SSA_FLAGS
_GROUP_CHUNK = 4 * L.SSA_CHUNK   # pixels per pass when only summed groups are wanted


def _int(v, lo: int, hi: int, fn: str, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise L.GandanetError(f"{fn}: {name} is an integer in {lo} .. {hi}, got {v!r}")
    return int(v)


def _input(x, window, rank, method, fn: str):
    x = _cube(x, fn)
    window = _int(window, 2, L.SSA_MAX_M, fn, "window")
    t_len = x.shape[0]
    if not 2 * window - 1 <= t_len <= L.SSA_MAX_T:
        raise L.GandanetError(f"{fn}: 2 * window - 1 <= T <= {L.SSA_MAX_T}, got T = {t_len} at window = {window}")
    rank = _int(rank, 1, min(window, L.SSA_MAX_RANK), fn, "n_components" if fn == "ssa_decompose" else "rank")
    if method not in L.SSA_METHODS:
        raise L.GandanetError(f"{fn}: method is one of {sorted(L.SSA_METHODS)}, got {method!r}")
    return x, t_len, tuple(x.shape[1:]), window, rank


class SSAResult:
    """What ``ssa_decompose`` returns.  ``eigenvalues`` and ``variance_fraction`` are ``(r, ...)``; ``n``, ``mean``, ``sd``,
    ``trace``, ``sweeps`` and ``flags`` (int32, the bits of ``ssa.FLAGS``) have the shape of one time step; ``components`` is
    ``(r, T, ...)`` or None, ``groups`` ``(len(groups), T, ...)`` or None.  All float maps are fp64 and NaN where the series is
    degenerate."""

    def __init__(self, eigenvalues, maps, tail, components=None, groups=None):
        named = dict(zip(MAPS, maps))
        self.eigenvalues = eigenvalues.reshape((-1,) + tail)
        self.trace = named["trace"].reshape(tail)
        self.variance_fraction = self.eigenvalues / self.trace
        self.n, self.mean, self.sd, self.sweeps = (named[k].reshape(tail) for k in ("n", "mean", "sd", "sweeps"))
        self.flags = named["flags"].to(torch.int32).reshape(tail)
        self.components = components
        self.groups = groups

    def reconstruct(self, group: Optional[Sequence[int]] = None) -> Tensor:
        """mean + the sum of the components listed in ``group`` (default: all r), added in the order listed, ``(T, ...)``
        fp64; needs ``components=True``"""
        if self.components is None:
            raise L.GandanetError("SSAResult.reconstruct: ask ssa_decompose for components=True")
        return _group_sum(self.components, range(self.components.shape[0]) if group is None else group, "reconstruct") + self.mean

    def pairs(self, rtol: float = 0.05) -> Tensor:
        """bool ``(r - 1, ...)``, on the device: entry k says that eigenvalues k and k + 1 lie closer than ``rtol`` times
        eigenvalue k -- the signature of an oscillatory pair (a sinusoid fills two components of nearly equal variance)"""
        rtol = float(rtol)
        if not rtol > 0.0:
            raise L.GandanetError(f"SSAResult.pairs: rtol must be > 0, got {rtol!r}")
        ev = self.eigenvalues
        return (ev[:-1] - ev[1:]) <= rtol * ev[:-1]


class SSAFill(NamedTuple):
    filled: Tensor
    filled64: Optional[Tensor]
    eigenvalues: Tensor
    iterations: Tensor
    converged: Tensor
    last_change: Tensor
    n_gaps: Tensor
    flags: Tensor


def _groups(groups, rank: int):
    try:
        out = [[_int(k, 0, rank - 1, "ssa_decompose", "a component of a group") for k in g] for g in groups]
    except TypeError:
        raise L.GandanetError(f"ssa_decompose: groups is a list of lists of component numbers, got {groups!r}") from None
    if not out or any(len(g) == 0 for g in out):
        raise L.GandanetError(f"ssa_decompose: groups is a non-empty list of non-empty lists, got {groups!r}")
    return out


def _group_sum(rc: Tensor, group, fn: str) -> Tensor:
    idx = [_int(k, 0, rc.shape[0] - 1, fn, "a component of a group") for k in group]
    if not idx:
        raise L.GandanetError(f"{fn}: an empty group")
    total = rc[idx[0]].clone()
    for k in idx[1:]:
        total += rc[k]
    return total


def ssa_decompose(x: Tensor, window: int, n_components: int = 6, method: str = "bk", mask: Optional[Tensor] = None,
                  components: bool = False, groups=None) -> SSAResult:
    """SSA of every COMPLETE series ``x[:, ...]``: the leading ``n_components`` (r <= min(window, 16)) eigenpairs of the
    ``window`` x ``window`` lag covariance (2 <= window <= 64, 2 * window - 1 <= T <= 2048) of the series centred by its mean.
    ``method``: "bk" (Broomhead & King: the trajectory matrix; eigenvalues are its squared singular values / K) or "vg"
    (Vautard & Ghil: the Toeplitz estimate).  ``mask`` (bool or uint8, the shape of one time step, nonzero = use the pixel).
    ``components=True`` also returns the r reconstructed components ``(r, T, ...)`` (r copies of the cube);
    ``groups=[[0], [1, 2]]`` returns only the sums of the listed components, one ``(T, ...)`` slab per group, added in the
    order listed -- the pixels are then walked in chunks so that the r components of the whole cube never exist at once.
    A series WITH A GAP (a NaN) is not decomposed: its outputs are NaN and its ``flags`` carry ``FLAGS["gaps"]``; run
    ``ssa_fill`` first.  A constant, masked or non-finite series is NaN and flagged likewise.  See ``SSAResult``."""
    x, t_len, tail, window, rank = _input(x, window, n_components, method, "ssa_decompose")
    mask = _series_mask(mask, tail, x.device)
    x2 = x.reshape(t_len, -1)
    if groups is None:
        eig, maps, rc = K.ssa_decompose(x2, window, rank, method, mask, bool(components))
        return SSAResult(eig, maps, tail, None if rc is None else rc.reshape((rank, t_len) + tail))
    groups = _groups(groups, rank)
    p = x2.shape[1]
    eig = torch.empty((rank, p), device=x.device, dtype=torch.float64)
    maps = torch.empty((len(MAPS), p), device=x.device, dtype=torch.float64)
    out = torch.empty((len(groups), t_len, p), device=x.device, dtype=torch.float64)
    for p0 in range(0, p, _GROUP_CHUNK):
        p1 = min(p, p0 + _GROUP_CHUNK)
        e, m, rc = K.ssa_decompose(x2[:, p0:p1].contiguous(), window, rank, method, None if mask is None else mask[p0:p1].contiguous(), True)
        eig[:, p0:p1], maps[:, p0:p1] = e, m
        for g, group in enumerate(groups):
            out[g, :, p0:p1] = _group_sum(rc, group, "ssa_decompose")
    return SSAResult(eig, maps, tail, None, out.reshape((len(groups), t_len) + tail))


def ssa_fill(x: Tensor, window: int, rank: int = 4, tol: float = 1e-3, max_iter: int = 20, min_valid: Optional[int] = None,
             method: str = "bk", mask: Optional[Tensor] = None, filled64: bool = False) -> SSAFill:
    """Fill the gaps (NaN) of every series ``x[:, ...]`` along time by iterative SSA (Kondrashov & Ghil 2006).  The gaps of the
    centred series start at 0; for each stage q = 1 .. ``rank`` the series is decomposed (``window``, ``method`` as in
    ``ssa_decompose``) and its gap samples -- only those -- are overwritten with the sum of the leading q reconstructed
    components, until the largest change is <= ``tol`` * sd (sd of the valid samples) or ``max_iter`` (1 .. 200) iterations
    have run; the next stage starts from the result.  ``min_valid`` (default 2 * window, at least 2): series with fewer valid
    samples are not filled.

    Returns ``filled`` (the dtype of ``x``: the input at every valid sample, bit for bit, and the fill at the gaps; NaN
    everywhere for a series that is masked, constant, non-finite or too short), ``filled64`` (fp64, on request),
    ``eigenvalues`` ``(rank, ...)`` of the last decomposition, ``iterations`` (int32, total over the stages), ``converged``
    (bool: every stage met ``tol``), ``last_change``, ``n_gaps`` (int32) and ``flags`` (int32, the bits of ``ssa.FLAGS``).

    Three limits.  THE MEAN IS HELD FIXED at the mean of the valid samples (Kondrashov & Ghil re-estimate it in every
    iteration; this version does not).  THE STATISTICAL UNCERTAINTY of the filled values IS NOT ESTIMATED: they are a smooth
    continuation of the leading modes, not data.  A GAP MUCH LONGER THAN ``window`` is filled by the leading modes only,
    which means trend plus cycle."""
    x, t_len, tail, window, rank = _input(x, window, rank, method, "ssa_fill")
    tol = float(tol)
    if not (np.isfinite(tol) and tol > 0.0):
        raise L.GandanetError(f"ssa_fill: tol must be finite and > 0, got {tol!r}")
    max_iter = _int(max_iter, 1, L.SSA_MAX_ITER, "ssa_fill", "max_iter")
    min_valid = 2 * window if min_valid is None else _int(min_valid, 2, L.SSA_MAX_T, "ssa_fill", "min_valid")
    f64, eig, maps = K.ssa_fill(x.reshape(t_len, -1), window, rank, method, _series_mask(mask, tail, x.device), tol, max_iter, min_valid)
    named = dict(zip(MAPS, maps))
    flags = named["flags"].to(torch.int32)
    f64 = f64.reshape((t_len,) + tail)
    filled = f64 if x.dtype == torch.float64 else f64.to(x.dtype)
    degenerate = FLAGS["masked"] | FLAGS["few"] | FLAGS["constant"] | FLAGS["nonfinite"]
    return SSAFill(filled, f64 if filled64 else None, eig.reshape((rank,) + tail), named["iterations"].nan_to_num(nan=0.0).to(torch.int32).reshape(tail),
                   ((flags & (degenerate | FLAGS["iter"])) == 0).reshape(tail), named["last_change"].reshape(tail),
                   named["n_gaps"].to(torch.int32).reshape(tail), flags.reshape(tail))
