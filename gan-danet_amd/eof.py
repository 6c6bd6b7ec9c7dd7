"""EOF / principal-component analysis of a (T, ...) cube on the device: which few patterns carry the variance of a TWSA
field, what their time series are, and what the field looks like with the tail of the modes cut off.  With T time steps
(months) and M pixels, T << M, the work is the T x T Gram matrix of the weighted anomalies -- one read of the cube on the
fp64 matrix pipe (``gd_eof_gram``) -- followed by one more read per 16 modes for the pattern maps (``gd_eof_project``).
The eigen-decomposition of the Gram matrix, at most 256 x 256 doubles and the only copy to the host, is
``numpy.linalg.eigh``.  Without this module the route was a copy of the cube to the host and ``numpy.linalg.svd`` of a
181 x 396 000 matrix.

The kernels are ``csrc/eof.hip`` over ``csrc/eof_core.h`` (``include/gandanet.h``, "EOF analysis"): fp32 or fp64 CUDA
tensors, time along axis 0, all arithmetic fp64, no atomics (the same bits on every run).  There is no CPU path in this
module (``kern.eof_*_host`` are the plain C++ twins the tests use).
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import kern as K
from .timeseries import _cube, _series_mask

Tensor = torch.Tensor
L = K.L


def _weights(weights, lat, shape, device) -> Optional[Tensor]:
    if weights is not None and lat is not None:
        raise L.GandanetError("eof_analysis: give weights or lat, not both")
    if lat is not None:
        if len(shape) != 2:
            raise L.GandanetError(f"eof_analysis: lat needs a (T, H, W) cube, got time steps of shape {tuple(shape)}")
        lat = np.asarray(lat.detach().cpu() if isinstance(lat, Tensor) else lat, dtype=np.float64)
        if lat.shape != (shape[0],):
            raise L.GandanetError(f"eof_analysis: lat holds one latitude (degrees) per row ({shape[0]}), got {lat.shape}")
        weights = torch.from_numpy(np.cos(np.deg2rad(lat))).to(device)[:, None].expand(shape)   # numpy's cos, as a caller's own
    if weights is None:
        return None
    if not isinstance(weights, Tensor) or not weights.is_cuda:
        raise L.GandanetError("eof_analysis: the weights are a GPU tensor (there is no CPU path)")
    if tuple(weights.shape) != tuple(shape):
        raise L.GandanetError(f"eof_analysis: weights of the shape of one time step {tuple(shape)}, got {tuple(weights.shape)}")
    return weights.to(torch.float64).contiguous().reshape(-1)


def fix_signs(u: np.ndarray) -> np.ndarray:
    """every column of ``u`` with the sign that makes its entry of largest magnitude (the first one on ties) positive"""
    u = u.copy()
    for k in range(u.shape[1]):
        if u[np.argmax(np.abs(u[:, k])), k] < 0:
            u[:, k] = -u[:, k]
    return u


def gram_modes(G: np.ndarray):
    """(lambda descending, U with fixed signs) of the symmetric Gram matrix ``G``: ``numpy.linalg.eigh`` in fp64"""
    lam, u = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    order = np.argsort(-lam, kind="stable")
    return lam[order], fix_signs(u[:, order])


class EOFResult:
    """The result of ``eof_analysis``.  K modes of a cube with T time steps, T' of them kept:

    ``eofs`` (K, *shape) fp64, of unit norm in the weighted space (sum over the valid pixels of eofs[k]^2 = 1), NaN where
    invalid; ``pcs`` (T, K) = sqrt(lambda_k) u_k, NaN rows at the dropped steps, so that the weighted anomalies are
    sum_k pcs[t, k] eofs[k]; ``eigenvalues`` lambda_k / (T' - ddof); ``variance_fraction`` lambda_k / trace G;
    ``total_variance`` trace G / (T' - ddof); ``north_error`` eigenvalue sqrt(2 / T') (North et al. 1982);
    ``mean`` (*shape) fp64 and ``valid`` (*shape) bool; ``n_valid``; ``kept_steps`` (T) bool; ``gram`` the (T', T') matrix
    on the host.  The result keeps a reference to the (gathered) cube for ``eofs_as_covariance``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_modes(self) -> int:
        return self.eofs.shape[0]

    def _flat(self):
        return self.mean.reshape(-1), self.valid.reshape(-1).to(torch.uint8)

    def eofs_as_covariance(self) -> Tensor:
        """(K, *shape) fp64: the covariance of every pixel's series with the standardised PC of every mode, in the units
        of the cube (``gd_eof_project`` with the standardised PCs over T' - ddof, without the weights)"""
        mean, valid = self._flat()
        std = np.sqrt(self._lam[: self.n_modes] / self._dof)
        with np.errstate(divide="ignore", invalid="ignore"):
            coef = np.where(std > 0, self._pcs_kept / std / self._dof, 0.0)
        return _project(self._x, mean, valid, coef, None, False).reshape((self.n_modes,) + self.shape)

    def reconstruct(self, n_modes: Optional[int] = None, dtype=None) -> Tensor:
        """the cube rebuilt from the leading ``n_modes`` (default all, at most 16 in one call): mean + sum_k pcs[t, k]
        eofs[k] / sqrt(weight), (T, *shape) in ``dtype`` (default the dtype of the analysed cube), NaN at invalid pixels and
        dropped steps"""
        k = self.n_modes if n_modes is None else int(n_modes)
        if not 1 <= k <= min(self.n_modes, L.EOF_MAX_K):
            raise L.GandanetError(f"EOFResult.reconstruct: n_modes must be 1 .. {min(self.n_modes, L.EOF_MAX_K)}, got {k} (this result "
                                  f"holds {self.n_modes} modes; one call sums at most {L.EOF_MAX_K}, because every element is rounded once)")
        mean, valid = self._flat()
        dev = self.eofs.device
        pcs = torch.from_numpy(np.ascontiguousarray(self._pcs_kept[:, :k])).to(dev)
        out = K.eof_reconstruct(self.eofs[:k].reshape(k, -1), pcs, mean, valid, self._weight, dtype or self._x.dtype)
        if bool(self.kept_steps.all()):
            return out.reshape((out.shape[0],) + self.shape)
        full = torch.full((self.kept_steps.numel(), out.shape[1]), float("nan"), device=dev, dtype=out.dtype)
        full[self.kept_steps] = out
        return full.reshape((full.shape[0],) + self.shape)

    def pattern_correlation(self, other: "EOFResult") -> Tensor:
        """(K) fp64: the weighted, centred correlation of every mode's pattern with that of ``other`` (same grid) over the
        pixels valid in both, K the smaller number of modes"""
        if self.shape != other.shape:
            raise L.GandanetError(f"pattern_correlation: patterns of {self.shape} against {other.shape}")
        k = min(self.n_modes, other.n_modes)
        both = (self.valid & other.valid).reshape(-1)
        w = (torch.ones_like(self.mean.reshape(-1)) if self._weight is None else self._weight) * both
        a = torch.where(both, self.eofs[:k].reshape(k, -1), torch.zeros((), dtype=torch.float64, device=w.device))
        b = torch.where(both, other.eofs[:k].reshape(k, -1), torch.zeros((), dtype=torch.float64, device=w.device))
        sw = w.sum()
        a = a - (a * w).sum(1, keepdim=True) / sw
        b = b - (b * w).sum(1, keepdim=True) / sw
        return (w * a * b).sum(1) / torch.sqrt((w * a * a).sum(1) * (w * b * b).sum(1))


def _project(x2: Tensor, mean: Tensor, valid: Tensor, coef: np.ndarray, weight: Optional[Tensor], use_weight: bool) -> Tensor:
    """``gd_eof_project`` for any number of columns, GD_EOF_MAX_K at a time"""
    k_all = coef.shape[1]
    out = torch.empty((k_all, x2.shape[1]), device=x2.device, dtype=torch.float64)
    for k0 in range(0, k_all, L.EOF_MAX_K):
        c = torch.from_numpy(np.ascontiguousarray(coef[:, k0:k0 + L.EOF_MAX_K])).to(x2.device)
        K.eof_project(x2, mean, valid, c, weight, use_weight, out=out[k0:k0 + c.shape[1]])
    return out


def eof_analysis(x: Tensor, n_modes: int = 4, *, weights: Optional[Tensor] = None, lat=None, mask: Optional[Tensor] = None,
                 center: bool = True, ddof: int = 1, drop_empty_steps: bool = True) -> EOFResult:
    """EOF analysis of ``x`` (T, ...), fp32 or fp64 on the GPU, time along axis 0.

    ``weights``: area weights >= 0 of the shape of one time step (a pixel of weight 0 is left out); ``lat`` (H,) in degrees
    is shorthand for cos(lat) broadcast over the columns of a (T, H, W) cube.  ``mask`` (bool or uint8, nonzero = use).  A
    pixel with a NaN or an infinity at any kept step is left out whole.  ``center`` removes every pixel's time mean.
    ``drop_empty_steps``: a time step that is NaN at every unmasked pixel (GRACE has whole months missing) is removed
    before the analysis; its row of ``pcs`` is NaN.  At most ``L.EOF_MAX_T`` steps may remain.  Raises ``GandanetError``
    with no valid pixel or fewer than 2 kept steps."""
    x = _cube(x, "eof_analysis")
    if x.dim() < 2:
        raise L.GandanetError("eof_analysis: expected a (T, ...) cube with at least one space axis")
    shape = tuple(x.shape[1:])
    t_all, m = x.shape[0], math.prod(shape)
    if ddof not in (0, 1):
        raise L.GandanetError(f"eof_analysis: ddof must be 0 or 1, got {ddof!r}")
    weight = _weights(weights, lat, shape, x.device)
    mask_flat = _series_mask(mask, shape, x.device)
    x2 = x.reshape(t_all, m)
    kept = torch.ones(t_all, dtype=torch.bool, device=x.device)
    if drop_empty_steps:
        gap = torch.isnan(x2)
        if mask_flat is not None:
            gap = gap | (mask_flat == 0)
        kept = ~gap.all(dim=1)
        del gap
        if not bool(kept.all()):
            x2 = x2.index_select(0, kept.nonzero().reshape(-1))
    t_kept = x2.shape[0]
    if t_kept < 2:
        raise L.GandanetError(f"eof_analysis: {t_kept} time steps are left, at least 2 are needed")
    if t_kept > L.EOF_MAX_T:
        raise L.GandanetError(f"eof_analysis: {t_kept} time steps, at most {L.EOF_MAX_T} are supported")
    if t_kept - ddof < 1:
        raise L.GandanetError(f"eof_analysis: {t_kept} time steps with ddof = {ddof}")
    k_modes = int(n_modes)
    if not 1 <= k_modes <= t_kept:
        raise L.GandanetError(f"eof_analysis: n_modes must be 1 .. {t_kept}, got {n_modes!r}")
    mean, valid = K.eof_prepare(x2, mask_flat, weight, center)
    n_valid = int(valid.sum().item())
    if n_valid == 0:
        raise L.GandanetError("eof_analysis: no valid pixel (every series is masked, has a gap or has no weight)")
    gram = K.eof_gram(x2, mean, valid, weight).cpu().numpy()
    lam, u = gram_modes(gram)
    lam = np.maximum(lam, 0.0)
    trace = float(np.trace(gram))
    dof = float(t_kept - ddof)
    lk, uk = lam[:k_modes], u[:, :k_modes]
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = np.where(lk > 0, uk / np.sqrt(lk), 0.0)          # U Lambda^-1/2; a null mode has a zero pattern
    eofs = _project(x2, mean, valid, coef, weight, weight is not None)
    pcs_kept = uk * np.sqrt(lk)
    pcs = np.full((t_all, k_modes), np.nan)
    pcs[kept.cpu().numpy()] = pcs_kept
    dev = x.device
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    eig = lk / dof
    return EOFResult(eofs=eofs.reshape((k_modes,) + shape), pcs=to_dev(pcs), eigenvalues=to_dev(eig),
                     variance_fraction=to_dev(lk / trace if trace > 0 else np.full(k_modes, np.nan)), total_variance=trace / dof,
                     north_error=to_dev(eig * math.sqrt(2.0 / t_kept)), mean=mean.reshape(shape), valid=valid.reshape(shape).bool(),
                     n_valid=n_valid, kept_steps=kept, gram=gram, shape=shape, _x=x2, _weight=weight, _lam=lam, _dof=dof,
                     _pcs_kept=pcs_kept)
