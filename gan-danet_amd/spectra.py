"""Spatial power and cross spectra on the device: does a super-resolved field carry real variance at the scales it claims to
resolve?  The radially averaged power spectrum of every field, the spectrum of a product over that of a reference, the
spectral coherence between the two and the effective resolution read off those curves -- the one diagnostic that
penalises blur, which every point-wise metric rewards.

The transform is a 2-D DFT written as matrix products on the fp64 matrix pipe (``csrc/spectra.hip`` over
``csrc/spectra_core.h``; ``include/gandanet.h``, "Spatial spectra", holds the definitions): fill, detrend and taper are
applied as the field is loaded, |Z|^2 is binned in the kernel's epilogue and no spectrum is stored, sizes need not be
powers of two, and every sum has a fixed order (the same bits on every run).  fp32 or fp64 CUDA tensors, all arithmetic
fp64, not differentiable.  There is no CPU path in this module (``kern.spec_*_host`` are the plain C++ twins the tests
use).  Results cross to the host as one copy of (T, nbins)-sized arrays.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np
import torch

from . import kern as K

Tensor = torch.Tensor
L = K.L


def window_vector(window, n: int) -> Optional[np.ndarray]:
    """the fp64 taper of ``n`` points: None / "none", "hann", "tukey" or ("tukey", alpha) (periodic forms), or an array"""
    if window is None or (isinstance(window, str) and window == "none"):
        return None
    if isinstance(window, str) or (isinstance(window, tuple) and isinstance(window[0], str)):
        name, alpha = (window, 0.5) if isinstance(window, str) else (window[0], float(window[1]))
        r = np.arange(n, dtype=np.float64) / n
        if name == "hann":
            return 0.5 - 0.5 * np.cos(2.0 * np.pi * r)
        if name == "tukey":
            if not 0.0 <= alpha <= 1.0:
                raise L.GandanetError(f"spectra: tukey alpha in [0, 1], got {alpha}")
            w = np.ones(n)
            if alpha > 0.0:
                d = np.minimum(r, 1.0 - r)
                edge = d < alpha / 2.0
                w[edge] = 0.5 - 0.5 * np.cos(2.0 * np.pi * d[edge] / alpha)
            return w
        raise L.GandanetError(f"spectra: window is 'none', 'hann', 'tukey', ('tukey', alpha) or an array, got {window!r}")
    w = np.ascontiguousarray(window.detach().cpu().numpy() if isinstance(window, Tensor) else window, dtype=np.float64)
    if w.shape != (n,):
        raise L.GandanetError(f"spectra: a window array holds {n} entries, got {w.shape}")
    return w


def _windows(window, H: int, W: int):
    if isinstance(window, (tuple, list)) and len(window) == 2 and not isinstance(window[0], str):
        return window_vector(window[0], H), window_vector(window[1], W)
    return window_vector(window, H), window_vector(window, W)


@dataclass
class _Plan:
    lead: tuple
    T: int
    H: int
    W: int
    nbins: int
    k: np.ndarray
    count: np.ndarray
    dx: float
    dy: float
    mask: Optional[Tensor]
    wy: Optional[Tensor]
    wx: Optional[Tensor]
    twh: Tensor
    tww: Tensor
    bins: Tensor
    detrend: str


def _fields(x, name: str) -> Tensor:
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise L.GandanetError(f"{name}: expected a GPU tensor (there is no CPU path)")
    if x.dtype not in (torch.float32, torch.float64) or x.dim() not in (2, 3, 4) or x.numel() == 0:
        raise L.GandanetError(f"{name}: expected a non-empty float32 / float64 (H, W), (T, H, W) or (T, C, H, W) tensor, got "
                              f"{x.dtype} {tuple(x.shape)}")
    return x.detach().contiguous()


def _plan(x: Tensor, dx, dy, mask, detrend, window, nbins) -> _Plan:
    H, W = x.shape[-2:]
    lead = tuple(x.shape[:-2])
    if H > L.SPEC_MAX_H or W > L.SPEC_MAX_W:
        raise L.GandanetError(f"spectra: fields of at most {L.SPEC_MAX_H} x {L.SPEC_MAX_W}, got {H} x {W}")
    if detrend not in L.SPEC_DETREND:
        raise L.GandanetError(f"spectra: detrend is one of {sorted(L.SPEC_DETREND)}, got {detrend!r}")
    dx, dy = float(dx), float(dy)
    if not (dx > 0 and dy > 0 and math.isfinite(dx) and math.isfinite(dy)):
        raise L.GandanetError(f"spectra: dx and dy are positive, got {dx}, {dy}")
    kmax = 0.0
    if nbins is None:
        nbins, kmax = K.spec_default_bins(H, W, dy, dx), 0.5 / max(dx, dy)
    bins, kc, count = K.spec_bins_host(H, W, dy, dx, int(nbins), kmax)
    wy, wx = _windows(window, H, W)
    dev = x.device
    if mask is not None:
        if not isinstance(mask, Tensor) or not mask.is_cuda or tuple(mask.shape) != (H, W):
            raise L.GandanetError(f"spectra: the mask is a GPU tensor of shape ({H}, {W})")
        mask = (mask != 0).to(torch.uint8).contiguous().reshape(-1)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    return _Plan(lead, int(np.prod(lead, dtype=np.int64)) if lead else 1, H, W, int(nbins), kc, count, dx, dy, mask, up(wy), up(wx),
                 up(K.spec_twiddle_host(H)), up(K.spec_twiddle_host(W)), up(bins), detrend)


def _loglog_slope(k, p, kmin, kmax) -> float:
    k, p = np.asarray(k, dtype=np.float64), np.asarray(p, dtype=np.float64)
    sel = np.isfinite(p) & (p > 0) & (k > 0)
    if kmin is not None:
        sel &= k >= kmin
    if kmax is not None:
        sel &= k <= kmax
    if sel.sum() < 2:
        return float("nan")
    return float(np.polyfit(np.log(k[sel]), np.log(p[sel]), 1)[0])


@dataclass
class Spectrum:
    """``k`` (nbins) bin centres in cycles per unit of dx; ``power`` (..., nbins): the sum of P over each bin; ``count``
    (nbins) wavenumbers per bin; ``dropped`` (...): power beyond the bins; ``variance`` (...) = power.sum(-1) + dropped, the
    windowed variance of the valid pixels (Parseval); ``valid_fraction`` (...); ``power_2d`` (..., H, W // 2 + 1) on the
    device with ``two_d=True``.  Host arrays otherwise."""
    k: np.ndarray
    power: np.ndarray
    count: np.ndarray
    dropped: np.ndarray
    variance: np.ndarray
    valid_fraction: np.ndarray
    dx: float
    dy: float
    shape: tuple
    coef: np.ndarray
    power_2d: Optional[Tensor] = None

    @property
    def wavelength(self) -> np.ndarray:
        return 1.0 / self.k

    def mean(self) -> np.ndarray:
        """the mean spectrum over the leading axes, fields without a valid pixel (NaN rows) left out"""
        p = self.power.reshape(-1, self.power.shape[-1])
        ok = ~np.isnan(p).any(axis=1)
        return p[ok].mean(axis=0) if ok.any() else np.full(p.shape[1], np.nan)

    def slope(self, kmin: Optional[float] = None, kmax: Optional[float] = None) -> float:
        """the log-log least-squares slope of the mean spectrum between ``kmin`` and ``kmax``"""
        return _loglog_slope(self.k, self.mean(), kmin, kmax)


@dataclass
class CrossSpectrum:
    """``power_a``, ``power_b``, ``co``, ``quad``: (..., nbins) bin sums of P_aa, P_bb and of the real and imaginary part of
    weight Z_a conj(Z_b) / (H W sqrt(S_a S_b))"""
    k: np.ndarray
    power_a: np.ndarray
    power_b: np.ndarray
    co: np.ndarray
    quad: np.ndarray
    count: np.ndarray
    dropped: np.ndarray
    dx: float
    dy: float

    @property
    def wavelength(self) -> np.ndarray:
        return 1.0 / self.k

    def _sum(self, a: np.ndarray, time_mean: bool) -> np.ndarray:
        if not time_mean:
            return a
        a = a.reshape(-1, a.shape[-1])
        ok = ~np.isnan(self.power_a.reshape(a.shape)).any(axis=1)
        return a[ok].sum(axis=0)

    def coherence(self, time_mean: bool = True) -> np.ndarray:
        """|sum (co + i quad)|^2 / (sum P_a sum P_b), the sums over the fields (``time_mean``) or none"""
        co, qd = self._sum(self.co, time_mean), self._sum(self.quad, time_mean)
        pa, pb = self._sum(self.power_a, time_mean), self._sum(self.power_b, time_mean)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (co * co + qd * qd) / (pa * pb)

    def phase(self, time_mean: bool = True) -> np.ndarray:
        return np.arctan2(self._sum(self.quad, time_mean), self._sum(self.co, time_mean))

    def ratio(self, time_mean: bool = True) -> np.ndarray:
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._sum(self.power_a, time_mean) / self._sum(self.power_b, time_mean)


def power_spectrum(x: Tensor, *, dx: float = 1.0, dy: float = 1.0, mask: Optional[Tensor] = None, detrend: str = "mean",
                   window="hann", nbins: Optional[int] = None, two_d: bool = False) -> Spectrum:
    """the radially binned spatial power spectrum of every field of ``x`` ((H, W), (T, H, W) or (T, C, H, W), fp32 / fp64 on
    the device).  ``dx``, ``dy``: grid spacing; ``mask`` (H, W): nonzero = use; ``detrend``: "none", "mean", "plane";
    ``window``: "none", "hann", "tukey", ("tukey", alpha), an array pair (wy, wx); ``nbins``: default up to the smaller
    Nyquist wavenumber."""
    x = _fields(x, "power_spectrum")
    p = _plan(x, dx, dy, mask, detrend, window, nbins)
    x3 = x.reshape(p.T, p.H, p.W)
    coef, S = K.spec_prepare(x3, p.mask, p.wy, p.wx, p.detrend)
    p2d = torch.empty((p.T, p.H, p.W // 2 + 1), device=x.device, dtype=torch.float64) if two_d else None
    out = torch.empty((p.T, p.nbins + 6), device=x.device, dtype=torch.float64)        # one copy: power | dropped | S, n | coef
    power, dropped = K.spec_power(x3, coef, S, p.twh, p.tww, p.bins, p.nbins, p.mask, p.wy, p.wx, p2d=p2d)
    out[:, :p.nbins], out[:, p.nbins], out[:, p.nbins + 1:p.nbins + 3], out[:, p.nbins + 3:] = power, dropped, S, coef
    h = out.cpu().numpy()
    pw, dr, n = h[:, :p.nbins].reshape(p.lead + (p.nbins,)), h[:, p.nbins].reshape(p.lead), h[:, p.nbins + 2].reshape(p.lead)
    return Spectrum(p.k, pw, p.count, dr, pw.sum(axis=-1) + dr, n / (p.H * p.W), p.dx, p.dy, (p.H, p.W),
                    h[:, p.nbins + 3:].reshape(p.lead + (3,)), None if p2d is None else p2d.reshape(p.lead + p2d.shape[1:]))


def cross_spectrum(a: Tensor, b: Tensor, *, dx: float = 1.0, dy: float = 1.0, mask: Optional[Tensor] = None, detrend: str = "mean",
                   window="hann", nbins: Optional[int] = None) -> CrossSpectrum:
    """the power, co- and quadrature spectra of two cubes of one shape and dtype, each detrended on its own"""
    a, b = _fields(a, "cross_spectrum"), _fields(b, "cross_spectrum")
    if a.shape != b.shape or a.dtype != b.dtype:
        raise L.GandanetError(f"cross_spectrum: a {tuple(a.shape)} {a.dtype} vs b {tuple(b.shape)} {b.dtype}")
    p = _plan(a, dx, dy, mask, detrend, window, nbins)
    a3, b3 = a.reshape(p.T, p.H, p.W), b.reshape(p.T, p.H, p.W)
    ca, sa = K.spec_prepare(a3, p.mask, p.wy, p.wx, p.detrend)
    cb, sb = K.spec_prepare(b3, p.mask, p.wy, p.wx, p.detrend)
    buf = torch.empty(4 * p.T * p.nbins + 4 * p.T, device=a.device, dtype=torch.float64)
    out, dropped = buf[:4 * p.T * p.nbins].view(4, p.T, p.nbins), buf[4 * p.T * p.nbins:].view(p.T, 4)
    K.spec_cross(a3, b3, ca, sa, cb, sb, p.twh, p.tww, p.bins, p.nbins, p.mask, p.wy, p.wx, out=out, dropped=dropped)
    h = buf.cpu().numpy()
    o = h[:4 * p.T * p.nbins].reshape((4,) + p.lead + (p.nbins,))
    return CrossSpectrum(p.k, o[0], o[1], o[2], o[3], p.count, h[4 * p.T * p.nbins:].reshape(p.lead + (4,)), p.dx, p.dy)


def spectral_ratio(spec_hi: Spectrum, spec_lo: Spectrum):
    """(k, mean power of ``spec_hi`` / mean power of ``spec_lo``) over the bins both have, for two products on different
    grids over ONE domain: equal domains give equal bin widths, so the bin edges coincide; anything else raises"""
    dom = lambda s: (Fraction(s.shape[0]) * Fraction(s.dy), Fraction(s.shape[1]) * Fraction(s.dx))
    (ph, qh), (pl, ql) = dom(spec_hi), dom(spec_lo)
    close = lambda u, v: abs(u - v) <= Fraction(1, 2 ** 40) * max(u, v)
    if not (close(ph, pl) and close(qh, ql)):
        raise L.GandanetError(f"spectral_ratio: the domains differ ({float(ph)} x {float(qh)} vs {float(pl)} x {float(ql)})")
    n = min(spec_hi.k.size, spec_lo.k.size)
    with np.errstate(divide="ignore", invalid="ignore"):
        return spec_lo.k[:n].copy(), spec_hi.mean()[:n] / spec_lo.mean()[:n]


def effective_resolution(curve, k, threshold: float = 0.5, sustain: int = 2) -> float:
    """the wavelength at which ``curve`` (a spectral ratio or a coherence over the bin centres ``k``) first falls below
    ``threshold`` and stays below for ``sustain`` bins (or to the end), linearly interpolated in log k; NaN when it never
    does or starts below"""
    c, k = np.asarray(curve, dtype=np.float64), np.asarray(k, dtype=np.float64)
    below = ~(c >= threshold)
    for i in range(1, c.size):
        if below[i] and not below[i - 1] and below[i:i + sustain].all() and np.isfinite(c[i]):
            f = (c[i - 1] - threshold) / (c[i - 1] - c[i])
            return float(1.0 / math.exp(math.log(k[i - 1]) + f * (math.log(k[i]) - math.log(k[i - 1]))))
    return float("nan")
