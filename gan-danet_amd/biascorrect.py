"""The skill maps say how far the downscaled field is from GRACE; this module acts on that distance.  Quantile-mapping bias
correction per pixel and calendar month, on the device:

* ``series_quantiles``: ``np.nanquantile(x, q, axis=0)`` of every pixel series, per calendar slot, bit for bit;
* ``QuantileMap.fit``: the quantile nodes of a model cube and of an observation cube on one grid (for a finer product:
  ``QuantileMap.fit(coarsen(product, (5, 5)), grace)``);
* ``QuantileMap.apply``: empirical quantile mapping (``"eqm"``: ``np.interp(x, model_q, obs_q)`` with the end node's
  correction carried outward, Boe et al. 2007, or clipped) and additive quantile delta mapping (``"qdm"``, Cannon et al.
  2015: the sample is ranked in its own distribution and only the quantile-dependent offset is added, so trends survive)
  of a cube on the table grid or on an f times finer one.

The kernels are ``csrc/quantmap.hip`` over ``csrc/quantmap_core.h`` (``include/gandanet.h``, "Bias correction"): fp32 or fp64
CUDA tensors, time along axis 0 (T <= 2048), all arithmetic fp64 and unfused, nothing transcendental, no atomics: the same
bits on every run, as the plain C++ twins (``kern.qm_*_host``) and as numpy.  Samples are ordered with -0.0 below +0.0
(numpy leaves the order of the two zeros to its partition).  There is no CPU path in this module.  torch allocates and views.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import kern as K
from .drought import _calendar
from .timeseries import _cube, _series_mask

Tensor = torch.Tensor
L = K.L

KINDS = tuple(L.QM_KINDS)
EXTRAPOLATE = tuple(L.QM_EXTRAPOLATE)


def _int(v, name: str, fn: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise L.GandanetError(f"{fn}: {name} must be an integer, got {v!r}")
    return int(v)


def series_quantiles(x: Tensor, q, period: int = 1, phase: int = 0, baseline: Optional[Tuple[int, int]] = None,
                     mask: Optional[Tensor] = None, _route: str = "auto") -> Tuple[Tensor, Tensor]:
    """``(quantiles (Q, period, ...) fp64, n (period, ...) int32)`` of every series ``x[:, ...]``: ``quantiles[j, s, pix]``
    is ``np.nanquantile(sample, q[j])`` (``method="linear"``) over the baseline steps t with (t + ``phase``) mod ``period``
    == s at that pixel, bit for bit; ``n`` is the size of that sample.  ``q``: up to 256 probabilities in [0, 1], on the
    host.  ``baseline`` = (b0, b1), a half-open step range (default: the whole record).  An empty sample and a pixel that
    ``mask`` (bool or uint8, the shape of one time step, nonzero = use the pixel) leaves out give NaN and n = 0."""
    x = _cube(x, "series_quantiles")
    qa = K.qm_probs(q, "series_quantiles")
    t_len, tail = x.shape[0], tuple(x.shape[1:])
    period, phase, b0, b1 = _calendar("series_quantiles", t_len, period, phase, baseline)
    quant, n = K.qm_quantiles(x.reshape(t_len, -1), qa, period, phase, b0, b1, _series_mask(mask, tail, x.device), _route=_route)
    return quant.reshape((qa.size, period) + tail), n.reshape((period,) + tail)


class QuantileMap:
    """The quantile nodes of a model cube and an observation cube per calendar slot and pixel of the table grid:
    ``model_q`` and ``obs_q`` (period, Q, H, W) fp64 at the probabilities ``p`` = j / (Q - 1); ``n`` (period, H, W) int32,
    the sample sizes (``pairwise``), or ``n_model`` and ``n_obs``; slot of step t = (t + ``phase``) mod ``period``.  A slot
    with fewer than ``min_samples`` samples has NaN tables, and everything mapped through them is NaN."""

    def __init__(self, model_q: Tensor, obs_q: Tensor, n_model: Tensor, n_obs: Tensor, period: int, phase: int, pairwise: bool,
                 min_samples: int, baseline: Tuple[int, int]):
        self.model_q, self.obs_q, self.n_model, self.n_obs = model_q, obs_q, n_model, n_obs
        self.period, self.phase, self.pairwise, self.min_samples = int(period), int(phase), bool(pairwise), int(min_samples)
        self.baseline = (int(baseline[0]), int(baseline[1]))

    @property
    def n(self) -> Tensor:
        if not self.pairwise:
            raise AttributeError("n: a map fitted with pairwise=False holds n_model and n_obs")
        return self.n_model

    @property
    def n_quantiles(self) -> int:
        return int(self.model_q.shape[1])

    @property
    def p(self) -> np.ndarray:
        return K.qm_nodes(self.n_quantiles)

    @classmethod
    def fit(cls, model: Tensor, obs: Tensor, n_quantiles: int = 51, period: int = 12, phase: int = 0,
            baseline: Optional[Tuple[int, int]] = None, mask: Optional[Tensor] = None, pairwise: bool = True,
            min_samples: int = 2) -> "QuantileMap":
        """the map from ``model`` to ``obs``, two (T, H, W) cubes of one dtype on one grid.  ``pairwise`` lets a step count
        for a pixel only where neither cube is NaN; without it each cube drops its own NaNs."""
        model, obs = _cube(model, "QuantileMap.fit"), _cube(obs, "QuantileMap.fit")
        if model.dim() != 3 or model.shape != obs.shape or model.dtype != obs.dtype:
            raise L.GandanetError(f"QuantileMap.fit: model and obs are (T, H, W) cubes of one shape and dtype, got {tuple(model.shape)} "
                                  f"{model.dtype} and {tuple(obs.shape)} {obs.dtype}")
        p = K.qm_nodes(n_quantiles)
        min_samples = _int(min_samples, "min_samples", "QuantileMap.fit")
        if min_samples < 1:
            raise L.GandanetError(f"QuantileMap.fit: min_samples >= 1, got {min_samples}")
        t_len, tail = model.shape[0], tuple(model.shape[1:])
        period, phase, b0, b1 = _calendar("QuantileMap.fit", t_len, period, phase, baseline)
        m = _series_mask(mask, tail, model.device)
        pd = torch.from_numpy(p).to(model.device)
        x, y = model.reshape(t_len, -1), obs.reshape(t_len, -1)
        args = dict(period=period, phase=phase, b0=b0, b1=b1, mask=m, min_samples=min_samples, layout=L.QM_LAYOUT_SQM)
        mq, nm = K.qm_quantiles(x, pd, x2=y if pairwise else None, **args)
        oq, no = K.qm_quantiles(y, pd, x2=x if pairwise else None, **args)
        shape = (period, p.size) + tail
        return cls(mq.reshape(shape), oq.reshape(shape), nm.reshape((period,) + tail), no.reshape((period,) + tail), period, phase, pairwise,
                   min_samples, (b0, b1))

    def apply(self, x: Tensor, kind: str = "eqm", extrapolate: str = "constant", t0: int = 0, out: Optional[Tensor] = None) -> Tensor:
        """``x`` (T', f H, f W), 1 <= f <= 16 read off the shapes, corrected; the shape and dtype of ``x``.  Pixel (h, w) uses
        the tables of (h // f, w // f), step t the slot (``t0`` + t + phase) mod period.

        ``"eqm"``: ``np.interp(x, model_q, obs_q)`` inside the model's range; outside, ``"constant"`` adds the end node's
        correction ``obs_q[e] - model_q[e]`` to x and ``"clip"`` returns ``obs_q[e]``.
        ``"qdm"``: with ``own_q`` the node table of ``x`` itself (per slot and pixel of its own grid) and
        tau = ``np.interp(x, own_q, p)``: x + (``np.interp(tau, p, obs_q)`` - ``np.interp(tau, p, model_q)``).
        A NaN x and NaN tables give NaN."""
        x = _cube(x, "QuantileMap.apply")
        if kind not in KINDS:
            raise L.GandanetError(f"QuantileMap.apply: kind is one of {KINDS}, got {kind!r}")
        if extrapolate not in EXTRAPOLATE:
            raise L.GandanetError(f"QuantileMap.apply: extrapolate is one of {EXTRAPOLATE}, got {extrapolate!r}")
        t0 = _int(t0, "t0", "QuantileMap.apply")
        if x.dim() != 3:
            raise L.GandanetError(f"QuantileMap.apply: expected a (T, f H, f W) cube, got {tuple(x.shape)}")
        if x.device != self.model_q.device:
            raise L.GandanetError(f"QuantileMap.apply: the cube is on {x.device}, the tables on {self.model_q.device}")
        phase = (t0 + self.phase) % self.period
        own = pd = None
        if kind == "qdm":
            t_len = x.shape[0]
            if t_len > L.QM_MAX_T:
                raise L.GandanetError(f"QuantileMap.apply: 'qdm' ranks x in its own record, T <= {L.QM_MAX_T}, got T = {t_len}")
            K._qm_factor(x.shape, self.model_q.shape[2], self.model_q.shape[3], "QuantileMap.apply")
            pd = torch.from_numpy(self.p).to(x.device)
            own, _ = K.qm_quantiles(x.reshape(t_len, -1), pd, self.period, phase, 0, t_len, layout=L.QM_LAYOUT_SQM)
            own = own.reshape((self.period, self.n_quantiles) + tuple(x.shape[1:]))
        return K.qm_apply(x, self.model_q, self.obs_q, kind, extrapolate, phase, own, pd, out)

    def state_dict(self) -> Dict[str, Tensor]:
        """plain tensors (the scalars as 0-d int64 tensors on the host), to be stored with a checkpoint"""
        sd = {"model_q": self.model_q, "obs_q": self.obs_q, "n_model": self.n_model, "n_obs": self.n_obs}
        for k in ("period", "phase", "pairwise", "min_samples"):
            sd[k] = torch.tensor(int(getattr(self, k)), dtype=torch.int64)
        sd["baseline"] = torch.tensor(self.baseline, dtype=torch.int64)
        return sd

    @classmethod
    def load_state_dict(cls, sd: Dict[str, Tensor], device=None) -> "QuantileMap":
        """the map of a ``state_dict()``; the tables go to ``device`` (default: where they are, which must be a GPU)"""
        keys = ("model_q", "obs_q", "n_model", "n_obs", "period", "phase", "pairwise", "min_samples", "baseline")
        missing = [k for k in keys if k not in sd]
        if missing:
            raise L.GandanetError(f"QuantileMap.load_state_dict: missing {missing}")
        mq, oq, nm, no = (sd[k] if device is None else sd[k].to(device) for k in keys[:4])
        if not mq.is_cuda:
            raise L.GandanetError("QuantileMap.load_state_dict: the tables belong on a GPU (there is no CPU path); pass device=")
        mq, oq = mq.to(torch.float64).contiguous(), oq.to(torch.float64).contiguous()
        period, Q, H, W = K._qm_tables(mq, oq, "QuantileMap.load_state_dict", True)
        for t in (nm, no):
            if tuple(t.shape) != (period, H, W):
                raise L.GandanetError(f"QuantileMap.load_state_dict: the counts are {(period, H, W)}, got {tuple(t.shape)}")
        phase = int(sd["phase"])
        if not 0 <= phase < period or int(sd["period"]) != period:
            raise L.GandanetError(f"QuantileMap.load_state_dict: period {int(sd['period'])} and phase {phase} do not fit tables of {period} slots")
        return cls(mq, oq, nm.to(torch.int32).contiguous(), no.to(torch.int32).contiguous(), period, phase, bool(int(sd["pairwise"])),
                   int(sd["min_samples"]), tuple(int(v) for v in sd["baseline"]))
