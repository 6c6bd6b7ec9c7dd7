"""Is the ensemble's spread the right size?  Verification of the members against the truth, kept on the device.

``evaluate_ensemble`` reduces the member axis to a mean and a std map, as ``compute_uncertainty`` of deep_ensemble.ipynb
does.  What tells whether that std means anything are the standard ensemble scores: the continuous ranked probability
score (CRPS), the rank (Talagrand) histogram, the spread against the error of the ensemble mean and the coverage of the
+-k sigma intervals.  ``gd_ens_verify`` (include/gandanet.h, "Ensemble verification") computes them from the slab of
members and the truth of the same batch as ONE record of ``L.ENSV_REC`` doubles plus optional per-pixel maps; the records
stay in a device tensor between batches, and ``compute`` copies them to the host once and adds them there.  Records carry
their counts, so a ragged last batch and uneven shards under data parallelism are exact.  There is no CPU path in this
module (``kern.ens_verify_host`` is the plain-C++ twin the tests compare against).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L
from . import kern as K
from . import parallel

__all__ = ["EnsembleVerification", "ensemble_scores"]


def _mask_u8(mask, device):
    from .evaluate import _mask_u8 as to_u8
    return to_u8(mask, device)


def _scale(scale) -> float:
    scale = float(scale)
    if not (scale > 0.0 and scale < float("inf")):
        raise L.GandanetError(f"ensemble verification: scale must be finite and > 0, got {scale!r}")
    return scale


class EnsembleVerification:
    """Streaming CRPS / rank histogram / spread-skill / coverage of all (members, truth) batches seen.

    ``update(slab, truth)`` enqueues one ``gd_ens_verify`` into the next row of a (K, L.ENSV_REC) fp64 device tensor and
    never waits for the device; ``compute`` makes the one device -> host copy.  ``slab`` is (M, ...) with every member
    dense and the members a constant stride apart (the slab of ``evaluate_ensemble`` with unused rows behind each member is
    fine), ``truth`` is (...).  ``mask`` (one entry per pixel of a plane, nonzero = valid), ``scale`` (the factor ``a`` of
    the scaler's inverse v * a + b; b cancels in every difference) and ``fair`` (the unbiased CRPS, M >= 2) apply to every
    update."""

    def __init__(self, device, M: int, mask=None, scale: float = 1.0, fair: bool = False, capacity: int = 16) -> None:
        self.device = torch.device(device)
        self.M = int(M)
        if not (1 <= self.M <= L.ENSV_MAX_M):
            raise L.GandanetError(f"EnsembleVerification: an ensemble of {M} members (1..{L.ENSV_MAX_M})")
        self.fair = bool(fair)
        if self.fair and self.M < 2:
            raise L.GandanetError("EnsembleVerification: the fair CRPS needs M >= 2")
        self.scale = _scale(scale)
        self.mask = _mask_u8(mask, self.device)
        self._recs = torch.zeros((max(1, int(capacity)), L.ENSV_REC), dtype=torch.float64, device=self.device)
        self._k = 0

    def __len__(self) -> int:
        return self._k

    def _next_row(self) -> torch.Tensor:
        if self._k == self._recs.shape[0]:                 # grow by doubling: a device-side copy, no sync
            grown = torch.zeros((2 * self._k, L.ENSV_REC), dtype=torch.float64, device=self.device)
            grown[:self._k].copy_(self._recs)
            self._recs = grown
        self._k += 1
        return self._recs[self._k - 1]

    def update(self, slab: torch.Tensor, truth: torch.Tensor, crps_map: Optional[torch.Tensor] = None,
               err_map: Optional[torch.Tensor] = None, spread_map: Optional[torch.Tensor] = None,
               rank_map: Optional[torch.Tensor] = None) -> None:
        slab, truth = slab.detach(), truth.detach()
        if slab.shape[0] != self.M:
            raise L.GandanetError(f"EnsembleVerification: {slab.shape[0]} members, built for {self.M}")
        row = self._next_row()
        try:
            K.ens_verify(slab, truth if truth.is_contiguous() else truth.contiguous(), row, self.mask, self.scale, self.fair,
                         crps_map, err_map, spread_map, rank_map)
        except Exception:
            self._k -= 1
            raise

    def add_records(self, records) -> None:
        """append ready-made records (k, L.ENSV_REC), e.g. read back from another pass"""
        recs = torch.as_tensor(np.asarray(records, dtype=np.float64).reshape(-1, L.ENSV_REC))
        for r in recs:
            self._next_row().copy_(r)

    def records(self) -> torch.Tensor:
        """the (k, L.ENSV_REC) records so far, on the device"""
        return self._recs[:self._k]

    def compute(self, pad_to: Optional[int] = None) -> Dict[str, object]:
        """add everything seen, on every rank of a data-parallel world: the ranks' records are all-gathered (zero rows are
        neutral) and added rank-major, so every rank returns the same floats.  ``pad_to`` as in
        ``RegressionMetrics.compute``: a row count common to all ranks and >= every rank's own; without it the ranks first
        agree on the largest count with an ``all_reduce`` read on the host."""
        recs = self.records()
        if parallel.is_distributed():
            if pad_to is None:
                kmax = torch.tensor([self._k], dtype=torch.int64, device=self.device)
                dist.all_reduce(kmax, op=dist.ReduceOp.MAX)
                pad_to = int(kmax.item())
            if pad_to < self._k:
                raise ValueError(f"pad_to={pad_to} is smaller than this rank's {self._k} records")
            mine = torch.zeros((max(1, pad_to), L.ENSV_REC), dtype=torch.float64, device=self.device)
            mine[:self._k].copy_(recs)
            gathered = [torch.zeros_like(mine) for _ in range(parallel.world_size())]
            dist.all_gather(gathered, mine)
            recs = torch.cat(gathered, 0)
        return K.ens_verify_merge_host(recs.cpu().numpy(), self.M)[1]


def ensemble_scores(members: torch.Tensor, truth: torch.Tensor, mask=None, scale: float = 1.0, fair: bool = False,
                    maps: bool = False):
    """the verification metrics of ``members`` (M, ...) against ``truth`` (...) in one call: the dict of
    ``kern.ens_verify_merge_host``; with ``maps`` also a dict of the per-element maps ``crps``, ``err`` (the error of the
    ensemble mean), ``spread`` (input dtype, NaN where invalid) and ``rank`` (uint8, 255 where invalid), shaped like
    ``truth``.  One device -> host copy of the record."""
    ev = EnsembleVerification(members.device, members.shape[0], mask=mask, scale=scale, fair=fair, capacity=1)
    out = None
    if maps:
        out = {k: torch.empty(truth.shape, device=members.device, dtype=members.dtype) for k in ("crps", "err", "spread")}
        out["rank"] = torch.empty(truth.shape, device=members.device, dtype=torch.uint8)
        ev.update(members, truth, out["crps"], out["err"], out["spread"], out["rank"])
    else:
        ev.update(members, truth)
    met = ev.compute()
    return (met, out) if maps else met
