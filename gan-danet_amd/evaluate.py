"""What the reference does right after ``train()``, kept on the device.

``ModelTrainer.evaluate`` (GAN_DANet_train.ipynb c0 "def evaluate"; deep_ensemble.ipynb:L249-293) concatenates every
prediction and target on the host -- 4 MiB per sample and tensor at 1024 x 1024 -- and hands them to sklearn.  Here each
batch is reduced where it was produced to one RECORD of 8 doubles (include/gandanet.h, "evaluation": n, the two means, the
co-moments, sum |p - t|, sum (p - t)^2), the records stay in a device tensor between batches, and ``compute`` copies them to
the host once and merges them there.  Records carry their counts, so a ragged last batch and uneven shards under data
parallelism are exact.

``EnsembleTrainer.compute_uncertainty`` (deep_ensemble.ipynb:L438-476) becomes ``evaluate_ensemble``: the members'
predictions of a batch sit in one slab, the member axis is reduced by ``gd_ensemble_stats`` and the masked spatial means by
``gd_masked_plane_mean``.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from . import kern as K
from . import parallel
from .verification import EnsembleVerification

METRIC_KEYS = ("n", "mse", "mae", "r2", "cc")


def _mask_u8(mask, device) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
    # "cuda" means the current device: compare resolved indices, or a ready mask on cuda:0 would be converted again
    index = lambda d: d.index if d.index is not None or d.type != "cuda" else torch.cuda.current_device()
    here = m.device.type == device.type and index(m.device) == index(device)
    return m if m.dtype == torch.uint8 and here and m.is_contiguous() else \
        (m != 0).to(torch.uint8).contiguous().to(device)


class RegressionMetrics:
    """Streaming ``mean_squared_error`` / ``mean_absolute_error`` / ``r2_score`` / ``np.corrcoef`` of all pairs seen.

    ``update`` enqueues one ``gd_eval_stats`` into the next row of a (K, 8) fp64 device tensor and never waits for the
    device; ``compute`` makes the one device -> host copy.  ``mask`` (one entry per pixel of a plane, nonzero = valid) and
    ``affine`` = (a, b) (both inputs read as v * a + b: the scaler's inverse) apply to every update."""

    def __init__(self, device, affine=None, mask=None, capacity: int = 16) -> None:
        self.device = torch.device(device)
        self.affine = None if affine is None else (float(affine[0]), float(affine[1]))
        self.mask = _mask_u8(mask, self.device)
        self._recs = torch.zeros((max(1, int(capacity)), 8), dtype=torch.float64, device=self.device)
        self._k = 0

    def __len__(self) -> int:
        return self._k

    def _next_row(self) -> torch.Tensor:
        if self._k == self._recs.shape[0]:                 # grow by doubling: a device-side copy, no sync
            grown = torch.zeros((2 * self._k, 8), dtype=torch.float64, device=self.device)
            grown[:self._k].copy_(self._recs)
            self._recs = grown
        self._k += 1
        return self._recs[self._k - 1]

    def update(self, pred: torch.Tensor, truth: torch.Tensor) -> None:
        pred, truth = pred.detach(), truth.detach()
        row = self._next_row()
        try:
            K.eval_stats(pred if pred.is_contiguous() else pred.contiguous(),
                         truth if truth.is_contiguous() else truth.contiguous(), row, self.mask, self.affine)
        except Exception:
            self._k -= 1
            raise

    def add_records(self, records) -> None:
        """append ready-made records (k, 8), e.g. read back from another pass"""
        recs = torch.as_tensor(np.asarray(records, dtype=np.float64).reshape(-1, 8))
        for r in recs:
            self._next_row().copy_(r)

    def records(self) -> torch.Tensor:
        """the (k, 8) records so far, on the device"""
        return self._recs[:self._k]

    def compute(self, pad_to: Optional[int] = None) -> Dict[str, float]:
        """merge everything seen, on every rank of a data-parallel world: the ranks' records are all-gathered (zero rows
        are neutral) and merged rank-major, so every rank returns the same floats.  ``pad_to``: a row count known to be
        common to all ranks and >= every rank's own (``evaluate`` derives it from the shard plan).  Without it the ranks
        first agree on the largest count with an ``all_reduce`` whose result is read on the host: under data parallelism
        that is a second host sync before the copy of the records; a single process never pays it."""
        recs = self.records()
        if parallel.is_distributed():
            if pad_to is None:
                kmax = torch.tensor([self._k], dtype=torch.int64, device=self.device)
                dist.all_reduce(kmax, op=dist.ReduceOp.MAX)
                pad_to = int(kmax.item())
            if pad_to < self._k:
                raise ValueError(f"pad_to={pad_to} is smaller than this rank's {self._k} records")
            mine = torch.zeros((max(1, pad_to), 8), dtype=torch.float64, device=self.device)
            mine[:self._k].copy_(recs)
            gathered = [torch.zeros_like(mine) for _ in range(parallel.world_size())]
            dist.all_gather(gathered, mine)
            recs = torch.cat(gathered, 0)
        return K.eval_merge_host(recs.cpu().numpy())[1]


@contextlib.contextmanager
def _eval_mode(modules: Sequence[Optional[nn.Module]]):
    """``.eval()`` on the way in; every sub-module's own train / eval flag back on the way out, also on error"""
    saved = [(m, m.training) for top in modules if top is not None for m in top.modules()]
    try:
        for top in modules:
            if top is not None:
                top.eval()
        yield
    finally:
        for m, flag in saved:
            m.training = flag


def _batch(dataset, lo: int, hi: int):
    """samples [lo, hi) as stored.  Evaluation never augments: a dataset built with ``augment=True`` would draw new
    flips, turns and noise on every ``get``, and the metrics would differ from run to run"""
    return dataset.lr_grace_05[lo:hi], dataset.lr_grace_025[lo:hi], dataset.hr_aux[lo:hi]


def _forward(model: nn.Module, gate: Optional[nn.Module], batch) -> torch.Tensor:
    lr_grace_05, _, hr_aux = batch
    x = K.combine_inputs(lr_grace_05, hr_aux, 0.5, 0.25)          # the preamble of GanTrainer.step_from_batch
    return model(x if gate is None else gate(x))


def _share(n: int, batch_size: int, rank: Optional[int], world: Optional[int]):
    """this rank's contiguous share of n samples cut into batches, and the largest batch count of any rank"""
    world = parallel.world_size() if world is None else world
    rank = parallel.rank() if rank is None else rank
    if batch_size < 1 or world < 1 or not (0 <= rank < world):
        raise ValueError(f"batch_size {batch_size}, rank {rank} / world {world}")
    sl = parallel.shard_batch(n, world, rank)
    most = parallel.shard_batch(n, world, 0)                      # the remainder goes to the first ranks
    nb = lambda s: -(-(s.stop - s.start) // batch_size)
    return [(lo, min(sl.stop, lo + batch_size)) for lo in range(sl.start, sl.stop, batch_size)], nb(most)


def evaluate(model: nn.Module, dataset, batch_size: int, input_attention: Optional[nn.Module] = None,
             rank: Optional[int] = None, world: Optional[int] = None, return_preds: bool = False):
    """``ModelTrainer.evaluate`` over a ``DeviceTileDataset``: eval-mode forwards without a tape, every sample exactly once
    (the last batch may be ragged), metrics of ``hr`` against ``lr_grace_025`` as a dict of floats (``METRIC_KEYS``).
    Under data parallelism every rank evaluates a contiguous share of the samples (shares may differ by one sample;
    ``batch_size`` is per rank) and all ranks return the same dict.  ``return_preds``: also this rank's predictions.
    The samples are read as stored, whatever the dataset's ``augment`` flag; an empty dataset gives NaN metrics, n = 0."""
    plan, most = _share(len(dataset), batch_size, rank, world)
    metrics = RegressionMetrics(dataset.device, capacity=max(1, most))
    preds = []
    with _eval_mode([model, input_attention]), torch.no_grad():
        for lo, hi in plan:
            batch = _batch(dataset, lo, hi)
            hr = _forward(model, input_attention, batch)
            metrics.update(hr, batch[1])
            if return_preds:
                preds.append(hr)
    out = metrics.compute(pad_to=most)
    return (out, preds) if return_preds else out


def evaluate_ensemble(models: Iterable[nn.Module], dataset, batch_size: int, mask=None, affine=None,
                      input_attentions: Optional[Sequence[Optional[nn.Module]]] = None, verify: bool = False,
                      fair: bool = False) -> Dict[str, object]:
    """``EnsembleTrainer.compute_uncertainty`` (deep_ensemble.ipynb:L438-476) with the member axis on the device.

    ``mask`` (H, W): nonzero = valid (the notebook's ``tpbh != 0``).  Per batch the members' predictions are written into
    one (M, B, C, H, W) slab; ``gd_ensemble_stats`` gives the per-pixel mean / std maps, ``gd_masked_plane_mean`` the
    spatial means.  Returns ``mean_preds`` / ``std_preds`` (T, C) fp64 and ``r2`` as the notebook does, each member's own
    metrics (``members``; ``affine`` = the scaler's inverse, and the mask, apply to them), the maps ``mean_map`` /
    ``std_map`` (T, C, H, W) and the series ``preds_ts`` (M, T, C) / ``trues_ts`` (T, C).  Tensors stay on the device; one
    device -> host copy at the end.  Single process: members are not spread over ranks here.  The samples are read as
    stored, whatever the dataset's ``augment`` flag, so every member sees the same batch and runs repeat.

    ``verify``: the slab of every batch also goes through ``EnsembleVerification`` (verification.py) against the batch's
    truth, under ``mask`` and with ``affine[0]`` (> 0) as the scale; the result gains ``verification`` (CRPS, rank
    histogram, spread-skill and coverage: the dict of ``kern.ens_verify_merge_host``; ``fair`` = the unbiased CRPS) and the
    maps ``crps_map`` (fp32, NaN where invalid) and ``rank_map`` (uint8, 255 where invalid), both (T, C, H, W).  Without
    it the result is what it was."""
    models = list(models)
    M, T, dev = len(models), len(dataset), dataset.device
    if not (1 <= M <= 32):
        raise ValueError(f"an ensemble of {M} members (1..32)")
    if T == 0:
        raise ValueError("evaluate_ensemble: the dataset is empty")
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size}")
    gates = list(input_attentions) if input_attentions is not None else [None] * M
    if len(gates) != M:
        raise ValueError("one input gate (or None) per member")
    mask_u8 = _mask_u8(mask, dev)
    verif = crps_map = rank_map = None
    if verify:
        verif = EnsembleVerification(dev, M, mask=mask_u8, scale=1.0 if affine is None else affine[0], fair=fair,
                                     capacity=-(-T // batch_size))
    member_metrics = [RegressionMetrics(dev, affine=affine, mask=mask_u8) for _ in range(M)]
    slab = mean_map = std_map = preds_ts = trues_ts = None
    with _eval_mode(models + gates), torch.no_grad():
        for lo in range(0, T, batch_size):
            hi = min(T, lo + batch_size)
            batch = _batch(dataset, lo, hi)
            truth = batch[1]
            for m, (G, gate) in enumerate(zip(models, gates)):
                hr = _forward(G, gate, batch)
                if slab is None:
                    Cn, H, W = hr.shape[1:]
                    slab = torch.empty((M, min(batch_size, T), Cn, H, W), device=dev, dtype=torch.float32)
                    mean_map = torch.empty((T, Cn, H, W), device=dev, dtype=torch.float32)
                    std_map = torch.empty_like(mean_map)
                    preds_ts = torch.empty((M, T, Cn), device=dev, dtype=torch.float64)
                    trues_ts = torch.empty((T, Cn), device=dev, dtype=torch.float64)
                    if verify:
                        crps_map = torch.empty_like(mean_map)
                        rank_map = torch.empty((T, Cn, H, W), device=dev, dtype=torch.uint8)
                K.copy_slab(hr, slab[m, :hi - lo])
                member_metrics[m].update(slab[m, :hi - lo], truth)
                preds_ts[m, lo:hi].copy_(K.masked_plane_mean(slab[m, :hi - lo], mask_u8)[0])
            K.ensemble_stats(slab[:, :hi - lo], mean_map[lo:hi], std_map[lo:hi])
            if verify:
                verif.update(slab[:, :hi - lo], truth, crps_map=crps_map[lo:hi], rank_map=rank_map[lo:hi])
            trues_ts[lo:hi].copy_(K.masked_plane_mean(truth if truth.is_contiguous() else truth.contiguous(), mask_u8)[0])
        mean_preds, std_preds = K.ensemble_stats(preds_ts)
        final = torch.zeros(8, dtype=torch.float64, device=dev)
        K.eval_stats(mean_preds, trues_ts, final, skip_nan=True)      # valid_mask of L470-472
        counts = [len(mm) for mm in member_metrics]
        host = torch.cat([mm.records() for mm in member_metrics] + [final.view(1, 8)], 0).cpu().numpy()
    members, at = [], 0
    for k in counts:
        members.append(K.eval_merge_host(host[at:at + k])[1])
        at += k
    out = {"mean_preds": mean_preds, "std_preds": std_preds, "r2": K.eval_merge_host(host[at:])[1]["r2"],
           "members": members, "mean_map": mean_map, "std_map": std_map, "preds_ts": preds_ts, "trues_ts": trues_ts}
    if verify:
        out.update(verification=verif.compute(), crps_map=crps_map, rank_map=rank_map)
    return out
