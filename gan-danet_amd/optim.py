"""AdamW on a HIP kernel, as a torch.optim.Optimizer so the reference's
``CosineAnnealingWarmRestarts`` schedulers drive it unchanged (GAN_DANet_train.ipynb:L182-187)."""
from __future__ import annotations

import math
from typing import Callable, Iterable, Optional

import torch
import torch.distributed as dist

from . import _lib as L
from . import kern as K


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics (decoupled weight decay, bias correction, eps outside the sqrt-bias term).
    ``grad_scale`` multiplies every gradient as it is read (1/world_size after a summing all-reduce).

    ``sharded``: ``parallel.ShardedParam`` objects for parameters whose update is split over the ranks: this rank
    holds optimiser state for its slice only, updates that slice from its slice of the summed gradient
    (``ShardedParam.wait_grad``) and starts the all-gather of the updated weight.  ``state_dict`` /
    ``load_state_dict`` exchange FULL state tensors (collective: call them on every rank), so checkpoints do not
    depend on the world size.
    ``update_fn``: the element-wise update kernel (default: the HIP ``gd_adamw``; the CPU tests of the sharding logic
    pass the oracle's).

    The GUARDED step: any of ``max_grad_norm`` (clip the global gradient norm, ``torch.nn.utils.clip_grad_norm_``'s
    formula), ``skip_nonfinite`` (a step whose gradient norm is inf or NaN changes nothing and does not advance Adam's
    time) and ``ema_decay`` (keep ``ema = d * ema + (1 - d) * p`` of every parameter, written by the update kernel itself)
    turns ``step()`` into: one norm over all gradients that exist (``gd_grad_sqnorm``, through ``grad_scale``: the norm
    of the AVERAGED gradient under data parallelism) -> ``gd_guard_finalize`` -> ``gd_adamw_guarded`` per tensor.  The
    decision lives in one 6-double record in device memory; ``grad_norm`` and ``skipped_steps`` are views into it, and
    reading them is the caller's sync.  With none of the three set, ``step()`` is the unguarded loop, unchanged.
    Sharded parameters: the shards' partial sum of squares is all-reduced (ONE double), the unsharded gradients -- the
    same on every rank after their all-reduce -- are added to it locally, so every rank holds the same record bit for bit.
    ``norm_fn(grads, rec, grad_scale, accumulate)``: the counterpart of ``update_fn`` for the norm (default: the HIP
    ``gd_grad_sqnorm``).  With it the record may live on the host and is finalised there: the seam the CPU tests of the
    distributed logic use.  In guarded mode ``update_fn`` has ``kern.adamw_guarded``'s signature."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale: float = 1.0,
                 sharded: Iterable = (), update_fn: Optional[Callable] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, ema_decay: Optional[float] = None, norm_fn: Optional[Callable] = None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.grad_scale = grad_scale
        self.sharded = {id(sp.p): sp for sp in sharded}
        self.guarded = max_grad_norm is not None or bool(skip_nonfinite) or ema_decay is not None
        if ema_decay is not None and not 0.0 <= ema_decay <= 1.0:
            raise ValueError(f"ema_decay {ema_decay} outside [0, 1]")
        self.max_grad_norm, self.skip_nonfinite, self.ema_decay = max_grad_norm, bool(skip_nonfinite), ema_decay
        self.norm_fn = norm_fn
        self.update_fn = update_fn or (K.adamw_guarded if self.guarded else K.adamw)
        self._rec: Optional[torch.Tensor] = None

    # ---- the guard record and what hangs off it ----
    def _record(self) -> torch.Tensor:
        if not self.guarded:
            raise RuntimeError("AdamW: no guard option is set (max_grad_norm / skip_nonfinite / ema_decay)")
        if self._rec is None:
            dev = self.param_groups[0]["params"][0].device
            self._rec = torch.zeros(L.GUARD_RECORD, device=dev, dtype=torch.float64)
        return self._rec

    @property
    def grad_norm(self) -> torch.Tensor:
        """norm of the last step's (scaled, unclipped) gradient: a 0-dim device view into the record"""
        return self._record()[L.GUARD_NORM]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """how many steps were skipped as non-finite so far: a 0-dim device view into the record"""
        return self._record()[L.GUARD_SKIPPED]

    def _target(self, p):
        sp = self.sharded.get(id(p))
        return sp, (p.data if sp is None else sp.param_shard())

    def _init_state(self, st: dict, target: torch.Tensor) -> None:
        if "exp_avg" not in st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(target, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(target, memory_format=torch.contiguous_format)
        if self.ema_decay is not None and "ema" not in st:      # also after a checkpoint written without shadows
            st["ema"] = target.detach().clone(memory_format=torch.contiguous_format)

    @torch.no_grad()
    def ema_params(self):
        """the averaged weights, one tensor per parameter in parameter order (this rank's slice for a sharded
        parameter); before the first step they equal the weights"""
        if self.ema_decay is None:
            raise RuntimeError("AdamW.ema_params: built without ema_decay")
        out = []
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state[p]
                self._init_state(st, self._target(p)[1])
                out.append(st["ema"])
        return out

    def _finalize_host(self, rec: torch.Tensor) -> None:
        """gd_guard_finalize's arithmetic on a record that ``norm_fn`` filled (host syncs: the CPU tests' seam only)"""
        norm = math.sqrt(rec[L.GUARD_SQNORM].item()) if rec[L.GUARD_SQNORM].item() >= 0 else float("nan")
        ok = math.isfinite(norm) if self.skip_nonfinite else True
        mx = self.max_grad_norm
        coef = min(1.0, mx / (norm + 1e-6)) if (mx is not None and mx > 0 and not math.isnan(norm)) else 1.0
        rec[L.GUARD_NORM], rec[L.GUARD_COEF], rec[L.GUARD_OK] = norm, coef, float(ok)
        rec[L.GUARD_APPLIED if ok else L.GUARD_SKIPPED] += 1.0

    def _step_guarded(self) -> None:
        rec = self._record()
        work = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                sp, target = self._target(p)
                g = sp.wait_grad() if sp is not None else (p.grad if p.grad.is_contiguous() else p.grad.contiguous())
                work.append((group, p, sp, g, target))
        plain = [w[3] for w in work if w[2] is None]
        shards = [w[3] for w in work if w[2] is not None]
        norm = self.norm_fn or K.grad_sqnorm
        if self.sharded:
            # collective whether or not this step has shard gradients: the shards' sum over the ranks first, then the
            # unsharded gradients (identical on every rank) on top of it -- the same two terms in the same order everywhere
            if shards:
                norm(shards, rec, self.grad_scale, False)
            else:
                rec[:1].zero_()
            dist.all_reduce(rec[:1], op=dist.ReduceOp.SUM, group=next(iter(self.sharded.values())).group)
            if plain:
                norm(plain, rec, self.grad_scale, True)
        elif plain:
            norm(plain, rec, self.grad_scale, False)
        else:
            return
        if self.norm_fn is None:
            K.guard_finalize(rec, self.max_grad_norm, self.skip_nonfinite)
        else:
            self._finalize_host(rec)
        for group, p, sp, g, target in work:
            st = self.state[p]
            self._init_state(st, target)
            b1, b2 = group["betas"]
            self.update_fn(target, g, st["exp_avg"], st["exp_avg_sq"], rec, group["lr"], b1, b2, group["eps"],
                           group["weight_decay"], self.grad_scale, st.get("ema"),
                           0.0 if self.ema_decay is None else self.ema_decay)
            if sp is not None:
                sp.launch_all_gather()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.guarded:
            self._step_guarded()
            return loss
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                sp = self.sharded.get(id(p))
                st = self.state[p]
                if sp is not None:
                    g, target = sp.wait_grad(), sp.param_shard()
                else:
                    g, target = (p.grad if p.grad.is_contiguous() else p.grad.contiguous()), p.data
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(target, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(target, memory_format=torch.contiguous_format)
                st["step"] += 1
                self.update_fn(target, g, st["exp_avg"], st["exp_avg_sq"], st["step"], group["lr"], b1, b2, group["eps"],
                               group["weight_decay"], self.grad_scale)
                if sp is not None:
                    sp.launch_all_gather()
        return loss

    # ---- checkpoints hold full tensors whatever the sharding ----
    _SLICED = ("exp_avg", "exp_avg_sq", "ema")

    def state_dict(self):
        rec = None
        if self.guarded:
            # the host learns the step count here, once: every parameter's `step` is the applied count, so the file
            # loads into the unguarded optimiser (and the other way round)
            rec = self._record().tolist()
            for st in self.state.values():
                if st:
                    st["step"] = int(rec[L.GUARD_APPLIED])
        saved = {}
        for p, st in self.state.items():
            sp = self.sharded.get(id(p))
            if sp is not None and st:
                saved[p] = {k: st[k] for k in self._SLICED if k in st}
                for k, t in saved[p].items():
                    st[k] = sp.gather_state(t)
        try:
            sd = super().state_dict()
            if saved:
                # the packed per-parameter dicts ARE self.state's dicts: copy them before the slices go back in
                sd["state"] = {k: dict(v) for k, v in sd["state"].items()}
        finally:
            for p, old in saved.items():
                self.state[p].update(old)
        if rec is not None:
            sd["skipped_steps"] = int(rec[L.GUARD_SKIPPED])
            sd["guard_record"] = [float(x) for x in rec]
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            sp = self.sharded.get(id(p))
            if sp is not None and st:
                for k in self._SLICED:
                    if k in st and st[k].numel() == p.numel():
                        st[k] = sp.slice_state(st[k])
        if self.guarded:
            vals = list(state_dict.get("guard_record", [0.0] * L.GUARD_RECORD))
            vals[L.GUARD_APPLIED] = float(max((int(st["step"]) for st in self.state.values() if st and "step" in st), default=0))
            vals[L.GUARD_SKIPPED] = float(state_dict.get("skipped_steps", 0))
            self._record().copy_(torch.tensor(vals, dtype=torch.float64))
            if self.ema_decay is None:
                for st in self.state.values():
                    st.pop("ema", None)
