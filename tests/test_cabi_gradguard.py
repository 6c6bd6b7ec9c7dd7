"""CPU: the guarded-step entry points of the C ABI (include/gandanet.h, "guarded step") are declared and bound, reject bad
arguments before any launch, and optim.AdamW's guarded step keeps two gloo ranks bit-identical through a clipped step, an
unclipped step and a step with a NaN in ONE rank's shard -- with numpy fp64 as the norm and the oracle's AdamW as the
update (the HIP kernels need a GPU; what is under test is the host-side partial-norm / all-reduce logic)."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gd_grad_sqnorm", "gd_grad_sqnorm_ws_bytes", "gd_guard_finalize", "gd_adamw_guarded")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_gradguard_symbols_are_declared_and_bound():
    L, lib = _lib()
    src = open(os.path.join(ROOT, "include", "gandanet.h")).read()
    assert "guarded step" in src.lower()
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name)
    from gan_danet_amd import kern as K
    for name in ("grad_sqnorm", "guard_finalize", "adamw_guarded"):
        assert callable(getattr(K, name))


def test_gradguard_argument_errors_before_any_launch():
    """null record, null table, null table entry, n = 0, empty list, workspace one byte short, null p / g / m / v / record:
    negative code + gd_last_error, no GPU needed (the pointers are never dereferenced: validation comes first)"""
    L, lib = _lib()
    p = 0x1000                      # a non-null, 16-byte aligned address that is never touched

    def bad(rc, word):
        assert rc < 0, rc
        assert word in L.last_error(), L.last_error()

    assert lib.gd_grad_sqnorm_ws_bytes(0) == 0 and lib.gd_grad_sqnorm_ws_bytes(-3) == 0
    assert lib.gd_grad_sqnorm_ws_bytes(5) == 40

    def table(ptrs, ns):
        return (L.c_fp * len(ptrs))(*ptrs), (C.c_long * len(ns))(*ns)

    ns3 = [10, L.GUARD_CHUNK * 2 + 1, 7]                       # 1 + 3 + 1 chunks
    ws = int(lib.gd_grad_sqnorm_ws_bytes(5))
    ptrs, ns = table([p, p, p], ns3)
    bad(lib.gd_grad_sqnorm(ptrs, ns, 3, 1.0, 0, None, p, ws, None), "null")
    bad(lib.gd_grad_sqnorm(ptrs, ns, 3, 1.0, 0, p, None, ws, None), "null")
    bad(lib.gd_grad_sqnorm(None, ns, 3, 1.0, 0, p, p, ws, None), "null")
    bad(lib.gd_grad_sqnorm(ptrs, None, 3, 1.0, 0, p, p, ws, None), "null")
    bad(lib.gd_grad_sqnorm(ptrs, ns, 0, 1.0, 0, p, p, ws, None), "n <= 0")
    bad(lib.gd_grad_sqnorm(ptrs, ns, 3, 1.0, 0, p, p, ws - 1, None), "workspace")
    bad(lib.gd_grad_sqnorm(ptrs, ns, 3, 1.0, 0, p + 4, p, ws, None), "aligned")
    hole, _ = table([p, None, p], ns3)
    bad(lib.gd_grad_sqnorm(hole, ns, 3, 1.0, 0, p, p, ws, None), "null pointer in the tensor list")
    _, zero = table([p, p, p], [10, 0, 7])
    bad(lib.gd_grad_sqnorm(ptrs, zero, 3, 1.0, 0, p, p, ws, None), "n <= 0")
    _, neg = table([p, p, p], [10, 5, -7])
    bad(lib.gd_grad_sqnorm(ptrs, neg, 3, 1.0, 0, p, p, ws, None), "n <= 0")
    odd, _ = table([p, p + 2, p], ns3)
    bad(lib.gd_grad_sqnorm(odd, ns, 3, 1.0, 0, p, p, ws, None), "aligned")
    _, huge = table([p, p, p], [10, L.GUARD_CHUNK << 31, 7])   # more chunks than one launch's grid holds
    bad(lib.gd_grad_sqnorm(ptrs, huge, 3, 1.0, 0, p, p, 1 << 40, None), "chunks")

    bad(lib.gd_guard_finalize(None, 1.0, 1, None), "null")
    bad(lib.gd_guard_finalize(p + 4, 1.0, 1, None), "aligned")
    bad(lib.gd_guard_finalize(p, float("nan"), 1, None), "NaN")

    def adam(pp=p, g=p, m=p, v=p, ema=None, n=100, rec=p, decay=0.0):
        return lib.gd_adamw_guarded(pp, g, m, v, ema, n, rec, 4e-4, 0.5, 0.999, 1e-8, 1e-4, 1.0, decay, None)

    bad(adam(pp=None), "null")
    bad(adam(g=None), "null")
    bad(adam(m=None), "null")
    bad(adam(v=None), "null")
    bad(adam(rec=None), "null")
    bad(adam(n=0), "n <= 0")
    bad(adam(n=-5), "n <= 0")
    bad(adam(ema=p + 2), "aligned")
    bad(adam(ema=p, decay=1.5), "ema_decay")


# ---- two gloo ranks ----------------------------------------------------------------------------------------------------
def _np_norm(grads, rec, gscale, accumulate):
    s = 0.0
    for g in grads:
        s += float(np.sum((g.detach().numpy().astype(np.float64).ravel() * gscale) ** 2))
    rec[0] = (rec[0].item() if accumulate else 0.0) + s


def _oracle_update(p, g, m, v, rec, lr, b1, b2, eps, wd, gscale, ema, decay):
    from oracle import functional as OF
    if rec[3].item() == 0.0:
        return
    OF.adamw_update(p, g * (gscale * rec[2].item()), m, v, int(rec[4].item()), lr, b1, b2, eps, wd)


def _same_on_all_ranks(t, world, what):
    got = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(got, t.contiguous())
    for r in range(1, world):
        assert torch.equal(got[0].view(torch.int64) if t.dtype == torch.float64 else got[0].view(torch.int32),
                           got[r].view(torch.int64) if t.dtype == torch.float64 else got[r].view(torch.int32)), what


def _worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from fill import seeded
    from gan_danet_amd.optim import AdamW
    from gan_danet_amd.parallel import GradReducer, broadcast_module, shard_batch, shard_big_params
    from oracle import functional as OF
    from oracle import modules as OM

    gb = 3                                   # uneven shards of the batch: rank 0 takes two samples, rank 1 one
    tgt = seeded((gb, 1, 32, 32), 5)
    sl = shard_batch(gb, world, rank)
    assert (sl.stop - sl.start) == (2 if rank == 0 else 1)
    # loss scales: gradient norm far above max_grad_norm = 1 (clipped), far below (not clipped), then the NaN step
    scales = (1e3, 1e-3, 1.0)
    results = []
    for sharded_mode in (False, True):
        torch.manual_seed(7)
        D = OM.Discriminator1()
        with torch.no_grad():
            D(tgt[:1])
        broadcast_module(D, src=0)
        # fc1 (8 MiB), conv4 (4.5 MiB), conv3 (1.1 MiB): three shards of different sizes per rank
        sps = shard_big_params(D, 1 << 20) if sharded_mode else []
        red = GradReducer(D.parameters(), bucket_bytes=64 << 10, sharded=sps)
        opt = AdamW(D.parameters(), lr=4e-4, betas=(0.5, 0.999), weight_decay=1e-4, grad_scale=1.0 / world, sharded=sps,
                    update_fn=_oracle_update, max_grad_norm=1.0, skip_nonfinite=True, norm_fn=_np_norm)
        fc1 = D.fc1.weight
        log = []
        for i, sc in enumerate(scales):
            for sp in sps:
                sp.wait_param()
            before = [p.detach().clone() for p in D.parameters()]
            opt.zero_grad(set_to_none=True)
            o = D(tgt[sl])
            (OF.bce_with_logits(o, torch.ones_like(o)) * sc).backward()
            red.reduce()
            if i == 2:                       # a NaN in an element that only rank 1 owns when fc1 is sharded
                k = fc1.numel() // world + 5
                if not sharded_mode:
                    fc1.grad.view(-1)[k] = float("nan")      # the summed gradient has it: on every rank
                elif rank == 1:
                    sp = [s for s in sps if s.p is fc1][0]
                    assert sp.lo <= k < sp.lo + sp.n
                    sp.wait_grad()[k - sp.lo] = float("nan")
            opt.step()
            for sp in sps:
                sp.wait_param()
            rec = opt._record().clone()
            _same_on_all_ranks(rec, world, f"step {i}: the guard record differs between the ranks")
            for (nm, p) in D.named_parameters():
                _same_on_all_ranks(p.detach(), world, f"step {i}: replicas diverged in {nm}")
            if i == 0:
                assert rec[2].item() < 1.0 and rec[3].item() == 1.0, rec
            elif i == 1:
                assert rec[2].item() == 1.0 and rec[3].item() == 1.0, rec
            else:
                assert rec[3].item() == 0.0 and not np.isfinite(rec[1].item()), rec
                for (nm, p), b in zip(D.named_parameters(), before):
                    assert torch.equal(p.detach(), b), f"the NaN step changed {nm}"
            assert np.array_equal(float(opt.grad_norm), rec[1].item(), equal_nan=True)
            assert float(opt.skipped_steps) == rec[5].item()
            log.append(rec)
        assert log[-1][4].item() == 2.0 and log[-1][5].item() == 1.0          # applied, skipped
        sd = opt.state_dict()                # collective: full tensors; `step` = the applied count
        idx = [j for j, p in enumerate(D.parameters()) if p is fc1][0]
        assert sd["state"][idx]["step"] == 2 and sd["skipped_steps"] == 1
        assert sd["state"][idx]["exp_avg"].shape == fc1.shape
        results.append(([p.detach().clone() for p in D.parameters()], sd["state"][idx]["exp_avg"].clone(), log))
        red.close()
    # sharded == unsharded on the summed gradients.  The two sum the squares in a different order (all shards' partials
    # first), so sqnorm may differ by a few fp64 ulps, coef with it, and the oracle update rounds gscale * coef to
    # fp32: at most one fp32 ulp (6e-8 relative) on the gradient of the clipped step.  An Adam step moves a weight
    # by about lr = 4e-4 whatever the gradient's scale, so the weights agree to 4e-4 * 6e-8 absolute plus 2 fp32 ulps
    for a, b in zip(results[0][2], results[1][2]):
        assert torch.allclose(a, b, rtol=1e-12, atol=0, equal_nan=True), (a, b)
    for (nm, _), a, b in zip(D.named_parameters(), results[0][0], results[1][0]):
        assert torch.allclose(a, b, rtol=2.4e-7, atol=1e-10), f"sharded guarded path changed {nm}: {(a - b).abs().max().item():.3e}"
    assert torch.allclose(results[0][1], results[1][1], rtol=2.4e-7, atol=1e-10)
    open(os.path.join(tmpdir, f"gg_ok{rank}"), "w").write("ok")
    dist.barrier()
    dist.destroy_process_group()


def test_guarded_adamw_two_ranks_gloo(tmp_path):
    world = 2
    port = 37500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"gg_ok{r}").exists() for r in range(world))


def test_guard_off_keeps_the_unguarded_optimiser():
    """no guard option: no record, no new state_dict keys, the unguarded update function"""
    from gan_danet_amd import kern as K
    from gan_danet_amd.optim import AdamW
    p = torch.nn.Parameter(torch.zeros(4))
    opt = AdamW([p], max_grad_norm=None, skip_nonfinite=False, ema_decay=None)
    assert not opt.guarded and opt.update_fn is K.adamw
    assert set(opt.state_dict().keys()) == {"state", "param_groups"}
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(ema_decay=0.9)):
        o = AdamW([p], **kw)
        assert o.guarded and o.update_fn is K.adamw_guarded
