"""GPU: the guarded optimiser step -- gd_grad_sqnorm / gd_guard_finalize / gd_adamw_guarded, optim.AdamW's guard options and
GanTrainer's.  References are numpy fp64, or torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ on CPU copies."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, assert_close

pytestmark = pytest.mark.gpu

CHUNK = 65536
BIG = CHUNK * 3 + 5                  # several chunks and a ragged tail
# 150 tensors (more than one launch's argument chunk): the edge sizes first, then small odd ones
SIZES = [1, 3, 257, BIG] + [5 + 7 * i for i in range(146)]
OFFSETS = {4: 1, 5: 3}               # tensor index -> element offset of its view: only 4-byte aligned pointers
BETAS, LR, WD = (0.5, 0.999), 4e-4, 1e-4


def _int_grads(seed=0):
    """k / 1024 with |k| <= 2048: every square and every partial sum of squares is exact in fp64"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-2048, 2049, (n,), generator=g).to(torch.float32) / 1024 for n in SIZES]


def _to_dev(cpu, offsets=OFFSETS):
    out = []
    for i, t in enumerate(cpu):
        off = offsets.get(i, 0)
        buf = torch.zeros(t.numel() + off + 4, device=DEV)
        view = buf[off:off + t.numel()]
        view.copy_(t)
        assert view.data_ptr() % 16 == (4 * off) % 16
        out.append(view)
    return out


def _np_sqnorm(cpu):
    return float(sum(np.sum(t.numpy().astype(np.float64) ** 2) for t in cpu))


@pytest.fixture(scope="module")
def K():
    from gan_danet_amd import kern
    return kern


def test_norm_exact_on_every_edge(K):
    cpu = _int_grads()
    assert len(cpu) == 150 and cpu[0].numel() == 1 and cpu[1].numel() == 3 and cpu[2].numel() == 257
    dev = _to_dev(cpu)
    want = _np_sqnorm(cpu)
    rec = K.guard_record(DEV)
    K.grad_sqnorm(dev, rec)
    first = rec.cpu()
    print("sqnorm", first[0].item(), "numpy", want)
    assert first[0].item() == want
    rec2 = K.guard_record(DEV)
    K.grad_sqnorm(dev, rec2)
    assert torch.equal(rec2.cpu().view(torch.int64), first.view(torch.int64))
    rec3 = K.guard_record(DEV)
    rec3[0] = 123.0                                            # accumulate = False overwrites what was there
    K.grad_sqnorm(dev[:70], rec3)
    K.grad_sqnorm(dev[70:], rec3, accumulate=True)
    assert torch.equal(rec3.cpu().view(torch.int64), first.view(torch.int64))
    # every tensor alone (each edge on its own, against its own exact value), and the scale
    for i in (0, 1, 2, 3, 4, 5):
        r = K.guard_record(DEV)
        K.grad_sqnorm([dev[i]], r)
        assert r[0].item() == _np_sqnorm([cpu[i]]), i
    r = K.guard_record(DEV)
    K.grad_sqnorm(dev, r, grad_scale=0.5)
    assert r[0].item() == want / 4
    # finalise on the exact value
    K.guard_finalize(rec, max_norm=1.0, skip_nonfinite=True)
    got = rec.cpu().tolist()
    assert got[0] == want and abs(got[1] - np.sqrt(want)) <= 2.0 ** -52 * got[1] and got[3] == 1.0 and got[4] == 1.0 and got[5] == 0.0
    assert abs(got[2] - 1.0 / (np.sqrt(want) + 1e-6)) <= 1e-15
    K.guard_finalize(rec, max_norm=None, skip_nonfinite=True)
    assert rec.cpu().tolist()[2:] == [1.0, 1.0, 2.0, 0.0]


def test_norm_random_data(K):
    g = torch.Generator().manual_seed(3)
    sizes = [1, 3, 257, BIG, 300_001, 2 * CHUNK, CHUNK - 1, 123_457]
    assert sum(sizes) <= 2 ** 20
    cpu = [torch.randn(n, generator=g) * (10.0 ** (i % 3 - 1)) for i, n in enumerate(sizes)]
    dev = _to_dev(cpu, {1: 1, 3: 3, 4: 2})
    rec = K.guard_record(DEV)
    K.grad_sqnorm(dev, rec)
    want, got = _np_sqnorm(cpu), rec[0].item()
    print("rel err", abs(got - want) / want)
    assert abs(got - want) <= 2.0 ** 20 * 2.0 ** -53 * want


def test_norm_64bit_indexing(K):
    n = 2 ** 31 + 5
    x = torch.full((n,), 2.0 ** -8, device=DEV)
    try:
        rec = K.guard_record(DEV)
        K.grad_sqnorm([x], rec)
        got = rec[0].item()
    finally:
        del x
        torch.cuda.empty_cache()
    assert got == n * 2.0 ** -16


# ---- optim.AdamW -----------------------------------------------------------------------------------------------------------
PLAIN = SIZES[:4] + SIZES[6:]        # the list of the norm test without the two offset views


def _pair(seed=1, **kw):
    """the same parameters on the CPU (reference) and on the GPU (optimiser under test)"""
    from gan_danet_amd import AdamW
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=g) for n in PLAIN]
    pr = [torch.nn.Parameter(p.clone()) for p in p0]
    pg = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    o_r = torch.optim.AdamW(pr, lr=LR, betas=BETAS, weight_decay=WD)
    o_g = AdamW(pg, lr=LR, betas=BETAS, weight_decay=WD, **kw)
    return pr, pg, o_r, o_g


def _grads(step, scale=1.0):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(n, generator=g) * scale for n in PLAIN]


def _set_grads(params, grads, dev=None):
    for p, g in zip(params, grads):
        p.grad = g.clone() if dev is None else g.clone().to(dev)


def test_clip_adamw_parity():
    scales = (4.0, 1.0, 0.25)
    norms = [float(np.sqrt(_np_sqnorm(_grads(t, s)))) for t, s in enumerate(scales)]
    max_norm = float(np.sqrt(norms[0] * norms[2]))
    pr, pg, o_r, o_g = _pair(max_grad_norm=max_norm)
    for t, s in enumerate(scales):
        gs = _grads(t, s)
        _set_grads(pr, gs)
        _set_grads(pg, gs, DEV)
        ref_norm = float(torch.nn.utils.clip_grad_norm_(pr, max_norm))
        if t == 0:
            assert ref_norm > max_norm * 1.5                  # step 1 clips ...
        if t == 2:
            assert ref_norm < max_norm / 1.5                  # ... step 3 does not
        o_r.step()
        o_g.step()
        got = float(o_g.grad_norm)
        print("step", t, "norm", got, "ref", ref_norm, "coef", o_g._record()[2].item())
        assert abs(got - ref_norm) <= 1e-6 * ref_norm
        assert (o_g._record()[2].item() < 1.0) == (ref_norm > max_norm)
    for i, (a, b) in enumerate(zip(pg, pr)):
        assert_close(a, b, 1e-6, f"clipped adamw param {i} (n = {b.numel()})")
    assert float(o_g.skipped_steps) == 0.0


def test_guard_off_equals_today():
    from gan_danet_amd import AdamW
    _, pa, _, oa = _pair(max_grad_norm=None, skip_nonfinite=False, ema_decay=None)
    _, pb, _, ob = _pair()
    assert not oa.guarded and type(oa) is AdamW
    for t in range(2):
        gs = _grads(t)
        _set_grads(pa, gs, DEV)
        _set_grads(pb, gs, DEV)
        oa.step()
        ob.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    assert set(oa.state_dict().keys()) == {"state", "param_groups"}


@pytest.mark.parametrize("where", ["nan_first_of_one_element_tensor", "inf_last_of_multi_chunk_tensor"])
def test_skip(where):
    pr, pg, o_r, o_g = _pair(skip_nonfinite=True, ema_decay=0.9)
    gs = _grads(0)
    _set_grads(pr, gs)
    _set_grads(pg, gs, DEV)
    o_r.step()
    o_g.step()
    before = [(p.detach().clone(), o_g.state[p]["exp_avg"].clone(), o_g.state[p]["exp_avg_sq"].clone(),
               o_g.state[p]["ema"].clone()) for p in pg]
    bad = _grads(1)
    if where.startswith("nan"):
        assert bad[0].numel() == 1
        bad[0][0] = float("nan")
    else:
        assert bad[3].numel() == BIG
        bad[3][-1] = float("inf")
    _set_grads(pg, bad, DEV)
    o_g.step()
    for p, (p0, m0, v0, e0) in zip(pg, before):
        st = o_g.state[p]
        assert torch.equal(p.detach(), p0) and torch.equal(st["exp_avg"], m0) and torch.equal(st["exp_avg_sq"], v0)
        assert torch.equal(st["ema"], e0)
    assert float(o_g.skipped_steps) == 1.0 and not np.isfinite(float(o_g.grad_norm))
    gs = _grads(2)                            # the reference took one step fewer: its step 2 is the optimiser's third call
    _set_grads(pr, gs)
    _set_grads(pg, gs, DEV)
    o_r.step()
    o_g.step()
    for i, (a, b) in enumerate(zip(pg, pr)):
        assert_close(a, b, 1e-6, f"param {i} after a skipped step")
    assert float(o_g.skipped_steps) == 1.0 and o_g.state_dict()["state"][0]["step"] == 2


def test_ema_and_no_extra_launch(monkeypatch, K):
    calls = {}

    def counted(name):
        fn = getattr(K, name)

        def wrapper(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        return wrapper

    for name in [n for n in dir(K) if callable(getattr(K, n)) and not n.startswith("_") and n not in ("lib", "Tensor")
                 and getattr(getattr(K, n), "__module__", "") == K.__name__]:
        monkeypatch.setattr(K, name, counted(name))
    d = 0.9
    pr, pg, o_r, o_g = _pair(ema_decay=d)
    _, pn, _, o_n = _pair(skip_nonfinite=True)          # guarded, no EMA
    ema = [p.detach().double().clone() for p in pr]
    per_opt = []
    for opt, params in ((o_g, pg), (o_n, pn)):
        calls.clear()
        for t in range(4):
            gs = _grads(t)
            _set_grads(params, gs, DEV)
            opt.step()
        per_opt.append(dict(calls))
    for t in range(4):
        _set_grads(pr, _grads(t))
        o_r.step()
        ema = [d * e + (1 - d) * p.detach().double() for e, p in zip(ema, pr)]
    print("kern calls with / without EMA:", per_opt)
    assert per_opt[0] == per_opt[1] == {"grad_sqnorm": 4, "guard_finalize": 4, "adamw_guarded": 4 * len(PLAIN)}
    shadows = o_g.ema_params()
    assert len(shadows) == len(PLAIN)
    for i, (s, e, p) in enumerate(zip(shadows, ema, pg)):
        assert_close(s, e.float(), 1e-6, f"ema shadow {i}")
        assert s.shape == p.shape
    for a, b in zip(pg, pn):                             # the EMA changes nothing about the weights
        assert torch.equal(a, b)


# ---- GanTrainer ----------------------------------------------------------------------------------------------------------------
def _nets(gd, Go0, Do0, tgt):
    G, D = gd.FlexibleUpsamplingModule(input_channels=8).to(DEV), gd.Discriminator1().to(DEV)
    with torch.no_grad(), gd.precision("fp32"):
        D(tgt.to(DEV))
    G.load_state_dict(Go0)
    D.load_state_dict(Do0)
    return G.train(), D.train()


def test_trainer_guarded(tmp_path):
    import gan_danet_amd as gd
    from gan_danet_amd import checkpoint as C
    from oracle import modules as OM
    from oracle import step as OS
    torch.manual_seed(0)
    Go, Do = OM.FlexibleUpsamplingModule(input_channels=8), OM.Discriminator1()
    x, tgt = torch.randn(2, 8, 16, 16), torch.randn(2, 1, 64, 64)
    with torch.no_grad():
        Do(tgt)
    Go.apply(OM.weights_init_normal)
    Do.apply(OM.weights_init_normal)
    for n, p in Go.named_parameters():
        if n.endswith("gamma"):
            p.data.fill_(0.1)
    Go0 = {k: v.clone() for k, v in Go.state_dict().items()}
    Do0 = {k: v.clone() for k, v in Do.state_dict().items()}
    MAX_G, MAX_D = 0.05, 0.05
    d_first = next(Do.parameters())
    ref_norms = []

    def clip(params):                         # clip_grad_norm_, restated: between backward and the update
        mx = MAX_D if params[0] is d_first else MAX_G
        norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params if p.grad is not None)))
        coef = min(1.0, mx / (norm + 1e-6))
        for p in params:
            if p.grad is not None:
                p.grad.mul_(coef)
        ref_norms.append((norm, coef))

    og, od = OS.AdamWState(lr=2e-4), OS.AdamWState(lr=4e-4)
    refs = [OS.train_step(Go.train(), Do.train(), og, od, x, tgt, 0.5, 1e-5, None, grad_hook=clip) for _ in range(2)]
    print("oracle (norm, coef) per backward:", ref_norms)
    assert ref_norms[0][1] < 1.0 and ref_norms[1][1] < 1.0          # the first D and G steps do clip

    G, D = _nets(gd, Go0, Do0, tgt)
    tr = gd.GanTrainer(G, D, perceptual=None, max_grad_norm_g=MAX_G, max_grad_norm_d=MAX_D, skip_nonfinite=True,
                       ema_decay=0.99)
    xd, td = x.to(DEV), tgt.to(DEV)
    gd.set_deterministic(True)
    try:
        with gd.precision("fp32"):
            for i in range(2):
                out = tr.step(xd, td, 0.5)
                for k in ("grad_norm_g", "grad_norm_d", "skipped_g", "skipped_d"):
                    assert k in out.parts and out.parts[k].is_cuda and out.parts[k].dim() == 0
                assert torch.isfinite(out.parts["grad_norm_g"]) and torch.isfinite(out.parts["grad_norm_d"])
                assert out.parts["grad_norm_g"].item() > 0 and out.parts["grad_norm_d"].item() > 0
                assert out.parts["skipped_g"].item() == 0 and out.parts["skipped_d"].item() == 0
                ld, lg = out.loss_d.item(), out.loss_g.item()
                print("step", i, "loss_d", ld, refs[i].loss_d, "loss_g", lg, refs[i].loss_g, "norms",
                      out.parts["grad_norm_d"].item(), out.parts["grad_norm_g"].item())
                assert abs(ld - refs[i].loss_d) <= 1e-3 * abs(refs[i].loss_d) + 1e-6, (i, ld)
                tol = 1e-4 if i == 0 else 3e-2
                assert abs(lg - refs[i].loss_g) <= tol * abs(refs[i].loss_g), (i, lg)
            for net, ora in ((G, Go), (D, Do)):
                n = float(torch.sqrt(sum((p.detach().double() ** 2).sum() for p in net.parameters())))
                r = float(torch.sqrt(sum((p.detach().double() ** 2).sum() for p in ora.parameters())))
                assert abs(n - r) <= 1e-5 * n

            # the averaged generator: same class, shadows as parameters, runs an eval forward, differs from G
            E = tr.ema_generator()
            assert type(E) is type(G)
            shadows = tr.opt_g.ema_params()
            assert all(p.data_ptr() == s.data_ptr() for p, s in zip(E.parameters(), shadows))
            assert all(torch.equal(a, b) for a, b in zip(E.buffers(), G.buffers()))
            with torch.no_grad():
                ye = E.eval()(xd)
                yg = G.eval()(xd)
            G.train()
            assert torch.isfinite(ye).all() and ye.shape == yg.shape and not torch.equal(ye, yg)
            assert any(not torch.equal(p, s) for p, s in zip(G.parameters(), shadows))

            # checkpoint round trip
            path = str(tmp_path / "state.pth")
            C.save_training_state(path, tr, epoch=1)
            kept = ([s.clone() for s in shadows], tr.opt_g.grad_norm.clone(), tr.opt_d.grad_norm.clone())
            out_a = tr.step(xd, td, 0.5)
            torch.manual_seed(123)
            G2, D2 = _nets(gd, {k: torch.randn_like(v) if v.is_floating_point() else v for k, v in Go0.items()}, Do0, tgt)
            tr2 = gd.GanTrainer(G2, D2, perceptual=None, max_grad_norm_g=MAX_G, max_grad_norm_d=MAX_D, skip_nonfinite=True,
                                ema_decay=0.99)
            C.load_training_state(path, tr2)
            assert torch.equal(tr2.opt_g.grad_norm, kept[1]) and torch.equal(tr2.opt_d.grad_norm, kept[2])
            assert torch.equal(tr2.opt_g.skipped_steps, tr.opt_g.skipped_steps)
            assert all(torch.equal(a, b) for a, b in zip(tr2.opt_g.ema_params(), kept[0]))
            out_b = tr2.step(xd, td, 0.5)
    finally:
        gd.set_deterministic(False)
    assert torch.equal(out_a.loss_g, out_b.loss_g) and torch.equal(out_a.loss_d, out_b.loss_d)
    for k in ("grad_norm_g", "grad_norm_d"):
        assert torch.equal(out_a.parts[k], out_b.parts[k])
    for (k, a), b in zip(G.state_dict().items(), G2.state_dict().values()):
        assert torch.equal(a, b), k
    for a, b in zip(tr.opt_g.ema_params(), tr2.opt_g.ema_params()):
        assert torch.equal(a, b)

    # a checkpoint written WITHOUT the feature loads; the shadows then start from the current weights
    G3, D3 = _nets(gd, Go0, Do0, tgt)
    plain = gd.GanTrainer(G3, D3, perceptual=None)
    with gd.precision("fp32"):
        out_p = plain.step(xd, td, 0.5)
    assert set(out_p.parts.keys()) == {"adv", "pix", "tv", "ssim"}        # exactly today's keys
    path2 = str(tmp_path / "plain.pth")
    C.save_training_state(path2, plain, epoch=1)
    C.load_training_state(path2, tr2)
    assert float(tr2.opt_g.skipped_steps) == 0.0 and tr2.opt_g._record()[4].item() == 1.0
    for s, p in zip(tr2.opt_g.ema_params(), G2.parameters()):
        assert torch.equal(s, p.detach())
