"""GPU: the fused flash PAM on exact fp32 operands (gd_pam_f32_fwd / gd_pam_f32_bwd, C <= 511) -- the kernels against an
fp64 restatement and against the product chain on the same inputs, generator-scale logits at the training tile size on
sampled rows / columns, the modules and the generator forced onto the route at the fp32-mode tolerances, bitwise
reproducibility, the auto routing threshold, and memory at N = 65 536 where the product chain cannot run."""
import math

import pytest
import torch

from fill import fill_module
from gpu_util import DEV, assert_close, load_golden, rell2, relmax, seeded
from pam_util import reference as _reference

pytestmark = pytest.mark.gpu

GAMMA = 0.7


@pytest.fixture(scope="module")
def gd():
    import gan_danet_amd as g
    from gan_danet_amd import _lib
    _lib.load()
    return g


def _pad(t, Np):
    B, R, N = t.shape
    if N == Np:
        return t.contiguous()
    out = torch.zeros(B, R, Np, device=t.device)
    out[:, :, :N] = t
    return out


def _run_f32(q, k, v, x, do, gamma=GAMMA):
    """the new entry points on fp32 q, k (B, r, N), v, x, dOut (B, C, N)"""
    from gan_danet_amd import kern as K
    B, r, N = q.shape
    C = v.shape[1]
    Np = (N + 255) // 256 * 256
    g = torch.tensor([gamma], device=DEV)
    qp, kp, vp = _pad(q, Np), _pad(k, Np), _pad(v, Np)
    out, o = torch.empty(B, C, N, device=DEV), torch.empty(B, C, N, device=DEV)
    lse = torch.empty(B, N, device=DEV)
    K.pam_f32_fwd(qp, kp, vp, B, N, Np, C, r, g, x, out, o, lse)
    _, delta = K.chan_dot(do, o, g)
    gdo = _pad(do * gamma, Np)
    dq, dk, dv = torch.empty(B, r, N, device=DEV), torch.empty(B, r, N, device=DEV), torch.empty(B, C, N, device=DEV)
    K.pam_f32_bwd(qp, kp, vp, gdo, lse, delta, B, N, Np, C, r, dq, dk, dv)
    torch.cuda.synchronize()
    return dict(out=out, o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)


def _run_chain(q, k, v, x, do, gamma=GAMMA):
    """the product chain (what GD_PAM_F32_FLASH=0 runs in fp32 mode) on the same projections"""
    from gan_danet_amd import _lib as L
    from gan_danet_amd import ops
    g = torch.tensor([gamma], device=DEV)
    out = torch.empty_like(x)
    saved = ops._pam_chain_fwd(q, k, v, x, g, out, L.PREC_FP32)
    dq, dk, dv, _ = ops._pam_chain_bwd(saved, g, do, L.PREC_FP32)
    p, o = saved[3], saved[4]
    # the chain keeps P, not the LSE: LSE_i = e_ij - log P_ij at the row's largest P (fp64 from the chain's own P)
    e = (q.double().transpose(1, 2) @ k.double())
    pm, jm = p.double().max(-1)
    lse = e.gather(-1, jm[..., None])[..., 0] - pm.log()
    torch.cuda.synchronize()
    return dict(out=out, o=o, lse=lse, dq=dq, dk=dk, dv=dv)


_CAP = dict(out=1e-5, o=1e-5, lse=1e-5, dq=2e-5, dk=2e-5, dv=2e-5)     # the fp32-mode figures of test_config2 (tol["fp32"])


@pytest.mark.parametrize("hw", [(24, 20), (45, 22)], ids=["24x20", "45x22"])
@pytest.mark.parametrize("c", [8, 64, 160, 176, 184, 192, 200, 256, 352, 504])
def test_pam_f32_kernels_vs_fp64_and_chain(gd, c, hw):
    """r = C // 8 from 1 to 63 (odd r: one padded k-step slot), one to three V chunks, N ragged against every tile size;
    every quantity within 2x the product chain's own error against fp64 (same inputs, same test) or the fp32-mode cap"""
    N, B, r = hw[0] * hw[1], 2, c // 8
    q, k = seeded((B, r, N), 300 + c, 0.6).to(DEV), seeded((B, r, N), 301 + c, 0.6).to(DEV)
    v, x, do = seeded((B, c, N), 302 + c).to(DEV), seeded((B, c, N), 303 + c).to(DEV), seeded((B, c, N), 304 + c).to(DEV)
    cpu = dict(q=q.double().cpu().transpose(1, 2), k=k.double().cpu().transpose(1, 2), v=v.double().cpu().transpose(1, 2),
               do=(do.double().cpu() * GAMMA).transpose(1, 2))
    ref = _reference(cpu, x, GAMMA)
    got, chain = _run_f32(q, k, v, x, do), _run_chain(q, k, v, x, do)
    errs = {}
    for name, res in (("fused", got), ("chain", chain)):
        e = {n: relmax(res[n], ref[n]) for n in ("out", "o", "lse")}
        e.update({n: rell2(res[n], ref[n]) for n in ("dq", "dk", "dv")})
        errs[name] = e
        print(f"pam_f32 C={c} N={N} {name}: " + " ".join(f"{n} {val:.2e}" for n, val in e.items()))
    for n, cap in _CAP.items():
        bound = max(2.0 * errs["chain"][n], cap)
        assert errs["fused"][n] <= bound, (n, errs["fused"][n], bound, errs)


def _max_logit_log2(q, k):
    """max |q_i . k_j| over all pairs in log2 units (fp32 on the device, 4096 queries at a time)"""
    best = 0.0
    for i0 in range(0, q.shape[1], 4096):
        best = max(best, (q[:, i0:i0 + 4096].T @ k).abs().max().item())
    return best / math.log(2.0)


def test_pam_f32_generator_scale_logits_at_tile_size(gd):
    """N = 65 536, C = 184, r = 23, B = 1 with q, k scaled to generator-scale logits (214 .. 410 log2 units:
    tools/pam_bound_probe.py): out_i, LSE_i, dQ_i for 256 sampled queries and dV_j, dK_j for 64 sampled keys (from the
    kernels' own LSE and delta) against exact fp64 values.  Bound: rounding S to fp32 at L log2 units perturbs P by about
    L ln2 2^-23 relative; 4x that for the achieved L.  The gradients are cancelling sums over a near-one-hot P, so theirs
    is the larger of that and 2x the error of the same rows / columns evaluated in plain fp32 torch on the CPU."""
    C, r, N = 184, 23, 256 * 256
    q1, k1 = seeded((1, r, N), 41).to(DEV), seeded((1, r, N), 42).to(DEV)
    scale = math.sqrt(300.0 / _max_logit_log2(q1[0], k1[0]))            # aim at 300 log2 units
    q, k = q1 * scale, k1 * scale
    L2 = _max_logit_log2(q[0], k[0])
    v, x, do = seeded((1, C, N), 43).to(DEV), seeded((1, C, N), 44).to(DEV), seeded((1, C, N), 45).to(DEV)
    tol = 4.0 * L2 * math.log(2.0) * 2.0 ** -23
    print(f"pam_f32 tile size: q/k scale {scale:.4f}, max |q.k| = {L2:.1f} log2 units, 4x bound {tol:.2e}")
    assert 214.0 <= L2 <= 410.0, L2
    got = _run_f32(q, k, v, x, do)
    for n in ("out", "o", "lse", "dq", "dk", "dv"):
        assert torch.isfinite(got[n]).all(), n

    g = torch.Generator().manual_seed(5)
    iq, jk = torch.randperm(N, generator=g)[:256], torch.randperm(N, generator=g)[:64]
    qc, kc, vc = q[0].T.cpu(), k[0].T.cpu(), v[0].T.cpu()               # (N, r), (N, r), (N, C) fp32
    dc = (do[0] * GAMMA).T.cpu()                                        # gamma * dOut as the kernels take it
    lse_k, delta_k = got["lse"][0].cpu(), got["delta"][0].cpu()

    def rows(dt):
        qd, kd, vd, dd = qc.to(dt), kc.to(dt), vc.to(dt), dc.to(dt)
        e = qd[iq] @ kd.T
        lse = torch.logsumexp(e, -1)
        pr = torch.softmax(e, -1)
        o = pr @ vd
        ds = pr * (dd[iq] @ vd.T - (dd[iq] * o).sum(-1, keepdim=True))
        pc = torch.exp(qd @ kd[jk].T - lse_k.to(dt)[:, None])          # (N, 64) columns of P from the kernels' LSE
        dsc = pc * (dd @ vd[jk].T - delta_k.to(dt)[:, None])
        return dict(lse=lse, o=o, dq=ds @ kd, dv=pc.T @ dd, dk=dsc.T @ qd)

    ref, f32 = rows(torch.float64), rows(torch.float32)
    xs = x[0][:, iq].T.double().cpu()
    meas = dict(lse=relmax(got["lse"][0, iq], ref["lse"]), o=relmax(got["o"][0][:, iq].T, ref["o"]),
                out=relmax(got["out"][0][:, iq].T, GAMMA * ref["o"] + xs),
                dq=rell2(got["dq"][0][:, iq].T, ref["dq"]), dv=rell2(got["dv"][0][:, jk].T, ref["dv"]),
                dk=rell2(got["dk"][0][:, jk].T, ref["dk"]))
    cpu32 = {n: rell2(f32[n], ref[n]) for n in ("dq", "dv", "dk")}
    print("pam_f32 tile size measured: " + " ".join(f"{n} {val:.2e}" for n, val in meas.items()))
    print("pam_f32 tile size fp32-CPU: " + " ".join(f"{n} {val:.2e}" for n, val in cpu32.items()))
    for n in ("lse", "o", "out"):
        assert meas[n] <= tol, (n, meas[n], tol)
    for n in ("dq", "dv", "dk"):
        bound = max(tol, 2.0 * cpu32[n])
        assert meas[n] <= bound, (n, meas[n], bound)


def _spies(monkeypatch):
    """count the fused fp32 forward calls and the product-chain forward calls"""
    from gan_danet_amd import kern as K
    from gan_danet_amd import ops
    calls = {"f32": 0, "chain": 0}
    fwd, chain = K.pam_f32_fwd, ops._pam_chain_fwd

    def spy_f32(*a, **kw):
        calls["f32"] += 1
        return fwd(*a, **kw)

    def spy_chain(*a, **kw):
        calls["chain"] += 1
        return chain(*a, **kw)
    monkeypatch.setattr(K, "pam_f32_fwd", spy_f32)
    monkeypatch.setattr(ops, "_pam_chain_fwd", spy_chain)
    return calls


def _force(monkeypatch, value=True):
    from gan_danet_amd import kern as K
    monkeypatch.setattr(K, "PAM_F32_FLASH", value)


def _check_fixture_grads(mod, fx, tol, metric=relmax, zero_tol=1e-2):
    params = dict(mod.named_parameters())
    n = 0
    for key, val in fx.items():
        if key.startswith("grad__") and not key.endswith("_head"):
            name = key[6:].replace("__", ".")
            if name.endswith("key.bias"):   # analytically zero (softmax shift invariance)
                assert params[name].grad.abs().max().item() < zero_tol * max(1.0, val.abs().max().item())
            else:
                assert_close(params[name].grad, val, tol, name, metric)
            n += 1
    assert n > 0


@pytest.mark.parametrize("tag,c", [("c32_8x8", 32), ("c160_16x16", 160)])
def test_pam_module_fixture_on_f32_route(gd, golden_dir, monkeypatch, tag, c):
    from gan_danet_amd.generator import PAMModule
    _force(monkeypatch)
    calls = _spies(monkeypatch)
    fx = load_golden(golden_dir, f"pam_{tag}")
    m = PAMModule(c)
    fill_module(m)
    with torch.no_grad():
        m.gamma.fill_(0.7)
    m.to(DEV)
    x = fx["x"].to(DEV).requires_grad_(True)
    with gd.precision("fp32"):
        y = m(x)
        y.backward(fx["go"].to(DEV))
    assert calls == {"f32": 1, "chain": 0}
    assert_close(y, fx["y"], 1e-4, "y")
    assert_close(x.grad, fx["gx"], 1e-3, "dx")
    _check_fixture_grads(m, fx, 1e-3)


def test_danet_fixture_on_f32_route(gd, golden_dir, monkeypatch):
    from gan_danet_amd.generator import DANetAttention
    _force(monkeypatch)
    calls = _spies(monkeypatch)
    fx = load_golden(golden_dir, "danet_c64_16x16")
    m = DANetAttention(64)
    fill_module(m)
    m.to(DEV).train()
    x = fx["x"].to(DEV).requires_grad_(True)
    with gd.precision("fp32"):
        y = m(x)
        y.backward(fx["go"].to(DEV))
    assert calls == {"f32": 1, "chain": 0}
    assert_close(y, fx["y"], 1e-4, "y")
    assert_close(x.grad, fx["gx"], 1e-3, "dx", rell2)
    _check_fixture_grads(m, fx, 1e-3, rell2)


def test_generator_fixture_on_f32_route(gd, golden_dir, monkeypatch):
    """bounds of test_generator_vs_reference_fixture[fp32]"""
    from gan_danet_amd import FlexibleUpsamplingModule
    _force(monkeypatch)
    calls = _spies(monkeypatch)
    fx = load_golden(golden_dir, "generator_8ch_16x16")
    G = FlexibleUpsamplingModule(input_channels=8)
    fill_module(G)
    G.to(DEV).train()
    x = fx["x"].to(DEV).requires_grad_(True)
    with gd.precision("fp32"):
        y = G(x)
        y.backward(fx["go"].to(DEV))
    assert calls == {"f32": 3, "chain": 0}
    assert_close(y, fx["y"], 1e-3, "y (north star 1e-3)")
    assert_close(y, fx["y"], 1e-4, "y", rell2)
    assert_close(x.grad, fx["gx"], 2e-2, "dx", rell2)
    assert_close(G.upsample[1].running_mean, fx["rm_up1"], 1e-4, "rm")
    _check_fixture_grads(G, fx, 2e-2, rell2)
    G.eval()
    with torch.no_grad(), gd.precision("fp32"):
        ye = G(x)
    assert_close(ye, load_golden(golden_dir, "generator_8ch_16x16_eval")["y"], 1e-3, "eval y")


@pytest.mark.parametrize("c", [224, 352])
def test_wide_pam_module_vs_oracle_on_f32_route(gd, monkeypatch, c):
    """widths past the narrow kernels (two V chunks; r = 28 and 44) at a ragged N, against the fp64 CPU oracle"""
    from gan_danet_amd.generator import PAMModule
    from oracle import modules as OM
    _force(monkeypatch)
    calls = _spies(monkeypatch)
    mo = OM.PAMModule(c)
    fill_module(mo)
    with torch.no_grad():
        mo.gamma.fill_(0.7)
    m = PAMModule(c)
    m.load_state_dict(mo.state_dict())
    m.to(DEV).train()
    mo.double().train()
    x, go = seeded((2, c, 45, 22), 91), seeded((2, c, 45, 22), 92)
    xo = x.double().requires_grad_(True)
    yo = mo(xo)
    yo.backward(go.double())
    xg = x.to(DEV).requires_grad_(True)
    with gd.precision("fp32"):
        y = m(xg)
        y.backward(go.to(DEV))
    assert calls == {"f32": 1, "chain": 0}
    assert_close(y, yo, 1e-4, "y")
    assert_close(xg.grad, xo.grad, 1e-3, "dx")
    po = dict(mo.named_parameters())
    n = 0
    for name, p in m.named_parameters():
        if name.endswith("key.bias"):          # analytically zero (softmax shift invariance)
            assert p.grad.abs().max().item() < 1e-2 * max(1.0, po[name].grad.abs().max().item())
        else:
            assert_close(p.grad, po[name].grad, 1e-3, name)
        n += 1
    assert n >= 7


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_pam_f32_route_is_bitwise_reproducible(gd, monkeypatch, det):
    from gan_danet_amd import kern as K
    from gan_danet_amd.generator import PAMModule
    _force(monkeypatch)
    calls = _spies(monkeypatch)
    m = PAMModule(184)
    fill_module(m)
    m.to(DEV).train()
    x, go = seeded((2, 184, 45, 22), 61).to(DEV), seeded((2, 184, 45, 22), 62).to(DEV)
    runs = []
    K.set_deterministic(det)
    try:
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            xg = x.clone().requires_grad_(True)
            with gd.precision("fp32"):
                y = m(xg)
                y.backward(go)
            runs.append([y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    finally:
        K.set_deterministic(False)
    assert calls == {"f32": 2, "chain": 0}
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), f"tensor {i} differs between two runs"


def _pam_forward_only(gd, prec, B, hw, override=None, c=16):
    from gan_danet_amd.generator import PAMModule
    m = PAMModule(c)
    fill_module(m)
    m.to(DEV).eval()
    x = seeded((B, c, *hw), 71).to(DEV)
    with torch.no_grad(), gd.precision(prec):
        if override:
            with gd.layer_override(pam=override):
                y = m(x)
        else:
            y = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()


def test_pam_f32_auto_routing(gd, monkeypatch):
    """default (GD_PAM_F32_FLASH unset): the fused kernels only where B N^2 > 2^31; the largest exact-mode PAMs of the
    existing suite (B = 4 at 180 x 88, B = 1 at 128 x 128) stay on the product chain; 16-bit modes never take the route"""
    _force(monkeypatch, None)
    calls = _spies(monkeypatch)
    _pam_forward_only(gd, "fp32", 4, (180, 88))
    assert calls == {"f32": 0, "chain": 1}
    _pam_forward_only(gd, "fp32", 1, (128, 128))
    assert calls == {"f32": 0, "chain": 2}
    _pam_forward_only(gd, "fp32", 2, (256, 256))
    assert calls == {"f32": 1, "chain": 2}
    _pam_forward_only(gd, "bf16", 2, (256, 256), override="exact")
    assert calls == {"f32": 2, "chain": 2}
    _pam_forward_only(gd, "bf16", 2, (256, 256))
    assert calls == {"f32": 2, "chain": 2}
    _force(monkeypatch, False)                      # GD_PAM_F32_FLASH=0: never
    _pam_forward_only(gd, "fp32", 1, (16, 16))
    assert calls == {"f32": 2, "chain": 3}
    _force(monkeypatch, True)                       # GD_PAM_F32_FLASH=1: always, but only for exact operands
    _pam_forward_only(gd, "fp32", 1, (16, 16))
    _pam_forward_only(gd, "bf16", 1, (16, 16))
    assert calls == {"f32": 3, "chain": 3}


def test_pam_f32_memory_at_tile_size(gd, monkeypatch):
    """PAMModule(184) on 256 x 256, B = 2, fp32 mode, default routing, forward + backward: peak growth <= 4 GiB (about
    fifteen planes of 96 MB must exist; ONE logits matrix of the product chain is 34 GB at this shape)"""
    from gan_danet_amd.generator import PAMModule
    _force(monkeypatch, None)
    calls = _spies(monkeypatch)
    c, hw = 184, 256
    m = PAMModule(c)
    fill_module(m)
    m.to(DEV).train()
    x = seeded((2, c, hw, hw), 93).to(DEV).requires_grad_(True)
    go = seeded((2, c, hw, hw), 94).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with gd.precision("fp32"):
        y = m(x)
        y.backward(go)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"pam_f32 at N=65536, B=2, C=184: peak growth {grew / 2**30:.2f} GiB")
    assert calls == {"f32": 1, "chain": 0}
    assert grew <= 4 * 2**30, grew
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_fp32_mode_trains_at_tile_size(gd, monkeypatch):
    """one GanTrainer step of the default generator on 256 x 256 inputs, B = 2, in fp32 mode: finite losses and a peak
    below the 3 * B * 17.2 GB that ONE attention block's saved chain matrices alone would take"""
    _force(monkeypatch, None)
    calls = _spies(monkeypatch)
    G = gd.FlexibleUpsamplingModule(input_channels=8).to(DEV)
    D = gd.Discriminator1().to(DEV)
    x = torch.randn(2, 8, 256, 256, device=DEV)
    tgt = torch.randn(2, 1, 1024, 1024, device=DEV)
    with torch.no_grad():
        D(tgt)
    torch.manual_seed(0)
    G.apply(gd.weights_init_normal)
    D.apply(gd.weights_init_normal)
    for n, p in G.named_parameters():
        if n.endswith("gamma"):
            p.data.fill_(0.1)
    tr = gd.GanTrainer(G, D, perceptual=None)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with gd.precision("fp32"):
        out = tr.step(x, tgt, 0.5)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"fp32 generator step at 256x256, B=2: peak {peak / 2**30:.1f} GiB, loss_G {out.loss_g.item():.4f}")
    assert calls["f32"] >= 3 and calls["chain"] == 0, calls
    assert torch.isfinite(out.loss_g).all() and torch.isfinite(out.loss_d).all()
    assert peak < 3 * 2 * 17.2e9, peak


def test_pam_f32_cabi(gd):
    from gan_danet_amd import _lib as L
    lib = L.load()
    for name in ("gd_pam_f32_fwd", "gd_pam_f32_bwd"):
        assert hasattr(lib, name), name
    x = torch.zeros(256 * 8, device=DEV)
    p = x.data_ptr()

    def fwd(C=8, r=1, Npad=256, q=p):
        return lib.gd_pam_f32_fwd(q, 0, p, 0, p, 0, 1, 16, Npad, C, r, p, p, 0, p, 0, p, p, None)

    def bwd(C=8, r=1, Npad=256, dq=p):
        return lib.gd_pam_f32_bwd(p, 0, p, 0, p, 0, p, 0, p, p, 1, 16, Npad, C, r, dq, p, p, None)
    for call in (fwd, bwd):
        assert call(C=512) == -1 and "C (" in L.last_error(), L.last_error()
        assert call(r=64) == -1 and "r (" in L.last_error(), L.last_error()
        assert call(Npad=250) == -1 and "Npad" in L.last_error(), L.last_error()
        assert call(Npad=0) == -1 and "Npad" in L.last_error(), L.last_error()
    assert fwd(q=None) == -1 and "null pointer" in L.last_error()
    assert bwd(dq=None) == -1 and "null pointer" in L.last_error()
