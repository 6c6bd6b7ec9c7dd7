"""GPU: the wide flash PAM (gd_pam_wide_fwd / gd_pam_wide_bwd, 192 < C <= 511) -- kernel level against an fp64
restatement on the kernels' own 16-bit operands, bitwise-reproducible deterministic mode, the PAM / DANet modules and
wide generators against the CPU oracle, and one attention block at the tile size the project trains on
(N = 65 536), where the product chain would need 17 GB per N x N matrix."""
import pytest
import torch

from fill import fill_module
from gpu_util import DEV, assert_close, bf16_round, rell2, relmax, seeded
from pam_util import reference as _reference

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def gd():
    import gan_danet_amd as g
    from gan_danet_amd import _lib
    _lib.load()
    return g


def _packed_problem(C, N, f16, seed, B=2, qk_scale=0.6):
    """random q, k, v, x, dOut packed for the wide kernels; returns the device packs and their fp64 CPU images"""
    from gan_danet_amd import kern as K
    r = C // 8
    Np, Cp, D = (N + 255) // 256 * 256, (C + 31) // 32 * 32, K.pam_wide_slots(r)
    q, k = seeded((B, r, N), seed, qk_scale).to(DEV), seeded((B, r, N), seed + 1, qk_scale).to(DEV)
    v, x, do = seeded((B, C, N), seed + 2).to(DEV), seeded((B, C, N), seed + 3).to(DEV), seeded((B, C, N), seed + 4).to(DEV)
    _, qt = K.pack_bf16(q, r, N, scale_imm=K.LOG2E, t_shape=(Np, D), f16=f16)
    kn, kt = K.pack_bf16(k, r, N, plain_shape=(D, Np), t_shape=(Np, D), perm16=True, ones_row=D - 1, f16=f16)
    vn, vt = K.pack_bf16(v, C, N, plain_shape=(Cp, Np), t_shape=(Np, Cp), perm16=True, f16=f16)
    _, dot_ = K.pack_bf16(do, C, N, t_shape=(Np, Cp), f16=f16)
    dev = dict(qt=qt, kt=kt, kn=kn, vn=vn, vt=vt, dot=dot_, x=x, B=B, N=N, Np=Np, C=C, Cp=Cp, D=D, r=r, f16=f16)
    cpu = dict(q=qt[:, :N, :r].double().cpu() / LOG2E,      # the operands exactly as the MFMAs see them
               k=kt[:, :N, :r].double().cpu(), v=vt[:, :N, :C].double().cpu(), do=dot_[:, :N, :C].double().cpu())
    return dev, cpu


def _run_wide(p, gamma=0.7, deterministic=None):
    from gan_danet_amd import kern as K
    B, N, Np, C, Cp, D, r = p["B"], p["N"], p["Np"], p["C"], p["Cp"], p["D"], p["r"]
    g = torch.tensor([gamma], device=DEV)
    out = torch.empty(B, C, N, device=DEV)
    o_attn = torch.empty(B, C, N, device=DEV)
    lse = torch.empty(B, N, device=DEV)
    K.pam_wide_fwd(p["qt"], p["kt"], p["vn"], B, N, Np, C, Cp, D, g, p["x"], out, o_attn, lse, r_alg=r, f16=p["f16"])
    # delta = rowsum(dO . O) on the packed dO, as chan_dot forms it from gamma * dOut in the product
    delta = (p["dot"][:, :N, :C].float().transpose(1, 2) * o_attn).sum(1).contiguous()
    dqn = torch.empty(B, D, Np, device=DEV)
    dkn = torch.empty(B, D, Np, device=DEV)
    dv = torch.empty(B, Cp, Np, device=DEV)
    K.pam_wide_bwd(p["qt"], p["kt"], p["kn"], p["vt"], p["dot"], lse, delta, B, N, Np, Cp, D, dqn, dkn, dv, r_alg=r,
                   c_alg=C, f16=p["f16"], deterministic=deterministic)
    torch.cuda.synchronize()
    return dict(out=out, o=o_attn, lse=lse, delta=delta, dq=dqn[:, :r, :N], dk=dkn[:, :r, :N], dv=dv[:, :C, :N])


# measured worst case over the grid below (bf16 / fp16): o 1.8e-3 / 2.3e-4 relmax, lse 1.3e-7 / 1.3e-7 relmax,
# dq 2.1e-3 / 2.7e-4, dk 2.0e-3 / 2.5e-4, dv 1.7e-3 / 2.1e-4 rel-L2; bounds ~2.5x
_KERNEL_TOL = {False: dict(out=5e-3, lse=3e-7, dq=5e-3, dk=5e-3, dv=4e-3),
               True: dict(out=6e-4, lse=3e-7, dq=7e-4, dk=6e-4, dv=5e-4)}


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hw", [(24, 20), (45, 22)], ids=["24x20", "45x22"])
@pytest.mark.parametrize("c", [200, 224, 240, 256, 268, 320, 352, 504])
def test_pam_wide_kernels_vs_fp64(gd, c, hw, f16):
    """r = C // 8 from 25 (32 q/k slots) to 63 (64 slots, the last one the spare), one to three V chunks; N not a
    multiple of the 32 / 64 / 128-row tiles nor of the 256-row padding"""
    N = hw[0] * hw[1]
    p, cpu = _packed_problem(c, N, f16, seed=100 + c)
    got = _run_wide(p)
    ref = _reference(cpu, p["x"])
    tol = _KERNEL_TOL[f16]
    errs = {"out": relmax(got["out"], ref["out"]), "o": relmax(got["o"], ref["o"]), "lse": relmax(got["lse"], ref["lse"])}
    for n in ("dq", "dk", "dv"):
        errs[n] = rell2(got[n], ref[n])
    print(f"pam_wide C={c} N={N} {'fp16' if f16 else 'bf16'}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["out"] <= tol["out"] and errs["o"] <= tol["out"], errs
    assert errs["lse"] <= tol["lse"], errs
    for n in ("dq", "dk", "dv"):
        assert errs[n] <= tol[n], (n, errs)


@pytest.mark.parametrize("c", [240, 352])
def test_pam_wide_deterministic_backward_is_bitwise(gd, c):
    """deterministic mode: dQ as bf16 parts per key block + the reduction pass -> two runs agree bit for bit (and with
    the fp32-atomic default to the parts' rounding)"""
    p, _ = _packed_problem(c, 45 * 22, False, seed=7)
    a = _run_wide(p, deterministic=True)
    b = _run_wide(p, deterministic=True)
    for n in ("dq", "dk", "dv"):
        assert torch.equal(a[n], b[n]), n
    at = _run_wide(p, deterministic=False)
    assert rell2(a["dq"], at["dq"]) <= 5e-3
    assert torch.equal(a["dv"], at["dv"]) and torch.equal(a["dk"], at["dk"])


def test_pam_wide_argument_errors(gd):
    from gan_danet_amd import _lib as L
    lib = L.load()
    assert lib.gd_pam_wide_fwd(None, None, None, 1, 16, 256, 224, 224, 32, 0, None, None, 0, None, 0, None, None, None) == -1
    x = torch.zeros(1, device=DEV)
    ptr = x.data_ptr()
    # C <= 192 belongs to gd_pam_flash_*; C > 511 to the product chain
    assert lib.gd_pam_wide_fwd(ptr, ptr, ptr, 1, 16, 256, 160, 160, 32, 0, ptr, ptr, 0, ptr, 0, ptr, ptr, None) == -1
    assert "Cp" in L.last_error()
    assert lib.gd_pam_wide_bwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1, 16, 256, 544, 64, 0, 0, ptr, ptr, ptr, None, 0, None) == -1
    assert lib.gd_pam_wide_bwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1, 16, 256, 256, 48, 0, 0, ptr, ptr, ptr, None, 0, None) == -1


def _route_spy(monkeypatch):
    from gan_danet_amd import kern as K
    calls = {"wide": 0}
    fwd = K.pam_wide_fwd

    def spy(*a, **kw):
        calls["wide"] += 1
        return fwd(*a, **kw)
    monkeypatch.setattr(K, "pam_wide_fwd", spy)
    return calls


# module bounds: the narrow-width tests of the same modules (test_pam_fused_other_widths_vs_oracle,
# test_danet_16bit_vs_reference_fixture)
@pytest.mark.parametrize("prec", ["bf16", "fp16", "mixed"])
@pytest.mark.parametrize("hw", [(16, 16), (45, 22)], ids=["16x16", "45x22"])
@pytest.mark.parametrize("c", [224, 256, 352])
@pytest.mark.parametrize("kind", ["pam", "danet"])
def test_wide_attention_modules_vs_oracle(gd, monkeypatch, kind, c, hw, prec):
    from gan_danet_amd.generator import DANetAttention, PAMModule
    from oracle import modules as OM
    calls = _route_spy(monkeypatch)
    mo = OM.PAMModule(c) if kind == "pam" else OM.DANetAttention(c)
    fill_module(mo)
    x = bf16_round(seeded((2, c, *hw), 91))
    go = bf16_round(seeded((2, c, *hw), 92))
    xo = x.clone().requires_grad_(True)
    yo = mo.train()(xo)
    yo.backward(go)
    m = PAMModule(c) if kind == "pam" else DANetAttention(c)
    m.load_state_dict(mo.state_dict())
    m.to(DEV).train()
    xg = x.to(DEV).requires_grad_(True)
    with gd.precision(prec):
        y = m(xg)
        y.backward(go.to(DEV))
    assert calls["wide"] == 1
    po = dict(mo.named_parameters())
    if kind == "pam":
        assert_close(y, yo, 2e-2, "y")
        assert_close(xg.grad, xo.grad, 5e-2, "dx", rell2)
        tol, zero_tol = 5e-2, 0.2
    else:
        assert_close(y, yo, 6e-3, "y", rell2)
        assert_close(xg.grad, xo.grad, 9e-2, "dx", rell2)
        tol, zero_tol = 0.25, 0.2
    n = 0
    for name, p in m.named_parameters():
        if name.endswith("key.bias"):          # analytically zero (softmax shift invariance)
            assert p.grad.abs().max().item() < zero_tol * max(1.0, po[name].grad.abs().max().item())
        elif kind == "danet" and name.endswith("gamma") and prec != "mixed":
            # the two gammas' gradients are cancelling sums over dOut . O with dOut from the fuse conv's 16-bit data
            # gradient (448 / 512 / 704 input channels): measured up to 0.44 in bf16 / fp16 (the PAM-only module's gamma,
            # fed an exact dOut, stays within 5e-2 in every mode, and both hold 0.25 in "mixed")
            assert_close(p.grad, po[name].grad, 0.6, name, rell2)
        else:
            assert_close(p.grad, po[name].grad, tol, name, rell2)
        n += 1
    assert n >= 7


def test_pam_wide_at_tile_size(gd):
    """PAMModule(256) on one 256 x 256 image (N = 65 536) in bf16, forward + backward: peak memory growth under 2 GiB
    (the product chain allocates 17.2 GB for the logits alone, three such matrices for its backward); then the kernels
    at the same size against exact fp64 values on sampled rows / columns: out_i, LSE_i and dQ_i for 128 queries, dV_j
    and dK_j for 64 keys (from the kernels' own LSE and delta)."""
    from gan_danet_amd.generator import PAMModule
    c, hw = 256, 256
    m = PAMModule(c)
    fill_module(m)
    m.to(DEV).train()
    x = seeded((1, c, hw, hw), 93).to(DEV).requires_grad_(True)
    go = seeded((1, c, hw, hw), 94).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with gd.precision("bf16"):
        y = m(x)
        y.backward(go)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"pam_wide at N=65536: peak growth {grew / 2**30:.2f} GiB")
    assert grew <= 2 * 2**30, grew
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    del y, x, go, m

    N = hw * hw
    p, cpu = _packed_problem(c, N, False, seed=17, B=1, qk_scale=0.35)
    got = _run_wide(p)
    g = torch.Generator().manual_seed(5)
    iq = torch.randperm(N, generator=g)[:128]
    jk = torch.randperm(N, generator=g)[:64]
    q, k, v, do = cpu["q"][0], cpu["k"][0], cpu["v"][0], cpu["do"][0]        # (N, r), (N, r), (N, C), (N, C)
    e = q[iq] @ k.T                                                           # (128, N)
    lse = torch.logsumexp(e, -1)
    pr = torch.softmax(e, -1)
    o = pr @ v
    ds = pr * (do[iq] @ v.T - (do[iq] * o).sum(-1, keepdim=True))
    assert_close(got["lse"][0, iq], lse, 1e-5, "lse (sampled)")
    assert_close(got["o"][0][:, iq].T, o, 8e-3, "o (sampled)")
    assert_close(got["out"][0][:, iq].T, 0.7 * o + p["x"][0][:, iq].T.double().cpu(), 8e-3, "out (sampled)")
    assert_close(got["dq"][0][:, iq].T, ds @ k, 1.5e-2, "dq (sampled)", rell2)
    lse_k = got["lse"][0].double().cpu()
    delta_k = got["delta"][0].double().cpu()
    pc = torch.exp(q @ k[jk].T - lse_k[:, None])                              # (N, 64) columns of P
    dsc = pc * (do @ v[jk].T - delta_k[:, None])
    assert_close(got["dv"][0][:, jk].T, pc.T @ do, 1e-2, "dv (sampled)", rell2)
    assert_close(got["dk"][0][:, jk].T, dsc.T @ q, 1.5e-2, "dk (sampled)", rell2)


def _wide_generator(gd, g_rate):
    from oracle import modules as OM
    mo = OM.FlexibleUpsamplingModule(input_channels=8, growth_rate=g_rate).double()
    torch.manual_seed(11)
    mo.apply(OM.weights_init_normal)
    for n, p in mo.named_parameters():
        if n.endswith("gamma"):
            p.data.fill_(0.1)
    return mo


@pytest.mark.parametrize("prec", ["bf16", "mixed"])
@pytest.mark.parametrize("g_rate", [32, 48])
def test_wide_generator_vs_oracle(gd, monkeypatch, g_rate, prec):
    """growth_rate 32 (attention widths 192 / 224 / 240: the narrow kernels, then the wide ones with 32 q/k slots) and
    48 (256 / 320 / 352: wide, 64 slots) against the fp64 oracle; bounds of the default-width 16-bit generator test"""
    calls = _route_spy(monkeypatch)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 8, 32, 32, generator=g)
    mo = _wide_generator(gd, g_rate)
    xo = x.double().requires_grad_(True)
    yo = mo.train()(xo)
    go = torch.randn(yo.shape, generator=g)
    yo.backward(go.double())
    mp = gd.FlexibleUpsamplingModule(input_channels=8, growth_rate=g_rate)
    mp.load_state_dict({k: v.float() for k, v in mo.state_dict().items()})
    mp.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    with gd.precision(prec):
        y = mp(xd)
        y.backward(go.to(DEV))
    assert calls["wide"] == (2 if g_rate == 32 else 3)
    b_y, b_dx = (1e-3, 5e-2) if prec == "mixed" else (3.5e-2, 0.45)
    ey, edx = rell2(y, yo.float()), rell2(xd.grad, xo.grad.float())
    print(f"wide generator g={g_rate} {prec}: y {ey:.2e} dx {edx:.2e}")
    assert_close(y, yo.float(), b_y, f"y {prec}", rell2)
    assert_close(xd.grad, xo.grad.float(), b_dx, f"dx {prec}", rell2)


def test_wide_generator_trains_at_tile_size(gd):
    """one GanTrainer step of the growth_rate=32 generator on 256 x 256 inputs, B = 2 (bf16): finite losses, and a
    peak far below the 3 * B * 17.2 GB the product chain's saved N x N matrices alone would take"""
    G = gd.FlexibleUpsamplingModule(input_channels=8, growth_rate=32).to(DEV)
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
    with gd.precision("bf16"):
        out = tr.step(x, tgt, 0.5)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"wide generator step at 256x256, B=2: peak {peak / 2**30:.1f} GiB, loss_G {out.loss_g.item():.4f}")
    assert torch.isfinite(out.loss_g).all() and torch.isfinite(out.loss_d).all()
    assert peak <= 40 * 2**30, peak          # measured 35.2 GiB (Discriminator1's fc1 + AdamW state: ~34 GB of it)
