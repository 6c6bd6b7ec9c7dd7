"""GPU: the PAM attention probe (gd_pam_attn_stats / _received / _rows, gd_round_to_16; gan_danet_amd.attention) against an
fp64 restatement in plain torch on the CPU: E = q^T k, P = softmax(E), lse, -sum P ln P (0 ln 0 = 0), P.max(-1), P.sum(-2).

Bounds.  lse, rows, peak, received: 4 L 2^-23 relative with L = max |q . k| of the case in nats, floor 1e-6 (the bound
tests/test_gpu_pam_f32.py derives: rounding S to fp32 at L nats perturbs P by about L 2^-23 relative); for lse relative to
the largest |lse|, for rows / peak / received element by element over the elements above 1e-30 (received sums N such terms
with positive weights, so the same relative bound holds).  entropy (absolute, nats): max(4 L 2^-23 ln N, 2 cpu32) with cpu32
the error of the checker's own formula evaluated in fp32 on the CPU; where P is uniform (k = 0) the floor, 1e-6 ln N.
lse_rows equals the stats' lse at the same pixels BIT FOR BIT: the rows kernel runs the same sweep in the same order."""
import math

import pytest
import torch

from fill import fill_module
from gpu_util import DEV, relmax, seeded

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
# (B, r, H, W, planes are channel slices of a wider buffer)
CASES = {"r3_16x16": (2, 3, 16, 16, False), "r23_20x13": (2, 23, 20, 13, False), "r63_32x32": (1, 63, 32, 32, False),
         "r8_32x40_sliced": (2, 8, 32, 40, True)}
HEAVY_L = {"r3_16x16": 155.0, "r23_20x13": 200.0, "r63_32x32": 250.0, "r8_32x40_sliced": 275.0}


@pytest.fixture(scope="module")
def K():
    from gan_danet_amd import _lib
    from gan_danet_amd import kern
    _lib.load()
    return kern


def _tol(L):
    return max(4.0 * L * 2.0 ** -23, 1e-6)


def _logits(q, k):
    return q.double().transpose(1, 2) @ k.double()          # (B, N, N): E[b, i, j] = q_i . k_j


def _scaled(q, k, target):
    """q, k scaled (in fp32) so that max |q . k| is ``target`` nats"""
    s = math.sqrt(target / _logits(q, k).abs().max().item())
    return q * s, k * s


def _inputs(case, kind):
    B, r, H, W, _ = CASES[case]
    N = H * W
    seed = 1000 + 10 * list(CASES).index(case)
    if kind in ("generic", "kzero", "dominant"):
        q, k = _scaled(seeded((B, r, N), seed), seeded((B, r, N), seed + 1), 30.0)
        if kind == "kzero":
            k = torch.zeros_like(k)
        if kind == "dominant":      # channel 0 belongs to key N // 3 alone: its logit is 260 for every query, the rest stay <= 30
            jd = N // 3
            q[:, 0], k[:, 0], k[:, :, jd] = 16.25, 0.0, 0.0
            k[:, 0, jd] = 16.0
            q, k = _rescale_rest(q, k)
        return q, k
    # heavy: k_j = t_j u + noise with t rising along j, q_i = c_i u + noise with c_i > 0: every query's logit rises along j
    u = torch.nn.functional.normalize(seeded((r,), seed + 2), dim=0)[None, :, None]
    t = torch.linspace(-1.0, 1.0, N)[None, None, :]
    c = 0.6 + 0.4 * torch.rand(B, 1, N, generator=torch.Generator().manual_seed(seed + 3))
    k = t * u + 0.002 * seeded((B, r, N), seed + 4)
    q = c * u + 0.002 * seeded((B, r, N), seed + 5)
    if kind == "heavy_falling":
        k = k.flip(-1).contiguous()
    return _scaled(q, k, HEAVY_L[case])


def _rescale_rest(q, k):
    """dominant case: channels 1.. scaled so that the other keys' logits stay within 30 nats"""
    rest = (q[:, 1:].double().transpose(1, 2) @ k[:, 1:].double()).abs().max().item()
    s = math.sqrt(30.0 / rest) if rest > 30.0 else 1.0
    q[:, 1:] *= s
    k[:, 1:] *= s
    return q, k


def _checker(q, k, scale=1.0):
    """fp64 on the CPU, and the entropy formula again in fp32 for its own error"""
    E = _logits(q, k) * scale
    lse = torch.logsumexp(E, -1)
    P = torch.softmax(E, -1)
    plogp = torch.where(P > 0, P * P.clamp_min(1e-300).log(), torch.zeros_like(P))
    ent = -plogp.sum(-1)
    P32 = torch.softmax(E.float(), -1)
    ent32 = -torch.where(P32 > 0, P32 * P32.clamp_min(1e-45).log(), torch.zeros_like(P32)).sum(-1)
    return dict(E=E, P=P, lse=lse, entropy=ent, peak=P.max(-1).values, received=P.sum(-2), L=E.abs().max().item(),
                cpu32=(ent32.double() - ent).abs().max().item())


_CACHE = {}


def _case(case, kind):
    """inputs and fp64 reference of one (case, kind), computed once and shared"""
    key = (case, kind)
    if key not in _CACHE:
        q, k = _inputs(case, kind)
        _CACHE[key] = (q, k, _checker(q, k))
    return _CACHE[key]


def _planes(q, k, sliced):
    """(B, r, Npad) device planes, zero past N; ``sliced``: channel slices of one wider buffer (batch stride > r Npad)"""
    B, r, N = q.shape
    Np = (N + 255) // 256 * 256
    if sliced:
        wide = torch.zeros(B, 2 * r + 8, Np, device=DEV)
        qp, kp = wide[:, :r], wide[:, r:2 * r]
    else:
        qp, kp = torch.zeros(B, r, Np, device=DEV), torch.zeros(B, r, Np, device=DEV)
    qp[:, :, :N] = q.to(DEV)
    kp[:, :, :N] = k.to(DEV)
    return qp, kp, Np


def _run_stats(K, q, k, sliced, scale=1.0):
    B, r, N = q.shape
    qp, kp, Np = _planes(q, k, sliced)
    out = {n: torch.full((B, N), float("nan"), device=DEV) for n in ("lse", "entropy", "peak", "received")}
    K.pam_attn_stats(qp, kp, B, N, Np, r, out["lse"], out["entropy"], out["peak"], logit_scale=scale)
    K.pam_attn_received(qp, kp, out["lse"], B, N, Np, r, out["received"], logit_scale=scale)
    torch.cuda.synchronize()
    return out, (qp, kp, Np)


def _elem_rel(got, ref):
    """largest relative error over the reference elements above 1e-30"""
    got, ref = got.double().cpu(), ref.double()
    big = ref > 1e-30
    return ((got - ref).abs()[big] / ref[big]).max().item()


def _check_maps(tag, got, ref, N, uniform=False):
    for n, t in got.items():
        assert torch.isfinite(t).all(), f"{tag}: {n} has non-finite values"
    tol = _tol(ref["L"])
    errs = dict(lse=relmax(got["lse"], ref["lse"]), peak=_elem_rel(got["peak"], ref["peak"]),
                received=_elem_rel(got["received"], ref["received"]),
                entropy=(got["entropy"].double().cpu() - ref["entropy"]).abs().max().item())
    ent_tol = 1e-6 * math.log(N) if uniform else max(tol * math.log(N), 2.0 * ref["cpu32"])
    total = (got["received"].double().sum(-1).cpu() - N).abs().max().item()
    print(f"pam_probe {tag}: L {ref['L']:.1f} nats, bound {tol:.2e}: " + " ".join(f"{n} {e:.2e}" for n, e in errs.items())
          + f" (entropy bound {ent_tol:.2e}, fp32-CPU {ref['cpu32']:.2e}) | sum received - N {total:.2e} (bound {N * 2.0 ** -20:.2e})")
    for n in ("lse", "peak", "received"):
        assert errs[n] <= tol, (tag, n, errs[n], tol)
    assert errs["entropy"] <= ent_tol, (tag, errs["entropy"], ent_tol)
    assert (got["entropy"] >= 0).all(), tag
    assert total <= N * 2.0 ** -20, (tag, total)


@pytest.mark.parametrize("kind", ["generic", "heavy_rising", "heavy_falling"])
@pytest.mark.parametrize("case", list(CASES))
def test_stats_and_received_vs_fp64(K, case, kind):
    B, r, H, W, sliced = CASES[case]
    N = H * W
    q, k, ref = _case(case, kind)
    if kind.startswith("heavy"):
        assert 150.0 <= ref["L"] <= 280.0
        tile_max = torch.nn.functional.pad(ref["E"], (0, -N % 64), value=-1e300).unflatten(-1, (-1, 64)).max(-1).values
        if kind == "heavy_rising":          # the running maximum rises in every key tile: the rescale of l and u runs every step
            assert (tile_max[..., 1:] > tile_max[..., :-1]).all()
        else:                               # ... and never after the first
            assert (tile_max[..., 1:] < tile_max[..., :1]).all()
    got, _ = _run_stats(K, q, k, sliced)
    _check_maps(f"{case} {kind}", got, ref, N)
    again, _ = _run_stats(K, q, k, sliced)
    for n in got:
        assert torch.equal(got[n], again[n]), f"{n} differs between two runs"


@pytest.mark.parametrize("case", list(CASES))
def test_uniform_attention(K, case):
    """k = 0: P is uniform, entropy = ln N, peak = 1 / N, received = 1, to rounding"""
    B, r, H, W, sliced = CASES[case]
    N = H * W
    q, k, ref = _case(case, "kzero")
    got, _ = _run_stats(K, q, k, sliced)
    _check_maps(f"{case} k=0", got, ref, N, uniform=True)
    assert (got["entropy"].double().cpu() - math.log(N)).abs().max().item() <= 1e-6 * math.log(N)
    assert (got["peak"].double().cpu() * N - 1).abs().max().item() <= 1e-6
    assert (got["received"].double().cpu() - 1).abs().max().item() <= 1e-6


@pytest.mark.parametrize("case", list(CASES))
def test_one_dominant_key(K, case):
    """one key's logit is more than 200 nats above the rest for every query: entropy in [0, 1e-6), peak 1, received N at that
    key, and no NaN from 0 ln 0"""
    B, r, H, W, sliced = CASES[case]
    N = H * W
    jd = N // 3
    q, k, ref = _case(case, "dominant")
    E = ref["E"]
    others = torch.cat([E[..., :jd], E[..., jd + 1:]], -1).max(-1).values
    assert (E[..., jd] - others).min().item() >= 200.0
    got, _ = _run_stats(K, q, k, sliced)
    _check_maps(f"{case} dominant", got, ref, N)
    ent = got["entropy"].cpu()
    assert (ent >= 0).all() and (ent < 1e-6).all(), (ent.min().item(), ent.max().item())
    assert (got["peak"].double().cpu() - 1).abs().max().item() <= _tol(ref["L"])
    assert (got["received"][:, jd].double().cpu() / N - 1).abs().max().item() <= _tol(ref["L"])


def _points(N, S):
    """S pixel indices holding pixel 0, pixel N - 1 and (from S = 3 on) a repeated pixel"""
    g = torch.Generator().manual_seed(S)
    idx = torch.randint(0, N, (S,), generator=g)
    idx[0] = 0
    if S > 1:
        idx[-1] = N - 1
    if S > 2:
        idx[S // 2] = idx[1]
    return idx


@pytest.mark.parametrize("kind", ["generic", "heavy_rising"])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_vs_fp64(K, case, kind):
    B, r, H, W, sliced = CASES[case]
    N = H * W
    q, k, ref = _case(case, kind)
    tol = _tol(ref["L"])
    stats, (qp, kp, Np) = _run_stats(K, q, k, sliced)
    for S in (1, 32, 33, 70):
        idx = _points(N, S)
        idx_d = idx.to(DEV, torch.int32)
        runs = []
        for _ in range(2):
            rows = torch.full((B, S, N), float("nan"), device=DEV)
            lse_rows = torch.full((B, S), float("nan"), device=DEV)
            K.pam_attn_rows(qp, kp, idx_d, B, N, Np, r, rows, lse_rows)
            torch.cuda.synchronize()
            runs.append((rows, lse_rows))
        rows, lse_rows = runs[0]
        assert torch.equal(rows, runs[1][0]) and torch.equal(lse_rows, runs[1][1]), "two runs differ"
        assert torch.isfinite(rows).all()
        err = _elem_rel(rows, ref["P"][:, idx])
        sums = (rows.double().sum(-1).cpu() - 1).abs().max().item()
        print(f"pam_probe rows {case} {kind} S={S}: rel {err:.2e} row sums - 1 {sums:.2e} (bound {tol:.2e})")
        assert err <= tol, (S, err, tol)
        assert sums <= tol, (S, sums, tol)
        assert torch.equal(lse_rows, stats["lse"][:, idx.to(DEV)]), "lse_rows is not bitwise the stats' lse"
        assert S < 3 or torch.equal(rows[:, S // 2], rows[:, 1])
    K.pam_attn_rows(qp, kp, _points(N, 5).to(DEV, torch.int32), B, N, Np, r, torch.empty(B, 5, N, device=DEV))    # lse_rows optional
    torch.cuda.synchronize()


def test_rows_unaligned_row_length(K):
    """N % 4 != 0: the rows cannot take 16-byte stores; N = 15 x 13 = 195 also ends inside the first 32-key half of a tile"""
    B, r, N = 2, 5, 195
    q, k = _scaled(seeded((B, r, N), 77), seeded((B, r, N), 78), 30.0)
    ref = _checker(q, k)
    qp, kp, Np = _planes(q, k, False)
    idx = _points(N, 33)
    rows = torch.full((B, 33, N), float("nan"), device=DEV)
    K.pam_attn_rows(qp, kp, idx.to(DEV, torch.int32), B, N, Np, r, rows)
    torch.cuda.synchronize()
    err = _elem_rel(rows, ref["P"][:, idx])
    print(f"pam_probe rows N=195: rel {err:.2e} (bound {_tol(ref['L']):.2e})")
    assert torch.isfinite(rows).all() and err <= _tol(ref["L"])


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_round_to_16_equals_the_cpu_cast_bit_for_bit(K):
    g = torch.Generator().manual_seed(9)
    rnd = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-12, 12, (4096,), generator=g).float())
    hi = torch.randint(0x3000, 0x4800, (64,), generator=g, dtype=torch.int32)
    bf_ties = ((hi << 16) | 0x8000).view(torch.float32)                            # halfway between two bf16 values
    bf_ties = torch.cat([bf_ties, -bf_ties])
    f16_ties = torch.arange(1024, 1088).float() + 0.5                              # halfway between two fp16 values in [1024, 2048)
    f16_sub = torch.cat([torch.rand(64, generator=g) * 6.0e-5,                     # fp16's subnormal range, and its ties
                         (torch.arange(0, 64).float() + 0.5) * 2.0 ** -24])
    edge = torch.tensor([0.0, -0.0, 65504.0 * (1.0 + 2.0 ** -12), -65504.0 * (1.0 + 2.0 ** -12), 65504.0, 1.0, -1.0])
    x = torch.cat([rnd, bf_ties, f16_ties, -f16_ties, f16_sub, -f16_sub, edge])
    for f16, dt in ((False, torch.bfloat16), (True, torch.float16)):
        for scale in (1.0, LOG2E):
            if f16 and scale != 1.0:
                xs = x.clamp(-40000.0, 40000.0)                                    # stay finite after the scale
            else:
                xs = x
            want = (xs * scale).to(dt).float()
            got = K.round_to_16(xs.to(DEV), scale, f16).cpu()
            bad = (_bits(got) != _bits(want)).nonzero().flatten()
            assert bad.numel() == 0, (str(dt), scale, xs[bad[:4]].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
    assert torch.isfinite(K.round_to_16(edge.to(DEV), 1.0, True)).all()             # 65504 (1 + 2^-12) rounds down, not to inf


@pytest.fixture()
def gd():
    import gan_danet_amd as g
    return g


def _scaled_pam(gd, c, x, target):
    """PAMModule(c) with filled weights, the query conv scaled so that max |q . k| on ``x`` is about ``target`` nats"""
    from gan_danet_amd import kern as K
    from gan_danet_amd.generator import PAMModule
    m = PAMModule(c)
    fill_module(m)
    m.to(DEV).eval()
    with torch.no_grad(), gd.precision("fp32"):
        q = K.conv2d_fwd(x, m.query.weight, m.query.bias, 1, 0, 0).flatten(2)
        k = K.conv2d_fwd(x, m.key.weight, m.key.bias, 1, 0, 0).flatten(2)
        s = target / _logits(q.cpu(), k.cpu()).abs().max().item()
        m.query.weight.mul_(s)
        m.query.bias.mul_(s)
    return m


@pytest.mark.parametrize("prec,dt", [("bf16", torch.bfloat16), ("fp16", torch.float16)])
def test_as_run_operands_are_the_rounded_ones(gd, prec, dt):
    """under a 16-bit mode the probe looks at softmax(ln 2 * rne16(q log2 e) . rne16(k)): the checker rounds the same
    projections on the CPU; ragged N = 16 x 13"""
    from gan_danet_amd import kern as K
    from gan_danet_amd import ops
    from gan_danet_amd.attention import pam_attention_rows, pam_attention_stats
    B, c, H, W = 2, 64, 16, 13
    N = H * W
    x = seeded((B, c, H, W), 5).to(DEV)
    m = _scaled_pam(gd, c, x, 30.0)
    pts = [(0, 0), (H - 1, W - 1), (7, 5), (7, 5)]
    idx = torch.tensor([a * W + b for a, b in pts])
    with torch.no_grad(), gd.precision(prec):
        p = ops._prec("conv1x1")
        q = K.conv2d_fwd(x, m.query.weight, m.query.bias, 1, 0, p).flatten(2).cpu()
        k = K.conv2d_fwd(x, m.key.weight, m.key.bias, 1, 0, p).flatten(2).cpu()
        got = pam_attention_stats(m, x, "as_run")
        rows = pam_attention_rows(m, x, pts, "as_run")
        exact = pam_attention_stats(m, x, "exact")
    torch.cuda.synchronize()
    ref = _checker((q * LOG2E).to(dt).float(), k.to(dt).float(), LN2)
    _check_maps(f"as_run {prec}", {n: t.flatten(1) for n, t in got.items()}, ref, N)
    err = _elem_rel(rows.flatten(2), ref["P"][:, idx])
    print(f"pam_probe as_run {prec}: rows rel {err:.2e}")
    assert rows.shape == (B, 4, H, W) and err <= _tol(ref["L"])
    _check_maps(f"exact under {prec}", {n: t.flatten(1) for n, t in exact.items()}, _checker(q, k), N)
    assert not torch.equal(exact["lse"], got["lse"])


def test_rows_are_consistent_with_the_kernel_that_trains(gd):
    """DANetAttention(64) at 16 x 16 in fp32 mode: rows @ v^T equals the o_attn of gd_pam_f32_fwd on the same projections at
    the probed pixels, within the o cap of test_gpu_pam_f32.py (1e-5 relative max)"""
    from gan_danet_amd import kern as K
    from gan_danet_amd.attention import pam_attention_rows
    from gan_danet_amd.generator import DANetAttention
    B, c, H, W = 2, 64, 16, 16
    N, r = H * W, 8
    m = DANetAttention(c)
    fill_module(m)
    m.to(DEV).eval()
    pa = m.position_attention
    x = seeded((B, c, H, W), 6).to(DEV)
    pts = [(0, 0), (15, 15), (3, 9), (8, 1), (3, 9)]
    idx = torch.tensor([a * W + b for a, b in pts])
    with torch.no_grad(), gd.precision("fp32"):
        q = K.conv2d_fwd(x, pa.query.weight, pa.query.bias, 1, 0, 0).view(B, r, N)
        k = K.conv2d_fwd(x, pa.key.weight, pa.key.bias, 1, 0, 0).view(B, r, N)
        v = K.conv2d_fwd(x, pa.value.weight, pa.value.bias, 1, 0, 0).view(B, c, N)
        out, o = torch.empty(B, c, N, device=DEV), torch.empty(B, c, N, device=DEV)
        lse = torch.empty(B, N, device=DEV)
        K.pam_f32_fwd(q, k, v, B, N, N, c, r, torch.tensor([0.7], device=DEV), x.view(B, c, N), out, o, lse)
        rows = pam_attention_rows(m, x, pts)
    torch.cuda.synchronize()
    want = o[:, :, idx.to(DEV)].transpose(1, 2)                               # (B, S, C)
    got = rows.flatten(2).double().cpu() @ v.double().cpu().transpose(1, 2)
    err = relmax(got, want)
    print(f"pam_probe rows @ v^T against o_attn: {err:.2e}")
    assert err <= 1e-5


def test_cam_attention_vs_fp64(gd):
    """softmax(max(E) - E), E = X X^T, at C = 64, N = 256, at the CAM fixture test's fp32 tolerance (1e-4 relative max)"""
    from gan_danet_amd.attention import cam_attention
    from gan_danet_amd.generator import CAMModule, DANetAttention
    x = seeded((2, 64, 16, 16), 8, 0.3)
    e = x.double().flatten(2) @ x.double().flatten(2).transpose(1, 2)
    want = torch.softmax(e.max(-1, keepdim=True).values - e, -1)
    for mod in (CAMModule(64), DANetAttention(64)):
        got = cam_attention(mod.to(DEV), x.to(DEV))
        assert got.shape == (2, 64, 64)
        err = relmax(got, want)
        print(f"cam_attention {type(mod).__name__}: {err:.2e}")
        assert err <= 1e-4
    with pytest.raises(TypeError):
        cam_attention(torch.nn.Identity(), x.to(DEV))


def test_attention_report_on_the_generator(gd):
    from gan_danet_amd import kern as K
    from gan_danet_amd.generator import DANetAttention
    G = gd.FlexibleUpsamplingModule(input_channels=8)
    fill_module(G)
    G.to(DEV).train()
    G.initial.eval()                                    # a mixed train / eval state that must come back as it was
    x = seeded((2, 8, 16, 16), 12).to(DEV)
    blocks = {n: m for n, m in G.named_modules() if isinstance(m, DANetAttention)}
    shapes, hooks = {}, []
    for n, m in blocks.items():
        hooks.append(m.register_forward_pre_hook(lambda mod, a, n=n: shapes.__setitem__(n, tuple(a[0].shape))))
    flags = {n: m.training for n, m in G.named_modules()}
    K.set_deterministic(True)
    try:
        with torch.no_grad():
            y0 = G(x)
        for h in hooks:
            h.remove()
        pts = [(0, 0), (15, 15), (4, 11)]
        rep = gd.attention_report(G, x, points=pts)
        with pytest.raises(ValueError):                 # hooks and modes also come back when the probe refuses its arguments
            gd.attention_report(G, x, points=[(99, 0)])
        # GanTrainer.attention_report delegates (no input gate here: the same maps, bit for bit)
        D = gd.Discriminator1().to(DEV)
        with torch.no_grad():
            D(torch.zeros(2, 1, 64, 64, device=DEV))
        rep2 = gd.GanTrainer(G, D, perceptual=None).attention_report(x)
        with torch.no_grad():
            y1 = G(x)
    finally:
        K.set_deterministic(False)
    assert torch.equal(y0, y1)
    assert {n: m.training for n, m in G.named_modules()} == flags
    assert all(len(m._forward_pre_hooks) == 0 and len(m._forward_hooks) == 0 for m in G.modules())
    assert len(blocks) > 0 and set(rep) == set(blocks)
    for n, entry in rep.items():
        B, C, H, W = shapes[n]
        assert set(entry) == {"lse", "entropy", "peak", "received", "rows", "channel"}
        for key in ("lse", "entropy", "peak", "received"):
            assert entry[key].shape == (B, H, W) and torch.isfinite(entry[key]).all(), (n, key)
        assert entry["rows"].shape == (B, len(pts), H, W) and entry["channel"].shape == (B, C, C)
        # sanity only (the logits of filled weights have no set size): the bounds are the kernel tests' business
        assert (entry["rows"].double().sum((-1, -2)) - 1).abs().max().item() <= 1e-4
        assert (entry["received"].double().mean((-1, -2)) - 1).abs().max().item() <= 1e-4
        assert (entry["entropy"] >= 0).all() and (entry["entropy"] <= math.log(H * W) * (1 + 1e-6)).all()
    assert set(rep2) == set(rep)
    for n in rep:
        assert set(rep2[n]) == {"lse", "entropy", "peak", "received", "channel"}
        assert torch.equal(rep2[n]["lse"], rep[n]["lse"])
