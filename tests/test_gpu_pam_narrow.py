"""GPU: the narrow flash PAM (gd_pam_flash_fwd / gd_pam_flash_fwd_shift / gd_pam_key_sqnorm_max / gd_pam_flash_bwd,
C <= 192: the route the benchmark and every generator run on) -- kernel level against the fp64 restatement of
tests/pam_util.py on the kernels' own packed 16-bit operands: the width / size / operand-type grid, r = 31, the
forward variants (running maximum, norm bound declined, sampled shift and its fallback pass, a maximum that rises along
the keys), the forward into a slab, the three backward forms, the shared output buffer of ops._pam_backward, the batch
slicing of gd_pam_flash_bwd, and the argument errors."""
import functools

import pytest
import torch

from gpu_util import DEV, rell2, relmax, seeded
from pam_util import reference
from test_gpu_pam_wide import _KERNEL_TOL

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
GAMMA = 0.7
NAN = float("nan")


@pytest.fixture(scope="module")
def gd():
    import gan_danet_amd as g
    from gan_danet_amd import _lib
    _lib.load()
    return g


def _per_image(shape, seed, scale=1.0):
    """one seed per image: no two images share a value, so a wrong batch offset cannot cancel"""
    return torch.cat([seeded((1, *shape[1:]), seed + 1000 * b, scale) for b in range(shape[0])])


def _inputs(C, N, r, B, seed, qk_scale, kind):
    q, k = _per_image((B, r, N), seed, qk_scale), _per_image((B, r, N), seed + 1, qk_scale)
    if kind == "large":
        # logits of +-60 log2 units and more, and (image 1, query 300 against key 304: 400 * log2 e = 577 units) one
        # key that a strided sample of 128 keys misses at N = 480 (stride 3) and N = 990 (stride 7)
        q[1, 0, :] = 0.0
        q[1, 0, 300] = 10.0
        k[1, 0, 304] = 40.0
    elif kind == "rising":
        # the construction of test_pam_online_softmax_rescale_branch -- the last pixel carries q and k six times as
        # large, so its key wins in the last tile -- on keys whose norm grows along the stream, so that every key tile
        # raises the running maximum of most queries
        k[:, :, :N - 1] *= torch.linspace(1.0, 2.0, N - 1)
        q[:, :, N - 1] *= 6.0
        k[:, :, N - 1] *= 6.0
    v, x, do = _per_image((B, C, N), seed + 2), _per_image((B, C, N), seed + 3), _per_image((B, C, N), seed + 4)
    return q, k, v, x, do


def _packed_problem(C, N, f16, seed, B=2, qk_scale=0.6, r=None, kind="plain"):
    """q, k, v, x, dOut packed as ops._pam_pack16 / ops._pam_backward pack them for the narrow route (32 q / k slots, 1.0
    in k's slot 31, V's ones row in channel Cp - 1 when C < Cp, q pre-scaled by log2 e); returns the device packs and
    their fp64 CPU images"""
    from gan_danet_amd import kern as K
    r = C // 8 if r is None else r
    Np, Cp, D = (N + 255) // 256 * 256, (C + 31) // 32 * 32, 32
    ones = Cp - 1 if C < Cp else -1
    q, k, v, x, do = (t.to(DEV) for t in _inputs(C, N, r, B, seed, qk_scale, kind))
    _, qt = K.pack_bf16(q, r, N, scale_imm=K.LOG2E, t_shape=(Np, D), f16=f16)
    kn, kt = K.pack_bf16(k, r, N, plain_shape=(D, Np), t_shape=(Np, D), perm16=True, ones_row=D - 1, f16=f16)
    vn, vt = K.pack_bf16(v, C, N, plain_shape=(Cp, Np), t_shape=(Np, Cp), perm16=True, ones_row=ones, f16=f16)
    _, dot_ = K.pack_bf16(do, C, N, t_shape=(Np, Cp), f16=f16)
    assert (kt[:, :, D - 1] == 1).all() and (ones < 0 or (vt[:, :, Cp - 1] == 1).all())
    dev = dict(qt=qt, kt=kt, kn=kn, vn=vn, vt=vt, dot=dot_, x=x, gamma=torch.tensor([GAMMA], device=DEV), B=B, N=N, Np=Np,
               C=C, Cp=Cp, r=r, ones=ones, f16=f16, kind=kind)
    cpu = dict(q=qt[:, :N, :r].double().cpu() / LOG2E,      # the operands exactly as the MFMAs see them
               k=kt[:, :N, :r].double().cpu(), v=vt[:, :N, :C].double().cpu(), do=dot_[:, :N, :C].double().cpu())
    return dev, cpu


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _forward(p, mode="bound", out=None, x=None):
    """mode "bound": as ops._pam_forward runs it (k_sqmax from pam_key_sqnorm_max); "runmax": without k_sqmax;
    "shift": gd_pam_flash_fwd_shift with 128 sample keys"""
    from gan_danet_amd import kern as K
    B, N, Np, C, Cp, r, f16 = p["B"], p["N"], p["Np"], p["C"], p["Cp"], p["r"], p["f16"]
    x = p["x"] if x is None else x
    out = _nan(B, C, N) if out is None else out
    o_attn, lse, flags = _nan(B, C, N), _nan(B, N), None
    if mode == "shift":
        flags = K.pam_flash_fwd_shift(p["qt"], p["kt"], p["vn"], B, N, Np, C, Cp, p["gamma"], x, out, o_attn, lse, r_alg=r,
                                      v_ones=p["ones"] >= 0, nsample=128, return_flags=True).cpu().view(B, -1)
    else:
        ksq = K.pam_key_sqnorm_max(p["kt"], N, f16) if mode == "bound" else None
        K.pam_flash_fwd(p["qt"], p["kt"], p["vn"], B, N, Np, C, Cp, p["gamma"], x, out, o_attn, lse, r_alg=r,
                        v_ones=p["ones"] >= 0, f16=f16, k_sqmax=ksq)
    torch.cuda.synchronize()
    return dict(out=out, o=o_attn, lse=lse, flags=flags)


def _backward(p, fwd, form=0, shared=False):
    """gd_pam_flash_bwd into NaN-filled outputs; shared: dq | dk | dv as the row blocks [0:32 | 32:64 | 64:64+Cp] of one
    (B, 64 + Cp, Np) buffer, as ops._pam_backward hands them over when Np == N"""
    from gan_danet_amd import kern as K
    B, N, Np, C, Cp, r = p["B"], p["N"], p["Np"], p["C"], p["Cp"], p["r"]
    # delta = rowsum(dO . O) on the packed dO, as chan_dot forms it from gamma * dOut in the product
    delta = (p["dot"][:, :N, :C].float().transpose(1, 2) * fwd["o"]).sum(1).contiguous()
    buf, out_bs = None, 0
    if shared:
        buf, out_bs = _nan(B, 64 + Cp, Np), (64 + Cp) * Np
        dqn, dkn, dv = buf[:, 0:32], buf[:, 32:64], buf[:, 64:]
    else:
        dqn, dkn, dv = _nan(B, 32, Np), _nan(B, 32, Np), _nan(B, Cp, Np)
    K.pam_flash_bwd(p["qt"], p["kt"], p["kn"], p["vt"], p["dot"], fwd["lse"], delta, B, N, Np, Cp, dqn, dkn, dv, r_alg=r,
                    c_alg=C, f16=p["f16"], form=form, out_bs=out_bs)
    torch.cuda.synchronize()
    return dict(dq=dqn[:, :r, :N], dk=dkn[:, :r, :N], dv=dv[:, :C, :N], buf=buf)


@functools.lru_cache(maxsize=8)
def _solved(C, N, f16, B=2, qk_scale=0.6, r=None, kind="plain"):
    """one problem, its fp64 reference and the forward as ops._pam_forward runs it -- computed once, shared by the tests
    that use the same problem, and never modified"""
    p, cpu = _packed_problem(C, N, f16, seed=100 + C + N, B=B, qk_scale=qk_scale, r=r, kind=kind)
    return p, reference(cpu, p["x"], GAMMA), _forward(p)


# Bounds: _KERNEL_TOL of test_gpu_pam_wide.py as it stands (the narrow kernels do the wide kernels' arithmetic on the
# same operand types at the same N).
# measured worst case over everything below (bf16 / fp16): out 1.1e-3 / 1.2e-4, o 3.1e-3 / 3.7e-4 relmax, lse (widths
# without a ones row) 1.5e-7 / 1.2e-7 relmax, dq 2.4e-3 / 2.9e-4, dk 2.3e-3 / 2.5e-4, dv 2.0e-3 / 2.3e-4 rel-L2 (the
# backward's worst cases are at N = 35; from N = 256 up they are the wide file's 2.1e-3 / 2.7e-4 and below)
#
# lse where V carries the ones row (C < Cp: 8, 176, 184): the forward takes the softmax denominator from the P . V
# MFMAs (row Cp - 1 of V^T is ones), i.e. it sums the probabilities AFTER their rounding to the operand type, so that
# O = sum(P~ v) / sum(P~) is an exact weighted mean; lse = m + log2(sum P~) then carries the mean rounding error of the
# row (at most 2^-8 absolute in bf16, 2^-11 in fp16; far less when many keys share the weight).  The widths without
# a spare channel (64, 160, 192) sum the fp32 probabilities on the VALU, as the wide kernels do, and meet the wide bound.
# Measured with a ones row (relmax, i.e. relative to the largest |lse| of the problem; bf16 / fp16), bounds 2.5x:
#   logits of a few units, N = 35 (one partial key tile: few keys share the weight)   3.11e-4 / 2.90e-5
#   the same, N = 256 / 480 / 990 (grid, running maximum, sampled shift, slab)        1.92e-4 / 1.68e-5
#   rising maximum (|lse| up to ~50)                                                  3.76e-5 / 4.41e-6
#   large logits (|lse| up to ~400), bound declined = running maximum / shift + redo  1.05e-5 / -
_LSE_ONES_TOL = {"small": {False: 7.8e-4, True: 7.3e-5}, "plain": {False: 4.8e-4, True: 4.2e-5},
                 "rising": {False: 9.4e-5, True: 1.1e-5}, "large": {False: 2.6e-5}}
# dQ of the parts forms against fp64: the rounding of every 256-key block's dQ part to bf16 (also with fp16 operands) on
# top of the grid's error.  Measured rel-L2 (form 1 bf16 / form 1 fp16): 2.79e-3 / 1.77e-3;
# bounds 2.5x, below the 1e-2 that test_pam_flash_backward_forms_agree_at_bench_and_max_size allows between the forms
_DQ_PARTS_TOL = {(1, False): 7.0e-3, (1, True): 4.4e-3}


def _tol(p):
    tol = dict(_KERNEL_TOL[p["f16"]])
    if p["ones"] >= 0:
        tol["lse"] = _LSE_ONES_TOL["small" if p["kind"] == "plain" and p["N"] < 64 else p["kind"]][p["f16"]]
    return tol


def _check_forward(what, p, got, ref, tol=None):
    tol = tol or _tol(p)
    errs = {n: relmax(got[n], ref[n]) for n in ("out", "o", "lse")}
    print(f"pam_narrow {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["out"] <= tol["out"] and errs["o"] <= tol["out"], errs
    assert errs["lse"] <= tol["lse"], errs
    return errs


def _check_backward(what, p, got, ref, names=("dq", "dk", "dv"), tol=None):
    tol = tol or _tol(p)
    errs = {n: rell2(got[n], ref[n]) for n in names}
    print(f"pam_narrow {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for n in names:
        assert errs[n] <= tol[n], (n, errs)
    return errs


def _name(p):
    return f"C={p['C']} r={p['r']} N={p['N']} B={p['B']} {'fp16' if p['f16'] else 'bf16'}"


def _check_key_sqnorm_max(p):
    """gd_pam_key_sqnorm_max against fp64 on the packed keys: slot 31 (the ones slot) excluded, padded keys ignored (they
    are given a huge norm here)"""
    from gan_danet_amd import kern as K
    kt = p["kt"].clone()
    kt[:, p["N"]:, :31] = 100.0
    got = K.pam_key_sqnorm_max(kt, p["N"], p["f16"])
    want = (p["kt"][:, :p["N"], :31].double() ** 2).sum(-1).max(-1).values
    err = ((got.double() - want).abs() / want).max().item()
    assert err <= 1e-6, (err, got.tolist(), want.tolist())


# ---- (a) the main grid, (b) r = 31 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hw", [(5, 7), (24, 20), (45, 22), (16, 16)], ids=["5x7", "24x20", "45x22", "16x16"])
@pytest.mark.parametrize("c", [8, 64, 160, 176, 184, 192])
def test_pam_narrow_kernels_vs_fp64(gd, c, hw, f16):
    """forward (as ops._pam_forward runs it) and the default backward (form 0, K64 with fp32 atomics) against fp64,
    r = C // 8.  C: Cp = 32 with r = 1; Cp == C without a ones row (64, 160, 192); the generator's 176 / 184, which pad
    to 192.  N = 35: one partial 64-key tile, Np = 256; 480: Np = 512; 990: 15 full key tiles + 30 keys; 256: N == Np."""
    p, ref, fwd = _solved(c, hw[0] * hw[1], f16)
    assert p["r"] == c // 8
    _check_key_sqnorm_max(p)
    _check_forward(_name(p), p, fwd, ref)
    _check_backward(_name(p), p, _backward(p, fwd), ref)


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
def test_pam_narrow_kernels_vs_fp64_r31(gd, f16):
    """r = 31 with C = 192: every q / k slot but the ones slot is live"""
    p, ref, fwd = _solved(192, 480, f16, r=31)
    assert p["r"] == 31
    _check_key_sqnorm_max(p)
    _check_forward(_name(p), p, fwd, ref)
    _check_backward(_name(p), p, _backward(p, fwd), ref)


# ---- (c) forward variants ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", [480, 990])
def test_pam_narrow_forward_running_maximum_vs_fp64(gd, n, f16):
    """gd_pam_flash_fwd without k_sqmax: the running-maximum sweep"""
    p, ref, fwd = _solved(184, n, f16)
    got = _forward(p, "runmax")
    _check_forward(_name(p) + " running maximum", p, got, ref)
    if not f16:       # bf16: these logits are inside the norm bound, so the grid above went through the max-free sweep
        assert not torch.equal(got["o"], fwd["o"]), "the max-free sweep was not taken where the norm bound holds"


@pytest.mark.parametrize("n", [480, 990])
def test_pam_narrow_forward_sampled_shift_vs_fp64(gd, n):
    p, ref, _ = _solved(184, n, False)
    got = _forward(p, "shift")
    _check_forward(_name(p) + " sampled shift", p, got, ref)
    assert not got["flags"].any(), got["flags"].tolist()


@pytest.mark.parametrize("n", [480, 990])
def test_pam_narrow_forward_large_logits_vs_fp64(gd, n):
    """qk_scale = 3.0 (logits of +-60 log2 units and more) plus one key outside the shift's sample that beats one
    query's sampled maximum by hundreds of units: the bound-based max-free path must be declined (bitwise the
    running-maximum sweep), the shift variant must flag that query's workgroup and redo it -- all against fp64.  (At
    this scale some row of every other workgroup leaves the fp32 range of the max-free sweep as well, so they are
    redone too; test_pam_narrow_forward_sampled_shift_vs_fp64 is the sweep without any redo.)"""
    p, ref, fwd = _solved(184, n, False, qk_scale=3.0, kind="large")
    _check_forward(_name(p) + " large logits, norm bound", p, fwd, ref)
    run = _forward(p, "runmax")
    for name in ("out", "o", "lse"):
        assert torch.equal(fwd[name], run[name]), f"{name}: the max-free sweep was taken beyond its norm bound"
    got = _forward(p, "shift")
    print(f"pam_narrow {_name(p)} large logits: redo flags {got['flags'].tolist()}")
    assert got["flags"][1, 300 // 256] == 1, got["flags"].tolist()
    _check_forward(_name(p) + " large logits, sampled shift", p, got, ref)


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", [480, 990])
def test_pam_narrow_forward_rising_maximum_vs_fp64(gd, n, f16):
    """a row maximum that rises from key tile to key tile and is set by the LAST key: the online-softmax rescale branch
    in every tile, with the running maximum and through ops._pam_forward's call"""
    p, ref, fwd = _solved(184, n, f16, kind="rising")
    _check_forward(_name(p) + " rising maximum", p, fwd, ref)
    _check_forward(_name(p) + " rising maximum, running maximum", p, _forward(p, "runmax"), ref)


# ---- (d) forward into a slab -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", [184, 64])
def test_pam_narrow_forward_into_a_slab(gd, c, f16):
    """out = the first C channels of a (B, 2C, N) buffer, x = a channel slice of a wider one: DualAttentionFn's batch
    strides.  The other half of the output buffer stays untouched."""
    p, ref, fwd = _solved(c, 480, f16)
    B, N = p["B"], p["N"]
    feats = _nan(B, 2 * c, N)
    xw = _nan(B, c + 5, N)
    xw[:, 3:3 + c] = p["x"]
    got = _forward(p, out=feats[:, :c], x=xw[:, 3:3 + c])
    _check_forward(_name(p) + " slab", p, got, ref)
    assert torch.equal(got["out"], fwd["out"]) and torch.equal(got["o"], fwd["o"])
    assert torch.isnan(feats[:, c:]).all(), "the forward wrote outside its half of the slab"


# ---- (e) the three backward forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", [480, 256])
def test_pam_narrow_backward_forms_vs_fp64(gd, n, f16):
    """0 K64 atomic, 1 K64 parts, 3 two-kernel (fp16: 0 and 1), each against fp64: dK and dV of every form and dQ of
    forms 0 and 3 at the bounds of the grid, dQ of the parts form with its bf16 rounding; the parts form is bitwise
    reproducible"""
    p, ref, fwd = _solved(184, n, f16)
    for form in (0, 1) if f16 else (0, 1, 3):
        got = _backward(p, fwd, form)
        what = f"{_name(p)} form {form}"
        _check_backward(what, p, got, ref, ("dk", "dv"))
        if form in (0, 3):
            _check_backward(what, p, got, ref, ("dq",))
        else:
            _check_backward(what + " (parts)", p, got, ref, ("dq",), {"dq": _DQ_PARTS_TOL[form, f16]})
            again = _backward(p, fwd, form)
            for name in ("dq", "dk", "dv"):
                assert torch.equal(got[name], again[name]), f"form {form} {name}: not bitwise reproducible"


# ---- (f) shared output buffer ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", [184, 64])
def test_pam_narrow_backward_shared_output_buffer(gd, c, f16):
    """form 0 with out_bs: dq | dk | dv as row blocks of one (B, 64 + Cp, Np) buffer, N = Np.  ops._pam_backward
    multiplies the rows r..31 and C..Cp-1 of that buffer by zero weights, so ALL of it must be finite."""
    p, ref, fwd = _solved(c, 256, f16)
    assert p["N"] == p["Np"]
    sep = _backward(p, fwd)
    got = _backward(p, fwd, shared=True)
    assert torch.equal(got["dk"], sep["dk"]) and torch.equal(got["dv"], sep["dv"])
    _check_backward(_name(p) + " shared buffer", p, got, ref, ("dq",))
    assert torch.isfinite(got["buf"]).all(), "rows the kernel left undefined would poison dx and the weight gradients"


# ---- (g) batch slicing -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
def test_pam_narrow_backward_batch_slicing(gd, monkeypatch, form):
    """scratch for ONE image: gd_pam_flash_bwd walks B = 3 one image at a time (b0 offsets into the packs, lse, delta
    and the outputs)"""
    from gan_danet_amd import kern as K
    p, ref, fwd = _solved(184, 480, False, B=3)
    whole = _backward(p, fwd, form)
    per_image = int(K.lib().gd_pam_bwd_scratch_bytes(p["Np"], form))
    assert per_image > 0
    monkeypatch.setattr(K, "PAM_SCRATCH_CAP", per_image)
    got = _backward(p, fwd, form)
    assert torch.equal(got["dk"], whole["dk"]) and torch.equal(got["dv"], whole["dv"])
    if form == 1:
        assert torch.equal(got["dq"], whole["dq"])
        _check_backward(f"{_name(p)} sliced, form 1 (parts)", p, got, ref, ("dq",), {"dq": _DQ_PARTS_TOL[1, False]})
        _check_backward(f"{_name(p)} sliced, form 1", p, got, ref, ("dk", "dv"))
    else:
        _check_backward(f"{_name(p)} sliced, form 0", p, got, ref)


# ---- (h) argument errors -----------------------------------------------------------------------------------------------
def test_pam_narrow_argument_errors(gd):
    from gan_danet_amd import _lib as L
    lib = L.load()
    x = torch.zeros(1, device=DEV)
    ptr = x.data_ptr()

    def bwd(Npad=256, Cp=192, f16=0, form=0, out_bs=0):
        return lib.gd_pam_flash_bwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1, 16, Npad, Cp, f16, form, ptr, ptr, ptr, out_bs, ptr,
                                    1 << 30, None)

    def fwd(C=184, Cp=192, v_ones=1):
        return lib.gd_pam_flash_fwd(ptr, ptr, ptr, 1, 16, 256, C, Cp, v_ones, 0, ptr, ptr, 0, ptr, 0, ptr, ptr, None, None)

    assert bwd(form=1, out_bs=(64 + 192) * 256) == -1
    assert "form 0" in L.last_error()
    assert bwd(f16=1, form=3) == -1
    assert "fp16" in L.last_error()
    assert bwd(form=2) == -1
    assert "form" in L.last_error()
    assert lib.gd_pam_bwd_scratch_bytes(256, 2) == 0
    assert bwd(Cp=224) == -1
    assert "Cp" in L.last_error()
    assert bwd(Npad=300) == -1
    assert "Npad" in L.last_error()
    assert fwd(C=192, Cp=192, v_ones=1) == -1
    assert "v_ones" in L.last_error()
    assert fwd(C=200, Cp=224, v_ones=1) == -1
    assert "Cp" in L.last_error()
