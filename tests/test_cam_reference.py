"""The float64 references of tests/cam_util.py (CAM, the PAM product chain) against float64 autograd through the literal
reference formulas, the conditioning of the CAM inputs, and the fp32 emulation margins, all on the CPU: the evidence that
what tests/test_gpu_cam.py compares the kernels with is right, that its inputs exercise the softmax, and that its
bounds leave an exact-fp32 kernel room."""
import pytest
import torch

import cam_util as CU
from gpu_util import bf16_round, seeded

TOL = 1e-12
GAMMA = 2.0
FP32_TOL = 2e-5       # tests/test_gpu_kernels.py: the exact-fp32 kernels
X3_TOL = 1e-4         # test_conv2d_generic_split_bf16_vs_fp64; also bf16 MFMAs on operands already rounded to bf16
MARGIN = 10.0         # the CPU's fp32 run of the same formulas must be this far inside each GPU bound


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _cam_problem(shape):
    B, C, H, W = shape
    return CU.cam_inputs(B, C, H, W, CU.CAM_SEED), seeded((B, C, H * W), CU.CAM_DOUT_SEED)


@pytest.mark.parametrize("shape", [(2, 40, 5, 7), (2, 33, 8, 12), (1, 72, 24, 20)])
def test_cam_reference_matches_autograd(shape):
    """y = gamma softmax(max(E) - E) X + X as the reference module writes it; the gradients that reach att and E are
    taken from autograd too (over gamma, as the kernels form them)"""
    x, dout = (t.double() for t in _cam_problem(shape))
    ref = CU.cam_reference(x, GAMMA, dout)
    xr, g = x.clone().requires_grad_(True), torch.tensor(GAMMA, dtype=torch.float64, requires_grad=True)
    e = xr @ xr.transpose(1, 2)
    att = torch.softmax(e.max(-1, keepdim=True).values.expand_as(e) - e, -1)
    apply = att @ xr
    y = g * apply + xr
    e.retain_grad(), att.retain_grad()
    y.backward(dout)
    errs = {"e": _rel(ref["e"], e.detach()), "att": _rel(ref["att"], att.detach()),
            "apply": _rel(ref["apply"], apply.detach()), "y": _rel(ref["y"], y.detach()),
            "da": _rel(GAMMA * ref["da"], att.grad), "de": _rel(GAMMA * ref["de"], e.grad),
            "dgamma": abs(ref["dgamma"].item() - g.grad.item()) / ref["dgamma_abs"].item(),
            "dx": _rel(ref["dx"], xr.grad),
            "dx terms": _rel(dout + GAMMA * (ref["dx_att"] + ref["dx_sym"]), xr.grad),
            "sym": _rel(ref["sym"], ref["de"] + ref["de"].transpose(1, 2))}
    for name, err in errs.items():
        assert err <= TOL, f"{name}: rel err {err:.3e} > {TOL:.0e}"
    assert (ref["sym"] - ref["sym"].transpose(1, 2)).abs().max().item() == 0.0


@pytest.mark.parametrize("shape", [(2, 4, 40, 35), (1, 23, 184, 480)])
def test_pam_chain_reference_matches_autograd(shape):
    """the bmm chain of the reference module on the channel-major projections"""
    B, r, C, N = shape
    q, k, v, x, dout = (t.double() for t in CU.chain_inputs(B, r, C, N, 11))
    ref = CU.pam_chain_reference(q, k, v, x, GAMMA, dout)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    g = torch.tensor(GAMMA, dtype=torch.float64, requires_grad=True)
    p = torch.softmax(torch.bmm(qr.transpose(1, 2), kr), -1)
    o = torch.bmm(vr, p.transpose(1, 2))
    out = g * o + x
    out.backward(dout)
    errs = {"p": _rel(ref["p"], p.detach()), "o_attn": _rel(ref["o_attn"], o.detach()), "out": _rel(ref["out"], out.detach()),
            "dq": _rel(ref["dq"], qr.grad), "dk": _rel(ref["dk"], kr.grad), "dv": _rel(ref["dv"], vr.grad),
            "dgamma": abs(ref["dgamma"].item() - g.grad.item()) / ref["dgamma_abs"].item()}
    for name, err in errs.items():
        assert err <= TOL, f"{name}: rel err {err:.3e} > {TOL:.0e}"
    assert ref["dq"].shape == (B, r, N) and ref["dk"].shape == (B, r, N) and ref["dv"].shape == (B, C, N)


@pytest.mark.parametrize("shape", CU.CAM_SHAPES)
def test_cam_inputs_are_well_conditioned(shape):
    """conditions on the inputs of the GPU tests, not measurements: no attention weight above 0.7 and no row whose
    effective support exp(entropy) is below 0.15 C, so that a wrong Gram entry, softmax-backward term or operand
    orientation moves the outputs.  (If a later seed breaks a cap, change the seed, not the cap.)
    measured (CAM_SEED = 1): largest weight 0.545, smallest exp(entropy) / C 0.225 over the seven shapes"""
    x, dout = _cam_problem(shape)
    amax, support = CU.conditioning(CU.cam_reference(x, GAMMA, dout)["att"])
    print(f"cam conditioning {shape}: max weight {amax:.3f}, min exp(entropy)/C {support:.3f}")
    assert amax <= 0.7, amax
    assert support >= 0.15, support


@pytest.mark.parametrize("shape", CU.CAM_SHAPES)
def test_cam_fp32_emulation_is_well_inside_the_gpu_bounds(shape):
    """the same closed forms in torch float32 on the CPU against float64: what fp32 arithmetic costs at these shapes,
    10x inside FP32_TOL for the always-fp32 part (att, dgamma) and the exact-fp32 products; and the two apply products
    in fp32 on bf16-rounded operands against fp64 on the same rounded operands, 10x inside the 1e-4 of the bf16 mode.
    measured (worst over the seven shapes): att 1.30e-6, apply 1.38e-6, dx_att + dx_sym 1.65e-6 relmax (12x inside; the
    rounding of rowmax(E) - E ~ sqrt(N) to float32 is most of it), dgamma 3.9e-8 of the sum of |terms|; on bf16-rounded
    operands apply 3.8e-7, att^T dOut 4.4e-7"""
    x, dout = _cam_problem(shape)
    ref = CU.cam_reference(x, GAMMA, dout)
    emu = CU.cam_reference(x, GAMMA, dout, dtype=torch.float32)
    errs = {"att": _rel(emu["att"].double(), ref["att"]), "apply": _rel(emu["apply"].double(), ref["apply"]),
            "dx": _rel((emu["dx_att"] + emu["dx_sym"]).double(), ref["dx_att"] + ref["dx_sym"]),
            "dgamma": abs(emu["dgamma"].item() - ref["dgamma"].item()) / ref["dgamma_abs"].item()}
    print(f"cam fp32 emulation {shape}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, err in errs.items():
        assert err * MARGIN <= FP32_TOL, f"{name}: {err:.3e} is not {MARGIN:.0f}x inside {FP32_TOL:.0e}"
    att_b, x_b, d_b = bf16_round(ref["att"].float()), bf16_round(x), bf16_round(dout)
    errs = {"apply": _rel((att_b @ x_b).double(), att_b.double() @ x_b.double()),
            "dx_att": _rel((att_b.transpose(1, 2) @ d_b).double(), att_b.double().transpose(1, 2) @ d_b.double())}
    print(f"cam fp32 emulation on bf16-rounded operands {shape}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, err in errs.items():
        assert err * MARGIN <= X3_TOL, f"{name} (bf16-rounded operands): {err:.3e} is not {MARGIN:.0f}x inside {X3_TOL:.0e}"


@pytest.mark.parametrize("shape", CU.GEMM_SHAPES)
def test_batched_gemm_fp32_emulation_is_well_inside_the_gpu_bounds(shape):
    """every product of test_batched_strided_conv_nn_vs_fp64 as a float32 matmul on the CPU against float64: on plain
    operands 10x inside FP32_TOL (and with that inside the 1e-4 of the split-bf16 mode), on bf16-rounded operands (exact
    products, fp32 accumulation: what is left of the bf16 mode) 10x inside 1e-4; plain and with alpha, residual and a
    prefilled output.
    measured (worst over the five shapes): plain operands 6.8e-7, bf16-rounded 3.0e-7"""
    M, Ck, P = shape
    t = CU.gemm_inputs(M, Ck, P, 40 + M)
    alpha = 0.37
    for name, rnd, bound in (("plain", lambda v: v, FP32_TOL), ("bf16-rounded", bf16_round, X3_TOL)):
        a, x = rnd(t["a"]), rnd(t["x"])
        ref = CU.gemm_reference(a, x)
        emu = CU.gemm_reference(a, x, dtype=torch.float32)
        err = _rel(emu.double(), ref)
        full = _rel((t["y0"] + (alpha * emu + t["res"])).double(), t["y0"].double() + alpha * ref + t["res"].double())
        print(f"gemm fp32 emulation {shape} {name}: product {err:.2e}, with alpha + res + accumulate {full:.2e}")
        assert max(err, full) * MARGIN <= bound, f"{name}: {max(err, full):.3e} is not {MARGIN:.0f}x inside {bound:.0e}"


@pytest.mark.parametrize("shape", CU.CHAIN_SHAPES)
def test_pam_chain_fp32_emulation_is_well_inside_the_gpu_bounds(shape):
    """the product chain in float32 on the CPU against float64, 10x inside FP32_TOL
    measured (worst over the three shapes): p 1.5e-7, o_attn 6.0e-7, dq 5.3e-7, dk 5.2e-7, dv 6.5e-7 relmax"""
    B, r, C, N = shape
    t = CU.chain_inputs(B, r, C, N, 300 + N)
    ref = CU.pam_chain_reference(*t[:4], GAMMA, t[4])
    emu = CU.pam_chain_reference(*t[:4], GAMMA, t[4], dtype=torch.float32)
    errs = {n: _rel(emu[n].double(), ref[n]) for n in ("p", "o_attn", "dq", "dk", "dv")}
    errs["dgamma"] = abs(emu["dgamma"].item() - ref["dgamma"].item()) / ref["dgamma_abs"].item()
    print(f"pam chain fp32 emulation {shape}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, err in errs.items():
        assert err * MARGIN <= FP32_TOL, f"{name}: {err:.3e} is not {MARGIN:.0f}x inside {FP32_TOL:.0e}"
