"""Wide flash PAM (gd_pam_wide_*) against the narrow kernels, kernel level, HIP-event times (median of repeats after
warm-up).  (The module-level A/B against the product chain is recorded in DESIGN.md section 5.4; the chain no longer serves
these widths.)
    python tools/pam_wide_bench.py --out profiles/r04_pam_wide.json
Work per image: 2 N^2 (r + C) forward, twice that backward; share of the 2.5 PF dense 16-bit peak."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import kern as K, ops  # noqa: E402

PEAK = 2.5e15

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--tile", type=int, default=256)
ap.add_argument("--channels", default="184,224,256,352")
ap.add_argument("--precisions", default="bf16,fp16")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def problem(B, C, N, f16):
    """packed operands as ops._pam_forward makes them for the route C selects (narrow: C <= 192)"""
    r = C // 8
    Np, Cp = (N + 255) // 256 * 256, (C + 31) // 32 * 32
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B, r, N, device=dev, generator=g) * 0.5
    k = torch.randn(B, r, N, device=dev, generator=g) * 0.5
    v = torch.randn(B, C, N, device=dev, generator=g)
    x = torch.randn(B, C, N, device=dev, generator=g)
    do = torch.randn(B, C, N, device=dev, generator=g)
    wide = C > 192
    D = K.pam_wide_slots(r) if wide else 32
    ones = -1 if wide or C == Cp else Cp - 1
    qt, kt, kn, vn, vt = ops._pam_pack16(q, k, v, r, C, N, D, ones, f16)
    _, dot_ = K.pack_bf16(do, C, N, t_shape=(Np, Cp), f16=f16)
    gamma = torch.tensor([0.7], device=dev)
    out, o_attn = torch.empty_like(x), torch.empty_like(x)
    lse = torch.empty(B, N, device=dev)
    delta = torch.randn(B, N, device=dev, generator=g) * 0.01
    dqn, dkn = torch.empty(B, D, Np, device=dev), torch.empty(B, D, Np, device=dev)
    dv = torch.empty(B, Cp, Np, device=dev)

    if wide:
        def fwd():
            K.pam_wide_fwd(qt, kt, vn, B, N, Np, C, Cp, D, gamma, x, out, o_attn, lse, r_alg=r, f16=f16)

        def bwd():
            K.pam_wide_bwd(qt, kt, kn, vt, dot_, lse, delta, B, N, Np, Cp, D, dqn, dkn, dv, r_alg=r, c_alg=C, f16=f16)
    else:
        def fwd():
            k_sqmax = K.pam_key_sqnorm_max(kt, N, f16)
            K.pam_flash_fwd(qt, kt, vn, B, N, Np, C, Cp, gamma, x, out, o_attn, lse, r_alg=r, v_ones=ones >= 0, f16=f16,
                            k_sqmax=k_sqmax)

        def bwd():
            K.pam_flash_bwd(qt, kt, kn, vt, dot_, lse, delta, B, N, Np, Cp, dqn, dkn, dv, r_alg=r, c_alg=C, f16=f16)
    return r, fwd, bwd


rows = []
N = a.tile * a.tile
for prec in a.precisions.split(","):
    for C in (int(c) for c in a.channels.split(",")):
        r, fwd, bwd = problem(a.batch, C, N, prec == "fp16")
        fwd()                                          # the backward reads the forward's LSE
        tf, tb = timed(fwd, a.reps, a.warmup), timed(bwd, a.reps, a.warmup)
        tfb = timed(lambda: (fwd(), bwd()), a.reps, a.warmup)
        work = 2.0 * N * N * (r + C) * a.batch
        row = dict(prec=prec, C=C, r=r, N=N, B=a.batch, route="wide" if C > 192 else "narrow",
                   fwd_ms=round(tf, 3), bwd_ms=round(tb, 3), fwdbwd_ms=round(tfb, 3),
                   fwd_tflops=round(work / tf * 1e-9, 1), bwd_tflops=round(2 * work / tb * 1e-9, 1),
                   fwdbwd_tflops=round(3 * work / tfb * 1e-9, 1),
                   fwdbwd_peak_share=round(3 * work / (tfb * 1e-3) / PEAK, 3))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del fwd, bwd
        torch.cuda.empty_cache()

if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), peak_flops=PEAK, rows=rows), f, indent=1)
