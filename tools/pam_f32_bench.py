"""Fused flash PAM on exact fp32 operands (gd_pam_f32_*), kernel level, HIP-event times (median of repeats after warm-up),
plus the product chain on the same projections at a size it can hold.
    python tools/pam_f32_bench.py --out profiles/r05_pam_f32_bench.txt
Work per image: 2 N^2 (r + C) forward, twice that backward; share of the 155 TF measured rate of
v_mfma_f32_32x32x2_f32."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gan_danet_amd import _lib as L  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402
from gan_danet_amd import ops  # noqa: E402

PEAK = 155e12

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--tile", type=int, default=256)
ap.add_argument("--channels", default="160,176,184,256")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--ab-tile", type=int, default=128, help="0: skip the product-chain comparison")
ap.add_argument("--ab-channels", type=int, default=184)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda")
lines = []


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    lines.append(line)


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


def problem(B, C, N):
    r = C // 8
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B, r, N, device=dev, generator=g) * 0.5
    k = torch.randn(B, r, N, device=dev, generator=g) * 0.5
    v, x, do = (torch.randn(B, C, N, device=dev, generator=g) for _ in range(3))
    return r, q, k, v, x, do


def fused_fns(B, C, N, r, q, k, v, x, do):
    assert N % 256 == 0
    gamma = torch.tensor([0.7], device=dev)
    out, o = torch.empty_like(x), torch.empty_like(x)
    lse = torch.empty(B, N, device=dev)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    state = {}

    def fwd():
        K.pam_f32_fwd(q, k, v, B, N, N, C, r, gamma, x, out, o, lse)

    def bwd():
        if "delta" not in state:
            state["delta"] = K.chan_dot(do, o, gamma)[1]
        K.pam_f32_bwd(q, k, v, do, lse, state["delta"], B, N, N, C, r, dq, dk, dv)
    return fwd, bwd


def row_for(name, B, C, N, r, fwd, bwd):
    fwd()                                          # the backward reads the forward's LSE
    tf, tb = timed(fwd, a.reps, a.warmup), timed(bwd, a.reps, a.warmup)
    work = 2.0 * N * N * (r + C) * B
    return dict(route=name, C=C, r=r, N=N, B=B, fwd_ms=round(tf, 2), bwd_ms=round(tb, 2),
                fwd_tflops=round(work / tf * 1e-9, 1), bwd_tflops=round(2 * work / tb * 1e-9, 1),
                fwd_peak_share=round(work / (tf * 1e-3) / PEAK, 3), bwd_peak_share=round(2 * work / (tb * 1e-3) / PEAK, 3))


emit(dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK * 1e-12, reps=a.reps))
N = a.tile * a.tile
for C in (int(c) for c in a.channels.split(",")):
    r, q, k, v, x, do = problem(a.batch, C, N)
    emit(row_for("fused_f32", a.batch, C, N, r, *fused_fns(a.batch, C, N, r, q, k, v, x, do)))
    del q, k, v, x, do
    torch.cuda.empty_cache()

if a.ab_tile:
    C, N, B = a.ab_channels, a.ab_tile * a.ab_tile, a.batch
    r, q, k, v, x, do = problem(B, C, N)
    emit(row_for("fused_f32", B, C, N, r, *fused_fns(B, C, N, r, q, k, v, x, do)))
    gamma = torch.tensor([0.7], device=dev)
    out = torch.empty_like(x)
    state = {}

    def chain_fwd():
        state["saved"] = None                      # one set of N x N matrices at a time
        state["saved"] = ops._pam_chain_fwd(q, k, v, x, gamma, out, L.PREC_FP32)

    def chain_bwd():
        ops._pam_chain_bwd(state["saved"], gamma, do, L.PREC_FP32)
    emit(row_for("chain", B, C, N, r, chain_fwd, chain_bwd))

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
