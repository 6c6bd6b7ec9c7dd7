"""Split reductions in three modes -- default (fp32 atomics), deterministic unsplit, deterministic ordered (partial slabs +
ordered sum) -- timed in one process with HIP events, the modes alternated launch by launch, medians reported.

    python tools/det_reduce_bench.py [--batch 32] [--tile 256] [--reps 5] [--step] [--out profiles/r07_det_reduce.txt]

Shapes (B = --batch, --tile² feature maps): the dense layer's 136 -> 24 and the fuse convs' 368 -> 184 and 184 -> 64 3x3
weight gradients on packed 16-bit operands, a Discriminator1 trunk layer (64 -> 128, stride 2, on the 2·tile² activation
of a 4·tile² image) with its bias sums, the 184 -> 184 1x1 weight gradient and CAM's Gram matrix at C = 184.  --step adds
one bench-configuration-3-shaped GanTrainer.step (no perceptual term) per mode with its peak memory."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd as gd  # noqa: E402
from gan_danet_amd import _lib as L  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402

MODES = (("default", False, "unsplit"), ("unsplit", True, "unsplit"), ("ordered", True, "ordered"))
dev = torch.device("cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def three_modes(fn, plan, reps):
    """{mode: (median ms, splits)}; round 0 warms up (and allocates the ordered mode's workspace)"""
    t = {m[0]: [] for m in MODES}
    splits = {}
    for it in range(reps + 1):
        for name, on, red in MODES:
            gd.set_deterministic(on, reduce=red)
            try:
                splits[name] = plan() if plan else None
                ms = timed(fn)
            finally:
                gd.set_deterministic(False, reduce="unsplit")
            if it:
                t[name].append(ms)
    return {k: (statistics.median(v), splits[k]) for k, v in t.items()}


def rnd16(*shape):
    return torch.randn(*shape, device=dev).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T = a.batch, a.tile
    torch.manual_seed(0)
    rows = []

    def report(name, res):
        d, u, o = res["default"], res["unsplit"], res["ordered"]
        rows.append(f"{name:44s} default {d[0]:9.3f} ms ({d[1]} splits)   unsplit {u[0]:9.3f} ms   ordered {o[0]:9.3f} ms "
                    f"({o[1]} splits)   ordered/default {o[0] / d[0]:5.2f}   unsplit/ordered {u[0] / o[0]:6.1f}")
        print(rows[-1], flush=True)

    for Cin, Cout in ((136, 24), (368, 184), (184, 64)):
        dy16, x16 = rnd16(B, Cout, T * T), rnd16(B, T * T, Cin)
        report(f"3x3 wgrad {Cin} -> {Cout}, {T}x{T}, B={B}",
               three_modes(lambda: K.conv3x3_wgrad16(dy16, x16, T, T, 1),
                           lambda: K.conv3x3_wgrad_plan(B, Cout, Cin, T, T, 1)[0], a.reps))
        del dy16, x16
    Hd = 2 * T                                                        # conv2 of Discriminator1 on a 4T x 4T image
    g, x = rnd16(B, Hd // 2, Hd // 2, 128), rnd16(B, Hd, Hd, 64)
    report(f"D trunk 64 -> 128 s2 wgrad + bias, {Hd}x{Hd}, B={B}",
           three_modes(lambda: K.conv3x3_wgrad_nhwc(g, x, 2, True), lambda: K.conv3x3_wgrad_plan(B, 128, 64, Hd, Hd, 2)[0], a.reps))
    del g, x
    img, g = torch.randn(B, 1, 4 * T, 4 * T, device=dev), rnd16(B, 2 * T, 2 * T, 64)
    report(f"D stem 1 -> 64 s2 wgrad + bias, {4 * T}x{4 * T}, B={B}", three_modes(lambda: K.disc_stem_wgrad(g, img), None, a.reps))
    del img, g
    C = 184
    xf, dyf = torch.randn(B, C, T, T, device=dev), torch.randn(B, C, T, T, device=dev)
    report(f"1x1 wgrad {C} -> {C}, {T}x{T}, B={B} (bf16)",
           three_modes(lambda: K.conv2d_wgrad(dyf, xf, 1, 1, 0, L.PREC_BF16),
                       lambda: K.gemm_nt_plan(B=1, M=C, N=C, kseg=B, klen=T * T)[0], a.reps))
    del dyf
    N = T * T
    gram = torch.empty(B, C, C, device=dev)
    x3 = xf.view(B, C, N)
    report(f"CAM Gram C={C}, N={N}, B={B} (bf16)",
           three_modes(lambda: K.gemm_nt(B=B, M=C, N=C, kseg=1, klen=N, a=x3, a_bs=C * N, a_ss=0, lda=N, bm=x3, b_bs=C * N, b_ss=0,
                                         ldb=N, c=gram, c_bs=C * C, ldc=C, precision=L.PREC_BF16),
                       lambda: K.gemm_nt_plan(B=B, M=C, N=C, kseg=1, klen=N)[0], a.reps))
    del xf, x3, gram
    if a.step:
        G, D = gd.FlexibleUpsamplingModule(input_channels=8).to(dev), gd.Discriminator1().to(dev)
        with torch.no_grad():
            D(torch.zeros(1, 1, 4 * T, 4 * T, device=dev))
        G.apply(gd.weights_init_normal), D.apply(gd.weights_init_normal)
        tr = gd.GanTrainer(G.train(), D.train(), perceptual=None)
        xs, tg = torch.randn(B, 8, T, T, device=dev), torch.randn(B, 1, 4 * T, 4 * T, device=dev)
        for name, on, red in MODES:
            gd.set_deterministic(on, reduce=red)
            try:
                tr.step(xs, tg, 0.5)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                tr.step(xs, tg, 0.5)
                torch.cuda.synchronize()
                rows.append(f"GanTrainer.step {T}x{T} -> {4 * T}x{4 * T}, B={B}, no perceptual, {name:8s} "
                            f"{(time.perf_counter() - t0) * 1e3:9.1f} ms   peak {torch.cuda.max_memory_allocated() / 2 ** 30:6.1f} GiB")
                print(rows[-1], flush=True)
            finally:
                gd.set_deterministic(False, reduce="unsplit")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/det_reduce_bench.py --batch {B} --tile {T} --reps {a.reps}: {torch.cuda.get_device_name(0)}, "
                    f"{time.strftime('%Y-%m-%d')}; HIP-event medians, modes alternated in one process\n")
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
