"""HIP-event medians of gd_eval_stats against gd_mse (da = NULL) on the same two (32, 1, 1024, 1024) fp32 tensors -- both
stream the same 268 MB -- and of gd_ensemble_stats at M = 5, 16 and 32.  Prints ms and GB/s; profiles/r10_eval_stats.txt holds a run.

    python tools/eval_bench.py [--iters 30] [--batch 32]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import kern as K  # noqa: E402


def median_ms(fns, rounds, calls=20, warmup=3):
    """per-call ms of every fn: HIP events around `calls` back-to-back calls, the fns alternating inside each round (so a
    drifting clock or a busy neighbour touches all of them alike); median and best over the rounds"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1) / calls)
    return [(statistics.median(t), min(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25, help="rounds; every round times 20 calls of each kernel")
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    dev = torch.device("cuda")
    shape = (args.batch, 1, 1024, 1024)
    g = torch.Generator(device=dev).manual_seed(0)
    truth = torch.randn(shape, device=dev, generator=g)
    pred = truth + 0.1 * torch.randn(shape, device=dev, generator=g)
    nbytes = 2 * pred.numel() * 4
    rec = torch.zeros(8, dtype=torch.float64, device=dev)
    mask = (torch.rand(1024, 1024, device=dev, generator=g) < 0.6).to(torch.uint8)
    rows = [("gd_mse (da = NULL)", lambda: K.diff_loss("mse", pred, truth, False), nbytes),
            ("gd_eval_stats", lambda: K.eval_stats(pred, truth, rec), nbytes),
            ("gd_eval_stats + mask", lambda: K.eval_stats(pred, truth, rec, mask=mask), nbytes),
            ("gd_eval_stats + affine", lambda: K.eval_stats(pred, truth, rec, affine=(2.0, 3.0)), nbytes)]
    def ensemble_row(M, Bm):                                     # M = 5: the 8-member instance; 16 and 32: the 32-member one
        slab = torch.randn((M, Bm, 1, 1024, 1024), device=dev, generator=g)
        mean, std = torch.empty_like(slab[0]), torch.empty_like(slab[0])
        return (f"gd_ensemble_stats M={M} fp32", lambda: K.ensemble_stats(slab, mean, std), (M + 2) * mean.numel() * 4)

    rows += [ensemble_row(5, 8), ensemble_row(16, 4), ensemble_row(32, 2)]
    rows.append(("gd_masked_plane_mean", lambda: K.masked_plane_mean(pred, mask), pred.numel() * 4))
    print(f"device {torch.cuda.get_device_name(0)}; tensors {shape} fp32; {args.iters} rounds x 20 calls each, alternating, HIP events (a call = its two launches)")
    res = median_ms([fn for _, fn, _ in rows], args.iters)
    base = res[0][0]
    for (name, fn, nb), (med, best) in zip(rows, res):
        print(f"{name:32s} median {med:8.4f} ms  best {best:8.4f} ms  {nb / 1e6:7.1f} MB  {nb / med / 1e6:8.1f} GB/s"
              f"  x{med / base:5.2f} of gd_mse")
    K.eval_stats(pred, truth, rec)
    m = K.eval_merge_host(rec.cpu().numpy())[1]
    want = ((pred.double() - truth.double()) ** 2).mean().item()
    print(f"check: mse {m['mse']:.12e} (torch fp64 {want:.12e})")


if __name__ == "__main__":
    main()
