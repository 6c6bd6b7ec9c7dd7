"""HIP-event medians of the guarded optimiser step against the unguarded per-tensor gd_adamw loop, on two tensor sets: the
generator's parameter list at config 3 (FlexibleUpsamplingModule(input_channels=8): ~150 tensors, launch-bound) and one
2^31-element tensor (Discriminator1.fc1 at config 3, HBM-bound).  Per row: ms, GB/s, share of 8 TB/s, and the time the
row's byte count would take at the unguarded loop's measured GB/s on the same tensors.

    python tools/gradguard_bench.py [--out profiles/r12_gradguard.txt] [--big-n 2147483648] [--rounds 7]

Bytes per element: unguarded 28 (p, m, v read and written, g read); guarded 32 (g read a second time by the norm);
guarded + EMA 40; the norm alone 4.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd as gd  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402

HP = dict(lr=4e-4, beta1=0.5, beta2=0.999, eps=1e-8, weight_decay=1e-4)


def median_ms(fns, rounds, calls, warmup=2):
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


def tensor_set(sizes, dev):
    mk = lambda s: [torch.randn(n, device=dev) * s for n in sizes]   # noqa: E731
    return dict(p=mk(0.02), g=mk(1e-3), m=mk(1e-4), v=[t.abs() for t in mk(1e-6)], ema=mk(0.02))


def rows_for(ts, rec):
    n = sum(t.numel() for t in ts["p"])
    hp = (HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"])

    def parent():
        for p, g, m, v in zip(ts["p"], ts["g"], ts["m"], ts["v"]):
            K.adamw(p, g, m, v, 3, *hp)

    def guarded(ema):
        def run():
            K.grad_sqnorm(ts["g"], rec)
            K.guard_finalize(rec, 1e9, True)
            for i, (p, g, m, v) in enumerate(zip(ts["p"], ts["g"], ts["m"], ts["v"])):
                K.adamw_guarded(p, g, m, v, rec, *hp, 1.0, ts["ema"][i] if ema else None, 0.999)
        return run

    return [("gd_adamw loop (unguarded)", parent, 28 * n), ("guarded", guarded(False), 32 * n),
            ("guarded + EMA", guarded(True), 40 * n), ("norm pass alone", lambda: K.grad_sqnorm(ts["g"], rec), 4 * n)]


def report(title, rows, res, out):
    out(title)
    base_rate = rows[0][2] / res[0][0]                       # bytes per ms of the unguarded loop on these tensors
    for (name, _, nb), (med, best) in zip(rows, res):
        budget = nb / base_rate
        out(f"  {name:28s} median {med:9.4f} ms  best {best:9.4f} ms  {nb / 1e9:8.3f} GB  {nb / med / 1e6:8.1f} GB/s"
            f"  {nb / med / 1e6 / 8000 * 100:5.1f} % of 8 TB/s  budget at the unguarded rate {budget:9.4f} ms"
            f"  measured / budget {med / budget:5.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--big-n", type=int, default=2 ** 31, help="elements of the big tensor (fc1 at config 3: 2^31)")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    rec = K.guard_record(dev)
    out(f"device {torch.cuda.get_device_name(0)}; HIP events, {args.rounds} rounds, the four variants alternating inside a round")
    sizes = [p.numel() for p in gd.FlexibleUpsamplingModule(input_channels=8).parameters()]
    small = tensor_set(sizes, dev)
    rows = rows_for(small, rec)
    report(f"generator parameter list at config 3: {len(sizes)} tensors, {sum(sizes)} elements (20 calls per event pair); "
           "launch-bound, no bound set", rows, median_ms([r[1] for r in rows], args.rounds, 20), out)
    del small, rows
    big = tensor_set([args.big_n], dev)
    rows = rows_for(big, rec)
    res = median_ms([r[1] for r in rows], args.rounds, 2, warmup=1)
    report(f"one tensor of {args.big_n} elements (2 calls per event pair)", rows, res, out)
    base_rate = rows[0][2] / res[0][0]
    for (name, _, nb), (med, _) in list(zip(rows, res))[1:3]:
        ratio = med / (nb / base_rate)
        out(f"  {name}: {'WITHIN' if ratio <= 1.15 else 'OVER'} the 15 % allowance over its traffic budget (x{ratio:.3f})")
    K.grad_sqnorm(big["g"], rec)
    want = float((big["g"][0][:1 << 24].double() ** 2).sum())
    r2 = K.guard_record(dev)
    K.grad_sqnorm([big["g"][0][:1 << 24]], r2)
    out(f"check: sqnorm of the first 2^24 elements {r2[0].item():.15e} (torch fp64 {want:.15e}); whole tensor {rec[0].item():.6e}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
