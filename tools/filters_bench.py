"""HIP-event medians of the device filters (gan_danet_amd/filters.py) on a (64, 7, 1024, 1024) fp32 tensor -- the size
of a stored hr_aux -- against the project's own one-read-one-write gather, gd_augment_d4 with op word 0, on the same
tensor.  GB/s counts one read plus one write of the tensor per pass (fill_masked: its two pointwise kernels and six
Gaussian passes by their own traffic).  --out writes the table to a file (profiles/r13_filters.txt).

    python tools/filters_bench.py [--rounds 7] [--calls 3] [--batch 64] [--out profiles/r13_filters.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import filters as F  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402


def median_ms(fns, rounds, calls, warmup=1):
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls inside one pair of events")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--hw", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    shape = (args.batch, 7, args.hw, args.hw)
    x = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    gappy = x.clone()
    gappy[torch.rand(shape, device=dev) < 0.2] = -9999.0
    rw = 2 * x.numel() * 4                                         # one read + one write of the tensor
    ops0 = torch.zeros(args.batch, dtype=torch.int32, device=dev)
    dst = torch.empty_like(x)

    def one_pass(axis, sigma):
        w, radius = K.gaussian_weights_host(sigma)
        return lambda: K.correlate1d_axis(x, dst, axis, w, radius)

    rows = [("gd_augment_d4 op 0 (yardstick)", lambda: K.augment_d4(x, ops0), rw)]
    for sigma in (2, 3):
        for axis, nm in ((0, "N"), (1, "C"), (2, "H"), (3, "W")):
            rows.append((f"gaussian pass axis {axis} ({nm}) sigma {sigma}", one_pass(axis, sigma), rw))
    rows += [("smooth_data_gaussian sigma 2 (4 passes)", lambda: F.smooth_data_gaussian(x, 2), 4 * rw),
             ("median 3x3 (axes 2, 3)", lambda: F.median_filter(x, 3, axes=(2, 3)), rw),
             ("smooth_data_median 3^4", lambda: F.smooth_data_median(x, 3), rw),
             ("smooth_data_savitzky_golay (5, 2)", lambda: F.smooth_data_savitzky_golay(x, 5, 2), rw),
             # prepare: 1 read + 2 writes; 6 Gaussian passes; ratio: 3 reads + 1 write
             ("fill_masked sigma 3 axes (0, 2, 3)", lambda: F.fill_masked(gappy, -9999, 3, axes=(0, 2, 3)),
              (3 + 12 + 4) * x.numel() * 4)]
    res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
    lines = [f"tools/filters_bench.py on {torch.cuda.get_device_name(0)}: tensor {shape} fp32 ({x.numel() * 4 / 1e6:.0f} MB); "
             f"{args.rounds} rounds x {args.calls} calls each, alternating, HIP events; a call includes its allocations",
             "GB/s = (one read + one write of the tensor per pass) / median; ratio = GB/s over the yardstick's GB/s"]
    base = rows[0][2] / res[0][0]
    for (name, _, nb), (med, best) in zip(rows, res):
        lines.append(f"{name:44s} median {med:9.3f} ms  best {best:9.3f} ms  {nb / 1e6:8.0f} MB  {nb / med / 1e6:8.1f} GB/s"
                     f"  x{(nb / med) / base:5.2f} of the yardstick's rate")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
