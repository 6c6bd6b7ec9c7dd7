"""HIP-event medians of the device spline zoom (gan_danet_amd/spline.py) on the inference product's workload,
zoom((181, 88, 180), (1, 5, 5), order=3) in fp64 and in fp32, against the project's own one-read-one-write gather,
gd_augment_d4 with op word 0, on an fp32 tensor of as many bytes as the zoom's output.  GB/s counts the bytes that must
move: one read of the input plus one write of the output (the fp64 coefficients and the stack between the two axes are
the implementation's own traffic and are not counted).  The two axis passes, and the order-0 and order-1 zooms of the
same stack, are listed too.  --out writes the table to a file (profiles/r14_zoom.txt).

    python tools/zoom_bench.py [--rounds 7] [--calls 3] [--steps 181] [--out profiles/r14_zoom.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import _lib as L  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402
from gan_danet_amd import spline  # noqa: E402


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
    ap.add_argument("--steps", type=int, default=181, help="time steps of the stack")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    T, H, W, f = args.steps, 88, 180, 5
    x64 = torch.randn((T, H, W), device=dev, dtype=torch.float64, generator=torch.Generator(device=dev).manual_seed(0))
    x32 = x64.float()
    n_in, n_out = x64.numel(), T * H * f * W * f
    # the yardstick moves the output's bytes once in and once out: an fp32 tensor of the fp64 output's size has two planes
    y64 = torch.randn((T, 2, H * f, W * f), device=dev)
    y32 = y64[:, :1].contiguous()
    ops0 = torch.zeros(T, dtype=torch.int32, device=dev)
    mid64 = K.zoom_axis(x64, 1, H * f, 3, L.ZOOM_MIRROR, torch.float64)

    rows = [("gd_augment_d4 op 0, output-sized fp64 (yardstick)", lambda: K.augment_d4(y64, ops0), 2 * y64.numel() * 4),
            ("gd_augment_d4 op 0, output-sized fp32", lambda: K.augment_d4(y32, ops0), 2 * y32.numel() * 4),
            ("zoom (1, 5, 5) order 3 fp64", lambda: spline.zoom(x64, (1, f, f), order=3), (n_in + n_out) * 8),
            ("zoom (1, 5, 5) order 3 fp32", lambda: spline.zoom(x32, (1, f, f), order=3), (n_in + n_out) * 4),
            ("  axis 1 pass 88 -> 440 (inner 180) fp64", lambda: K.zoom_axis(x64, 1, H * f, 3, L.ZOOM_MIRROR),
             (n_in + n_in * f) * 8),
            ("  axis 2 pass 180 -> 900 (inner 1) fp64", lambda: K.zoom_axis(mid64, 2, W * f, 3, L.ZOOM_MIRROR),
             (n_in * f + n_out) * 8),
            ("  prefilter alone, axis 1 fp64", lambda: K.spline_prefilter_axis(x64, 1), 2 * n_in * 8),
            ("  prefilter alone, axis 2 of the 440-row stack", lambda: K.spline_prefilter_axis(mid64, 2), 2 * n_in * f * 8),
            ("zoom (1, 5, 5) order 3 'nearest' fp64", lambda: spline.zoom(x64, (1, f, f), order=3, mode="nearest"),
             (n_in + n_out) * 8),
            ("zoom (1, 5, 5) order 1 fp64", lambda: spline.zoom(x64, (1, f, f), order=1), (n_in + n_out) * 8),
            ("zoom (1, 5, 5) order 0 'nearest' fp32", lambda: spline.zoom(x32, (1, f, f), order=0, mode="nearest"),
             (n_in + n_out) * 4)]
    res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
    lines = [f"tools/zoom_bench.py on {torch.cuda.get_device_name(0)}: stack {(T, H, W)} -> {(T, H * f, W * f)} "
             f"({n_out * 8 / 1e6:.0f} MB in fp64); {args.rounds} rounds x {args.calls} calls each, alternating, HIP events; "
             "a call includes its allocations",
             "GB/s = (one read of the input + one write of the output) / median; ratio = GB/s over the yardstick's GB/s"]
    base = rows[0][2] / res[0][0]
    for (name, _, nb), (med, best) in zip(rows, res):
        lines.append(f"{name:50s} median {med:9.3f} ms  best {best:9.3f} ms  {nb / 1e6:8.0f} MB  {nb / med / 1e6:8.1f} GB/s"
                     f"  x{(nb / med) / base:5.2f} of the yardstick's rate")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f_:
            f_.write(text + "\n")


if __name__ == "__main__":
    main()
