"""HIP-event medians of the device STL (gan_danet_amd/stl.py) on the reference's own workload: detrend_and_compare of
datasets.py runs STL(y, seasonal=13, period=12) on every grid point of the (181, 88, 180) and the (181, 44, 90) GRACE array,
15 840 + 3 960 series of 181 months.  fp64 and fp32, non-robust (5 inner passes) and robust=True (2 inner, 15 outer
iterations).  For scale, the project's one-read-one-write gather, gd_augment_d4 with op word 0, on an fp32 tensor of the
bytes of the larger fp64 array.  Nothing comparable exists to compare with: statsmodels has not been timed on this
workload.  --out writes the table to a file (profiles/r17_stl.txt).

    python tools/stl_bench.py [--rounds 7] [--calls 3] [--out profiles/r17_stl.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import kern as K  # noqa: E402
from gan_danet_amd import stl  # noqa: E402
from filters_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(181, device=dev, dtype=torch.float64)[:, None, None]
    rows = []
    for shape in ((181, 88, 180), (181, 44, 90)):
        base = 0.01 * t + torch.sin(2 * torch.pi * t / 12) + 0.3 * torch.randn(shape, device=dev, dtype=torch.float64, generator=gen)
        for dtype in (torch.float64, torch.float32):
            x = base.to(dtype)
            for robust in (False, True):
                name = f"stl_decompose {shape} {'fp64' if dtype == torch.float64 else 'fp32'} {'robust (2, 15)' if robust else 'non-robust (5, 0)'}"
                rows.append((name, (lambda x=x, robust=robust: stl.stl_decompose(x, robust=robust)), shape[1] * shape[2]))
    x = 0.01 * t + torch.randn((181, 88, 180), device=dev, dtype=torch.float64, generator=gen)
    rows.append(("detrend_and_compare (181, 88, 180) fp64, its host copy included", lambda: stl.detrend_and_compare(x), 88 * 180))
    nbytes = 181 * 88 * 180 * 8
    y = torch.empty(nbytes // 4 // (2 * 88 * 180), 2, 88, 180, device=dev)
    ops0 = torch.zeros(y.shape[0], dtype=torch.int32, device=dev)
    rows.append(("gd_augment_d4 op 0 on the bytes of (181, 88, 180) fp64 (yardstick)", lambda: K.augment_d4(y, ops0), None))
    res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
    lines = [f"tools/stl_bench.py on {torch.cuda.get_device_name(0)}: STL(seasonal=13, period=12) of every grid point of the reference's "
             f"two GRACE arrays, 181 months each; {args.rounds} rounds x {args.calls} calls each, alternating, HIP events; a call "
             f"includes its allocations",
             "no speed threshold was set in advance and statsmodels has not been timed on this workload; the yardstick moves "
             f"{2 * y.numel() * 4 / 1e6:.0f} MB (one read + one write)"]
    for (name, _, series), (med, best) in zip(rows, res):
        tail = "" if series is None else f"  {series:6d} series  {series / med / 1e3:9.3f} M series/s"
        lines.append(f"{name:72s} median {med:9.3f} ms  best {best:9.3f} ms{tail}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
