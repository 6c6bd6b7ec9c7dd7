"""HIP-event medians of the per-pixel time-series module (gan_danet_amd/timeseries.py) on the product's own shape, a
(181, 440, 900) cube, fp64 and fp32: skill_maps (two reads of the cube: prediction and truth), harmonic_fit with P = 6 (two
reads of one cube: the normal equations, then the residuals) and coarsen by (5, 5) (one read).  Each is timed next to the
project's one-read-one-write yardstick, gd_augment_d4 with op word 0, on an fp32 tensor sized to move the same bytes.
GB/s are the bytes the algorithm needs (the cube reads; the maps written are below 1 % of them) over the median.  No
speed threshold was set in advance.  --out writes the table to a file (profiles/r18_series.txt).

    python tools/series_bench.py [--rounds 7] [--calls 3] [--out profiles/r18_series.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import kern as K  # noqa: E402
from gan_danet_amd import timeseries as TS  # noqa: E402
from filters_bench import median_ms  # noqa: E402

SHAPE = (181, 440, 900)


def yardstick(moved_bytes, dev):
    """gd_augment_d4 with op word 0 on an fp32 (B, 2, 440, 900) batch that reads and writes ``moved_bytes`` in all"""
    b = max(1, moved_bytes // 2 // 4 // (2 * SHAPE[1] * SHAPE[2]))
    y = torch.empty(b, 2, SHAPE[1], SHAPE[2], device=dev)
    ops0 = torch.zeros(b, dtype=torch.int32, device=dev)
    return (lambda: K.augment_d4(y, ops0)), 2 * y.numel() * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(SHAPE[0], device=dev, dtype=torch.float64)[:, None, None]
    truth64 = 0.01 * t + torch.sin(2 * torch.pi * t / 12) + 0.3 * torch.randn(SHAPE, device=dev, dtype=torch.float64, generator=gen) + 2.0
    pred64 = 0.8 * truth64 + 0.3 + 0.2 * torch.randn(SHAPE, device=dev, dtype=torch.float64, generator=gen)
    rows = []
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        p, q = pred64.to(dtype), truth64.to(dtype)
        cube = p.numel() * p.element_size()
        rows.append((f"skill_maps {SHAPE} {tag} (6 maps)", (lambda p=p, q=q: TS.skill_maps(p, q)), 2 * cube))
        rows.append((f"harmonic_fit P = 6 {SHAPE} {tag}", (lambda q=q: TS.harmonic_fit(q)), 2 * cube))
        rows.append((f"gd_augment_d4 op 0, the bytes of two {tag} cube reads (yardstick)", *yardstick(2 * cube, dev)))
        rows.append((f"coarsen (5, 5) {SHAPE} {tag}", (lambda p=p: TS.coarsen(p, 5)), cube))
        rows.append((f"gd_augment_d4 op 0, the bytes of one {tag} cube read (yardstick)", *yardstick(cube, dev)))
    res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
    lines = [f"tools/series_bench.py on {torch.cuda.get_device_name(0)}: per-pixel time series of a {SHAPE} cube; {args.rounds} rounds x "
             f"{args.calls} calls each, alternating, HIP events; a call includes its allocations and its finalising kernels",
             "no speed threshold was set in advance; GB/s = the cube bytes the algorithm reads (the yardstick: read + write) over the median"]
    for (name, _, nbytes), (med, best) in zip(rows, res):
        lines.append(f"{name:72s} median {med:9.3f} ms  best {best:9.3f} ms  {nbytes / 1e6:8.0f} MB  {nbytes / med / 1e6:8.1f} GB/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
