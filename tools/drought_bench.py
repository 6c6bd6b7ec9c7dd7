"""HIP-event medians of the drought module's entry points (gan_danet_amd/drought.py, csrc/drought.hip) on the product's
own shape, a (181, 440, 900) cube, fp64 and fp32 storage, period 12: gd_drought_clim (one read of the cube), gd_drought_index
(read + write), gd_drought_rank (read + write; the baseline samples of a slot are re-read from cache), gd_drought_events
without and with in_event (read; read + T M bytes), and the area series of the five DSI classes (per class: gd_drought_exceed
read + write, gd_zone_mean read).  All alternate with the project's one-read-one-write yardstick, gd_augment_d4 with op
word 0, on fp32 tensors that move the bytes of one and of two cubes.  GB/s are the bytes a step must move (as listed; the
maps and the climatology are below 7 % of a cube and not counted) over the median; the ratio is that rate over the rate of
the yardstick of the nearer size.  No speed threshold was set in advance.  --out writes the table to a file
(profiles/r24_drought.txt).

    python tools/drought_bench.py [--rounds 7] [--calls 3] [--out profiles/r24_drought.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import drought as D  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import SHAPE, yardstick  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    T, M = SHAPE[0], SHAPE[1] * SHAPE[2]
    t = torch.arange(T, device=dev, dtype=torch.float64)[:, None]
    x64 = torch.sin(2 * torch.pi * t / 12) + torch.randn((T, M), device=dev, dtype=torch.float64, generator=gen).cumsum(0) * 0.3
    x64[::17, ::5] = float("nan")                                    # GRACE's missing months, on a fifth of the pixels
    nmax = -(-T // 12) + 1
    table = torch.from_numpy(D.rank_table("empirical", nmax).copy()).to(dev)
    bits = torch.ones(SHAPE[1:], device=dev, dtype=torch.int32).view(torch.uint32)
    rows = []
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        x = x64.to(dtype)
        cube = x.numel() * x.element_size()
        clim = K.drought_clim(x, 12)
        z = K.drought_index(x, clim)
        out = torch.empty_like(x)
        maps = torch.empty((len(D.MAPS), M), device=dev, dtype=torch.float64)
        steps = torch.empty((T, M), device=dev, dtype=torch.uint8)
        cube3 = z.reshape(SHAPE)

        def area(cube3=cube3, out=out):
            for thr in D.DSI_CLASSES:
                K.drought_exceed(cube3, thr, out=out.reshape(SHAPE))
                K.zone_mean(out.reshape(SHAPE), bits, 1)

        rows.append((f"gd_augment_d4 op 0, the bytes of one {tag} cube (yardstick)", *yardstick(cube, dev), None))
        rows.append((f"gd_augment_d4 op 0, the bytes of two {tag} cubes (yardstick)", *yardstick(2 * cube, dev), None))
        rows.append((f"gd_drought_clim period 12 {tag}", (lambda x=x, clim=clim: K.drought_clim(x, 12, out=clim)), cube, 0))
        rows.append((f"gd_drought_index standardized {tag}", (lambda x=x, clim=clim, out=out: K.drought_index(x, clim, out=out)), 2 * cube, 1))
        rows.append((f"gd_drought_rank empirical {tag} (n <= {nmax - 1} per slot)",
                     (lambda x=x, out=out: K.drought_rank(x, table, 12, out=out)), 2 * cube, 1))
        rows.append((f"gd_drought_events 12 maps {tag}", (lambda z=z, maps=maps: K.drought_events(z, -0.8, 3, out=maps)), cube, 0))
        rows.append((f"gd_drought_events 12 maps + in_event {tag}",
                     (lambda z=z, maps=maps, steps=steps: K.drought_events(z, -0.8, 3, out=maps, in_event=steps)), cube + T * M, 0))
        rows.append((f"drought area, 5 DSI classes: 5 x (gd_drought_exceed + gd_zone_mean) {tag}", area, 15 * cube, 1))
    res = median_ms([r[1] for r in rows], args.rounds, args.calls)
    lines = [f"tools/drought_bench.py on {torch.cuda.get_device_name(0)}: drought analysis of a {SHAPE} cube, period 12; {args.rounds} rounds x "
             f"{args.calls} calls each, alternating, HIP events; outputs preallocated",
             "no speed threshold was set in advance; GB/s = the bytes the step must move over the median; ratio = that rate over the rate of "
             "the yardstick of the nearer size"]
    yard = []
    for (name, _, nbytes, ref), (med, best) in zip(rows, res):
        rate = nbytes / med / 1e6
        if ref is None:
            yard = (yard + [rate])[-2:] if len(yard) < 2 else [rate]
            ratio = ""
        else:
            ratio = f"  {rate / yard[ref]:5.2f} of the yardstick"
        lines.append(f"{name:78s} median {med:9.3f} ms  best {best:9.3f} ms  {nbytes / 1e6:8.0f} MB  {rate:8.1f} GB/s{ratio}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
