"""HIP-event medians of the dataset preparation (gan_danet_amd/prepare.py) on a (181, 88, 180, 45) tensor -- the reference's
hr_aux -- in fp64 and fp32: the scaler fit, the transform (same layout, and to the stored (N, C, H, W) layout in fp32) and
one frequency augmentation along the time axis, against the project's own one-read-one-write gather, gd_augment_d4 with op
word 0, on an fp32 tensor of the same bytes.  GB/s counts each kernel's traffic budget: fit = one read of the tensor,
transform = one read + one write, augmentation = one read + one write + the K1 / L noise slices.  --out writes the table to
a file (profiles/r15_prepare.txt).

    python tools/prepare_bench.py [--rounds 7] [--calls 3] [--out profiles/r15_prepare.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import kern as K  # noqa: E402
from gan_danet_amd import prepare as P  # noqa: E402
from filters_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls inside one pair of events")
    ap.add_argument("--steps", type=int, default=181)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    shape = (args.steps, 88, 180, 45)
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"tools/prepare_bench.py on {torch.cuda.get_device_name(0)}: tensor {shape}; {args.rounds} rounds x {args.calls} calls "
             f"each, alternating, HIP events; a call includes its allocations (and, for the fit, its one host copy)",
             "GB/s = the kernel's traffic budget / median; ratio = GB/s over the yardstick's GB/s on the same bytes"]
    for dtype in (torch.float64, torch.float32):
        x = torch.randn(shape, device=dev, dtype=dtype, generator=gen) * 3.0 + 1.0
        nbytes = x.numel() * x.element_size()
        k1 = P.used_bins(12, shape[0])
        noise = torch.randn((k1,) + shape[1:], device=dev, dtype=torch.float64, generator=gen) * 0.1
        out = torch.empty_like(x)
        sc = P.ChannelScaler().fit(x)
        # the yardstick on the same bytes: an fp32 (B, C, H, W) tensor, op word 0 = a plain copy through the gather
        y = torch.empty(nbytes // 4 // (45 * 88 * 180), 45, 88, 180, device=dev)
        ops0 = torch.zeros(y.shape[0], dtype=torch.int32, device=dev)
        f32 = 4 * x.numel()
        rows = [("gd_augment_d4 op 0 (yardstick)", lambda: K.augment_d4(y, ops0), 2 * y.numel() * 4),
                ("ChannelScaler.fit (45 channels)", lambda: P.ChannelScaler().fit(x), nbytes),
                ("gd_channel_moments alone (no host copy)", lambda: K.channel_moments(x, 45), nbytes),
                ("transform, same layout and dtype", lambda: sc.transform(x), 2 * nbytes),
                ("transform -> fp32 (N, C, H, W)", lambda: sc.transform(x, out_dtype=torch.float32, to_nchw=True), nbytes + f32),
                ("inverse_transform", lambda: sc.inverse_transform(x), 2 * nbytes),
                (f"frequency augmentation axis 0, K1 = {k1}",
                 lambda: P.frequency_domain_augmentation(x, 12, 0.1, 0, noise=noise, out=out), 2 * nbytes + noise.numel() * 8)]
        res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
        base = rows[0][2] / res[0][0]
        lines.append(f"-- {str(dtype).replace('torch.', '')} ({nbytes / 1e6:.0f} MB)")
        for (name, _, nb), (med, best) in zip(rows, res):
            lines.append(f"{name:44s} median {med:9.3f} ms  best {best:9.3f} ms  {nb / 1e6:8.0f} MB  {nb / med / 1e6:8.1f} GB/s"
                         f"  x{(nb / med) / base:5.2f} of the yardstick's rate")
        del x, noise, out, y
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
