"""HIP-event medians of the spatial-spectra kernels (gan_danet_amd/spectra.py, csrc/spectra.hip) on a (181, 440, 900) and a
(181, 88, 180) cube, fp64 and fp32 storage: gd_spec_prepare, gd_spec_power with the TFLOP/s its MFMAs imply and their
share of the register-only fp64 MFMA loop of tools/eof_bench.py (run as a child process first), and gd_spec_cross.  For
scale: torch.fft.rfft2 -> abs()**2 -> index_add_ on the same cube with the peak memory of both paths
(torch.cuda.max_memory_allocated), and gd_augment_d4 moving the cube's bytes.  All candidates of a shape and dtype
alternate inside every round.  No speed threshold was set in advance.

    python tools/spectra_bench.py [--rounds 5] [--calls 2] [--out profiles/r23_spectra.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import kern as K  # noqa: E402
from gan_danet_amd import spectra as SP  # noqa: E402
from eof_bench import mfma_rate  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import yardstick  # noqa: E402


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tf, tf_line = mfma_rate()                      # before this process opens the device for its own work
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"tools/spectra_bench.py on {torch.cuda.get_device_name(0)}: {args.rounds} rounds x {args.calls} calls each, alternating, "
             "HIP events, median and best; no speed threshold was set in advance", tf_line]
    for shape, d in (((181, 440, 900), 0.05), ((181, 88, 180), 0.25)):
        T, H, W = shape
        x64 = torch.randn(shape, device=dev, dtype=torch.float64, generator=gen) + 2.0
        y64 = 0.7 * x64 + 0.3 * torch.randn(shape, device=dev, dtype=torch.float64, generator=gen)
        for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
            x, y = x64.to(dtype), y64.to(dtype)
            p = SP._plan(x, d, d, None, "plane", "hann", None)
            coef, S = K.spec_prepare(x, None, p.wy, p.wx, "plane")
            cy, sy = K.spec_prepare(y, None, p.wy, p.wx, "plane")
            ws = torch.empty(K.spec_cross_ws_bytes(T, H, W, p.nbins), device=dev, dtype=torch.uint8)
            power, dropped = torch.empty((T, p.nbins), device=dev, dtype=torch.float64), torch.empty(T, device=dev, dtype=torch.float64)
            out, d4 = torch.empty((4, T, p.nbins), device=dev, dtype=torch.float64), torch.empty((T, 4), device=dev, dtype=torch.float64)
            slot = torch.where(p.bins < 0, p.nbins, p.bins).reshape(-1).long()
            win = (p.wy[:, None] * p.wx[None, :])

            def f_prepare():
                K.spec_prepare(x, None, p.wy, p.wx, "plane", coef=coef, S=S)

            def f_power():
                K.spec_power(x, coef, S, p.twh, p.tww, p.bins, p.nbins, None, p.wy, p.wx, power=power, dropped=dropped, ws=ws)

            def f_cross():
                K.spec_cross(x, y, coef, S, cy, sy, p.twh, p.tww, p.bins, p.nbins, None, p.wy, p.wx, out=out, dropped=d4, ws=ws)

            def f_fft():
                z = torch.fft.rfft2((x - x.mean(dim=(1, 2), keepdim=True)).double() * win)
                acc = torch.zeros((T, p.nbins + 1), device=dev, dtype=torch.float64)
                acc.index_add_(1, slot, (z.abs() ** 2).reshape(T, -1))
                return acc

            yard, moved = yardstick(x.numel() * x.element_size() * 2, dev)
            names = ("gd_spec_prepare", "gd_spec_power", "gd_spec_cross", "rfft2 + abs^2 + index_add_", "gd_augment_d4 (same bytes)")
            res = median_ms((f_prepare, f_power, f_cross, f_fft, yard), args.rounds, args.calls)
            # the MFMAs the power kernel issues: per tile, stage 1 (64-row blocks x 32-column chunks) and stage 2
            tiles, hp, wp = -(-(W // 2 + 1) // 8), -(-H // 64) * 64, -(-W // 32) * 32
            flop = T * tiles * 2048.0 * ((hp // 16) * (wp // 4) + 2 * (-(-H // 16)) * (-(-H // 4)))
            lines.append(f"--- {shape} {tag}, detrend plane, Hann, {p.nbins} bins")
            for n, (med, best) in zip(names, res):
                extra = ""
                if n == "gd_spec_power":
                    extra = f"  {flop / med / 1e9:.2f} TFLOP/s issued, {flop / med / 1e9 / tf:.2f} of the register-only loop ({tf:.1f})"
                lines.append(f"{n:32s} median {med:9.3f} ms  best {best:9.3f} ms{extra}")
            lines.append(f"memory above the inputs: gd_spec_power allocates {peak(f_power):.1f} MiB and needs a workspace of "
                         f"{K.spec_power_ws_bytes(T, H, W, p.nbins) / 2 ** 20:.1f} MiB, gd_spec_cross one of "
                         f"{K.spec_cross_ws_bytes(T, H, W, p.nbins) / 2 ** 20:.1f} MiB; the rfft2 pipeline peaks at {peak(f_fft):.1f} MiB")
            del x, y, ws
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
