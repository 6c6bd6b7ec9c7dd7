"""HIP-event medians of the EOF kernels (gan_danet_amd/eof.py, csrc/eof.hip) on the product's own shape, a (181, 440, 900)
cube, fp64 and fp32: gd_eof_gram next to its two floors -- the fp64 matrix rate of a register-only
v_mfma_f64_16x16x4_f64 loop (tools/micro/mfma_f64_rate.hip, built and run as a child process) for its 78 blocks, and the
byte rate of the project's one-read-one-write yardstick, gd_augment_d4 with op word 0, on an fp32 tensor that moves the
same bytes -- then gd_eof_prepare, gd_eof_project (K = 4, 16) and gd_eof_reconstruct (K = 4) against the same yardstick.
For scale only: torch's fp64 A @ A.T on the centred cube and numpy.linalg.svd on the host (once).  All candidates of a
dtype alternate inside every round.  No speed threshold was set in advance.

    python tools/eof_bench.py [--rounds 7] [--calls 3] [--no-svd] [--out profiles/r22_eof.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import kern as K  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import SHAPE, yardstick  # noqa: E402


def mfma_rate():
    """TFLOP/s of the register-only fp64 MFMA loop, and the line it printed"""
    src = os.path.join(ROOT, "tools", "micro", "mfma_f64_rate.hip")
    exe = src[:-4]
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()
    return float(out[-1].split()[1]), out[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls inside one pair of events")
    ap.add_argument("--no-svd", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tf, tf_line = mfma_rate()                      # before this process opens the device for its own work
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    T, M = SHAPE[0], SHAPE[1] * SHAPE[2]
    t = torch.arange(T, device=dev, dtype=torch.float64)[:, None]
    x64 = 0.01 * t + torch.sin(2 * torch.pi * t / 12) * torch.rand((1, M), device=dev, dtype=torch.float64, generator=gen) \
        + 0.3 * torch.randn((T, M), device=dev, dtype=torch.float64, generator=gen) + 2.0
    w = torch.cos(torch.deg2rad(torch.linspace(-54.975, 54.975, SHAPE[1], device=dev, dtype=torch.float64)))[:, None] \
        .expand(SHAPE[1:]).contiguous().reshape(-1)
    nblk = (T + 15) // 16 * ((T + 15) // 16 + 1) // 2
    mfma_flop = nblk * 2048.0 * (-(-M // 4))       # the MFMAs the kernel issues: 78 blocks per 4 series
    lines = [f"tools/eof_bench.py on {torch.cuda.get_device_name(0)}: EOF kernels on a {SHAPE} cube ({T} x {M}); {args.rounds} rounds x "
             f"{args.calls} calls each, alternating, HIP events, median and best",
             "no speed threshold was set in advance; GB/s = the bytes the algorithm needs (yardstick: read + write) over the median",
             tf_line]
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        x = x64.to(dtype)
        cube = x.numel() * x.element_size()
        mean, valid = K.eof_prepare(x, None, w)
        G = torch.empty((T, T), device=dev, dtype=torch.float64)
        ws = torch.empty(K.eof_gram_ws_bytes(T, M), device=dev, dtype=torch.uint8)
        lam, u = np.linalg.eigh(K.eof_gram(x, mean, valid, w, out=G, ws=ws).cpu().numpy())
        coef16 = torch.from_numpy(np.ascontiguousarray(u[:, ::-1][:, :16] / np.sqrt(lam[::-1][:16]))).to(dev)
        coef4 = coef16[:, :4].contiguous()
        eofs4 = K.eof_project(x, mean, valid, coef4, w, True)
        pcs4 = torch.from_numpy(np.ascontiguousarray(u[:, ::-1][:, :4] * np.sqrt(lam[::-1][:4]))).to(dev)
        a64 = ((x.double() - mean[None, :]) * torch.sqrt(w)[None, :]) if dtype == torch.float64 else None
        rows = [(f"gd_eof_gram {tag} ({nblk} blocks, {ws.numel() >> 20} MiB of slabs)", lambda: K.eof_gram(x, mean, valid, w, out=G, ws=ws), cube),
                (f"gd_augment_d4 op 0, the bytes of one {tag} cube read (yardstick)", *yardstick(cube, dev)),
                (f"gd_eof_prepare {tag}", lambda: K.eof_prepare(x, None, w), cube),
                (f"gd_eof_project K = 4 {tag}", lambda: K.eof_project(x, mean, valid, coef4, w, True), cube + 4 * M * 8),
                (f"gd_eof_project K = 16 {tag}", lambda: K.eof_project(x, mean, valid, coef16, w, True), cube + 16 * M * 8),
                (f"gd_eof_reconstruct K = 4 -> {tag}", lambda: K.eof_reconstruct(eofs4, pcs4, mean, valid, w, dtype), cube + 4 * M * 8)]
        if a64 is not None:
            rows.append(("torch fp64 A @ A.T on the centred, weighted cube (for scale)", lambda: a64 @ a64.T, cube))
        res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
        yard = res[1][0]
        for (name, _, nbytes), (med, best) in zip(rows, res):
            extra = f"  {yard / med:5.2f} of the yardstick's rate" if "yardstick" not in name and "torch" not in name else ""
            if name.startswith("gd_eof_gram"):
                extra += f"; {mfma_flop / med / 1e9:6.2f} TFLOP/s issued = {mfma_flop / med / 1e9 / tf:4.2f} of the MFMA loop's {tf:.2f}"
            lines.append(f"{name:66s} median {med:8.3f} ms  best {best:8.3f} ms  {nbytes / 1e6:6.0f} MB  {nbytes / med / 1e6:7.1f} GB/s{extra}")
        del a64
    if not args.no_svd:
        a = ((x64 - x64.mean(0, keepdim=True)) * torch.sqrt(w)[None, :]).cpu().numpy()
        t0 = time.perf_counter()
        np.linalg.svd(a, full_matrices=False)
        lines.append(f"numpy.linalg.svd of the {T} x {M} fp64 anomaly matrix on the host, once (for scale; without the copy of the cube)"
                     f"  {1e3 * (time.perf_counter() - t0):9.0f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
