"""HIP-event medians of the regionalisation kernels (csrc/kmeans.hip) on a (181, 440, 900) cube of planted blobs, fp64 and fp32
storage: gd_km_assign (with and without the second-nearest outputs) and gd_km_update at K = 8, 32, 64, each next to the
project's one-read-one-write yardstick, gd_augment_d4 with op word 0 on an fp32 tensor sized to move the bytes of one cube
read, in ms, GB/s and as a ratio; a whole kmeans_series run at K = 8 with its iteration count; and, for scale, the torch form
users have today (cdist + argmin + index_add_, with its peak memory) and a numpy Lloyd iteration on the host, timed on one row
of 900 pixels and extrapolated linearly to the cube.  No speed threshold was set in advance.  Every GPU step runs once (its
timed rounds aside); a failing step ends the tool, nothing is tried again.  --out writes the table to a file
(profiles/r33_regions.txt).

    python tools/regions_bench.py [--rounds 5] [--calls 2] [--out profiles/r33_regions.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd as gd  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import yardstick  # noqa: E402

SHAPE = (181, 440, 900)
KS = (8, 32, 64)


def torch_form(x, cent):
    """one Lloyd iteration the way users write it: an (M, K) distance matrix, argmin, index_add_ (atomics: not reproducible)"""
    xt = x.t().to(torch.float64)
    d = torch.cdist(xt, cent)
    lab = d.argmin(dim=1)
    new = torch.zeros_like(cent).index_add_(0, lab, xt)
    cnt = torch.zeros(cent.shape[0], device=x.device, dtype=torch.float64).index_add_(0, lab, torch.ones_like(lab, dtype=torch.float64))
    return new / cnt[:, None], lab


def numpy_row_seconds(xr, cent):
    t0 = time.perf_counter()
    d = ((xr.T[:, None, :] - cent[None, :, :]) ** 2).sum(axis=2)
    lab = d.argmin(axis=1)
    for k in range(cent.shape[0]):
        if (lab == k).any():
            xr[:, lab == k].mean(axis=1)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    T, M = SHAPE[0], SHAPE[1] * SHAPE[2]
    centres = 3.0 * torch.randn((64, T), device=dev, dtype=torch.float64, generator=gen)
    planted = torch.randint(0, 64, (M,), device=dev, generator=gen)
    x64 = centres[planted].t().contiguous()
    x64 += 0.5 * torch.randn((T, M), device=dev, dtype=torch.float64, generator=gen)
    rows = []
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        x = x64.to(dtype)
        cube = x.numel() * x.element_size()
        rows.append((f"gd_augment_d4 op 0, the bytes of one {tag} cube read (yardstick)", *yardstick(cube, dev), None))
        for k in KS:
            cent = centres[:k].contiguous()
            label, dist, _, _ = K.km_assign(x, cent)
            ws = torch.empty(K.km_update_workspace(T, M, k), device=dev, dtype=torch.uint8)
            rows.append((f"gd_km_assign {tag} K = {k:2d}", (lambda x=x, c=cent: K.km_assign(x, c)), cube, tag))
            rows.append((f"gd_km_assign {tag} K = {k:2d} with second nearest", (lambda x=x, c=cent: K.km_assign(x, c, second=True)), cube, tag))
            rows.append((f"gd_km_update {tag} K = {k:2d}", (lambda x=x, c=cent, l=label, d=dist, ws=ws: K.km_update(x, l, d, c, ws=ws)), cube, tag))
    res = median_ms([fn for _, fn, _, _ in rows], args.rounds, args.calls)
    lines = [f"tools/regions_bench.py on {torch.cuda.get_device_name(0)}: k-means on a {SHAPE} cube (64 planted blobs); {args.rounds} rounds x "
             f"{args.calls} calls each, alternating, HIP events; a call includes its output allocations (the update workspace is reused)",
             "no speed threshold was set in advance; GB/s = the bytes of one cube read (the yardstick: read + write) over the median"]
    yard = {}
    for (name, _, nbytes, tag), (med, bst) in zip(rows, res):
        line = f"{name:64s} median {med:9.3f} ms  best {bst:9.3f} ms  {nbytes / 1e6:7.0f} MB  {nbytes / med / 1e6:8.1f} GB/s"
        if tag is None:
            yard["fp64" if "fp64" in name else "fp32"] = med
        else:
            line += f"  {med / yard[tag]:6.2f}x the yardstick"
        lines.append(line)
    # a whole run at K = 8 (maximin, tol = 0: runs until no label changes), timed once on the wall clock after one warm-up
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        x = x64.to(dtype).reshape(SHAPE)
        gd.kmeans_series(x, 8, max_iter=2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = gd.kmeans_series(x, 8)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        lines.append(f"kmeans_series {tag} k = 8, maximin, tol = 0: {sec * 1e3:9.1f} ms wall clock for {r.n_iter} iterations (converged "
                     f"{r.converged}), the initialisation and the closing assign + update included; inertia {float(r.inertia):.6e}")
    # the torch form, once per K after a warm-up, with its peak memory above the cube
    for k in KS:
        cent = centres[:k].contiguous()
        torch_form(x64, cent)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_form(x64, cent)
        e1.record()
        torch.cuda.synchronize()
        lines.append(f"torch cdist + argmin + index_add_ fp64 K = {k:2d}: {e0.elapsed_time(e1):9.3f} ms, peak memory above the resident tensors "
                     f"{(torch.cuda.max_memory_allocated() - base) / 1e6:8.0f} MB (atomics: the centroids differ from run to run)")
    xr = x64[:, :SHAPE[2]].cpu().numpy()
    for k in KS:
        sec = numpy_row_seconds(xr, centres[:k].cpu().numpy())
        lines.append(f"numpy on the host, fp64, K = {k:2d}: {sec * 1e3:8.1f} ms for one row of {SHAPE[2]} pixels, {sec * SHAPE[1]:7.1f} s per iteration "
                     f"extrapolated to the cube")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
