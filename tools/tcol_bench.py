"""HIP-event medians of the triple-collocation kernels (csrc/tcol.hip) on three (181, 440, 900) cubes, fp64 and fp32 storage:
gd_tc_estimate next to the project's one-read-one-write yardstick, gd_augment_d4 with op word 0 on an fp32 tensor sized to move
the same bytes (two reads of each cube), and gd_tc_bootstrap at B = 100 and B = 1000 replicates of blocks of 6 steps, with the
gathered triplets per second (T x B x M over the median) and the share of the device time that the sort and summary kernels
take (per-kernel device times of one call from torch.profiler, a pass of its own after the timed rounds).  For scale, a numpy
version of the bootstrap on the host (fp64, fancy-indexed gather, np.nanquantile) is timed on one row of 900 pixels at B = 100
and extrapolated linearly to the cube and to B.  No speed threshold was set in advance.  --out writes the table to a file
(profiles/r30_tcol.txt).

    python tools/tcol_bench.py [--rounds 5] [--calls 2] [--out profiles/r30_tcol.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import kern as K  # noqa: E402
from gan_danet_amd.collocation import bootstrap_indices  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import yardstick  # noqa: E402

SHAPE = (181, 440, 900)
Q3 = (0.025, 0.5, 0.975)


def numpy_row_seconds(x, y, z, idx):
    """the bootstrap in numpy on one (T, 900) row: gather, listwise deletion, covariances, the eight formulas, nanquantile"""
    t_start = time.perf_counter()
    xs, ys, zs = x[idx], y[idx], z[idx]                               # (T, B, M)
    ok = ~(np.isnan(xs) | np.isnan(ys) | np.isnan(zs))
    n = ok.sum(axis=0)
    d = [np.where(ok, a - np.where(ok, a, 0).sum(axis=0) / n, 0) for a in (xs, ys, zs)]
    q = {(a, b): (d[a] * d[b]).sum(axis=0) / (n - 1) for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))}
    with np.errstate(all="ignore"):
        st = np.stack([q[0, 0] - q[0, 1] * q[0, 2] / q[1, 2], q[1, 1] - q[0, 1] * q[1, 2] / q[0, 2], q[2, 2] - q[0, 2] * q[1, 2] / q[0, 1],
                       q[0, 1] * q[0, 2] / (q[0, 0] * q[1, 2]), q[0, 1] * q[1, 2] / (q[1, 1] * q[0, 2]), q[0, 2] * q[1, 2] / (q[2, 2] * q[0, 1]),
                       q[1, 2] / q[0, 2], q[1, 2] / q[0, 1]])
        st[:, ~((q[0, 1] > 0) & (q[0, 2] > 0) & (q[1, 2] > 0))] = np.nan
        np.nanmean(st, axis=1), np.nanstd(st, axis=1, ddof=1), np.nanquantile(st, Q3, axis=1)
    return time.perf_counter() - t_start


def stage_share(fn):
    """(share of the sort and summary kernels, {kernel: ms}) of one call, from the profiler's device times; None if it has none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        t = {"replicates": 0.0, "quantiles": 0.0, "moments": 0.0}
        for ev in prof.key_averages():
            us = getattr(ev, "device_time_total", None)
            us = getattr(ev, "cuda_time_total", 0.0) if us is None else us
            for key, word in (("replicates", "tc_replicate"), ("quantiles", "tc_quantile"), ("moments", "MomentBody")):
                if word in ev.key:
                    t[key] += us / 1e3
        total = sum(t.values())
        return (None, t) if total <= 0.0 else ((t["quantiles"] + t["moments"]) / total, t)
    except Exception as e:                                            # the table still stands without this column
        return None, {"error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    T, M = SHAPE[0], SHAPE[1] * SHAPE[2]
    t64 = torch.randn((T, M), device=dev, dtype=torch.float64, generator=gen)
    for k in range(1, T):                                             # AR(1), coefficient 0.6
        t64[k] = 0.6 * t64[k - 1] + 0.8 * t64[k]
    x64 = 5.0 + t64 + 0.3 * torch.randn((T, M), device=dev, dtype=torch.float64, generator=gen)
    y64 = -2.0 + 0.8 * t64 + 0.4 * torch.randn((T, M), device=dev, dtype=torch.float64, generator=gen)
    z64 = 1.3 * t64 + 0.5 * torch.randn((T, M), device=dev, dtype=torch.float64, generator=gen)
    x64[torch.rand((T, M), device=dev, generator=gen) < 0.02] = float("nan")
    del t64
    tables = {B: torch.from_numpy(bootstrap_indices(T, B, 6)).to(dev) for B in (100, 1000)}
    rows, shares = [], []
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        x, y, z = x64.to(dtype), y64.to(dtype), z64.to(dtype)
        cube = x.numel() * x.element_size()
        rows.append((f"gd_tc_estimate {tag} (two reads of three cubes)", (lambda x=x, y=y, z=z: K.tc_estimate(x, y, z)), 6 * cube, 0))
        rows.append((f"gd_augment_d4 op 0, the bytes of six {tag} cube reads (yardstick)", *yardstick(6 * cube, dev), 0))
        for B, idx in tables.items():
            ws = torch.empty(max(min(K.tc_bootstrap_workspace(T, M, B), 1 << 28), K.tc_bootstrap_min_workspace(T, B)), device=dev, dtype=torch.uint8)
            fn = (lambda x=x, y=y, z=z, idx=idx, ws=ws: K.tc_bootstrap(x, y, z, idx, Q3, ws=ws))
            rows.append((f"gd_tc_bootstrap {tag}, B = {B}, block 6, 256 MiB workspace", fn, 3 * cube, T * B * M))
            shares.append((f"gd_tc_bootstrap {tag}, B = {B}", fn))
    res = median_ms([fn for _, fn, _, _ in rows], args.rounds, args.calls)
    lines = [f"tools/tcol_bench.py on {torch.cuda.get_device_name(0)}: triple collocation of three {SHAPE} cubes (2 % NaN in x); {args.rounds} "
             f"rounds x {args.calls} calls each, alternating, HIP events; a call includes its allocations (the bootstrap workspace is reused)",
             "no speed threshold was set in advance; GB/s = the cube bytes the algorithm reads (the yardstick: read + write) over the median"]
    med_of = {}
    for (name, _, nbytes, triplets), (med, bst) in zip(rows, res):
        line = f"{name:72s} median {med:9.3f} ms  best {bst:9.3f} ms  {nbytes / 1e6:8.0f} MB  {nbytes / med / 1e6:8.1f} GB/s"
        if triplets:
            line += f"  {triplets / med / 1e6:8.2f} G triplets/s"
        lines.append(line)
        med_of[name] = med
    for tag in ("fp64", "fp32"):
        e, yd = med_of[f"gd_tc_estimate {tag} (two reads of three cubes)"], med_of[f"gd_augment_d4 op 0, the bytes of six {tag} cube reads (yardstick)"]
        lines.append(f"gd_tc_estimate {tag} over its yardstick: {e / yd:5.2f}x")
    for name, fn in shares:
        share, t = stage_share(fn)
        detail = ", ".join(f"{k} {v:9.3f} ms" if isinstance(v, float) else f"{k} {v}" for k, v in t.items())
        lines.append(f"{name}: sort and summary share of the device time {'not measured' if share is None else f'{100 * share:5.1f} %'} ({detail})")
    xn, yn, zn = (c[:, :SHAPE[2]].cpu().numpy() for c in (x64, y64, z64))
    sec = numpy_row_seconds(xn, yn, zn, tables[100].cpu().numpy())
    lines.append(f"numpy on the host, fp64, B = 100: {sec:7.2f} s for one row of {SHAPE[2]} pixels, {sec * SHAPE[1]:8.0f} s extrapolated to the cube, "
                 f"{sec * SHAPE[1] * 10:8.0f} s to B = 1000")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
