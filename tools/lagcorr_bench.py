"""HIP-event medians of the lagged-correlation kernels (csrc/lagcorr.hip) on two (181, 440, 900) cubes, fp64 and fp32 storage:
gd_lag_corr at the lags +-3, +-12 and +-64 with and without the curve, gd_series_acf at K = 12 and gd_corr_signif.  GB/s are
the cube bytes the algorithm needs (one read of each cube; the maps written are not counted) over the median.  Each row is
timed next to the project's one-read-one-write yardstick, gd_augment_d4 with op word 0 on an fp32 tensor sized to move the
same bytes, a torch implementation (one pass per lag over shifted views with a NaN mask; its peak memory is reported) and a
numpy loop over lags with pairwise deletion on the host, timed on one row of 900 pixels and extrapolated to the cube.
No speed threshold was set in advance.  --out writes the table to a file (profiles/r29_lagcorr.txt).

    python tools/lagcorr_bench.py [--rounds 5] [--calls 2] [--out profiles/r29_lagcorr.txt]
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
from filters_bench import median_ms  # noqa: E402
from series_bench import yardstick  # noqa: E402

SHAPE = (181, 440, 900)


def torch_lag_corr(a, b, lo, hi):
    """best |r| over the lags, one pass per lag over shifted, masked views (fp64 arithmetic)"""
    T = a.shape[0]
    best = torch.full(a.shape[1:], float("nan"), device=a.device, dtype=torch.float64)
    for l in range(lo, hi + 1):
        t0, t1 = max(0, -l), min(T, T - l)
        x, y = a[t0:t1].double(), b[t0 + l:t1 + l].double()
        ok = ~(torch.isnan(x) | torch.isnan(y))
        n = ok.sum(0).clamp(min=1)
        x, y = torch.where(ok, x, 0.0), torch.where(ok, y, 0.0)
        dx, dy = torch.where(ok, x - x.sum(0) / n, 0.0), torch.where(ok, y - y.sum(0) / n, 0.0)
        r = (dx * dy).sum(0) / torch.sqrt((dx * dx).sum(0) * (dy * dy).sum(0))
        best = torch.where(torch.isnan(best) | (r.abs() > best.abs()), r, best)
    return best


def numpy_row_seconds(a, b, lo, hi):
    """a numpy loop over lags and pixels with pairwise deletion, on one (T, 900) row"""
    t_start = time.perf_counter()
    T, M = a.shape
    for m in range(M):
        for l in range(lo, hi + 1):
            t0, t1 = max(0, -l), min(T, T - l)
            x, y = a[t0:t1, m], b[t0 + l:t1 + l, m]
            ok = ~(np.isnan(x) | np.isnan(y))
            if ok.sum() >= 3:
                np.corrcoef(x[ok], y[ok])
    return time.perf_counter() - t_start


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    T, M = SHAPE[0], SHAPE[1] * SHAPE[2]
    a64 = torch.randn((T, M), device=dev, dtype=torch.float64, generator=gen) + 2.0
    b64 = 0.6 * torch.randn((T, M), device=dev, dtype=torch.float64, generator=gen)
    b64[3:] += 0.8 * a64[:-3]
    a64[torch.rand((T, M), device=dev, generator=gen) < 0.02] = float("nan")
    rows, extra = [], []
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        a, b = a64.to(dtype), b64.to(dtype)
        cube = a.numel() * a.element_size()
        for lag in (3, 12, 64):
            rows.append((f"gd_lag_corr +-{lag} {tag}, best lag only", (lambda a=a, b=b, lag=lag: K.lag_corr(a, b, -lag, lag, curve=False)), 2 * cube))
            rows.append((f"gd_lag_corr +-{lag} {tag}, with the curve", (lambda a=a, b=b, lag=lag: K.lag_corr(a, b, -lag, lag)), 2 * cube))
        rows.append((f"gd_series_acf K = 12 standard {tag}", (lambda b=b: K.series_acf(b, 12)), cube))
        rows.append((f"gd_augment_d4 op 0, the bytes of two {tag} cube reads (yardstick)", *yardstick(2 * cube, dev)))
        rows.append((f"gd_augment_d4 op 0, the bytes of one {tag} cube read (yardstick)", *yardstick(cube, dev)))
        for lag in (3, 12):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            (med, best), = median_ms([lambda a=a, b=b, lag=lag: torch_lag_corr(a, b, -lag, lag)], 2, 1)
            extra.append(f"torch, one pass per lag, +-{lag} {tag}: median {med:9.3f} ms, peak memory above the inputs "
                         f"{(torch.cuda.max_memory_allocated() - base) / 2 ** 20:8.0f} MiB")
    r, n, best = K.lag_corr(a64, b64, -12, 12, curve=False)
    r1 = K.series_acf(b64, 1)[0][1]
    rows.append(("gd_corr_signif, 396 000 pixels", (lambda: K.corr_signif(best[1], best[2], r1, r1)), 4 * 8 * M))
    res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
    lines = [f"tools/lagcorr_bench.py on {torch.cuda.get_device_name(0)}: lagged correlation of two {SHAPE} cubes (2 % NaN in a); {args.rounds} "
             f"rounds x {args.calls} calls each, alternating, HIP events; a call includes its allocations",
             "no speed threshold was set in advance; GB/s = the cube bytes the algorithm reads (the yardstick: read + write) over the median"]
    for (name, _, nbytes), (med, bst) in zip(rows, res):
        lines.append(f"{name:72s} median {med:9.3f} ms  best {bst:9.3f} ms  {nbytes / 1e6:8.0f} MB  {nbytes / med / 1e6:8.1f} GB/s")
    lines += extra
    an, bn = a64[:, :SHAPE[2]].cpu().numpy(), b64[:, :SHAPE[2]].cpu().numpy()
    for lag in (3, 12):
        sec = numpy_row_seconds(an, bn, -lag, lag)
        lines.append(f"numpy on the host, a loop over lags and pixels, +-{lag} fp64: {sec:7.2f} s for one row of {SHAPE[2]} pixels, "
                     f"{sec * SHAPE[1]:8.0f} s extrapolated to the cube")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
