"""HIP-event medians of the trend module (gan_danet_amd/trend.py) on the product's own shape, a synthetic (181, 440, 900)
cube, fp64 and fp32: mann_kendall (the count sweep alone), sen_slope without and with the confidence interval (the radix
select on top of it), and the same three with period=12.  Pair evaluations per second: the pairs of the definition
(T (T - 1) / 2 per series, the within-season pairs in the seasonal form) over the median, whatever the number of sweeps
that looked at them.  For scale, the per-series time of scipy.stats.theilslopes on 200 of the same series on the host.  No
speed threshold was set in advance.  --out writes the table to a file (profiles/r19_trend.txt).

    python tools/trend_bench.py [--rounds 5] [--calls 1] [--out profiles/r19_trend.txt]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import trend as TR  # noqa: E402
from filters_bench import median_ms  # noqa: E402

SHAPE = (181, 440, 900)


def pairs(t_len, period):
    if not period:
        return t_len * (t_len - 1) // 2
    sizes = [len(range(s, t_len, period)) for s in range(period)]
    return sum(n * (n - 1) // 2 for n in sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(SHAPE[0], device=dev, dtype=torch.float64)[:, None, None]
    cube64 = 0.01 * t + torch.sin(2 * torch.pi * t / 12) + 0.3 * torch.randn(SHAPE, device=dev, dtype=torch.float64, generator=gen) + 2.0
    m = SHAPE[1] * SHAPE[2]
    rows = []
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        x = cube64.to(dtype)
        for period in (None, 12):
            ptag = "" if period is None else " period=12"
            rows.append((f"mann_kendall{ptag} {tag}", (lambda x=x, p=period: TR.mann_kendall(x, period=p)), period))
            rows.append((f"sen_slope ci=False{ptag} {tag}", (lambda x=x, p=period: TR.sen_slope(x, period=p, ci=False)), period))
            rows.append((f"sen_slope ci=True{ptag} {tag}", (lambda x=x, p=period: TR.sen_slope(x, period=p)), period))
    res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
    lines = [f"tools/trend_bench.py on {torch.cuda.get_device_name(0)}: Mann-Kendall / Theil-Sen of the {m} series of a {SHAPE} cube; "
             f"{args.rounds} rounds x {args.calls} calls each, alternating, HIP events; a call includes its allocations and the upload of the times",
             "no speed threshold was set in advance; Gpair/s = the pairs of the definition (16 290 per series, 1 275 with period=12) over the median"]
    for (name, _, period), (med, best) in zip(rows, res):
        lines.append(f"{name:40s} median {med:9.3f} ms  best {best:9.3f} ms  {pairs(SHAPE[0], period) * m / med / 1e6:9.2f} Gpair/s")
    ratio = {}
    for (name, _, _), (med, _) in zip(rows, res):
        ratio[name] = med
    for tag in ("fp64", "fp32"):
        for ptag in ("", " period=12"):
            mk = ratio[f"mann_kendall{ptag} {tag}"]
            lines.append(f"ratio to mann_kendall{ptag} {tag}: sen_slope ci=False {ratio[f'sen_slope ci=False{ptag} {tag}'] / mk:6.2f}, "
                         f"ci=True {ratio[f'sen_slope ci=True{ptag} {tag}'] / mk:6.2f}")
    try:
        from scipy import stats
        import numpy as np
        host = cube64[:, 0, :200].cpu().numpy()
        tt = np.arange(SHAPE[0], dtype=np.float64)
        t0 = time.perf_counter()
        for k in range(host.shape[1]):
            stats.theilslopes(host[:, k], tt, 0.95)
        per = (time.perf_counter() - t0) / host.shape[1]
        lines.append(f"scipy.stats.theilslopes on the host, 200 of the same series: {per * 1e3:.3f} ms per series = {per * m:.0f} s for the cube")
    except ImportError:
        lines.append("scipy is not installed: no host figure")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
