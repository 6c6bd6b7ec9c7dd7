"""HIP-event medians of the change-point module (gan_danet_amd/changepoint.py) on the product's own shape, a synthetic
(181, 440, 900) cube with a planted shift in every series, fp64 and fp32: pettitt alone, all four families of change_point,
and change_points(max_breaks=3, method="pettitt").  Each is set next to mann_kendall on the same cube (the same kind of
O(T^2) sweep per series: the yardstick of profiles/r19_trend.txt) and next to the project's one-read-one-write yardstick,
gd_augment_d4 with op word 0, on the bytes of one cube read.  For scale, a numpy loop on the host over one row of the same
series (all four families, vectorised over the candidates), extrapolated to the cube.  No speed threshold was set in
advance.  --out writes the table to a file (profiles/r31_changepoint.txt).

    python tools/changepoint_bench.py [--rounds 5] [--calls 1] [--out profiles/r31_changepoint.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import changepoint as CP  # noqa: E402
from gan_danet_amd import trend as TR  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import SHAPE, yardstick  # noqa: E402


def host_one(y, t, min_seg=5):
    """all four families of one series in numpy (float64, candidates vectorised): what a user's host loop would run"""
    n = y.size
    u = np.cumsum(np.sign(y[:, None] - y[None, :]).sum(1))[:n - 1]
    k = np.argmax(np.abs(u))
    d = y - y.mean()
    s = np.cumsum(d)
    q = np.abs(s).max() / np.sqrt((d * d).mean()) / np.sqrt(n)
    ks = np.arange(min_seg - 1, n - min_seg)
    before = np.arange(n)[None, :] <= ks[:, None]
    out = [u[k], q]
    for fit_line in (False, True):
        rss = 0.0
        for w in (before, ~before):
            c = w.sum(1)
            yb = (w * y).sum(1) / c
            dy = (y[None, :] - yb[:, None]) * w
            if fit_line:
                tb = (w * t).sum(1) / c
                dt = (t[None, :] - tb[:, None]) * w
                dy = dy - ((dt * dy).sum(1) / (dt * dt).sum(1))[:, None] * dt
            rss = rss + (dy * dy).sum(1)
        out.append(ks[np.argmin(rss)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(SHAPE[0], device=dev, dtype=torch.float64)[:, None, None]
    at = torch.randint(40, 140, SHAPE[1:], device=dev, generator=gen)[None]
    cube64 = 0.3 * torch.randn(SHAPE, device=dev, dtype=torch.float64, generator=gen) + (t > at) * 1.0 + 2.0
    m = SHAPE[1] * SHAPE[2]
    rows = []
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        x = cube64.to(dtype)
        cube = x.numel() * x.element_size()
        rows.append((f"pettitt {tag}", lambda x=x: CP.pettitt(x)))
        rows.append((f"change_point, all four families {tag}", lambda x=x: CP.change_point(x)))
        rows.append((f"change_points max_breaks=3 pettitt {tag}", lambda x=x: CP.change_points(x, max_breaks=3)))
        rows.append((f"mann_kendall {tag} (yardstick: r19_trend)", lambda x=x: TR.mann_kendall(x)))
        rows.append((f"gd_augment_d4 op 0, the bytes of one {tag} cube read", yardstick(cube, dev)[0]))
    res = median_ms([fn for _, fn in rows], args.rounds, args.calls)
    lines = [f"tools/changepoint_bench.py on {torch.cuda.get_device_name(0)}: change points of the {m} series of a {SHAPE} cube; "
             f"{args.rounds} rounds x {args.calls} calls each, alternating, HIP events; a call includes its allocations and the upload of the times",
             "no speed threshold was set in advance; mann_kendall (4.9 ms in profiles/r19_trend.txt) is the same kind of O(T^2) sweep per series"]
    med_of = {}
    for (name, _), (med, best) in zip(rows, res):
        med_of[name] = med
        lines.append(f"{name:56s} median {med:9.3f} ms  best {best:9.3f} ms")
    for tag in ("fp64", "fp32"):
        mk = med_of[f"mann_kendall {tag} (yardstick: r19_trend)"]
        lines.append(f"ratio to mann_kendall {tag}: pettitt {med_of[f'pettitt {tag}'] / mk:6.2f}, all four families "
                     f"{med_of[f'change_point, all four families {tag}'] / mk:6.2f}, change_points {med_of[f'change_points max_breaks=3 pettitt {tag}'] / mk:6.2f}")
    host = cube64[:, 0, :].cpu().numpy()
    tt = np.arange(SHAPE[0], dtype=np.float64)
    t0 = time.perf_counter()
    for k in range(host.shape[1]):
        host_one(host[:, k], tt)
    per = (time.perf_counter() - t0) / host.shape[1]
    lines.append(f"numpy on the host, all four families, one row of {host.shape[1]} of the same series: {per * 1e3:.3f} ms per series = "
                 f"{per * m:.0f} s for the cube")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
