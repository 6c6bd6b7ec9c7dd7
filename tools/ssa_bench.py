"""HIP-event medians of the SSA module (gan_danet_amd/ssa.py) on the product's own shape, a synthetic (181, 440, 900) cube
(trend + annual + semi-annual + noise), fp64 and fp32 storage: ssa_decompose at window 24, 6 components, without and with
the reconstructed components, and ssa_fill at window 24, rank 4 over the GRACE gap pattern (11 consecutive steps plus 20
scattered single steps, the same steps in every pixel).  Each is set next to mann_kendall on the same cube and next to the
project's one-read-one-write yardstick, gd_augment_d4 with op word 0, on the bytes of one cube read.  Where the time goes is
estimated by differences: the "vg" method forms the covariance from 24 lagged sums where "bk" forms 300 entries, so
bk - vg is (almost all of) the covariance IF both matrices take the same Jacobi work -- the mean number of sweeps of both
runs is printed beside the split so that this can be judged; components - no components is the reconstruction with its
(6, T, ...) write; the rest is the Jacobi sweeps.  The split is an estimate, not a measurement of the phases.  For scale, numpy on the host
(numpy.linalg.eigh per series and iteration) over one row of the same series, extrapolated to the cube.  No speed threshold was set in advance.  --out writes the table to a file
(profiles/r32_ssa.txt).

    python tools/ssa_bench.py [--rounds 3] [--out profiles/r32_ssa.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import ssa as S  # noqa: E402
from gan_danet_amd import trend as TR  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import SHAPE, yardstick  # noqa: E402

WINDOW, COMPONENTS, RANK = 24, 6, 4


def gap_steps(t_len):
    """the GRACE pattern: 11 consecutive steps and 20 scattered single steps"""
    rng = np.random.default_rng(0)
    a = int(0.6 * t_len)
    rest = np.setdiff1d(np.arange(t_len), np.arange(a - 1, a + 12))
    return np.sort(np.concatenate((np.arange(a, a + 11), rng.choice(rest, size=20, replace=False))))


def host_solve(y, m, q):
    k = y.size - m + 1
    x = np.lib.stride_tricks.sliding_window_view(y, k).T          # (K, M)
    w, e = np.linalg.eigh(x.T @ x / k)
    e = e[:, ::-1][:, :q]
    pc = x @ e
    out = np.zeros(y.size)
    cnt = np.zeros(y.size)
    for j in range(m):
        out[j:j + k] += pc @ e[j]
        cnt[j:j + k] += 1
    return out / cnt


def host_fill(col, m, rank, tol=1e-3, max_iter=20):
    gap = np.isnan(col)
    mean, sd = col[~gap].mean(), col[~gap].std()
    y = np.where(gap, 0.0, col - mean)
    for q in range(1, rank + 1):
        for _ in range(max_iter):
            r = host_solve(y, m, q)
            change = np.abs(r[gap] - y[gap]).max()
            y[gap] = r[gap]
            if change <= tol * sd:
                break
    return mean + y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(SHAPE[0], device=dev, dtype=torch.float64)[:, None, None]
    phase = 6.0 * torch.rand(SHAPE[1:], device=dev, dtype=torch.float64, generator=gen)[None]
    cube64 = 0.01 * t + torch.sin(2 * torch.pi * t / 12 + phase) + 0.4 * torch.cos(2 * torch.pi * t / 6 + phase) \
        + 0.3 * torch.randn(SHAPE, device=dev, dtype=torch.float64, generator=gen) + 2.0
    steps = torch.from_numpy(gap_steps(SHAPE[0])).to(dev)
    m = SHAPE[1] * SHAPE[2]
    rows, last = [], {}
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        x = cube64.to(dtype)
        gappy = x.clone()
        gappy[steps] = float("nan")
        cube = x.numel() * x.element_size()

        def fill(g=gappy, tag=tag):
            last[tag] = S.ssa_fill(g, WINDOW, RANK)

        def dec(method, x=x, tag=tag):
            last[tag, method] = S.ssa_decompose(x, WINDOW, COMPONENTS, method=method)

        rows.append((f"ssa_decompose bk, no components {tag}", lambda dec=dec: dec("bk")))
        rows.append((f"ssa_decompose vg, no components {tag}", lambda dec=dec: dec("vg")))
        rows.append((f"ssa_decompose bk, with components {tag}", lambda x=x: S.ssa_decompose(x, WINDOW, COMPONENTS, components=True)))
        rows.append((f"ssa_fill bk, rank {RANK}, GRACE gaps {tag}", fill))
        rows.append((f"mann_kendall {tag} (yardstick: r19_trend)", lambda x=x: TR.mann_kendall(x)))
        rows.append((f"gd_augment_d4 op 0, the bytes of one {tag} cube read", yardstick(cube, dev)[0]))
    res = median_ms([fn for _, fn in rows], args.rounds, 1)
    lines = [f"tools/ssa_bench.py on {torch.cuda.get_device_name(0)}: SSA of the {m} series of a {SHAPE} cube, window {WINDOW}; "
             f"{args.rounds} rounds x 1 call each, alternating, HIP events; a call includes its allocations",
             "no speed threshold was set in advance"]
    med = {}
    for (name, _), (md, best) in zip(rows, res):
        med[name] = md
        lines.append(f"{name:56s} median {md:10.3f} ms  best {best:10.3f} ms")
    for tag in ("fp64", "fp32"):
        bk, vg, rc = (med[f"ssa_decompose {k} {tag}"] for k in ("bk, no components", "vg, no components", "bk, with components"))
        f = last[tag]
        it = f.iterations.double()
        lines.append(f"{tag}: by differences, of ssa_decompose with components: covariance {100 * (bk - vg) / rc:5.1f} %, reconstruction and its write "
                     f"{100 * (rc - bk) / rc:5.1f} %, Jacobi sweeps and the rest {100 * vg / rc:5.1f} %; mean sweeps per series: bk "
                     f"{last[tag, 'bk'].sweeps.mean().item():.2f}, vg {last[tag, 'vg'].sweeps.mean().item():.2f} (max {int(last[tag, 'bk'].sweeps.max().item())}, "
                     f"{int(last[tag, 'vg'].sweeps.max().item())})")
        fl = med[f"ssa_fill bk, rank {RANK}, GRACE gaps {tag}"]
        lines.append(f"{tag}: ssa_fill ran {it.mean().item():.1f} iterations per pixel (max {int(it.max().item())}), {100 * f.converged.double().mean().item():.1f} % of the "
                     f"pixels converged in every stage; {fl / it.mean().item():.2f} ms per iteration of the cube; ratio to mann_kendall "
                     f"{fl / med[f'mann_kendall {tag} (yardstick: r19_trend)']:.0f}, ssa_decompose bk without components {bk / med[f'mann_kendall {tag} (yardstick: r19_trend)']:.1f}")
    host = cube64[:, 0, :64].cpu().numpy()
    t0 = time.perf_counter()
    for k in range(host.shape[1]):
        host_solve(host[:, k] - host[:, k].mean(), WINDOW, COMPONENTS)
    per_dec = (time.perf_counter() - t0) / host.shape[1]
    hg = host[:, :16].copy()
    hg[gap_steps(SHAPE[0])] = np.nan
    t0 = time.perf_counter()
    for k in range(hg.shape[1]):
        host_fill(hg[:, k], WINDOW, RANK)
    per_fill = (time.perf_counter() - t0) / hg.shape[1]
    lines.append(f"numpy on the host (eigh), 64 / 16 of the same series: decompose {per_dec * 1e3:.3f} ms per series = {per_dec * m:.0f} s for the cube; "
                 f"fill {per_fill * 1e3:.2f} ms per series = {per_fill * m:.0f} s for the cube")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
