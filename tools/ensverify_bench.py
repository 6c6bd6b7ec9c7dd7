"""HIP-event medians of gd_ens_verify -- record only, and with all four maps -- against gd_ensemble_stats on the same slab
as the yardstick, interleaved in one process: M = 5 on (5, 8, 1, 1024, 1024) fp32 (the 8-member instantiation) and M = 32 on
(32, 2, 1, 1024, 1024) (the 32-member one).  Prints ms, GB/s of the bytes that must move and the ratio to the yardstick; no
pass threshold.  profiles/r21_ensverify.txt holds a run.

    python tools/ensverify_bench.py [--iters 25] [--out profiles/r21_ensverify.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import _lib as L  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402
from eval_bench import median_ms  # noqa: E402


def rows_for(M, B, dev, g):
    slab = torch.randn((M, B, 1, 1024, 1024), device=dev, generator=g)
    truth = slab.mean(0) + 0.5 * torch.randn((B, 1, 1024, 1024), device=dev, generator=g)
    n = truth.numel()
    mean, std = torch.empty_like(truth), torch.empty_like(truth)
    crps, err, spread = torch.empty_like(truth), torch.empty_like(truth), torch.empty_like(truth)
    rank = torch.empty(truth.shape, dtype=torch.uint8, device=dev)
    rec = torch.zeros(L.ENSV_REC, dtype=torch.float64, device=dev)
    return [(f"gd_ensemble_stats M={M} (yardstick)", lambda: K.ensemble_stats(slab, mean, std), (M + 2) * n * 4),
            (f"gd_ens_verify M={M} record only", lambda: K.ens_verify(slab, truth, rec), (M + 1) * n * 4),
            (f"gd_ens_verify M={M} all maps", lambda: K.ens_verify(slab, truth, rec, None, 1.0, False, crps, err, spread, rank),
             (M + 1) * n * 4 + 3 * n * 4 + n)], (slab, truth, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25, help="rounds; every round times 20 calls of each kernel")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"device {torch.cuda.get_device_name(0)}; fp32 slabs (M, B, 1, 1024, 1024); {args.iters} rounds x 20 calls each, alternating, "
             "HIP events (a call = its launches); GB/s of the bytes that must move"]
    for M, B in ((5, 8), (32, 2)):
        rows, (slab, truth, rec) = rows_for(M, B, dev, g)
        res = median_ms([fn for _, fn, _ in rows], args.iters)
        base = rows[0][2] / res[0][0]
        for (name, _, nb), (med, best) in zip(rows, res):
            lines.append(f"{name:38s} median {med:8.4f} ms  best {best:8.4f} ms  {nb / 1e6:7.1f} MB  {nb / med / 1e6:8.1f} GB/s"
                         f"  rate x{nb / med / base:5.2f} of the yardstick")
        K.ens_verify(slab, truth, rec)
        m = K.ens_verify_merge_host(rec.cpu().numpy(), M)[1]
        lines.append(f"check M={M}: n {m['n']:.0f}  crps {m['crps']:.6f}  crps_gauss {m['crps_gauss']:.6f}  mae {m['mae']:.6f}  "
                     f"spread_skill {m['spread_skill']:.4f}  reliability {m['reliability']:.4f}  coverage {[round(v, 4) for v in m['coverage'].values()]}")
        del rows, slab, truth
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
