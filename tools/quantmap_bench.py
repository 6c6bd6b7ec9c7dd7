"""HIP-event medians of the bias-correction module (gan_danet_amd/biascorrect.py, csrc/quantmap.hip) on the product's own
shapes: a (181, 440, 900) cube against an (181, 88, 180) table grid (f = 5), fp64 and fp32 storage, 51 nodes:

* QuantileMap.fit at period 12 on the table grid (two gd_qm_quantiles, register route, 15 or 16 samples per slot: each
  reads both cubes and writes one table; counted: both cubes once and both tables);
* series_quantiles at period 1 on the table grid (gd_qm_quantiles, LDS route, 181 samples: reads the cube, writes 5 planes);
* QuantileMap.apply "eqm" on the fine cube (gd_qm_apply: reads and writes the cube, reads both tables);
* QuantileMap.apply "qdm" on the fine cube (gd_qm_quantiles of the cube itself on its own grid, which writes a
  (12, 51, 440, 900) table, then gd_qm_apply, which reads it back), and that own-table pass alone.

All alternate with the project's one-read-one-write yardstick, gd_augment_d4 with op word 0, on fp32 tensors that move
about the same bytes.  GB/s are the bytes a step must move (as listed) over the median; the ratio is that rate over the
yardstick's.  For scale, the numpy oracle of tests/quantmap_util.py runs the fit and the eqm apply on the host for one row
of table pixels and is extrapolated to the grid.  No speed threshold was set in advance.  --out writes the table to a file
(profiles/r27_quantmap.txt).

    python tools/quantmap_bench.py [--rounds 5] [--calls 2] [--out profiles/r27_quantmap.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gan_danet_amd as gd  # noqa: E402
import quantmap_util as U  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import SHAPE, yardstick  # noqa: E402

F, Q, PERIOD = 5, 51, 12
ORACLE_PIXELS = 20


def host_oracle(model, obs, x):
    """seconds of the numpy oracle: (the fit of one row of table pixels, the eqm apply of the fine pixels over the first
    ORACLE_PIXELS of them)"""
    T, W = model.shape
    t0 = time.perf_counter()
    mq, oq, _, _ = U.fit(model, obs, Q, PERIOD)
    t1 = time.perf_counter()
    n = ORACLE_PIXELS
    U.apply(x[:, :, :n * F], mq[:, :, :n].reshape(PERIOD, Q, 1, n).copy(), oq[:, :, :n].reshape(PERIOD, Q, 1, n).copy(), "eqm")
    return t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    T, Hx, Wx = SHAPE
    H, W = Hx // F, Wx // F
    t = torch.arange(T, device=dev, dtype=torch.float64)[:, None, None]
    season = torch.sin(2 * torch.pi * t / 12)
    fine64 = season * 8.0 + torch.randn(SHAPE, device=dev, dtype=torch.float64, generator=gen).cumsum(0) * 0.6
    obs64 = season * 10.0 + 1.5 + torch.randn((T, H, W), device=dev, dtype=torch.float64, generator=gen).cumsum(0) * 0.8
    obs64[::17, ::2, ::3] = float("nan")                            # GRACE's missing months, on a sixth of the pixels
    rows = []
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        fine, obs = fine64.to(dtype), obs64.to(dtype)
        model = gd.timeseries.coarsen(fine, (F, F))
        qm = gd.QuantileMap.fit(model, obs, n_quantiles=Q, period=PERIOD)
        out = torch.empty_like(fine)
        cube, small = fine.numel() * fine.element_size(), model.numel() * model.element_size()
        tables = 2 * qm.model_q.numel() * 8
        own = PERIOD * Q * Hx * Wx * 8
        pd = torch.from_numpy(qm.p).to(dev)
        x2 = fine.reshape(T, -1)
        steps = [
            (f"QuantileMap.fit period 12, {Q} nodes, table grid {tag}", lambda model=model, obs=obs: gd.QuantileMap.fit(model, obs, Q, PERIOD),
             2 * small + tables),
            (f"series_quantiles period 1, 5 probabilities, table grid {tag} (LDS route)",
             lambda model=model: gd.series_quantiles(model, (0.05, 0.25, 0.5, 0.75, 0.95)), small + 5 * H * W * 8),
            (f"QuantileMap.apply eqm, fine cube {tag}", lambda qm=qm, fine=fine, out=out: qm.apply(fine, "eqm", out=out), 2 * cube + tables),
            (f"own table of the fine cube {tag} (gd_qm_quantiles, {Q} nodes)",
             lambda x2=x2, pd=pd: gd.kern.qm_quantiles(x2, pd, PERIOD, layout=gd.kern.L.QM_LAYOUT_SQM), cube + own),
            (f"QuantileMap.apply qdm, fine cube {tag} (own table + apply)", lambda qm=qm, fine=fine, out=out: qm.apply(fine, "qdm", out=out),
             3 * cube + 2 * own + tables),
        ]
        for name, fn, nbytes in steps:
            rows.append((f"gd_augment_d4 op 0, {nbytes / 1e6:.0f} MB (yardstick)", *yardstick(nbytes, dev), None))
            rows.append((name, fn, nbytes, 0))
    res = median_ms([r[1] for r in rows], args.rounds, args.calls)
    lines = [f"tools/quantmap_bench.py on {torch.cuda.get_device_name(0)}: quantile mapping of a {SHAPE} cube against a {(T, H, W)} table grid, "
             f"{Q} nodes; {args.rounds} rounds x {args.calls} calls each, alternating, HIP events",
             "no speed threshold was set in advance; GB/s = the bytes the step must move over the median; ratio = that rate over the rate of "
             "the yardstick above it"]
    yard = 0.0
    for (name, _, nbytes, ref), (med, best) in zip(rows, res):
        rate = nbytes / med / 1e6
        if ref is None:
            yard, ratio = rate, ""
        else:
            ratio = f"  {rate / yard:5.2f} of the yardstick"
        lines.append(f"{name:82s} median {med:9.3f} ms  best {best:9.3f} ms  {nbytes / 1e6:8.0f} MB  {rate:8.1f} GB/s{ratio}")
    model = gd.timeseries.coarsen(fine64, (F, F))
    fit_s, apply_s = host_oracle(model[:, 0].cpu().numpy(), obs64[:, 0].cpu().numpy(), fine64[:, :F].cpu().numpy())
    lines.append(f"numpy oracle on the host: fit of one row of {W} table pixels {fit_s:.2f} s, eqm apply of the fine pixels over {ORACLE_PIXELS} "
                 f"table pixels {apply_s:.2f} s; extrapolated to the {H} x {W} grid: fit {fit_s * H:.0f} s, apply "
                 f"{apply_s * H * W / ORACLE_PIXELS:.0f} s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
