"""HIP-event medians of the fractions skill score (gan_danet_amd/neighborhood.py, csrc/neighborhood.hip) on the product's own
shape: two (181, 440, 900) cubes -- a smoothed random field and a displaced, noisier copy of it -- the five DSI class
thresholds and the scales 1, 3, 5, 9, 17, 33, 65, 129, in fp64 and fp32 storage.  Timed apart, through the C entry with a
preallocated workspace: the call with the one scale n = 1 (the table build and a single scoring pass), the call with all
eight scales (the difference is seven further scoring passes), the same with maps, normalize="valid", and the fraction field
of one cube.  All alternate with the project's one-read-one-write yardstick, gd_augment_d4 with op word 0, on an fp32 tensor
of the bytes of the two cubes.  A torch implementation (int64 cumsum tables, clipped index gathers) is timed once with its
peak memory and must give the same integers; scipy.ndimage.correlate on the host is timed for one step, one threshold and
n = 9, for scale.  No speed threshold was set in advance.  --out writes the table to a file (profiles/r26_neighborhood.txt).

    python tools/neighborhood_bench.py [--rounds 5] [--calls 1] [--out profiles/r26_neighborhood.txt]
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
from gan_danet_amd.drought import DSI_CLASSES  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import SHAPE, yardstick  # noqa: E402

SCALES = (1, 3, 5, 9, 17, 33, 65, 129)


def cubes(dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn((1, 1) + SHAPE, device=dev, generator=gen)
    for _ in range(3):                                       # three box passes: close to a Gaussian of a few pixels
        z = torch.nn.functional.avg_pool3d(z, (3, 9, 9), stride=1, padding=(1, 4, 4), count_include_pad=False)
    z = ((z - z.mean()) / z.std()).reshape(SHAPE).to(torch.float64)
    o = z.contiguous()
    f = (0.9 * torch.roll(z, (3, 5), dims=(1, 2)) + 0.3 * torch.randn(SHAPE, device=dev, generator=gen, dtype=torch.float64)).contiguous()
    return f, o


def torch_fss(f, o, thresholds, scales):
    """the window-mode records with torch alone: int64 summed-area tables by cumsum, windows by clipped index gathers"""
    T, H, W = f.shape
    valid = ~(torch.isnan(f) | torch.isnan(o))
    sums = torch.zeros((T, len(thresholds), len(scales), 3), dtype=torch.int64, device=f.device)
    rows, cols = torch.arange(H, device=f.device), torch.arange(W, device=f.device)

    def table(ind):
        return torch.nn.functional.pad(ind.to(torch.int64).cumsum(1).cumsum(2), (1, 0, 1, 0))

    for k, thr in enumerate(thresholds):
        sf, so = table(valid & (f <= thr)), table(valid & (o <= thr))
        for s, n in enumerate(scales):
            h = n // 2
            r0, r1, c0, c1 = (rows - h).clamp(min=0), (rows + h + 1).clamp(max=H), (cols - h).clamp(min=0), (cols + h + 1).clamp(max=W)
            win = lambda t: t[:, r1][:, :, c1] - t[:, r0][:, :, c1] - t[:, r1][:, :, c0] + t[:, r0][:, :, c0]   # noqa: E731
            cf, co = win(sf) * valid, win(so) * valid
            sums[:, k, s, 0] = ((cf - co) ** 2).sum((1, 2))
            sums[:, k, s, 1] = (cf * cf).sum((1, 2))
            sums[:, k, s, 2] = (co * co).sum((1, 2))
    return sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-reference", action="store_true", help="skip the torch and scipy implementations")
    args = ap.parse_args()
    dev = torch.device("cuda")
    T, H, W = SHAPE
    n = T * H * W
    thr = np.array([DSI_CLASSES] * T)
    windows = n * len(DSI_CLASSES) * len(SCALES)
    f64, o64 = cubes(dev)
    planes = max(1, min(T, K.NBR_WS_BUDGET // K.nbr_ws_bytes(H, W, len(DSI_CLASSES), 1)))
    ws = torch.empty(K.nbr_ws_bytes(H, W, len(DSI_CLASSES), planes), device=dev, dtype=torch.uint8)
    lines = [f"tools/neighborhood_bench.py on {torch.cuda.get_device_name(0)}: fractions skill score of two {SHAPE} cubes ({n / 1e6:.1f} M voxels "
             f"each), thresholds {DSI_CLASSES}, scales {SCALES}: {windows / 1e9:.2f} G windows; {args.rounds} rounds x {args.calls} calls "
             f"each, alternating, HIP events; workspace preallocated ({ws.numel() / 2 ** 20:.0f} MiB, {planes} steps in flight)",
             "no speed threshold was set in advance; yardstick = gd_augment_d4 op 0 moving the bytes of one read and one write of both "
             "cubes as fp32; Gwin/s = windows (voxels x thresholds x scales of the call) over the median"]
    print("\n".join(lines), flush=True)
    for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        done = len(lines)
        f, o = f64.to(dtype), o64.to(dtype)
        call = lambda sc, **kw: K.nbr_fss(f, o, thr, thr, sc, ws=ws, **kw)      # noqa: E731
        yard, _ = yardstick(2 * 2 * n * 4, dev)
        rows = [("gd_augment_d4 op 0 (yardstick)", yard, 0),
                ("gd_nbr_fss, scale 1 only: tables + one scoring pass", lambda: call((1,)), 1),
                ("gd_nbr_fss, all 8 scales", lambda: call(SCALES), 8),
                ("gd_nbr_fss, all 8 scales, maps", lambda: call(SCALES, maps=True), 8),
                ("gd_nbr_fss, all 8 scales, normalize=valid", lambda: call(SCALES, normalize="valid"), 8),
                ("gd_nbr_fss, all 8 scales, normalize=valid, maps", lambda: call(SCALES, normalize="valid", maps=True), 8),
                ("gd_nbr_fraction, one cube, n = 9", lambda: K.nbr_fraction(f, DSI_CLASSES[1], 9, ws=ws), 0)]
        res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
        lines.append(f"-- {tag} storage")
        base = res[0][0]
        for (nm, _, ns), (med, best) in zip(rows, res):
            rate = f"{n * len(DSI_CLASSES) * ns / med / 1e6:8.2f} Gwin/s" if ns else " " * 15
            lines.append(f"{nm:56s} median {med:9.3f} ms  best {best:9.3f} ms  {rate}  {med / base:7.2f} x the yardstick")
        lines.append(f"{'seven further scales (8 scales - scale 1 only)':56s} {res[2][0] - res[1][0]:16.3f} ms  "
                     f"{(res[2][0] - res[1][0]) / 7:9.3f} ms per scale;  maps add {res[3][0] - res[2][0]:9.3f} ms")
        if not args.no_reference:
            sums, _, _ = call(SCALES)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ref = torch_fss(f, o, DSI_CLASSES, SCALES)
            e1.record()
            e1.synchronize()
            peak = torch.cuda.max_memory_allocated() - before
            assert torch.equal(ref, sums), "the torch implementation and gd_nbr_fss disagree"
            lines.append(f"{'torch: int64 cumsum tables + index gathers (one call)':56s} {e0.elapsed_time(e1):16.1f} ms  peak {peak / 2 ** 20:9.0f} MiB "
                         f"of temporaries; the same integers")
            del ref
        print("\n".join(lines[done:]), flush=True)
        del f, o
    if not args.no_reference:
        from scipy import ndimage
        ind = (o64[0] <= DSI_CLASSES[1]).cpu().numpy().astype(np.int64)
        t0 = time.perf_counter()
        for _ in range(3):      # cf, co, cv
            ndimage.correlate(ind, np.ones((9, 9), dtype=np.int64), mode="constant")
        dt = (time.perf_counter() - t0) * 1e3
        lines.append(f"{'scipy.ndimage.correlate, host: 1 step, 1 threshold, n = 9':56s} {dt:16.1f} ms  (x {T * len(DSI_CLASSES)} for the cube at this "
                     f"one scale)")
        print(lines[-1], flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
