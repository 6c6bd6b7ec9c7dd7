"""HIP-event medians of the connected-component entries (gan_danet_amd/clusters.py, csrc/ccl.hip) on the product's own
shape, a (181, 440, 900) cube: a smoothed random field thresholded at the D1 class (-0.8) so that clusters have realistic
sizes, and the two extremes, an all-foreground cube (one giant cluster: every atomic of the tables goes to one root) and a
3-D checkerboard (under structure 1 every other voxel is a cluster of its own).  Structure 2 for the field and the full
cube, 1 for the checkerboard.  Timed apart: label with the LDS tile stage, label with the tile stage skipped (every union
in global memory -- the comparison the tile stage has to win), the size filter, relabel, the tables (bounds + offsets), and
the tracks + totals.  All alternate with the project's one-read-one-write yardstick, gd_augment_d4 with op word 0, on an
fp32 tensor of the bytes of the cube.  scipy.ndimage.label on the host is timed once per cube, for scale.  No speed
threshold was set in advance.  --out writes the table to a file (profiles/r25_clusters.txt).

    python tools/clusters_bench.py [--rounds 5] [--calls 1] [--out profiles/r25_clusters.txt]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import clusters as C  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402
from filters_bench import median_ms  # noqa: E402
from series_bench import SHAPE, yardstick  # noqa: E402


def cubes(dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn((1, 1) + SHAPE, device=dev, generator=gen)
    for _ in range(3):                                       # three box passes: close to a Gaussian of a few pixels
        z = torch.nn.functional.avg_pool3d(z, (3, 9, 9), stride=1, padding=(1, 4, 4), count_include_pad=False)
    z = ((z - z.mean()) / z.std()).reshape(SHAPE).contiguous()
    t, h, w = torch.meshgrid(*(torch.arange(n, device=dev) for n in SHAPE), indexing="ij")
    return (("smoothed field <= -0.8 (D1), fp32", z, -0.8, 2), ("all foreground, uint8", torch.ones(SHAPE, device=dev, dtype=torch.uint8), 0.0, 2),
            ("3-D checkerboard, uint8", ((t + h + w) % 2 == 0).to(torch.uint8).contiguous(), 0.0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1, help="back-to-back calls inside one pair of events")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    lines = [f"tools/clusters_bench.py on {torch.cuda.get_device_name(0)}: connected components of a {SHAPE} cube ({n / 1e6:.1f} M voxels); "
             f"{args.rounds} rounds x {args.calls} calls each, alternating, HIP events; outputs and workspaces preallocated",
             "no speed threshold was set in advance; Mvox/s = the voxels of the cube over the median; yardstick = gd_augment_d4 op 0 moving "
             "the bytes of one read and one write of an fp32 cube"]
    print("\n".join(lines), flush=True)
    for name, x, thr, structure in cubes(dev):
        done = len(lines)
        word = C.structure_word(structure)
        values = x.dtype != torch.uint8
        parent = K.ccl_label(x, thr, word)
        flat = K.ccl_label(x, thr, word, tiles=False)
        assert torch.equal(parent, flat), "the tile stage and the global-only pass disagree"
        ws = torch.empty(K.lib().gd_ccl_ws_bytes(n), device=dev, dtype=torch.uint8)
        labels, count = K.ccl_relabel(parent, ws=ws)
        k = int(count.item())
        bounds = K.ccl_bounds(labels, k)
        offsets = K.ccl_offsets(bounds)
        records = int(offsets[-1].item())
        scratch = parent.clone()
        kws = torch.empty(K.lib().gd_ccl_ws_bytes(k), device=dev, dtype=torch.uint8)
        tracks, _ = K.ccl_tracks(x if values else None, labels, bounds, offsets, records, thr, None, values)
        totals = K.ccl_totals(tracks, bounds, offsets)

        def tables():
            K.ccl_bounds(labels, k, out=bounds)
            K.ccl_offsets(bounds, out=offsets, ws=kws)

        def track_pass():
            t, _ = K.ccl_tracks(x if values else None, labels, bounds, offsets, records, thr, None, values)
            K.ccl_totals(t, bounds, offsets, out=totals)

        yard, _ = yardstick(2 * n * 4, dev)
        rows = [("gd_augment_d4 op 0 (yardstick)", yard),
                ("gd_ccl_label, LDS tiles + border unions + flatten", lambda: K.ccl_label(x, thr, word, out=scratch)),
                ("gd_ccl_label, GD_CCL_NO_TILES: global union-find only", lambda: K.ccl_label(x, thr, word, tiles=False, out=scratch)),
                ("gd_ccl_filter min_size 2 (count + drop)", lambda: K.ccl_filter(scratch, 2, ws)),
                ("gd_ccl_relabel (flag, 3-pass scan, labels)", lambda: K.ccl_relabel(parent, out=labels, count=count, ws=ws)),
                ("tables: gd_ccl_bounds + gd_ccl_offsets", tables),
                ("tracks: gd_ccl_tracks + gd_ccl_totals (allocates its records)", track_pass)]
        res = median_ms([fn for _, fn in rows], args.rounds, args.calls)
        lines.append(f"-- {name}, structure {structure}: K = {k} clusters, R = {records} track records, largest cluster "
                     f"{int(bounds[:, 0].max())} voxels, foreground {int((labels > 0).sum()) / n:.3f}")
        base = res[0][0]
        for (nm, _), (med, best) in zip(rows, res):
            lines.append(f"{nm:64s} median {med:9.3f} ms  best {best:9.3f} ms  {n / med / 1e3:9.1f} Mvox/s  {med / base:7.2f} x the yardstick")
        lines.append(f"{'label: global-only over tiled':64s} {res[2][0] / res[1][0]:9.2f} x")
        if not args.no_scipy:
            import scipy.ndimage as ndi
            host = (x <= thr).cpu().numpy() if values else x.cpu().numpy()
            t0 = time.perf_counter()
            _, kh = ndi.label(host, ndi.generate_binary_structure(3, structure))
            dt = (time.perf_counter() - t0) * 1e3
            assert kh == k
            lines.append(f"{'scipy.ndimage.label on the host (one call, the copy not counted)':64s} {dt:16.1f} ms  {n / dt / 1e3:30.1f} Mvox/s")
        print("\n".join(lines[done:]), flush=True)
        del tracks, totals, bounds, offsets, labels, parent, flat, scratch, ws, kws
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
