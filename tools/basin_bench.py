"""HIP-event medians of the basin analysis (gan_danet_amd/basins.py): 12 synthetic star-shaped basins of 20 000 vertices each
on the 440 x 900 grid of the 0.05-degree product, and a (181, 440, 900) fp64 product.  `rasterize` (host packing and the
upload of the edges included, and the kernel alone); `zone_mean` over the 12 zones in one pass against today's way, 12
calls of K.masked_plane_mean_f64 with ZoneMap.mask(z), each a read of the whole product; and the project's own
one-read-one-write gather, gd_augment_d4 with op word 0, on an fp32 tensor of the same bytes as the yardstick.  GB/s counts
the bytes of the product each way has to read (the yardstick: one read + one write).  --out writes the table to a file
(profiles/r16_basins.txt).

    python tools/basin_bench.py [--rounds 7] [--calls 3] [--out profiles/r16_basins.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_danet_amd  # noqa: E402,F401
from gan_danet_amd import basins as B  # noqa: E402
from gan_danet_amd import kern as K  # noqa: E402
from filters_bench import median_ms  # noqa: E402


def star_basins(n_basins, n_vertices, lon, lat, seed=0):
    rs = np.random.RandomState(seed)
    zones = []
    for _ in range(n_basins):
        cx, cy = rs.uniform(lon[0] + 8, lon[-1] - 8), rs.uniform(lat[0] + 5, lat[-1] - 5)
        ang = (np.arange(n_vertices) + rs.uniform(0.1, 0.9, n_vertices)) * (2 * np.pi / n_vertices)
        r = rs.uniform(2.0, 5.0) * (1.0 + 0.3 * np.sin(7 * ang) + 0.02 * rs.uniform(-1, 1, n_vertices))
        zones.append([np.stack([cx + 1.6 * r * np.cos(ang), cy + r * np.sin(ang)], axis=1)])
    return zones


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls inside one pair of events")
    ap.add_argument("--steps", type=int, default=181)
    ap.add_argument("--basins", type=int, default=12)
    ap.add_argument("--vertices", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    h, w = 440, 900
    lon, lat = 65.025 + 0.05 * np.arange(w), 24.025 + 0.05 * np.arange(h)
    zones = star_basins(args.basins, args.vertices, lon, lat)
    edges, offsets = B.pack_polygons(zones)
    edges_dev, xs, ys = torch.from_numpy(edges).to(dev), torch.from_numpy(lon).to(dev), torch.from_numpy(lat).to(dev)
    zm = B.rasterize(zones, xs, ys)
    bits = torch.empty_like(zm.bits[0])
    inside = [int(zm.mask(z).sum().item()) for z in range(len(zm))]
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(args.steps, h, w, device=dev, dtype=torch.float64, generator=gen) + 2.0
    x[torch.rand(x.shape, device=dev, generator=gen) < 0.02] = float("nan")
    nbytes = x.numel() * 8
    masks = [zm.mask(z) for z in range(len(zm))]
    area = torch.cos(torch.deg2rad(ys))[:, None].expand(h, w).contiguous()
    # the yardstick on the same bytes: an fp32 (B, C, H, W) tensor, op word 0 = a plain copy through the gather
    y = torch.empty(nbytes // 4 // (2 * h * w), 2, h, w, device=dev)
    ops0 = torch.zeros(y.shape[0], dtype=torch.int32, device=dev)
    # the two ways must agree before they are timed
    mean, count = B.zone_mean(x, zm)
    for z, m in enumerate(masks):
        mz, cz = K.masked_plane_mean_f64(x, m)
        assert torch.equal(cz, count[:, z]) and torch.allclose(mz, mean[:, z], rtol=1e-10, atol=0, equal_nan=True)
    nz = len(zm)
    rows = [("gd_augment_d4 op 0 (yardstick)", lambda: K.augment_d4(y, ops0), 2 * y.numel() * 4),
            (f"rasterize, {nz} basins (pack + upload + kernel)", lambda: B.rasterize(zones, xs, ys), None),
            ("gd_zone_rasterize alone", lambda: K.zone_rasterize(edges_dev, offsets, xs, ys, out=bits), None),
            (f"zone_mean, {nz} zones, one pass", lambda: B.zone_mean(x, zm), nbytes),
            (f"zone_mean, {nz} zones, cos(lat) weights", lambda: B.zone_mean(x, zm, area), nbytes),
            (f"{nz} x masked_plane_mean_f64 with mask(z)", lambda: [K.masked_plane_mean_f64(x, m) for m in masks], nz * nbytes)]
    res = median_ms([fn for _, fn, _ in rows], args.rounds, args.calls)
    base = rows[0][2] / res[0][0]
    lines = [f"tools/basin_bench.py on {torch.cuda.get_device_name(0)}: {nz} star-shaped basins of {args.vertices} vertices "
             f"({edges.shape[0]} edges) on the {h} x {w} grid, {min(inside)}..{max(inside)} points inside each; product "
             f"{tuple(x.shape)} fp64 ({nbytes / 1e6:.0f} MB), 2 % NaN; {args.rounds} rounds x {args.calls} calls each, "
             f"alternating, HIP events; a call includes its allocations",
             "GB/s = the bytes of the product the way reads / median; ratio = GB/s over the yardstick's GB/s (one read + one "
             "write of the same bytes)"]
    for (name, _, nb), (med, best) in zip(rows, res):
        tail = "" if nb is None else (f"  {nb / 1e6:8.0f} MB  {nb / med / 1e6:8.1f} GB/s  x{(nb / med) / base:5.2f} of the "
                                      f"yardstick's rate")
        lines.append(f"{name:48s} median {med:9.3f} ms  best {best:9.3f} ms{tail}")
    one, many = res[3][0], res[5][0]
    lines.append(f"zone_mean reads the product once where the masked means read it {nz} times: {many / one:.2f} x the time")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
