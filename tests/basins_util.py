"""helpers shared by the basin-analysis tests (test_cabi_basins.py on the CPU, test_gpu_basins.py on the GPU): the test
zones, the grids, the independent containment oracle and the precondition that makes the comparison exact.

Oracle: ``matplotlib.path.Path(ring).contains_points`` per ring, XORed over the rings of a zone by the test (matplotlib
does not XOR the sub-paths of a compound path itself).  Precondition, asserted by ``checked_zones``: no grid point is
closer than 1e-9 degrees to any edge, so both sides are unambiguous and the masks must be EQUAL; vertices are seeded
random and drawn again with the next seed where the precondition fails."""
import math

import numpy as np
from matplotlib.path import Path

MIN_DIST = 1e-9


def grid(h, w, step=0.25):
    """the notebook's grids: lon 65.125 + 0.25 j, lat 24.125 + 0.25 i, and the 0.05-degree analogue"""
    off = step / 2
    return np.round(65.0 + off + step * np.arange(w), 5), np.round(24.0 + off + step * np.arange(h), 5)


def star(rs, cx, cy, r_in, r_out, n=37):
    """a star-shaped (concave) ring of n vertices around (cx, cy), open"""
    ang = (np.arange(n) + rs.uniform(0.1, 0.9, n)) * (2 * np.pi / n)
    r = rs.uniform(r_in, r_out, n)
    return np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], axis=1)


def convex(rs, cx, cy, rx, ry, n=11):
    ang = np.sort(rs.uniform(0, 2 * np.pi, n))
    return np.stack([cx + rx * np.cos(ang), cy + ry * np.sin(ang)], axis=1)


def make_zones(seed, lon, lat):
    """the named test zones, each a list of rings, sized for a grid that spans at least 50 x 60 points of 0.25 degrees"""
    rs = np.random.RandomState(seed)
    jit = lambda: rs.uniform(-0.05, 0.05)
    zones = {
        "convex": [convex(rs, 70.3 + jit(), 29.1 + jit(), 3.1, 2.2)],
        "star": [star(rs, 73.2 + jit(), 31.4 + jit(), 1.2, 4.3)],
        "star_hole": [star(rs, 70.0 + jit(), 30.0 + jit(), 2.6, 4.4), star(rs, 70.0, 30.0, 0.7, 2.2, 19)[::-1]],
        "multi": [star(rs, 68.4 + jit(), 27.3 + jit(), 1.9, 2.9, 23), convex(rs, 68.4, 27.3, 1.1, 0.9, 9),
                  convex(rs, 76.6 + jit(), 33.2 + jit(), 2.3, 1.7, 13)],
        "outside": [convex(rs, 120.0, 10.0, 2.0, 2.0)],
        "cover": [np.array([[40.0 + jit(), 5.0 + jit()], [140.0 + jit(), 5.5 + jit()], [141.0 + jit(), 60.0 + jit()],
                            [39.0 + jit(), 61.0 + jit()]])],
    }
    # a ring with vertices whose y is a grid row's y exactly and whose x lies between two columns: the ray of that row
    # runs through the vertex (pass-through vertices and local extrema both occur)
    ring = star(rs, 72.0 + jit(), 30.0 + jit(), 2.0, 4.0, 31)
    for k in range(0, len(ring), 3):
        i = int(np.argmin(np.abs(lat - ring[k, 1])))
        j = int(np.clip(np.searchsorted(lon, ring[k, 0]), 1, len(lon) - 1))
        ring[k] = [lon[j - 1] + (lon[j] - lon[j - 1]) * rs.uniform(0.3, 0.7), lat[i]]
    zones["vertex_on_row"] = [ring]
    return zones


def edges_of(rings):
    out = []
    for r in rings:
        r = np.asarray(r, dtype=np.float64)
        if not np.array_equal(r[0], r[-1]):
            r = np.concatenate([r, r[:1]])
        out.append(np.concatenate([r[:-1], r[1:]], axis=1))
    return np.concatenate(out)


def min_distance(rings, lon, lat):
    """the smallest distance from any grid point to any edge of the rings, in numpy"""
    e = edges_of(rings)
    px, py = np.meshgrid(lon, lat)
    p = np.stack([px.ravel(), py.ravel()], axis=1)
    best = np.inf
    for lo in range(0, len(e), 256):
        a, b = e[lo:lo + 256, None, :2], e[lo:lo + 256, None, 2:]
        d = b - a
        t = np.clip(((p[None] - a) * d).sum(-1) / np.maximum((d * d).sum(-1), 1e-300), 0.0, 1.0)
        best = min(best, float(np.sqrt((((a + t[..., None] * d) - p[None]) ** 2).sum(-1)).min()))
    return best


def oracle(rings, lon, lat):
    """(H, W) bool: matplotlib per ring, XOR over the rings"""
    px, py = np.meshgrid(lon, lat)
    p = np.stack([px.ravel(), py.ravel()], axis=1)
    inside = np.zeros(len(p), dtype=bool)
    for r in rings:
        inside ^= Path(np.asarray(r, dtype=np.float64)).contains_points(p)
    return inside.reshape(len(lat), len(lon))


def checked(make, lon, lat, seed=0):
    """``make(seed)`` -> {name: rings} (or a list of ring lists), redrawn with the next seed until every grid point keeps
    MIN_DIST from every edge; the precondition is asserted on what is returned"""
    for s in range(seed, seed + 20):
        zones = make(s)
        items = list(zones.values()) if isinstance(zones, dict) else list(zones)
        d = min(min_distance(r, lon, lat) for r in items)
        if d >= MIN_DIST:
            break
    assert d >= MIN_DIST, f"precondition: a grid point within {d} degrees of an edge"
    return zones


def bits_of(masks):
    """(Z <= 32 boolean masks) -> the uint32 words of gd_zone_rasterize"""
    out = np.zeros(masks[0].shape, dtype=np.uint32)
    for z, m in enumerate(masks):
        out |= m.astype(np.uint32) << np.uint32(z)
    return out


def two_prod(a, b):
    """(p, e) with p + e == a * b exactly (Dekker / Veltkamp, no FMA needed)"""
    p = a * b

    def split(v):
        c = 134217729.0 * v
        hi = c - (c - v)
        return hi, v - hi

    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def zone_mean_ref(x, masks, weights=None):
    """per (plane, zone): the correctly rounded sums (math.fsum) -> (mean, count, mean|x|) fp64 / int64 arrays of shape
    lead + (Z,); x: numpy (..., H, W) in fp64, masks: Z boolean (H, W), weights: (H, W) fp64 or None.  With weights the
    products w x are split exactly (two_prod), so the numerator is the correctly rounded exact sum as well."""
    lead = x.shape[:-2]
    xf = x.reshape((-1,) + x.shape[-2:])
    nz = len(masks)
    mean = np.full((len(xf), nz), np.nan)
    mabs = np.zeros((len(xf), nz))
    count = np.zeros((len(xf), nz), dtype=np.int64)
    for t, plane in enumerate(xf):
        for z, m in enumerate(masks):
            sel = m & ~np.isnan(plane)
            v = plane[sel]
            if weights is None:
                num, den, nabs = math.fsum(v), float(len(v)), math.fsum(np.abs(v))
            else:
                w = weights[sel]
                p, e = two_prod(w, v)
                num, den = math.fsum(np.concatenate([p, e])), math.fsum(w)
                pa, ea = two_prod(w, np.abs(v))
                nabs = math.fsum(np.concatenate([pa, ea]))
            if len(v) and den != 0.0:
                mean[t, z], count[t, z], mabs[t, z] = num / den, len(v), nabs / den
    return mean.reshape(lead + (nz,)), count.reshape(lead + (nz,)), mabs.reshape(lead + (nz,))
