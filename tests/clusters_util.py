"""Oracles and cases of the connected-component tests (test_cabi_clusters.py on the host twins, test_gpu_clusters.py on
the device).  Labels: scipy.ndimage.label.  Integer tables: numpy.  fp64 fields: math.fsum of the same rounded terms, with the
bound of a recursive sum in any order, (n - 1) 2^-53 sum |term| for n terms (Higham, Accuracy and Stability, 4.2, first
order), so a field of one term is exact.  The shapes come from the tile constants of the library: every big cube spans two
tiles and a ragged remainder along every axis.  Each property a case is there for is asserted on the oracle's own output."""
import functools
import math

import numpy as np
import scipy.ndimage as ndi

from gan_danet_amd import _lib as L

TT, TH, TW = L.CCL_TILE_T, L.CCL_TILE_H, L.CCL_TILE_W
BIG = (2 * TT + 1, 2 * TH + 1, 2 * TW + 1)
SMALL = ((1, 1, 1), (2, 1, 300), (1, 33, 65))
U = 2.0 ** -53
THRESHOLD = -0.8

# 8-connected in space, the same pixel in time
SPACE8_TIME1 = np.zeros((3, 3, 3), dtype=bool)
SPACE8_TIME1[1] = True
SPACE8_TIME1[:, 1, 1] = True
STRUCTURES = (1, 2, 3, "planar4", "planar8", SPACE8_TIME1)


def structure_id(s):
    return s if isinstance(s, str) else (f"conn{s}" if isinstance(s, int) else "space8time1")


def structure_array(s):
    """the 3 x 3 x 3 bool array scipy takes"""
    if isinstance(s, int):
        return ndi.generate_binary_structure(3, s)
    if isinstance(s, str):
        a = np.zeros((3, 3, 3), dtype=bool)
        a[1] = ndi.generate_binary_structure(2, 1 if s == "planar4" else 2)
        return a
    return np.asarray(s, dtype=bool)


def word_oracle(s):
    """bit k = entry k of the flattened array, the 13 entries before the centre"""
    flat = structure_array(s).reshape(-1)
    return sum(1 << k for k in range(13) if flat[k])


class Case:
    def __init__(self, name, x, threshold=None, mask=None, min_size=1):
        self.name, self.x, self.threshold, self.mask, self.min_size = name, x, threshold, mask, min_size

    @property
    def fg(self):
        if self.x.dtype == np.uint8:
            return self.x != 0
        with np.errstate(invalid="ignore"):
            fg = self.x <= self.threshold
        return fg & (self.mask != 0)[None] if self.mask is not None else fg

    def __repr__(self):
        return self.name


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def checkerboard(shape):
    t, h, w = np.indices(shape)
    return _u8((t + h + w) % 2 == 0)


def serpentine(shape):
    """even planes: a snake over the rows (full even rows, joined at alternating ends); odd planes: one voxel that joins
    the planes at alternating ends of the snake -- one long chain through every tile border"""
    T, H, W = shape
    x = np.zeros(shape, dtype=np.uint8)
    last = (H - 1) // 2 * 2
    for t in range(T):
        if t % 2 == 0:
            x[t, 0:last + 1:2, :] = 1
            for h in range(1, last, 2):
                x[t, h, W - 1 if (h // 2) % 2 == 0 else 0] = 1
        else:
            h, w = (0, 0) if (t // 2) % 2 else (last, W - 1)
            x[t, h, w] = 1
    return x


def spiral(shape):
    """the same one-pixel-wide rectangular spiral in every plane"""
    T, H, W = shape
    a = np.zeros((H, W), dtype=np.uint8)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    h = w = d = turned = 0
    a[0, 0] = 1

    def inside(p, q):
        return 0 <= p < H and 0 <= q < W

    while turned < 2:
        dh, dw = dirs[d]
        n1, n2 = (h + dh, w + dw), (h + 2 * dh, w + 2 * dw)
        if inside(*n1) and not a[n1] and (not inside(*n2) or not a[n2]):
            h, w = n1
            a[h, w] = 1
            turned = 0
        else:
            d, turned = (d + 1) % 4, turned + 1
    return _u8(np.broadcast_to(a, shape))


def diagonal_pairs(shape):
    """two blocks that touch only at a 3-D corner, across the corner of a tile, and two that touch only at an in-plane
    corner across a tile edge"""
    x = np.zeros(shape, dtype=np.uint8)
    x[TT - 2:TT, TH - 2:TH, TW - 2:TW] = 1
    x[TT:TT + 2, TH:TH + 2, TW:TW + 2] = 1
    x[0, TH - 2:TH, 2 * TW - 2:2 * TW] = 1
    x[0, TH:TH + 2, 2 * TW:2 * TW + 1] = 1
    return x


def random_fill(shape, p, seed):
    return _u8(np.random.default_rng(seed).random(shape) < p)


def index_cube(shape, dtype, seed):
    """a smooth-ish drought index quantised to 1/8 (samples exactly on the threshold -0.75 exist) with NaNs"""
    rng = np.random.default_rng(seed)
    z = ndi.uniform_filter(rng.standard_normal(shape), size=(3, 3, 5), mode="nearest") * 6.0
    z = np.round(z * 8) / 8
    z[rng.random(shape) < 0.03] = np.nan
    return np.ascontiguousarray(z, dtype=dtype)


def pixel_mask(shape, seed):
    m = (np.random.default_rng(seed).random(shape[1:]) < 0.9).astype(np.uint8)
    m[0, 0] = 0
    return m


def weights_of(shape):
    """cos(lat)-like cell weights, positive, not representable in a few bits"""
    H, W = shape[1:]
    lat = np.linspace(-1.2, 1.3, H)[:, None]
    return np.ascontiguousarray(np.cos(lat) * (1.0 + 0.001 * np.arange(W)[None, :]))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    corner = np.zeros(BIG, dtype=np.uint8)
    corner[-1, -1, -1] = 1
    out += [Case("empty", np.zeros(BIG, dtype=np.uint8)), Case("full", np.ones(BIG, dtype=np.uint8)), Case("corner", corner),
            Case("checkerboard", checkerboard(BIG)), Case("serpentine", serpentine(BIG)), Case("spiral", spiral(BIG)),
            Case("diagonal", diagonal_pairs(BIG))]
    out += [Case(f"random{p}", random_fill(BIG, p, k)) for k, p in enumerate((0.2, 0.35, 0.5, 0.6))]
    out += [Case("small-clusters", random_fill(BIG, 0.2, 11), min_size=4)]
    out += [Case("index-f64", index_cube(BIG, np.float64, 21), -0.75, pixel_mask(BIG, 22)),
            Case("index-f32", index_cube(BIG, np.float32, 23), -0.75, pixel_mask(BIG, 24)),
            Case("index-f64-min3", index_cube(BIG, np.float64, 25), -0.75, None, 3)]
    for shape in SMALL:
        tag = "x".join(map(str, shape))
        out += [Case(f"full-{tag}", np.ones(shape, dtype=np.uint8)), Case(f"checkerboard-{tag}", checkerboard(shape)),
                Case(f"random0.5-{tag}", random_fill(shape, 0.5, 31)), Case(f"index-f32-{tag}", index_cube(shape, np.float32, 32), -0.75)]
    return tuple(out)


CASES = cases()


def n_components(x, s):
    return ndi.label(x, structure_array(s))[1]


def check_case_properties():
    """each case has what it is there for, by scipy's own count"""
    by = {c.name: c for c in CASES}
    assert all(a > 2 * b for a, b in zip(BIG, (TT, TH, TW)))
    assert max(c.x.size for c in CASES) <= 100_000
    assert by["empty"].fg.sum() == 0 and by["full"].fg.all() and by["corner"].fg.sum() == 1 and by["corner"].fg[-1, -1, -1]
    cb = by["checkerboard"].x
    assert n_components(cb, 1) == cb.sum() == (cb.size + 1) // 2 and n_components(cb, 3) == 1
    for nm in ("serpentine", "spiral"):
        x = by[nm].x
        assert n_components(x, 1) == 1 and n_components(x, "planar4") == (x.sum((1, 2)) > 0).sum() >= BIG[0] // 2
        assert x.sum() > 5 * max(BIG) and x.mean() < 0.6
    assert n_components(by["serpentine"].x, "planar4") == BIG[0]
    d = by["diagonal"].x
    assert [n_components(d, s) for s in (1, 2, 3, "planar4", "planar8")] == [4, 3, 2, 6, 5]
    for p in (0.2, 0.35, 0.5, 0.6):
        assert abs(by[f"random{p}"].x.mean() - p) < 0.02
    sc = by["small-clusters"]
    sizes = np.bincount(ndi.label(sc.x, structure_array(1))[0].reshape(-1))[1:]
    assert (sizes < sc.min_size).any() and (sizes >= sc.min_size).any()
    for nm in ("index-f64", "index-f32", "index-f64-min3"):
        c = by[nm]
        assert np.isnan(c.x).any() and (c.x == c.threshold).any() and 0.1 < c.fg.mean() < 0.6
    assert by["index-f64"].mask is not None and (by["index-f64"].mask == 0).any()
    assert by["index-f32"].x.dtype == np.float32 and by["index-f64"].x.dtype == np.float64


def labels_oracle(case, s, min_size=None):
    """(labels, K) by scipy: components under min_size dropped, the rest numbered in raster order of their first voxel"""
    sa = structure_array(s)
    min_size = case.min_size if min_size is None else min_size
    lab, k = ndi.label(case.fg, sa)
    if min_size > 1 and k:
        sizes = np.bincount(lab.reshape(-1), minlength=k + 1)
        keep = sizes >= min_size
        keep[0] = False
        lab, k = ndi.label(keep[lab], sa)
    first = np.full(k + 1, lab.size, dtype=np.int64)
    np.minimum.at(first, lab.reshape(-1), np.arange(lab.size))
    assert np.all(np.diff(first[1:]) > 0), "scipy numbers the components in raster order of their first voxel"
    return lab.astype(np.int32), k


def bounds_oracle(lab, k):
    out = np.zeros((k, 7), dtype=np.int64)
    t, h, w = np.nonzero(lab)
    idx = lab[t, h, w] - 1
    out[:, 0] = np.bincount(idx, minlength=k)
    for col, v in ((1, t), (3, h), (5, w)):
        lo, hi = np.full(k, 1 << 30), np.full(k, -1)
        np.minimum.at(lo, idx, v)
        np.maximum.at(hi, idx, v)
        out[:, col], out[:, col + 1] = lo, hi
    return out


def _sum_check(got, terms, what):
    """got against the exact sum of the float64 `terms`: (n - 1) 2^-53 sum |term|; returns err / bound (0 for an exact one)"""
    exact = math.fsum(terms)
    bound = (len(terms) - 1) * U * math.fsum(abs(v) for v in terms)
    err = abs(got - exact)
    assert err <= bound, (what, got, exact, err, bound)
    return err / bound if bound else 0.0


def check_tracks(case, lab, bounds, offsets, tracks, index, weights, values):
    """every record against the oracle; returns the largest error over its bound"""
    k = bounds.shape[0]
    dur = bounds[:, 2] - bounds[:, 1] + 1
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(dur)])) and tracks.shape == (offsets[-1], 6)
    assert np.array_equal(index[:, 0], np.repeat(np.arange(k), dur))
    assert np.array_equal(index[:, 1], np.concatenate([np.arange(b[1], b[2] + 1) for b in bounds]) if k else np.zeros(0))
    x = None if case.x.dtype == np.uint8 else case.x.astype(np.float64)
    worst = 0.0
    for r in range(tracks.shape[0]):
        c, t = index[r]
        _, _, _, h0, h1, w0, w1 = bounds[c]
        sel = lab[t, h0:h1 + 1, w0:w1 + 1] == c + 1
        hh, ww = np.nonzero(sel)
        hh, ww = hh + h0, ww + w0
        a = weights[hh, ww] if weights is not None else np.ones(len(hh))
        got = tracks[r]
        assert got[0] == len(hh) > 0, (r, got[0], len(hh))
        worst = max(worst, _sum_check(got[1], list(a), "area"), _sum_check(got[3], list(a * hh), "sum_h"),
                    _sum_check(got[4], list(a * ww), "sum_w"))
        if values:
            xv = x[t, hh, ww]
            worst = max(worst, _sum_check(got[2], list(a * (case.threshold - xv)), "severity"))
            assert got[5] == xv.min()
        else:
            assert np.isnan(got[2]) and np.isnan(got[5])
    return worst


def check_totals(bounds, offsets, tracks, totals, values):
    """the totals against exact sums of the records they were made of; a quotient of two sums of n and m terms carries
    (n - 1) + (m - 1) + 1 roundings, first order"""
    worst = 0.0
    for c in range(bounds.shape[0]):
        rec = tracks[offsets[c]:offsets[c + 1]]
        n = len(rec)
        steps = np.arange(bounds[c, 1], bounds[c, 2] + 1).astype(np.float64)
        got = totals[c]
        worst = max(worst, _sum_check(got[0], list(rec[:, 1]), "volume"))
        assert got[2] == rec[:, 1].max() and got[3] == steps[np.argmax(rec[:, 1])]
        if values:
            worst = max(worst, _sum_check(got[1], list(rec[:, 2]), "severity"))
            assert got[4] == rec[:, 5].min()
        else:
            assert np.isnan(got[1]) and np.isnan(got[4])
        vol = math.fsum(rec[:, 1])
        for col, terms in ((5, rec[:, 1] * steps), (6, rec[:, 3]), (7, rec[:, 4])):
            exact = math.fsum(terms) / vol
            bound = (2 * (n - 1) + 1) * U * abs(exact) * (1 + 1e-9)
            err = abs(got[col] - exact)
            assert err <= bound, ("centroid", c, col, got[col], exact, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    return worst


def andreadis_oracle(case, s, min_step_pixels, min_size):
    """every step labelled on its own with the spatial part of the structure, small patches dropped, the rest linked in 3-D"""
    sa = structure_array(s)
    fg = case.fg.copy()
    for t in range(fg.shape[0]):
        lab, k = ndi.label(fg[t], sa[1])
        sizes = np.bincount(lab.reshape(-1), minlength=k + 1)
        keep = sizes >= min_step_pixels
        keep[0] = False
        fg[t] = keep[lab]
    return labels_oracle(Case(case.name + "-steps", _u8(fg)), s, min_size)


def host_pipeline(K, case, s, weights=None, tiles=True):
    """the host twins end to end: (labels, K, bounds, offsets, tracks, index, totals); tables None without clusters"""
    from gan_danet_amd import clusters as C
    values = case.x.dtype != np.uint8
    parent = K.ccl_label_host(case.x, case.threshold if values else 0.0, C.structure_word(s), case.mask if values else None, tiles)
    if case.min_size > 1:
        parent = K.ccl_filter_host(parent, case.min_size)
    labels, k = K.ccl_relabel_host(parent)
    if k == 0:
        return parent, labels, 0, None, None, None, None, None
    bounds = K.ccl_bounds_host(labels, k)
    offsets = K.ccl_offsets_host(bounds)
    tracks, index = K.ccl_tracks_host(case.x if values else None, labels, bounds, offsets, case.threshold if values else 0.0, weights, values)
    return parent, labels, k, bounds, offsets, tracks, index, K.ccl_totals_host(tracks, bounds, offsets)
