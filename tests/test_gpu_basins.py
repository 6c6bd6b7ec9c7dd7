"""GPU: the basin analysis (gan_danet_amd/basins.py, csrc/basins.hip).

Rasteriser: the device words equal the host entry point and the matplotlib XOR oracle bit for bit (every grid point keeps
1e-9 degrees from every edge: basins_util.checked), over the named test zones, row lengths that are no multiple of 64,
a single row, 1 / 32 / 33 zones (two groups), a ring longer than four edge chunks, and a pre-filled output.

Zonal means: the reference is the correctly rounded math.fsum per (plane, zone) (basins_util.zone_mean_ref), so all error
belongs to the kernel.  Counts are exact; means hold |got - want| <= n * 2^-52 * mean|x| with n the zone's contributing
pixels -- the bound of any fp64 summation order of n terms (n - 1 additions of relative error 2^-53 each, plus, with
weights, one rounding per product and the same again for the weight sum, plus the division), not a measured number.
Inputs are randn + 2 so that mean|x| is about |mean|.  Two runs give identical bits."""
import numpy as np
import pytest
import torch

import basins_util as U
from gpu_util import DEV

pytestmark = pytest.mark.gpu

ZONES = ("convex", "star", "star_hole", "multi", "outside", "cover", "vertex_on_row")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_raster(zones, lon, lat, what, prefill=None):
    """device == host entry == oracle for a list of zones (each a list of rings) on one grid"""
    from gan_danet_amd import basins
    from gan_danet_amd import kern as K
    edges, offsets = basins.pack_polygons(zones)
    out = None
    if prefill is not None:
        out = torch.full((len(lat), len(lon)), prefill, dtype=torch.int32, device=DEV).view(torch.uint32)
    got = K.zone_rasterize(_dev(edges), offsets, _dev(lon), _dev(lat), out=out).cpu().numpy()
    host = K.zone_rasterize_host(edges, offsets, lon, lat)
    want = U.bits_of([U.oracle(z, lon, lat) for z in zones])
    assert got.dtype == np.uint32 and got.shape == (len(lat), len(lon))
    assert np.array_equal(host, want), f"{what}: host entry differs from the oracle at {np.sum(host != want)} points"
    assert np.array_equal(got, want), f"{what}: device differs from the oracle at {np.sum(got != want)} points"
    return got


@pytest.mark.parametrize("h,w", [(50, 60), (50, 61), (50, 130), (1, 130)])
def test_rasterize_named_zones(h, w):
    lon, lat = U.grid(h, w)
    if h == 1:
        lat = U.grid(50, 60)[1][23:24]                            # one row through the middle of the zones
    ref_lon, ref_lat = U.grid(50, 60)                             # the zones are laid out for the 50 x 60 grid
    zones = U.checked(lambda s: U.make_zones(11 + s, ref_lon, ref_lat), lon, lat)
    got = _check_raster([zones[n] for n in ZONES], lon, lat, f"{h} x {w}")
    inside = [int(((got >> np.uint32(z)) & 1).sum()) for z in range(len(ZONES))]
    print(f"{h} x {w}: points inside {dict(zip(ZONES, inside))}")
    assert inside[ZONES.index("outside")] == 0 and inside[ZONES.index("cover")] == h * w and inside[ZONES.index("star")] > 0


@pytest.mark.parametrize("grid", ["descending_lat", "nonuniform_lon"])
def test_rasterize_other_grids(grid):
    lon, lat = U.grid(50, 60)
    if grid == "descending_lat":
        lat = lat[::-1].copy()
    else:
        lon = lon + 0.09 * np.sin(1.7 * np.arange(60))
    zones = U.checked(lambda s: U.make_zones(11 + s, lon, lat), lon, lat)
    _check_raster([zones[n] for n in ZONES], lon, lat, grid)


def _many(seed, n):
    rs = np.random.RandomState(seed)
    return [[U.star(rs, rs.uniform(66.0, 71.5), rs.uniform(24.8, 28.2), 0.3, 1.4, 9)] for _ in range(n)]


@pytest.mark.parametrize("nz", [1, 32, 33])
def test_rasterize_zone_counts(nz):
    """33 zones make two groups of words; ZoneMap.mask(z) finds zone z in either"""
    from gan_danet_amd import basins
    lon, lat = U.grid(20, 30)
    zones = U.checked(lambda s: _many(100 + s, nz), lon, lat)
    zm = basins.rasterize(zones, lon, lat, device=DEV)
    assert len(zm) == nz and zm.bits.shape == ((nz + 31) // 32, 20, 30) and zm.bits.dtype == torch.uint32
    got = zm.bits.cpu().numpy()
    for g in range(got.shape[0]):
        sub = zones[32 * g:32 * g + 32]
        assert np.array_equal(got[g], U.bits_of([U.oracle(z, lon, lat) for z in sub])), f"group {g}"
    for z in (0, nz - 1):
        m = zm.mask(z)
        assert m.dtype == torch.uint8 and m.shape == (20, 30) and m.is_cuda
        assert np.array_equal(m.cpu().numpy().astype(bool), U.oracle(zones[z], lon, lat))
    assert zm.to(DEV).names == zm.names


def test_rasterize_ring_longer_than_four_chunks_into_a_prefilled_buffer():
    from gan_danet_amd import _lib as L
    n = 4 * L.ZONE_EDGE_CHUNK + 7
    lon, lat = U.grid(20, 30)
    zones = U.checked(lambda s: [[U.star(np.random.RandomState(200 + s), 68.7, 26.4, 1.0, 2.2, n)]], lon, lat)
    from gan_danet_amd import basins
    assert basins.pack_polygons(zones)[0].shape == (n, 4)
    got = _check_raster(zones, lon, lat, "chunk boundary", prefill=-1)                # 0xFFFFFFFF in every word
    assert 0 < got.sum() < got.size and got.max() == 1             # every word written: no bit of the fill survives


# ---- zonal means -------------------------------------------------------------------------------------------------------
def _blob_masks(rs, h, w):
    """five overlapping zones: ellipses of different size, zone 3 empty"""
    yy, xx = np.mgrid[0:h, 0:w]
    masks = []
    for z in range(5):
        cy, cx, ry, rx = rs.uniform(0.3, 0.7) * h, rs.uniform(0.3, 0.7) * w, rs.uniform(0.2, 0.45) * h, rs.uniform(0.2, 0.45) * w
        masks.append(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0)
    masks[3] = np.zeros((h, w), dtype=bool)
    assert (masks[0] & masks[1]).any() or (masks[1] & masks[2]).any()
    return masks


def _zone_mean_case(shape, dtype, weighted, offset=0, seed=0):
    from gan_danet_amd import basins
    rs = np.random.RandomState(seed)
    h, w = shape[-2:]
    masks = _blob_masks(rs, h, w)
    x = (rs.randn(*shape) + 2.0).astype(np.float32 if dtype == torch.float32 else np.float64)
    x[rs.rand(*shape) < 0.03] = np.nan                              # scattered NaNs
    x.reshape((-1, h, w))[1][masks[2]] = np.nan                     # zone 2 all-NaN at one step only
    weights = np.cos(np.deg2rad(np.linspace(24.0, 46.0, h)))[:, None] * np.ones((1, w)) if weighted else None
    n = x.size
    buf = torch.empty(n + offset + 3, dtype=dtype, device=DEV)
    xd = buf[offset:offset + n].view(shape)                         # a plane view that starts `offset` elements in
    xd.copy_(torch.from_numpy(x))
    assert xd.is_contiguous() and xd.data_ptr() == buf.data_ptr() + offset * buf.element_size()
    lon, lat = U.grid(h, w)
    zm = basins.ZoneMap(_dev(U.bits_of(masks))[None], [f"z{i}" for i in range(5)], _dev(lon), _dev(lat))
    wd = None if weights is None else _dev(weights)
    mean, count = basins.zone_mean(xd, zm, wd)
    mean2, count2 = basins.zone_mean(xd, zm, wd)
    want, wcount, mabs = U.zone_mean_ref(x.astype(np.float64), masks, weights)
    assert mean.dtype == torch.float64 and count.dtype == torch.int64 and tuple(mean.shape) == tuple(shape[:-2]) + (5,)
    got, gcount = mean.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(gcount, wcount), "counts differ"
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.all(np.isnan(got[..., 3])) and np.all(gcount[..., 3] == 0)                    # the empty zone
    flat = got.reshape(-1, 5)
    assert np.isnan(flat[1, 2]) and gcount.reshape(-1, 5)[1, 2] == 0 and not np.isnan(flat[0, 2])
    ok = ~np.isnan(want)
    err, bound = np.abs(got - want)[ok], (wcount * 2.0 ** -52 * mabs)[ok]
    print(f"{shape} {dtype} weighted={weighted} offset={offset}: max err / bound = {np.max(err / bound):.3f}, "
          f"max err {err.max():.2e}, zone pixels up to {wcount.max()}")
    assert np.all(err <= bound)
    assert torch.equal(mean.view(torch.int64), mean2.view(torch.int64)) and torch.equal(count, count2)
    return zm, xd, mean, count


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(3, 37, 53), (7, 130, 257), (2, 3, 16, 24)])
def test_zone_mean(shape, dtype, weighted):
    _zone_mean_case(shape, dtype, weighted)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zone_mean_plane_view_at_an_odd_offset(dtype):
    _zone_mean_case((3, 37, 53), dtype, True, offset=1, seed=1)
    _zone_mean_case((3, 37, 53), dtype, False, offset=3, seed=2)


def test_zone_mean_above_sixteen_zones_and_two_groups():
    """17 and 33 zones: the widest accumulator instance, and a second group of words"""
    from gan_danet_amd import basins
    rs = np.random.RandomState(5)
    h, w = 20, 30
    lon, lat = U.grid(h, w)
    x = rs.randn(4, h, w) + 2.0
    for nz in (17, 33):
        masks = [rs.rand(h, w) < 0.3 for _ in range(nz)]
        bits = np.stack([U.bits_of(masks[g:g + 32]) for g in range(0, nz, 32)])
        zm = basins.ZoneMap(_dev(bits), [str(i) for i in range(nz)], _dev(lon), _dev(lat))
        mean, count = basins.zone_mean(_dev(x), zm)
        want, wcount, mabs = U.zone_mean_ref(x, masks)
        assert tuple(mean.shape) == (4, nz) and np.array_equal(count.cpu().numpy(), wcount)
        assert np.all(np.abs(mean.cpu().numpy() - want) <= wcount * 2.0 ** -52 * mabs)


def test_zone_mask_feeds_masked_plane_mean():
    """ZoneMap.mask(z) as the mask= of the existing gd_masked_plane_mean_f64: the same count as zone_mean for that zone"""
    from gan_danet_amd import kern as K
    zm, xd, mean, count = _zone_mean_case((3, 37, 53), torch.float64, False, seed=3)
    for z in (0, 1, 4):
        m, c = K.masked_plane_mean_f64(xd, zm.mask(z))
        assert torch.equal(c, count[:, z]) and c.min().item() > 0
        assert torch.equal(torch.isnan(m), torch.isnan(mean[:, z]))


# ---- the notebook's loop -------------------------------------------------------------------------------------------------
def test_basin_series():
    from gan_danet_amd import basins
    t = 6
    lon25, lat25 = U.grid(8, 12, 0.25)
    lon05, lat05 = U.grid(40, 60, 0.05)

    def toy(seed):
        rs = np.random.RandomState(300 + seed)
        return {"upper": [U.star(rs, 65.9, 25.3, 0.45, 0.8, 11)],
                "lower": [U.star(rs, 67.2, 24.8, 0.4, 0.7, 9), U.convex(rs, 67.2, 24.8, 0.2, 0.15, 7)],
                "east": [U.convex(rs, 67.3, 25.6, 0.6, 0.35, 8), U.convex(rs, 65.6, 24.5, 0.35, 0.3, 6)]}

    for seed in range(20):                                          # both grids must keep their distance from every edge
        zones = toy(seed)
        if min(min(U.min_distance(r, lo, la) for r in zones.values()) for lo, la in ((lon25, lat25), (lon05, lat05))) >= U.MIN_DIST:
            break
    U.checked(lambda s: zones, lon25, lat25)
    U.checked(lambda s: zones, lon05, lat05)
    rs = np.random.RandomState(9)
    g25 = rs.randn(t, 8, 12) + 2.0
    d05 = np.repeat(np.repeat(g25, 5, axis=1), 5, axis=2) + 0.3 * rs.randn(t, 40, 60)
    d05[rs.rand(t, 40, 60) < 0.05] = np.nan
    g25[2, 3:5, 2:6] = np.nan
    names = list(zones)
    out = basins.basin_series(_dev(g25), (lon25, lat25), _dev(d05), (_dev(lon05), _dev(lat05)), [zones[n] for n in names], names)
    assert list(out) == names
    for name in names:
        res = out[name]
        m25, m05 = U.oracle(zones[name], lon25, lat25), U.oracle(zones[name], lon05, lat05)
        assert m25.sum() >= 2 and m05.sum() >= 50, name
        for key, data, mask in (("grace", g25, m25), ("downscaled", d05, m05)):
            want = np.nanmean(data[:, mask], axis=1)
            ref, cnt, mabs = U.zone_mean_ref(data, [mask])
            assert np.array_equal(res["count_" + key], cnt[:, 0]) and res[key].shape == (t,)
            assert np.all(np.abs(res[key] - ref[:, 0]) <= cnt[:, 0] * 2.0 ** -52 * mabs[:, 0])
            assert np.all(np.abs(res[key] - want) <= 2 * cnt[:, 0] * 2.0 ** -52 * mabs[:, 0])   # numpy's own sum order
        a, b = res["downscaled"], res["grace"]
        ok = ~(np.isnan(a) | np.isnan(b))
        cc = np.corrcoef(a[ok], b[ok])[0, 1]
        rmse = np.sqrt(np.mean((a[ok] - b[ok]) ** 2))
        print(f"{name}: {int(m25.sum())} / {int(m05.sum())} points, cc {res['cc']:.6f} (numpy {cc:.6f}), rmse {res['rmse']:.6f}")
        assert abs(res["cc"] - cc) <= 1e-12 * abs(cc) and abs(res["rmse"] - rmse) <= 1e-12 * rmse
