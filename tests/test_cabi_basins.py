"""CPU: the basin-analysis entry points of the C ABI (include/gandanet.h, "Basin analysis") are declared and bound, every
device entry point rejects bad arguments before any launch, gd_zone_rasterize_host -- plain loops over the predicate the
device kernel shares (csrc/zones.h) -- equals the matplotlib XOR oracle exactly, pack_polygons reads ring lists, GeoJSON
mappings and __geo_interface__ objects, and the public module refuses CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import basins_util as U

NAMES = ("gd_zone_rasterize", "gd_zone_rasterize_host", "gd_zone_mean_ws_bytes", "gd_zone_mean")
ZONES = ("convex", "star", "star_hole", "multi", "outside", "cover", "vertex_on_row")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_basin_symbols_are_declared_and_bound():
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    assert "Basin analysis" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
    assert f"#define GD_ZONE_EDGE_CHUNK {L.ZONE_EDGE_CHUNK}" in src and f"#define GD_ZONE_MAX {L.ZONE_MAX}" in src


def test_basin_argument_errors_before_any_launch():
    """negative code + gd_last_error with no GPU: validation comes first, so the device pointers (never-dereferenced
    addresses) are not touched; the offsets are a host array and are read"""
    L, lib = _lib()
    p, q, r, s, t, u = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000

    def bad(rc, word):
        assert rc < 0, rc
        assert word in L.last_error(), L.last_error()

    def off(*v):
        return (C.c_long * len(v))(*v)

    ras = lib.gd_zone_rasterize
    o2 = off(0, 4, 10)
    bad(ras(None, 10, o2, 2, q, 5, r, 4, s, None), "null")
    bad(ras(p, 10, None, 2, q, 5, r, 4, s, None), "null")
    bad(ras(p, 10, o2, 2, None, 5, r, 4, s, None), "null")
    bad(ras(p, 10, o2, 2, q, 5, None, 4, s, None), "null")
    bad(ras(p, 10, o2, 2, q, 5, r, 4, None, None), "null")
    bad(ras(p, 10, o2, 0, q, 5, r, 4, s, None), "Z outside")
    bad(ras(p, 10, o2, -1, q, 5, r, 4, s, None), "Z outside")
    bad(ras(p, 10, off(*([0] * 33 + [10])), 33, q, 5, r, 4, s, None), "Z outside")
    bad(ras(p, 10, off(0, 6, 4, 10), 3, q, 5, r, 4, s, None), "offsets")          # not monotone
    bad(ras(p, 10, off(0, 4, 9), 2, q, 5, r, 4, s, None), "offsets")              # last != E
    bad(ras(p, 10, off(1, 4, 10), 2, q, 5, r, 4, s, None), "offsets")             # first != 0
    bad(ras(p, 10, off(0, -2, 10), 2, q, 5, r, 4, s, None), "offsets")
    bad(ras(p, 0, off(0, 0, 0), 2, q, 5, r, 4, s, None), "<= 0")
    bad(ras(p, 10, o2, 2, q, 0, r, 4, s, None), "<= 0")
    bad(ras(p, 10, o2, 2, q, -5, r, 4, s, None), "<= 0")
    bad(ras(p, 10, o2, 2, q, 5, r, 0, s, None), "<= 0")
    bad(ras(p, 10, o2, 2, q, 5, r, -1, s, None), "<= 0")
    bad(ras(p + 4, 10, o2, 2, q, 5, r, 4, s, None), "aligned")
    bad(ras(p, 10, o2, 2, q + 4, 5, r, 4, s, None), "aligned")
    bad(ras(p, 10, o2, 2, q, 5, r + 2, 4, s, None), "aligned")
    bad(ras(p, 10, o2, 2, q, 5, r, 4, s + 2, None), "aligned")

    zm = lib.gd_zone_mean
    big = 1 << 30
    bad(zm(None, 1, 3, 100, q, 5, None, r, s, t, big, None), "null")
    bad(zm(p, 1, 3, 100, None, 5, None, r, s, t, big, None), "null")
    bad(zm(p, 1, 3, 100, q, 5, None, None, s, t, big, None), "null")
    bad(zm(p, 1, 3, 100, q, 5, None, r, None, t, big, None), "null")
    bad(zm(p, 1, 3, 100, q, 5, None, r, s, None, big, None), "null")
    bad(zm(p, 2, 3, 100, q, 5, None, r, s, t, big, None), "dtype")
    bad(zm(p, -1, 3, 100, q, 5, None, r, s, t, big, None), "dtype")
    bad(zm(p, 1, 3, 100, q, 0, None, r, s, t, big, None), "Z outside")
    bad(zm(p, 1, 3, 100, q, 33, None, r, s, t, big, None), "Z outside")
    bad(zm(p, 1, 0, 100, q, 5, None, r, s, t, big, None), "<= 0")
    bad(zm(p, 1, -2, 100, q, 5, None, r, s, t, big, None), "<= 0")
    bad(zm(p, 1, 3, 0, q, 5, None, r, s, t, big, None), "<= 0")
    bad(zm(p, 1, 3, -7, q, 5, None, r, s, t, big, None), "<= 0")
    bad(zm(p, 1, 65536, 100, q, 5, None, r, s, t, big, None), "65535")
    need = lib.gd_zone_mean_ws_bytes(7, 130 * 257, 5)
    assert need > 0 and need % (7 * 5 * 24) == 0
    bad(zm(p, 1, 7, 130 * 257, q, 5, None, r, s, t, need - 1, None), "workspace")
    bad(zm(p + 4, 1, 3, 100, q, 5, None, r, s, t, big, None), "aligned")
    bad(zm(p + 2, 0, 3, 100, q, 5, None, r, s, t, big, None), "aligned")
    bad(zm(p, 1, 3, 100, q + 2, 5, None, r, s, t, big, None), "aligned")
    bad(zm(p, 1, 3, 100, q, 5, u + 4, r, s, t, big, None), "aligned")
    bad(zm(p, 1, 3, 100, q, 5, None, r + 4, s, t, big, None), "aligned")
    bad(zm(p, 1, 3, 100, q, 5, None, r, s + 4, t, big, None), "aligned")
    bad(zm(p, 1, 3, 100, q, 5, None, r, s, t + 4, big, None), "aligned")
    assert lib.gd_zone_mean_ws_bytes(0, 100, 5) == 0 and lib.gd_zone_mean_ws_bytes(3, 0, 5) == 0
    assert lib.gd_zone_mean_ws_bytes(3, 100, 0) == 0 and lib.gd_zone_mean_ws_bytes(3, 100, 33) == 0

    host = lib.gd_zone_rasterize_host
    d8, w8 = (C.c_double * 8)(), (C.c_uint32 * 8)()
    bad(host(None, 2, off(0, 2), 1, d8, 2, d8, 2, w8), "null")
    bad(host(d8, 2, off(0, 2), 0, d8, 2, d8, 2, w8), "Z outside")
    bad(host(d8, 2, off(0, 1), 1, d8, 2, d8, 2, w8), "offsets")
    bad(host(d8, 2, off(0, 2), 1, d8, 0, d8, 2, w8), "<= 0")


GRIDS = {
    "notebook": lambda: U.grid(50, 60),
    "descending_lat": lambda: (U.grid(50, 60)[0], U.grid(50, 60)[1][::-1].copy()),
    "nonuniform_lon": lambda: (U.grid(50, 60)[0] + 0.09 * np.sin(1.7 * np.arange(60)), U.grid(50, 60)[1]),
}


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_rasterize_host_equals_the_oracle(grid):
    from gan_danet_amd import basins
    from gan_danet_amd import kern as K
    lon, lat = GRIDS[grid]()
    assert np.all(np.diff(lon) > 0)
    zones = U.checked(lambda s: U.make_zones(11 + s, lon, lat), lon, lat)
    assert sorted(zones) == sorted(ZONES)
    ring = zones["vertex_on_row"][0]
    assert np.sum(np.isin(ring[:, 1], lat)) >= 5 and not np.any(np.isin(ring[:, 0], lon))
    edges, offsets = basins.pack_polygons([zones[n] for n in ZONES])
    bits = K.zone_rasterize_host(edges, offsets, lon, lat)
    assert bits.shape == (50, 60) and bits.dtype == np.uint32 and not np.any(bits >> np.uint32(len(ZONES)))
    for z, name in enumerate(ZONES):
        want = U.oracle(zones[name], lon, lat)
        got = ((bits >> np.uint32(z)) & np.uint32(1)).astype(bool)
        assert np.array_equal(got, want), f"{grid} / {name}: {np.sum(got != want)} of {want.size} points differ"
        print(f"{grid} / {name}: {int(want.sum())} of {want.size} points inside")
    assert not np.any(U.oracle(zones["outside"], lon, lat)) and np.all(U.oracle(zones["cover"], lon, lat))
    hole = U.oracle(zones["star_hole"][1:], lon, lat)
    assert hole.sum() >= 20 and not np.any(((bits >> np.uint32(ZONES.index("star_hole"))) & np.uint32(1)).astype(bool) & hole)


def test_rasterize_host_writes_every_word():
    from gan_danet_amd import kern as K
    lon, lat = U.grid(6, 7)
    edges = U.edges_of([np.array([[65.3, 24.3], [66.2, 24.3], [66.2, 25.2], [65.3, 25.2]])])
    got = K.zone_rasterize_host(edges, [0, 4], lon, lat)
    want = U.oracle([edges[:, :2]], lon, lat)
    assert np.array_equal(got, want.astype(np.uint32)) and want.sum() == 16


def test_pack_polygons():
    from gan_danet_amd import basins
    sq = [[0.0, 0.0], [2.0, 0.0], [2.0, 2.0], [0.0, 2.0]]
    hole = [[0.5, 0.5], [0.5, 1.5], [1.5, 1.5], [1.5, 0.5], [0.5, 0.5]]                       # already closed
    tri = [[5.0, 5.0], [6.0, 5.0], [6.0, 5.0], [5.5, 6.0]]                                     # a repeated vertex
    edges, off = basins.pack_polygons([[sq], [sq, hole], [tri]])
    assert edges.dtype == np.float64 and off.dtype == np.int64 and edges.shape == (4 + 8 + 3, 4)
    assert off.tolist() == [0, 4, 12, 15]
    assert edges[3].tolist() == [0.0, 2.0, 0.0, 0.0]                                           # the closing edge
    assert np.array_equal(edges[:4], edges[4:8]) and np.array_equal(edges[8:12, :2], np.array(hole[:4]))
    assert not np.any(np.all(edges[:, :2] == edges[:, 2:], axis=1))                            # no zero-length edge
    # GeoJSON mappings and __geo_interface__ objects give the same table as their rings
    poly = {"type": "Polygon", "coordinates": [sq, hole]}
    multi = {"type": "MultiPolygon", "coordinates": [[sq, hole], [tri]]}
    geom = type("Geom", (), {"__geo_interface__": {"type": "Polygon", "coordinates": (tuple(map(tuple, sq)),)}})()
    e2, o2 = basins.pack_polygons([geom, poly, multi])
    assert o2.tolist() == [0, 4, 12, 23]
    assert np.array_equal(e2[:12], edges[:12]) and np.array_equal(e2[12:], edges[4:])
    e3, _ = basins.pack_polygons([{"type": "Polygon", "coordinates": [[[0, 0, 9.0], [2, 0, 9.0], [2, 2, 9.0], [0, 2, 9.0]]]}])
    assert np.array_equal(e3, edges[:4])                                                       # a z coordinate is ignored
    for degenerate in ([[0.0, 0.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [0.0, 0.0], [1.0, 1.0]], [[3.0, 3.0]] * 4):
        with pytest.raises(ValueError):
            basins.pack_polygons([[degenerate]])
    with pytest.raises(ValueError):
        basins.pack_polygons([{"type": "Point", "coordinates": [0.0, 0.0]}])
    with pytest.raises(ValueError):
        basins.pack_polygons([])


def test_cpu_tensors_are_refused():
    import gan_danet_amd
    from gan_danet_amd import _lib as L
    from gan_danet_amd import basins
    assert gan_danet_amd.basins is basins
    sq = [[[65.3, 24.3], [66.2, 24.3], [66.2, 25.2], [65.3, 25.2]]]
    lon, lat = U.grid(6, 7)
    x = torch.zeros(3, 6, 7, dtype=torch.float64)
    zm = basins.ZoneMap(torch.zeros(1, 6, 7, dtype=torch.uint32), ["a"], torch.from_numpy(lon), torch.from_numpy(lat))
    assert len(zm) == 1 and zm.shape == (6, 7) and zm.mask(0).dtype == torch.uint8
    calls = [lambda: basins.rasterize([sq], torch.from_numpy(lon), torch.from_numpy(lat)),
             lambda: basins.rasterize([sq], lon, torch.from_numpy(lat)),
             lambda: basins.rasterize([sq], lon, lat, device="cpu"),
             lambda: basins.zone_mean(x, zm),
             lambda: basins.basin_series(x, (lon, lat), x, (lon, lat), [sq])]
    for call in calls:
        with pytest.raises(L.GandanetError):
            call()
