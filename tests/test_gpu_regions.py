"""GPU: the regionalisation kernels (csrc/kmeans.hip) against their host twins bit for bit on every output of gd_km_assign,
gd_km_update and gd_km_farthest -- around the staging chunk of 64 steps, the block of 256 series, the four register instances
(K <= 8 / 16 / 32 / 64), the slab of 1024 pixels and the limits of T and K -- and against the long-double oracle of
regions_util.py; run-to-run, placement and workspace independence; and the public module gan_danet_amd.regions.

Measured on an MI355X: the device equalled the host twin bit for bit in every case; the file takes 5 s."""
import numpy as np
import pytest
import torch

import regions_util as U

pytestmark = pytest.mark.gpu


def _K():
    from gan_danet_amd import kern
    return kern


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _np(t):
    return None if t is None else t.cpu().numpy()


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), what
        if g is not None:
            assert _eq(_np(g), w), (what, i)


def _both(x, cent, w=None, shift=None, scale=None, mask=None, what=None, ws=None):
    """assign and update on the device, each held against its twin bit for bit; returns the device outputs as numpy"""
    K = _K()
    xd = _dev(x)
    got = K.km_assign(xd, _dev(cent), _dev(shift), _dev(scale), _dev(mask), True)
    want = K.km_assign_host(x, cent, shift, scale, mask, True)
    _same(got, want, (what, "assign"))
    up = K.km_update(xd, got[0], got[1], _dev(cent), _dev(w), _dev(shift), _dev(scale), ws)
    _same(up, K.km_update_host(x, want[0], want[1], cent, w, shift, scale), (what, "update"))
    return [_np(g) for g in got], [_np(u) for u in up]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", (1, 3, 63, 64, 65, 181))
def test_device_equals_twin_and_oracle(T, dtype):
    for M, Ks in ((1, (1, 64)), (65, (2, 9)), (257, (7, 8, 33, 64))):
        for Kc in Ks:
            x, cent, _ = U.blobs(T, M, Kc, dtype)
            mask = U.mask_for(M) if M == 65 else None
            w = np.cos(np.linspace(-1.2, 1.2, M)) if M == 257 else None
            got, up = _both(x, cent, w, mask=mask, what=(T, M, Kc))
            want = U.assign(x, cent, mask=mask)
            U.check_assign(got, want, (T, M, Kc))
            U.check_update(up, U.update(x, want["label"], want["dist"], want["bound"], cent, w), (T, M, Kc))


def test_limits_and_slabs():
    """T = 2048 with K = 64 at M = 3; three slabs with shift and scale"""
    x, cent, _ = U.blobs(2048, 3, 64)
    got, _ = _both(x, cent, what="T = 2048")
    U.check_assign(got, U.assign(x, cent), "T = 2048")
    x, cent, _ = U.blobs(33, 2500, 17, np.float32)
    shift, scale = x.mean(axis=0).astype(np.float64), np.linspace(0.5, 2.0, 2500)
    _both(x, cent, np.linspace(0.25, 1.75, 2500), shift, scale, U.mask_for(2500), what="three slabs")


def test_integer_data_and_ties_on_the_device():
    rng = np.random.default_rng(5)
    x = rng.integers(-8, 9, size=(65, 300)).astype(np.float64)
    cent = rng.integers(-4, 5, size=(9, 65)).astype(np.float64) / 4.0
    cent[3] = cent[1]
    x[:, 7] = cent[1]
    got, _ = _both(x, cent, what="ties")
    want = U.assign(x, cent)
    assert _eq(got[0], want["label"]) and _eq(got[2], want["label2"]) and _eq(got[1], want["dist"].astype(np.float64))
    assert got[0][7] == 1 and got[2][7] == 3


def test_two_runs_and_a_shifted_placement_give_the_same_bits():
    K = _K()
    for dtype in (np.float64, np.float32):
        x, cent, _ = U.blobs(65, 257, 9, dtype)
        xd, cd = _dev(x), _dev(cent)
        a = K.km_assign(xd, cd, second=True)
        b = K.km_assign(xd, cd, second=True)
        buf = torch.empty(x.size + 8, dtype=xd.dtype, device="cuda")
        off = next(o for o in range(1, 8) if (buf.data_ptr() + o * buf.element_size()) % 16 == buf.element_size())
        moved = buf[off:off + x.size].view(x.shape)
        moved.copy_(xd)
        assert moved.data_ptr() % 16 == moved.element_size()              # one element past a 16-byte boundary
        c = K.km_assign(moved, cd, second=True)
        for p, q, r in zip(a, b, c):                                      # no NaN here: nothing masked, K > 1
            assert torch.equal(p, q) and torch.equal(p, r)
        ua, ub, uc = (K.km_update(t, a[0], a[1], cd) for t in (xd, xd, moved))
        for p, q, r in zip(ua, ub, uc):
            assert torch.equal(p, q) and torch.equal(p, r)


def test_workspace_independence():
    K = _K()
    x, cent, _ = U.blobs(33, 5000, 7)
    w = np.linspace(0.25, 1.75, 5000)
    need, full = K.km_update_min_workspace(33, 7), K.km_update_workspace(33, 5000, 7)
    assert full == 6 * need // 2
    _, a = _both(x, cent, w, what="full workspace")
    _, b = _both(x, cent, w, what="smallest workspace", ws=torch.empty(need, dtype=torch.uint8, device="cuda"))
    _, c = _both(x, cent, w, what="two slabs at a time", ws=torch.empty(need // 2 * 3 + 5, dtype=torch.uint8, device="cuda"))
    for p, q, r in zip(a, b, c):
        assert _eq(p, q) and _eq(p, r)
    with pytest.raises(K.L.GandanetError, match="workspace"):
        _both(x, cent, w, ws=torch.empty(need - 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(K.L.GandanetError):
        K.km_assign(torch.zeros(4, 8, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64))   # CPU tensors are refused


def test_farthest_equals_twin():
    K = _K()
    rng = np.random.default_rng(2)
    for M in (1, 63, 1024, 1025, 70001):
        d = rng.integers(0, 40, size=M).astype(np.float64)
        d[rng.integers(0, M, size=M // 7)] = np.nan
        ex = []
        for _ in range(5):
            e = np.array(ex, dtype=np.int32) if ex else None
            got = int(K.km_farthest(_dev(d), _dev(e)).cpu()[0])
            assert got == int(K.km_farthest_host(d, e)[0]) == U.farthest(d, ex), (M, ex)
            ex.append(got if got >= 0 else 0)
    assert int(K.km_farthest(_dev(np.full(300, np.nan))).cpu()[0]) == -1


def _cube(seed=0, T=24, H=9, W=11, k=4, spread=0.05, sep=3.0):
    rng = np.random.default_rng(seed)
    centres = sep * rng.standard_normal((k, T))
    lab = rng.integers(0, k, size=(H, W))
    lab.reshape(-1)[:k] = np.arange(k)
    return centres[lab].transpose(2, 0, 1) + spread * rng.standard_normal((T, H, W)), lab, centres


def test_kmeans_series_equals_the_loop_over_the_twins():
    """explicit starting centroids and "maximin" on a (24, 9, 11) cube, k = 4: labels, centroids, inertia and n_iter"""
    import gan_danet_amd as gd
    K = _K()
    x, _, centres = _cube()
    x2 = np.ascontiguousarray(x.reshape(24, -1))
    rng = np.random.default_rng(1)
    start = centres + 2.0 * rng.standard_normal(centres.shape)
    start[3] = 50.0                                                   # starts empty: re-seated on the farthest pixel
    for init_host, init_dev in ((start, _dev(start)), (U.host_maximin(K, x2, 4), "maximin")):
        label, cent, inertia, n_iter, converged = U.host_kmeans(K, x2, init_host)
        r = gd.kmeans_series(_dev(x), 4, init=init_dev)
        assert _eq(_np(r.labels).reshape(-1), label) and _eq(_np(r.centroids), cent)
        assert float(r.inertia) == inertia and r.n_iter == n_iter and r.converged == converged and converged
        assert int(r.counts.sum()) == 99 and int(r.counts.min()) > 0


@pytest.mark.parametrize("init", ["maximin", "random", "kmeans++", "explicit"])
def test_planted_partition_is_recovered(init):
    """k = 4 blobs on a (24, 12, 13) cube: the steps of a centre are 10 N(0, 1), a member adds 0.005 N(0, 1) per step.  Two
    centres are then about 10 sqrt(2 * 24) ~ 69 apart (squared: ~4800) while two members of one blob are about 0.005 sqrt(2 * 24)
    ~ 0.035 apart (squared: ~1.2e-3), a ratio of 2.5e-7 per pixel.  D^2 sampling ("kmeans++") picks a pixel of an already
    covered blob at draw j with probability ~ 2.5e-7 * (covered pixels / uncovered pixels) = 2.5e-7 * (1/3, 2/2, 3/1): about 1e-6
    over the three draws; otherwise every blob holds one starting centre and Lloyd's first assignment is the planted partition.
    "maximin" and explicit centres are deterministic.  "random" puts its 4 pixels into 4 different blobs in only 4! / 4^4 = 9 % of
    the draws and Lloyd does not leave the local optimum it starts in otherwise, so it is run with n_init = 8, which keeps the
    run of least inertia: for the seed used here the second run (seed + 1) draws one pixel per blob, which the host twins
    confirm without a GPU."""
    import gan_danet_amd as gd
    x, lab, centres = _cube(seed=4, H=12, W=13, spread=0.005, sep=10.0)
    start = _dev(centres + 0.5) if init == "explicit" else init
    r = gd.kmeans_series(_dev(x), 4, init=start, seed=3, n_init=8 if init == "random" else 1)
    assert U.ari(_np(r.labels), lab) == 1.0
    assert torch.equal(r.predict(_dev(x)), r.labels)
    s_map, s_mean = r.silhouette()
    assert float(s_mean) > 0.99 and float(s_map.min()) > 0.99


def test_zonemap_region_series_and_centroids():
    import gan_danet_amd as gd
    from gan_danet_amd.basins import zone_mean
    x, lab, _ = _cube(seed=7, H=12, W=13)
    xd = _dev(x)
    r = gd.kmeans_series(xd, 4)
    zm = r.to_zonemap(np.arange(13.0), np.arange(12.0))
    assert len(zm) == 4 and zm.bits.shape == (1, 12, 13) and zm.bits.dtype == torch.uint32
    for z in range(4):
        assert torch.equal(zm.mask(z).bool(), r.labels == z)
    mean, count = zone_mean(xd, zm)
    rs_mean, rs_count = r.region_series(xd)
    assert torch.equal(mean, rs_mean) and torch.equal(count, rs_count) and torch.equal(count[0], r.counts)
    o = U.update(x.reshape(24, -1), _np(r.labels).reshape(-1), np.zeros(156), np.zeros(156), np.zeros((4, 24)))
    # zone_mean adds the same members in another order: the same bound holds for it, so the two lie within two bounds
    assert U.worst(_np(r.centroids).astype(U.LD) - o["cent"], o["cent_bound"]) <= 1.0
    assert U.worst(_np(mean).T.astype(U.LD) - o["cent"], o["cent_bound"]) <= 1.0
    big = gd.kmeans_series(_dev(np.random.default_rng(1).standard_normal((6, 12, 40))), 40, max_iter=2)   # two words of bits
    zb = big.to_zonemap(np.arange(40.0), np.arange(12.0))
    assert zb.bits.shape == (2, 12, 40) and all(torch.equal(zb.mask(z).bool(), big.labels == z) for z in (0, 31, 32, 39))


def test_region_agreement_and_reorder():
    import gan_danet_amd as gd
    x, lab, _ = _cube(seed=9, H=12, W=13)
    r = gd.kmeans_series(_dev(x), 4)
    perm = np.array([2, 0, 3, 1])
    other = torch.where(r.labels >= 0, _dev(perm.astype(np.int32))[r.labels.clamp_min(0).long()], r.labels)
    out = gd.region_agreement(r.labels, other)
    assert out["ari"] == 1.0 and out["purity"] == 1.0 and sorted(out["matching"]) == [(k, int(perm[k])) for k in range(4)]
    assert int(out["table"].sum()) == 156
    s = r.reorder("size")
    c = _np(s.counts)
    assert (np.diff(c) <= 0).all() and gd.region_agreement(r.labels, s.labels)["ari"] == 1.0
    for z in range(4):
        assert int((s.labels == z).sum()) == c[z]
    m = _np(r.reorder("centroid_mean").centroids).mean(axis=1)
    assert (np.diff(m) >= 0).all()


def test_scan_inertia_falls_with_k():
    """nested blobs: 8 tight blobs in 4 groups in 2 super-groups; under "maximin" the inertia does not rise with k"""
    import gan_danet_amd as gd
    rng = np.random.default_rng(11)
    top = 20.0 * rng.standard_normal((2, 12))
    mid = top[np.arange(4) // 2] + 4.0 * rng.standard_normal((4, 12))
    leaf = mid[np.arange(8) // 2] + 0.8 * rng.standard_normal((8, 12))
    lab = np.arange(160) % 8
    x = (leaf[lab].T + 0.05 * rng.standard_normal((12, 160))).reshape(12, 10, 16)
    out = gd.kmeans_scan(_dev(x), (1, 2, 3, 4, 6, 8), init="maximin")
    assert out["k"] == [1, 2, 3, 4, 6, 8] and (np.diff(out["inertia"]) <= 0).all()
    assert np.isnan(out["silhouette"][0]) and np.isnan(out["calinski_harabasz"][0]) and np.isfinite(out["calinski_harabasz"][1:]).all()
    assert U.ari(_np(out["regions"][-1].labels), lab) == 1.0


def test_normalize_weights_and_no_sync_mode():
    import gan_danet_amd as gd
    x, lab, _ = _cube(seed=13, H=12, W=13)
    x = x + 100.0 * np.random.default_rng(0).standard_normal((1, 12, 13))     # offsets that only "center" / "zscore" remove
    xd = _dev(x.astype(np.float32))
    for norm in ("center", "zscore"):
        r = gd.kmeans_series(xd, 4, normalize=norm, lat=np.linspace(20.0, 40.0, 12))
        assert U.ari(_np(r.labels), lab) == 1.0 and torch.equal(r.predict(xd), r.labels)
    a = gd.kmeans_series(xd, 4, normalize="center", max_iter=5, tol=None)
    b = gd.kmeans_series(xd, 4, normalize="center", max_iter=5, tol=None)
    assert a.converged is None and a.n_iter == 5 and torch.equal(a.labels, b.labels) and torch.equal(a.centroids, b.centroids)
    mask = torch.ones(12, 13, dtype=torch.bool, device="cuda")
    mask[0] = False
    m = gd.kmeans_series(xd, 4, normalize="center", mask=mask)
    assert (m.labels[0] == -1).all() and (m.labels[1:] >= 0).all() and torch.isnan(m.distance[0]).all()


def test_too_few_valid_series_is_an_error_not_a_pick():
    """explicit centroids: an all-NaN cube and a cube with fewer valid series than k are refused before the loop, so no re-seat
    ever looks for a pixel that does not exist; NaN centroids are refused too"""
    import gan_danet_amd as gd
    K = _K()
    x, _, centres = _cube()
    start = _dev(centres)
    with pytest.raises(K.L.GandanetError, match="0 valid series"):
        gd.kmeans_series(_dev(np.full_like(x, np.nan)), 4, init=start)
    gaps = x.copy()
    gaps[5, :, :] = np.nan
    gaps[:, 0, :3] = x[:, 0, :3]                                          # three complete series for k = 4
    mask = torch.zeros(9, 11, dtype=torch.bool, device="cuda")
    mask[0, :3] = True
    for kw in (dict(), dict(mask=mask)):
        src = gaps if not kw else x
        with pytest.raises(K.L.GandanetError, match="3 valid series"):
            gd.kmeans_series(_dev(src), 4, init=start, **kw)
        with pytest.raises(K.L.GandanetError, match="3 valid series"):
            gd.kmeans_series(_dev(src), 4, **kw)
    r = gd.kmeans_series(_dev(gaps), 3, init=_dev(centres[:3]))            # exactly k valid series: every cluster gets one
    assert sorted(_np(r.counts).tolist()) == [1, 1, 1] and int((r.labels >= 0).sum()) == 3
    bad = centres.copy()
    bad[2, 7] = np.nan
    with pytest.raises(K.L.GandanetError, match="NaN or an inf"):
        gd.kmeans_series(_dev(x), 4, init=_dev(bad))


def test_kmeans_pp_never_lands_on_a_left_out_pixel():
    """duplicate series (every remaining D is 0 after the first pick) with the LAST flat pixel masked: the searchsorted pick
    falls on a pixel of zero mass and the farthest valid pixel stands in, so no centroid is NaN"""
    import gan_danet_amd as gd
    x = np.tile(np.linspace(0.0, 1.0, 6)[:, None, None], (1, 4, 5))
    x[:, 3, 4] = np.nan
    r = gd.kmeans_series(_dev(x), 3, init="kmeans++", seed=1, max_iter=3)
    assert bool(torch.isfinite(r.centroids).all()) and int(r.labels[3, 4]) == -1 and int((r.labels >= 0).sum()) == 19
