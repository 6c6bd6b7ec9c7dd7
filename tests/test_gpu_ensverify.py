"""GPU: gd_ens_verify (csrc/ensverify.hip) equals its host twin bit for bit on every map and every record field but
sum crps_gauss (each side's erf and exp), and stays inside the bounds of tests/ensverify_util.py against the numpy oracle:
M on both sides of the 8-member instantiation, ragged and one-element planes, both dtypes, arrays one element past a
16-byte boundary, member strides larger than n, a second trip of the grid-stride loop and of the plane loop, NaN, masks and
the scale.  Then EnsembleVerification over the batches of a slab, and evaluate_ensemble(verify=True) on a tiny ensemble.
Each test prints its largest error over its bound (python -m pytest -s)."""
import math

import numpy as np
import pytest
import torch

import ensverify_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _to_dev(a):
    """a device tensor with the strides and the offset of the numpy view `a` (the whole base buffer travels)"""
    base = a
    while base.base is not None:
        base = base.base
    t = torch.from_numpy(np.ascontiguousarray(base).reshape(-1)).to(DEV)
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    return t, torch.as_strided(t, a.shape, [s // a.itemsize for s in a.strides], off)


def _run(x, y, mask=None, scale=1.0, fair=False, ref=None, what="", twin=True):
    from gan_danet_amd import kern as K
    M, dtype = x.shape[0], x.dtype.type
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    xb, xt = _to_dev(x)
    yb, yt = _to_dev(y)
    xb0, yb0 = xb.clone(), yb.clone()
    n = y.size
    pad = 3
    bufs = {k: torch.full((n + 2 * pad,), U.SENTINEL, dtype=tdt, device=DEV) for k in ("crps", "err", "spread")}
    bufs["rank"] = torch.full((n + 2 * pad,), U.SENTINEL_U8, dtype=torch.uint8, device=DEV)
    maps = {k: v[pad:pad + n].view(y.shape) for k, v in bufs.items()}
    rec2 = torch.full((3, U.REC), U.SENTINEL, dtype=torch.float64, device=DEV)
    mt = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(DEV)
    K.ens_verify(xt, yt, rec2[1], mt, scale, fair, maps["crps"], maps["err"], maps["spread"], maps["rank"])
    only = torch.zeros(U.REC, dtype=torch.float64, device=DEV)
    K.ens_verify(xt, yt, only, mt, scale, fair)                              # record only: the same bits
    torch.cuda.synchronize()
    assert all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in ((xb, xb0), (yb, yb0))), what + ": an input was written"
    for k, v in bufs.items():                                                 # nothing around a map is touched
        s = U.SENTINEL_U8 if k == "rank" else U.SENTINEL
        assert (v[:pad] == s).all() and (v[pad + n:] == s).all(), f"{what}: {k} map overran"
    assert (rec2[0] == U.SENTINEL).all() and (rec2[2] == U.SENTINEL).all(), what + ": the record overran"
    rec = rec2[1].cpu().numpy()
    assert np.array_equal(rec, only.cpu().numpy()), what + ": record-only call differs"
    got = {k: v.cpu().numpy() for k, v in maps.items()}
    worst = {}
    if twin:
        hrec, hmaps = K.ens_verify_host(x, y, mask, scale, fair)
        for k in got:
            assert np.array_equal(got[k], hmaps[k], equal_nan=(k != "rank")), f"{what}: {k} map differs from the host twin"
        for f in range(U.REC):
            if f != U.CRPS_GAUSS:
                assert rec[f] == hrec[f], f"{what}: record field {f}: device {rec[f]!r} host twin {hrec[f]!r}"
        scale_g = math.fsum(np.abs(np.nan_to_num(np.asarray(hmaps["err"], np.float64)).ravel())) + \
            math.fsum(np.nan_to_num(np.asarray(hmaps["spread"], np.float64)).ravel())
        assert abs(rec[U.CRPS_GAUSS] - hrec[U.CRPS_GAUSS]) <= 2 * (U.G_RTOL + n * U.U) * scale_g + 1e-300, what + ": sum crps_gauss vs twin"
    if ref is None:
        ref = U.oracle(x, y, mask, scale, fair)
    worst.update(U.check_maps(got, ref, dtype, what))
    worst.update(U.check_rec(rec, ref, what))
    if dtype == np.float64:
        worst["gauss"] = U.check_gauss_sum(rec[U.CRPS_GAUSS], got["err"], got["spread"], ref["valid"], scale, what)
    print(what, {k: f"{v:.3g}" for k, v in worst.items()})
    return rec, got, ref


# M on both sides of 8 and at the bounds; hw 1, around a wave, ragged, several workgroups; 1 to 3 planes
SHAPES = [(1, 1, 1), (2, 3, 63), (3, 2, 64), (7, 1, 65), (8, 3, 257), (9, 2, 4099), (31, 1, 257), (32, 2, 65), (32, 1, 4099), (8, 1, 4099)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("M,planes,hw", SHAPES)
def test_against_twin_and_oracle(M, planes, hw, dtype):
    """every kind at this shape: arrays start one element past a 16-byte boundary, members are n + 5 elements apart"""
    for kind in U.KINDS:
        if kind == "near" and dtype == np.float32:
            continue
        m = U.even_m(M) if kind == "ints" and M < 32 else M
        x, y = U.make(kind, m, planes, hw, dtype, offset=1)
        _run(x, y, what=f"{kind} M={m} {planes}x{hw} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_mask_scale_fair(dtype):
    hw = 257
    mask = (np.random.default_rng(5).random(hw) < 0.7).astype(np.uint8)
    x, y = U.make("gauss", 5, 3, hw, dtype, nans=True, offset=1)
    _run(x, y, mask=mask, scale=509.7, fair=True, what="gauss nan mask fair")
    x, y = U.make("ints", 4, 2, hw, dtype, nans=True)
    _run(x, y, mask=mask, scale=509.7, what="ints nan mask")
    x, y = U.make("gauss", 9, 3, 65, dtype, nans=True)
    one_plane = np.ones((3, 65), np.uint8)
    one_plane[1] = 0                                   # a mask over all three planes with one plane's worth of zeros
    rec, got, ref = _run(x, y, mask=one_plane.reshape(-1), what="one plane masked")
    assert np.isnan(got["crps"][1]).all() and (got["rank"][1] == 255).all() and rec[U.N] == ref["n"] < 2 * 65 + 1
    rec, got, _ = _run(x, y, mask=np.zeros(65, np.uint8), what="all masked")
    assert not rec.any() and np.isnan(got["err"]).all() and (got["rank"] == 255).all()


def test_second_trip_of_the_grid_stride_loop():
    """M = 2 just past 1024 workgroups x 256 threads, and 513 planes of 257 under a mask (gx = 2, gy = 512): ~3 MB each"""
    n = 1024 * 256 + 37
    x, y = U.make("gauss", 2, 1, n, np.float32, offset=1)
    rec, _, _ = _run(x, y, what="grid stride")
    assert rec[U.N] == n
    x, y = U.make("gauss", 2, 513, 257, np.float32, nans=True)
    mask = (np.random.default_rng(6).random(257) < 0.8).astype(np.uint8)
    _run(x, y, mask=mask, what="plane stride")


def test_crps_gauss_per_element():
    """one call per element gives crps_gauss of that element alone: the largest error against this file's formula on the
    call's own fp64 err and spread, relative to s (|z| + 1) = |e| + s, is what ensverify_util.G_MEASURED records"""
    from gan_danet_amd import kern as K
    worst = 0.0
    for kind, M, scale in (("gauss", 5, 1.0), ("near", 8, 509.7), ("outlier", 32, 1.0), ("ints", 2, 1.0)):
        x, y = U.make(kind, M, 1, 96, np.float64, seed=3)
        _, xt = _to_dev(x)
        _, yt = _to_dev(y)
        n = y.size
        recs = torch.zeros((n, U.REC), dtype=torch.float64, device=DEV)
        err, spread = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, dtype=torch.float64, device=DEV)
        for j in range(n):
            K.ens_verify(xt[:, :, j:j + 1], yt[:, j:j + 1], recs[j], None, scale, False, None, err[j:j + 1], spread[j:j + 1])
        g, e, s = recs[:, U.CRPS_GAUSS].cpu().numpy(), err.cpu().numpy(), spread.cpu().numpy()
        diff, w = np.abs(g - U.gauss_formula(e, s)), U.gauss_weight(e, s)
        assert not diff[w == 0].any()                  # e = s = 0: exactly 0
        worst = max(worst, float(np.max(diff[w > 0] / w[w > 0])))
        assert (recs[:, U.N] == 1).all()
    print(f"crps_gauss: largest error / (s (|z| + 1)) = {worst:.4g}  (G_MEASURED {U.G_MEASURED:.4g}, bound {U.G_RTOL:.4g})")
    assert worst <= U.G_RTOL


def test_chunks_add_up():
    """EnsembleVerification over the batches of a slab: the counts of one call exactly, the sums within the bound"""
    import gan_danet_amd as gd
    M, B, hw = 5, 7, 257
    x, y = U.make("gauss", M, B, hw, np.float32, nans=True, seed=2)
    mask = (np.random.default_rng(7).random(hw) < 0.75).astype(np.uint8)
    ref = U.oracle(x, y, mask, 509.7, True)
    _, xt = _to_dev(x)
    _, yt = _to_dev(y)
    mt = torch.from_numpy(mask).to(DEV)
    whole, maps = gd.ensemble_scores(xt, yt, mask=mt, scale=509.7, fair=True, maps=True)
    ev = gd.EnsembleVerification(DEV, M, mask=mt, scale=509.7, fair=True, capacity=1)
    for lo in range(0, B, 3):
        ev.update(xt[:, lo:lo + 3], yt[lo:lo + 3])
    assert len(ev) == 3 and ev.records().shape == (3, U.REC)
    got = ev.compute()
    from gan_danet_amd import kern as K
    rec = np.asarray(K.ens_verify_merge_host(ev.records().cpu().numpy(), M)[0])
    U.check_rec(rec, ref, "chunks")
    assert got["n"] == whole["n"] == ref["n"] and got["rank_counts"] == whole["rank_counts"] and got["cover_counts"] == whole["cover_counts"]
    want = U.metrics_np(ref["rec"], M)
    for k in ("crps", "mae", "rmse", "spread", "spread_skill", "reliability", "tied"):
        assert math.isclose(got[k], want[k], rel_tol=1e-12) and math.isclose(whole[k], want[k], rel_tol=1e-12), k
    U.check_maps({k: v.cpu().numpy() for k, v in maps.items()}, ref, np.float32, "ensemble_scores maps")
    again = gd.EnsembleVerification(DEV, M, mask=mt, scale=509.7, fair=True)
    again.add_records(ev.records().cpu().numpy())
    assert again.compute() == got
    with pytest.raises(gd.verification.L.GandanetError):
        gd.EnsembleVerification(DEV, 1, fair=True)
    with pytest.raises(gd.verification.L.GandanetError):
        gd.EnsembleVerification(DEV, 3, scale=-1.0)


def test_evaluate_ensemble_verify():
    """three generators of the smallest configuration of test_gpu_eval.py: evaluate_ensemble(verify=True) against the
    oracle on the members' own predictions, and against checkpoint.predict_ensemble's mean / std"""
    import gan_danet_amd as gd
    from gan_danet_amd import checkpoint
    from gan_danet_amd import kern as K
    from gan_danet_amd.data import DeviceTileDataset

    rs = np.random.RandomState(0)
    T = 5
    ds = DeviceTileDataset(rs.randn(T, 32, 32).astype(np.float32), rs.randn(T, 64, 64).astype(np.float32),
                           rs.randn(T, 64, 64, 7).astype(np.float32), device=DEV)

    def member(seed):
        torch.manual_seed(seed)
        G = gd.FlexibleUpsamplingModule(input_channels=8).to(DEV)
        G.apply(gd.weights_init_normal)
        G.train()
        with torch.no_grad():                       # one train-mode pass: the BN running statistics leave (0, 1)
            G(K.combine_inputs(ds.lr_grace_05[:2], ds.hr_aux[:2], 0.5, 0.25))
        return G

    affine = (509.7, -3.25)
    valid = np.random.default_rng(1).random((64, 64)) < 0.6
    with gd.precision("fp32"):
        Gs = [member(42 + i) for i in range(3)]
        plain = gd.evaluate_ensemble(Gs, ds, batch_size=2, mask=valid, affine=affine)
        res = gd.evaluate_ensemble(Gs, ds, batch_size=2, mask=valid, affine=affine, verify=True, fair=True)
        for g in Gs:
            g.eval()
        with torch.no_grad():
            xs = [K.combine_inputs(*[ds.get(lo, min(T, lo + 2))[i] for i in (0, 2)], 0.5, 0.25) for lo in (0, 2, 4)]
            members = torch.cat([torch.stack([g(x) for g in Gs], 0) for x in xs], 1).cpu().numpy()       # (M, T, C, H, W)
            mean, std = [torch.cat(t, 0).cpu().numpy().astype(np.float64) for t in zip(*[checkpoint.predict_ensemble(Gs, x) for x in xs])]
        for g in Gs:
            g.train()
        with pytest.raises(gd.verification.L.GandanetError, match="scale"):
            gd.evaluate_ensemble(Gs, ds, batch_size=2, affine=(-1.0, 0.0), verify=True)
    assert set(plain) == {"mean_preds", "std_preds", "r2", "members", "mean_map", "std_map", "preds_ts", "trues_ts"}
    assert set(res) == set(plain) | {"verification", "crps_map", "rank_map"}
    for k in plain:
        a, b = plain[k], res[k]
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b, k
    truth = ds.lr_grace_025.cpu().numpy().reshape(members.shape[1:])
    ref = U.oracle(members, truth, valid.astype(np.uint8), affine[0], True)
    ver = res["verification"]
    assert res["crps_map"].shape == res["rank_map"].shape == res["mean_map"].shape and res["rank_map"].dtype == torch.uint8
    assert np.array_equal(res["rank_map"].cpu().numpy(), ref["rank"])
    crps = res["crps_map"].cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(crps), ~ref["valid"])
    bound = ref["tol"]["crps"] + U.ulp(ref["crps"], np.float32)
    assert (np.abs(crps - ref["crps"])[ref["valid"]] <= bound[ref["valid"]]).all()
    want = U.metrics_np(ref["rec"], 3)
    assert ver["n"] == ref["n"] == T * int(valid.sum()) and ver["rank_counts"] == list(ref["rec"][U.HIST:U.HIST + 4])
    assert ver["cover_counts"] == list(ref["rec"][U.COVER:U.COVER + 4])
    for k in ("crps", "mae", "rmse", "spread", "spread_skill", "reliability", "tied"):
        assert math.isclose(ver[k], want[k], rel_tol=1e-12), k
    # predict_ensemble: fp32 mean and population std of the same members
    e = np.abs((mean - truth) * affine[0])[:, :, valid]
    s2 = (std ** 2 * 1.5 * affine[0] ** 2)[:, :, valid]
    assert math.isclose(ver["mae"], e.mean(), rel_tol=1e-4) and math.isclose(ver["spread"], math.sqrt(s2.mean()), rel_tol=1e-4)
