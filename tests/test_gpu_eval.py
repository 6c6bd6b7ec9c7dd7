"""GPU: the evaluation kernels (evalstats.hip) and the passes built on them against numpy in fp64 on the same fp32 inputs
(tests/eval_np.py).  Shapes are the smallest that reach every path: scalar-only sizes, a ragged tail behind a vector body,
more than one workgroup, pointers one element off a 16-byte boundary, the mask, the affine, both dtypes."""
import math

import numpy as np
import pytest
import torch

from eval_np import check_metrics, metrics, offset_pair, record
from gpu_util import DEV

pytestmark = pytest.mark.gpu


def _K():
    from gan_danet_amd import kern as K
    return K


def _stats(p, t, **kw):
    rec = torch.zeros(8, dtype=torch.float64, device=DEV)
    _K().eval_stats(p, t, rec, **kw)
    return rec.cpu().numpy()


def _check_record(got, want, where):
    assert got[0] == want[0], (where, got[0], want[0])
    scale = math.sqrt(want[3] * want[4])
    for i in (1, 2, 6, 7):
        assert abs(got[i] - want[i]) <= 1e-9 * abs(want[i]), (where, i, got[i], want[i])
    for i in (3, 4, 5):                                # M2_p, M2_t, C_pt relative to sqrt(M2_p M2_t)
        assert abs(got[i] - want[i]) <= 1e-9 * scale, (where, i, got[i], want[i])


def _pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g) * 2.0 + 0.5
    p = t + 0.3 * torch.randn(*shape, generator=g)
    return p, t


@pytest.mark.parametrize("shape", [(1,), (3,), (255,), (256 * 4 + 1,), (2, 1, 64, 64)])
def test_eval_stats_shapes(shape):
    K = _K()
    p, t = _pair(shape, 11 + len(shape) + shape[0])
    got = _stats(p.to(DEV), t.to(DEV))
    want = record(p.numpy(), t.numpy())
    _check_record(got, want, f"shape {shape}")
    m = K.eval_merge_host([got])[1]
    if p.numel() > 1:
        check_metrics(m, metrics(p.numpy(), t.numpy()), f"shape {shape}")
    else:
        # one sample: r2_score and np.corrcoef are undefined, so the check is what include/gandanet.h defines --
        # SS_tot == 0 with an imperfect prediction gives r2 0.0, a zero variance gives cc NaN
        d = float(p[0]) - float(t[0])
        assert d != 0.0 and m["n"] == 1.0
        assert abs(m["mse"] - d * d) <= 1e-9 * d * d and abs(m["mae"] - abs(d)) <= 1e-9 * abs(d), (m, d)
        assert m["r2"] == 0.0 and math.isnan(m["cc"]), m
    # two calls on the same input: bit-identical records
    again = _stats(p.to(DEV), t.to(DEV))
    assert got.tobytes() == again.tobytes()


def test_eval_stats_pointers_one_element_off():
    n = 256 * 4 * 3 + 2
    p, t = _pair((n + 1,), 5)
    pd, td = p.to(DEV), t.to(DEV)
    assert pd.data_ptr() % 16 == 0 and td.data_ptr() % 16 == 0
    K = _K()
    # both one element past a 16-byte boundary: head of 3, vector body, tail
    got = _stats(pd[1:], td[1:])
    _check_record(got, record(p[1:].numpy(), t[1:].numpy()), "both offset")
    check_metrics(K.eval_merge_host([got])[1], metrics(p[1:].numpy(), t[1:].numpy()), "both offset")
    # only one of them offset: the two never share a 16-byte boundary, scalar sweep
    got = _stats(pd[1:], td[:-1])
    _check_record(got, record(p[1:].numpy(), t[:-1].numpy()), "one offset")
    check_metrics(K.eval_merge_host([got])[1], metrics(p[1:].numpy(), t[:-1].numpy()), "one offset")


def test_eval_stats_mask_affine_offset_data():
    K = _K()
    shape = (2, 1, 64, 64)
    p, t = _pair(shape, 21)
    rng = np.random.default_rng(4)
    mask = (rng.random((64, 64)) < 0.6)
    pm, tm = p.numpy()[:, :, mask], t.numpy()[:, :, mask]          # the mask is shared by the two planes
    got = _stats(p.to(DEV), t.to(DEV), mask=torch.from_numpy(mask.astype(np.uint8)).to(DEV))
    _check_record(got, record(pm, tm), "mask")
    check_metrics(K.eval_merge_host([got])[1], metrics(pm, tm), "mask")
    # masked-out pixels may hold anything, NaN included
    p2 = p.clone()
    p2[:, :, torch.from_numpy(~mask)] = float("nan")
    got2 = _stats(p2.to(DEV), t.to(DEV), mask=torch.from_numpy(mask.astype(np.uint8)).to(DEV))
    _check_record(got2, record(pm, tm), "mask over NaN")

    a, b = 37.25, -1234.5                                            # StandardScaler inverse: v * scale + mean
    got = _stats(p.to(DEV), t.to(DEV), affine=(a, b))
    pa, ta = p.numpy().astype(np.float64) * a + b, t.numpy().astype(np.float64) * a + b
    _check_record(got, record(pa, ta), "affine")
    check_metrics(K.eval_merge_host([got])[1], metrics(pa, ta), "affine")

    x, y = offset_pair(2 * 64 * 64, seed=1)                          # 1000 +- 0.01: no raw fp32 sum of squares survives
    xt, yt = torch.from_numpy(x).view(shape), torch.from_numpy(y).view(shape)
    got = _stats(yt.to(DEV), xt.to(DEV))
    _check_record(got, record(y, x), "offset data")
    check_metrics(K.eval_merge_host([got])[1], metrics(y, x), "offset data")
    assert got.tobytes() == _stats(yt.to(DEV), xt.to(DEV)).tobytes()


def test_eval_stats_fp64_and_nan_rows():
    """the (T, C) series of evaluate_ensemble: fp64 inputs, pairs with a NaN on either side skipped"""
    rng = np.random.default_rng(9)
    t = rng.standard_normal((37, 3)) + 4.0
    p = t + 0.1 * rng.standard_normal((37, 3))
    t[5, 1] = np.nan
    p[5, 1] = np.nan
    p[20, 0] = np.nan
    ok = ~np.isnan(t) & ~np.isnan(p)
    got = _stats(torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV), skip_nan=True)
    _check_record(got, record(p[ok], t[ok]), "fp64 skip-nan")


def test_masked_plane_mean():
    K = _K()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 2, 16, 24, generator=g) + 2.0
    rng = np.random.default_rng(2)
    mask = rng.random((16, 24)) < 0.6
    xm = x.numpy().astype(np.float64).copy()
    xm[:, :, ~mask] = np.nan
    want = np.nanmean(xm, axis=(2, 3))
    mean, count = K.masked_plane_mean(x.to(DEV), torch.from_numpy(mask.astype(np.uint8)).to(DEV))
    assert mean.shape == (3, 2) and mean.dtype == torch.float64 and count.dtype == torch.int64
    assert np.all(count.cpu().numpy() == mask.sum())
    np.testing.assert_allclose(mean.cpu().numpy(), want, rtol=1e-12, atol=0)
    # a mask that leaves no valid pixel: NaN and count 0 in every plane
    none = torch.zeros(16, 24, dtype=torch.uint8, device=DEV)
    mean, count = K.masked_plane_mean(x.to(DEV), none)
    assert torch.isnan(mean).all() and (count == 0).all()
    # planes that are not 16-byte aligned (hw = 15 * 23 is odd) and no mask
    y = torch.randn(5, 15, 23, generator=g) - 1.0
    mean, count = K.masked_plane_mean(y.to(DEV)[1:], None)
    np.testing.assert_allclose(mean.cpu().numpy(), y[1:].double().mean((1, 2)).numpy(), rtol=1e-12, atol=0)
    assert (count == 15 * 23).all()
    # the invalid pixels of a plane may hold NaN (the notebook's own masked arrays do)
    xn = x.clone()
    xn[:, :, torch.from_numpy(~mask)] = float("nan")
    mean, _ = K.masked_plane_mean(xn.to(DEV), torch.from_numpy(mask.astype(np.uint8)).to(DEV))
    np.testing.assert_allclose(mean.cpu().numpy(), want, rtol=1e-12, atol=0)


_MB_SHAPE = (2, 3, 37, 61)   # 6 planes of 2257 elements: three workgroups per plane, every 16-byte misalignment of a plane


def _multiblock_case(dtype):
    """(x, mask, np.nanmean of the masked planes in fp64) for test_masked_plane_mean_multiblock"""
    if dtype not in _multiblock_case.cache:
        g = torch.Generator().manual_seed(17)
        x = torch.randn(*_MB_SHAPE, generator=g, dtype=dtype) + 2.0
        mask = np.random.default_rng(6).random(_MB_SHAPE[2:]) < 0.6
        xm = x.numpy().astype(np.float64)
        xm[:, :, ~mask] = np.nan
        _multiblock_case.cache[dtype] = (x, mask, np.nanmean(xm, axis=(2, 3)))
    return _multiblock_case.cache[dtype]


_multiblock_case.cache = {}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_masked_plane_mean_multiblock(dtype):
    """planes of 2257 elements take three workgroups each (2257 > 2 * 1024; the cap of 2048 / planes does not bind), so
    the per-plane partials and their ordered final add are in play; 2257 is odd, so successive planes start 0, 3, 2, 1
    (fp32) or 0, 1 (fp64) elements before a 16-byte boundary.  Means against np.nanmean in fp64 at rtol 1e-12 (a few
    1e-16 expected over ~1350 fp64 addends), counts exact.  A NaN at a mask-valid pixel: the fp32 entry propagates it
    into that plane's mean, the fp64 entry leaves the pixel out and counts one less."""
    K = _K()
    fn = K.masked_plane_mean if dtype == torch.float32 else K.masked_plane_mean_f64
    x, mask, want = _multiblock_case(dtype)
    hw = math.prod(_MB_SHAPE[2:])
    assert hw == 2257 and mask[0, 0] and not mask.all()
    md = torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    xd = x.to(DEV)
    assert xd.data_ptr() % 16 == 0

    def check(mean, count, want_mean, want_count, where):
        print(where, dtype, "max rel err", np.max(np.abs(mean.cpu().numpy() / want_mean - 1.0)))
        assert mean.shape == _MB_SHAPE[:2] and mean.dtype == torch.float64 and count.dtype == torch.int64, where
        assert np.array_equal(count.cpu().numpy(), np.broadcast_to(want_count, _MB_SHAPE[:2])), where
        np.testing.assert_allclose(mean.cpu().numpy(), want_mean, rtol=1e-12, atol=0, err_msg=where)

    check(*fn(xd, md), want, mask.sum(), "mask")
    check(*fn(xd, None), np.nanmean(x.numpy().astype(np.float64), axis=(2, 3)), hw, "no mask")
    # the same planes one element into a larger buffer: every plane's head changes
    buf = torch.empty(x.numel() + 1, dtype=dtype, device=DEV)
    buf[1:] = xd.reshape(-1)
    check(*fn(buf[1:].view(_MB_SHAPE), md), want, mask.sum(), "offset view")
    # the masked-out pixels may hold NaN
    xn = x.clone()
    xn[:, :, torch.from_numpy(~mask)] = float("nan")
    check(*fn(xn.to(DEV), md), want, mask.sum(), "mask over NaN")
    # a NaN at a valid pixel of plane (1, 2)
    xv = x.clone()
    xv[1, 2, 0, 0] = float("nan")
    mean, count = fn(xv.to(DEV), md)
    mean, count = mean.cpu().numpy(), count.cpu().numpy()
    other = np.ones(_MB_SHAPE[:2], dtype=bool)
    other[1, 2] = False
    np.testing.assert_allclose(mean[other], want[other], rtol=1e-12, atol=0)
    if dtype == torch.float32:
        assert np.isnan(mean[1, 2]) and np.all(count == mask.sum())
    else:
        xm = xv.numpy().copy()
        xm[:, :, ~mask] = np.nan
        np.testing.assert_allclose(mean[1, 2], np.nanmean(xm[1, 2]), rtol=1e-12, atol=0)
        assert count[1, 2] == mask.sum() - 1 and np.all(count[other] == mask.sum())


@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 2.4e-7), (torch.float64, 1e-14)])
@pytest.mark.parametrize("M", [1, 5, 32])
def test_ensemble_stats(M, dtype, rtol):
    K = _K()
    g = torch.Generator().manual_seed(100 + M)
    for shape in [(5,), (1024 + 3,), (2, 1, 64, 64)]:
        n = math.prod(shape)
        for stride in (n, n + 12, n + 5):             # dense; padded and 16-byte friendly; padded and not
            slab = torch.zeros(M, stride, dtype=dtype)
            slab[:, :n] = torch.randn(M, n, generator=g, dtype=torch.float64).to(dtype) * 0.5 + 3.0
            dslab = slab.to(DEV)
            x = dslab[:, :n].unflatten(1, shape)               # a view: members `stride` elements apart
            assert x.stride(0) == stride or M == 1
            mean, std = K.ensemble_stats(x)
            ref = slab[:, :n].numpy().astype(np.float64)
            assert mean.shape == shape and mean.dtype == dtype
            np.testing.assert_allclose(mean.cpu().numpy().ravel(), ref.mean(0), rtol=rtol, atol=0)
            want_std = ref.std(0, ddof=0)
            if M == 1:
                assert (std == 0).all()
            else:
                np.testing.assert_allclose(std.cpu().numpy().ravel(), want_std, rtol=rtol, atol=0)
    # identical members: std exactly 0, mean exactly the member
    one = (torch.randn(1, 1027, generator=g, dtype=torch.float64) * 0.1 + 0.1).to(dtype)
    same = one.repeat(M, 1).to(DEV)
    mean, std = K.ensemble_stats(same)
    assert (std == 0).all() and torch.equal(mean.cpu(), one[0])
    # outputs one element off a 16-byte boundary
    buf_m, buf_s = torch.zeros(1028, dtype=dtype, device=DEV), torch.zeros(1028, dtype=dtype, device=DEV)
    K.ensemble_stats(same, buf_m[1:], buf_s[1:])
    assert torch.equal(buf_m[1:].cpu(), one[0]) and (buf_s == 0).all()


def test_evaluate_end_to_end():
    import gan_danet_amd as gd
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

    def forwards(G):
        G.eval()
        with torch.no_grad():
            out = [G(K.combine_inputs(*[ds.get(lo, min(T, lo + 2))[i] for i in (0, 2)], 0.5, 0.25)) for lo in (0, 2, 4)]
        G.train()
        return torch.cat(out, 0).cpu().numpy()

    with gd.precision("fp32"):
        Gs = [member(42 + i) for i in range(3)]
        G = Gs[0]
        own = forwards(G)
        truth = ds.lr_grace_025.cpu().numpy()
        buffers = {k: v.clone() for k, v in G.state_dict().items() if "running" in k or "num_batches" in k}
        assert buffers and any(v.abs().sum() > 0 for k, v in buffers.items() if "running_mean" in k)

        got, preds = gd.evaluate(G, ds, batch_size=2, return_preds=True)
        assert [len(p) for p in preds] == [2, 2, 1]                       # every sample once, ragged tail kept
        assert all(p.grad_fn is None and not p.requires_grad for p in preds)
        np.testing.assert_allclose(torch.cat(preds, 0).cpu().numpy(), own, rtol=1e-5, atol=1e-6)
        check_metrics(got, metrics(own, truth), "evaluate")
        assert all(isinstance(got[k], float) for k in ("n", "mse", "mae", "r2", "cc")) and got["n"] == T * 64 * 64
        assert G.training and all(m.training for m in G.modules())       # back in train mode
        for k, v in G.state_dict().items():
            if k in buffers:
                assert torch.equal(v, buffers[k]), k                     # running statistics and counters untouched
        D = gd.Discriminator1().to(DEV)
        with torch.no_grad():
            D(torch.zeros(1, 1, 64, 64, device=DEV))
        tr = gd.GanTrainer(G, D, perceptual=None)
        assert tr.evaluate(ds, 2) == got
        # evaluation reads the samples as stored: an augmenting dataset gives the same numbers, run after run
        rs2 = np.random.RandomState(0)
        ds_aug = DeviceTileDataset(rs2.randn(T, 32, 32).astype(np.float32), rs2.randn(T, 64, 64).astype(np.float32),
                                   rs2.randn(T, 64, 64, 7).astype(np.float32), augment=True, device=DEV)
        assert gd.evaluate(G, ds_aug, batch_size=2) == got
        empty = DeviceTileDataset(np.zeros((0, 32, 32), np.float32), np.zeros((0, 64, 64), np.float32),
                                  np.zeros((0, 64, 64, 7), np.float32), device=DEV)
        none = gd.evaluate(G, empty, batch_size=2)
        assert none["n"] == 0.0 and all(math.isnan(none[k]) for k in ("mse", "mae", "r2", "cc"))
        with pytest.raises(ValueError, match="empty"):
            gd.evaluate_ensemble([G], empty, batch_size=2)
        # two emulated ranks with uneven shares (3 + 2 samples) cover the same pairs
        r0 = gd.evaluate(G, ds, 2, rank=0, world=2)
        r1 = gd.evaluate(G, ds, 2, rank=1, world=2)
        assert r0["n"] + r1["n"] == got["n"] and r0["n"] == 3 * 64 * 64
        # a mixed train / eval state comes back as it was, also when a forward raises
        class Boom(torch.nn.Module):
            def forward(self, x):
                raise RuntimeError("boom")

        G.eval()
        list(G.modules())[-1].train()
        flags = [m.training for m in G.modules()]
        boom = Boom().train()
        with pytest.raises(RuntimeError, match="boom"):
            gd.evaluate(G, ds, batch_size=2, input_attention=boom)
        assert [m.training for m in G.modules()] == flags and boom.training
        gd.evaluate(G, ds, batch_size=5)
        assert [m.training for m in G.modules()] == flags
        G.train()

        # ---- the ensemble: numpy restatement of compute_uncertainty (deep_ensemble.ipynb:L438-476) ----
        rng = np.random.default_rng(1)
        valid = rng.random((64, 64)) < 0.6
        all_preds = np.stack([forwards(g) for g in Gs], 0)                # (M, T, C, lat, lon)
        res = gd.evaluate_ensemble(Gs, ds, batch_size=2, mask=valid)
    mask = ~valid                                                          # the notebook masks where tpbh == 0
    all_preds_masked = all_preds.astype(np.float64).copy()
    all_preds_masked[:, :, :, mask] = np.nan
    trues_masked = truth.astype(np.float64).copy()
    trues_masked[:, :, mask] = np.nan
    preds_ts = np.nanmean(all_preds_masked, axis=(3, 4))
    trues_ts = np.nanmean(trues_masked, axis=(2, 3))
    mean_preds = np.nanmean(preds_ts, axis=0)
    std_preds = np.nanstd(preds_ts, axis=0)
    valid_mask = ~np.isnan(trues_ts) & ~np.isnan(mean_preds)
    tv, pv = trues_ts[valid_mask].flatten(), mean_preds[valid_mask].flatten()
    r2 = 1.0 - ((tv - pv) ** 2).sum() / ((tv - tv.mean()) ** 2).sum()
    np.testing.assert_allclose(res["mean_preds"].cpu().numpy(), mean_preds, rtol=1e-9, atol=0)
    np.testing.assert_allclose(res["std_preds"].cpu().numpy(), std_preds, rtol=1e-9, atol=0)
    assert abs(res["r2"] - r2) <= 1e-9
    np.testing.assert_allclose(res["trues_ts"].cpu().numpy(), trues_ts, rtol=1e-12, atol=0)
    # maps: one rounding of the fp64 mean / population std over the members
    np.testing.assert_allclose(res["mean_map"].cpu().numpy(), all_preds.astype(np.float64).mean(0), rtol=2.4e-7, atol=0)
    np.testing.assert_allclose(res["std_map"].cpu().numpy(), all_preds.astype(np.float64).std(0), rtol=2.4e-7, atol=0)
    for m in range(3):
        check_metrics(res["members"][m], metrics(all_preds[m][:, :, valid], truth[:, :, valid]), f"member {m}")
    assert all(g.training for g in Gs)
