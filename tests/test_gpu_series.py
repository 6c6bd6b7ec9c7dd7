"""GPU: the per-pixel time-series module (gan_danet_amd/timeseries.py, csrc/series.hip) against the independent oracles
of tests/series_util.py within its derived bounds, and against the host twins bit for bit (records, maps, coefficients,
rss, block means: they share csrc/series_core.h and the order).  The exact oracle visits the columns around every wave,
workgroup and vector boundary and both ends; the host twins -- held to the oracle on the CPU -- every column.  amp and phase
are compared with np.hypot / np.arctan2 of the device's own coefficients within 8 ulp.  Each test prints its largest
error over its bound (python -m pytest -s).

Largest figures observed on an MI355X, as fractions of the bounds of tests/series_util.py: records 0.230 (T = 2, fp64),
maps 0.109, coefficients 0.587 (P = 1, T = 2), rss 0.027, block means 0.245 (fp32 output 0.497); amp / phase 1.00 ulp.  The
device equalled the host twin bit for bit in every case."""
import numpy as np
import pytest
import torch

import series_util as U

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _off(a):
    """a copy of ``a`` on the device whose first element lies one element past a 16-byte boundary"""
    buf = torch.empty(a.size + 1, device="cuda", dtype=torch.from_numpy(a[:0].reshape(-1)).dtype)
    v = buf[1:].view(a.shape)
    v.copy_(_dev(a))
    assert v.data_ptr() % 16 == a.itemsize
    return v


def _records(p, t, mask=None, skip_nan=True, views=(False, False)):
    from gan_danet_amd import timeseries as TS
    pd, td = (_off(a) if o else _dev(a) for a, o in zip((p, t), views))
    s = TS.SeriesSkill(p.shape[1:], None if mask is None else _dev(mask), skip_nan).update(pd, td)
    return s, s.records().cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", U.TS)
def test_records_and_maps(T, dtype):
    """M on both sides of a wave, of the workgroup and of the vector width: the device equals the host twin bit for bit on
    every column and holds the record and map bounds on the oracle's columns; a column's bits do not depend on M"""
    from gan_danet_amd import kern as K
    key = np.dtype(dtype).name
    big = None
    worst = worst_map = 0.0
    for M in reversed(U.MS):
        p, t = U.pair(T, M, dtype)
        skill, rec = _records(p, t)
        assert rec.shape == (8, M) and np.array_equal(rec, K.series_stats_host(p, t)), M
        big = rec if big is None else big
        assert np.array_equal(rec, big[:, :M]), M
        cols = U.oracle_columns(M)
        want, scale = U.records_oracle(p, t, cols, key=key)
        err, bound = np.abs(rec[:, cols] - want), U.record_bound(T, scale)
        assert np.array_equal(rec[0], np.full(M, float(T))) and np.all(err <= bound), M
        worst = max(worst, float((err[1:] / np.maximum(bound[1:], 1e-300)).max()))
        for ddof in (0, 1):
            got = {k: v.cpu().numpy() for k, v in skill.compute(U.MAPS, ddof).items()}
            host = K.series_skill_host(rec, U.MAPS, ddof)
            assert all(np.array_equal(got[k], host[k], equal_nan=True) for k in U.MAPS), (M, ddof)
            worst_map = max(worst_map, U.check_maps({k: v[cols] for k, v in got.items()}, U.skill_numpy(want, ddof), T, f"M={M}"))
    print(f"T = {T} {key}: records at most {worst:.3f} of the bound, maps {worst_map:.3f}; device == host twin on every column")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_unaligned_views_chunks_and_determinism(dtype):
    from gan_danet_amd import timeseries as TS
    for T, M in ((181, 64), (181, 1003), (7, 65), (2, 64)):
        p, t = U.pair(T, M, dtype)
        _, rec = _records(p, t)
        assert np.array_equal(_records(p, t)[1], rec)                                   # two runs, the same bits
        assert np.array_equal(_records(p, t, views=(True, False))[1], rec)              # pred alone one element off: scalar path
        assert np.array_equal(_records(p, t, views=(True, True))[1], rec)               # both: a head and a tail around the vectors
        pd, td = _dev(p), _dev(t)
        for cuts in ([0, 1, T], list(range(0, T, (T + 2) // 3)) + [T]):
            s = TS.SeriesSkill((M,))
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                if hi > lo:
                    s.update(pd[lo:hi], td[lo:hi])
            assert np.array_equal(s.records().cpu().numpy(), rec), (T, M, cuts)
    one = TS.skill_maps(_dev(p.reshape(T, 8, 8)), _dev(t.reshape(T, 8, 8)), metrics=("rmse", "kge"))
    assert set(one) == {"rmse", "kge"} and one["kge"].shape == (8, 8) and one["kge"].dtype == torch.float64


def test_masks_and_nans():
    from gan_danet_amd import kern as K
    T, M = 181, 65
    p, t = (v.copy() for v in U.pair(T, M))
    p[:, 3] = np.nan                      # a series of all NaN
    t[1:, 4] = np.nan                     # one valid pair
    p[5:9, 5] = np.nan                    # NaN on one side only
    mask = np.ones(M, dtype=np.uint8)
    mask[[0, 31, M - 1]] = 0              # the first, a middle and the last series
    skill, rec = _records(p, t, mask)
    assert np.array_equal(rec, K.series_stats_host(p, t, mask), equal_nan=True)
    cols = [1, 3, 4, 5, 63]
    want, scale = U.records_oracle(p, t, cols)
    assert np.all(np.abs(rec[:, cols] - want) <= U.record_bound(T, scale))
    assert np.array_equal(rec[0, [3, 4, 5]], [0, 1, T - 4]) and np.all(rec[:, [0, 31, M - 1]] == 0)
    maps = {k: v.cpu().numpy() for k, v in skill.compute(U.MAPS).items()}
    U.check_maps({k: v[cols] for k, v in maps.items()}, U.skill_numpy(want), T)
    assert all(np.isnan(v[[0, 3, 31, M - 1]]).all() for k, v in maps.items() if k != "n") and np.all(maps["n"][[0, 3, 31, M - 1]] == 0)
    assert np.isnan(maps["cc"][4]) and maps["rmse"][4] == abs(p[0, 4] - t[0, 4])
    # a boolean mask of the time step's shape; without SKIP_NAN the NaN propagates and the count is T
    _, again = _records(p, t, mask.astype(bool))
    assert np.array_equal(again, rec, equal_nan=True)
    _, raw = _records(p, t, skip_nan=False)
    assert np.array_equal(raw, K.series_stats_host(p, t, skip_nan=False), equal_nan=True)
    assert np.all(raw[0] == T) and np.isnan(raw[[1, 3, 5, 6, 7], 5]).all() and np.isfinite(raw[[2, 4], 5]).all()


def test_taylor_stats():
    from gan_danet_amd import timeseries as TS
    p, t = (v.copy() for v in U.pair(181, 257))
    p[3, 5] = np.nan
    r = TS.taylor_stats(_dev(p), _dev(t))
    ok = ~np.isnan(p)
    pv, tv = p[ok], t[ok]
    want = (np.std(tv, ddof=1), np.std(pv, ddof=1), np.corrcoef(tv, pv)[0, 1],
            np.sqrt(np.mean(((pv - pv.mean()) - (tv - tv.mean())) ** 2)))
    for g, w in zip(r, want):                                     # both sides are fp64 sums of n terms in some order
        assert g.dim() == 0 and g.dtype == torch.float64 and abs(g.item() - w) <= 4 * pv.size * U.U53 * abs(w)


@pytest.mark.parametrize("P", [1, 2, 6, 8])
def test_fit(P):
    from gan_danet_amd import kern as K
    from gan_danet_amd import timeseries as TS
    for T, M, dtype in ((181, 1003, np.float64), (181, 257, np.float32), (181, 65, np.float64), (2 * P, 64, np.float64), (P, 1, np.float64)):
        y, a = U.fit_series(P, T, M, dtype)
        got = [v.cpu().numpy() for v in TS.lstsq_series(_dev(y), a)]
        host = K.series_lstsq_host(y, a)
        assert all(np.array_equal(g, h, equal_nan=True) for g, h in zip(got, host)), (P, T, M)
        assert got[0].shape == (P, M) and got[1].shape == (M,)
        want = U.lstsq_oracle(y, a)
        if M > 4 and T >= 2 * P:
            assert got[2][2] == P - 1 and got[2][3] == P and got[2][4] == 0 and np.isnan(got[0][:, [2, 4]]).all()
            assert got[1][3] <= 1e-24 * np.abs(y[~np.isnan(y[:, 3]), 3]).max() ** 2          # exactly P samples: rss about 0
        ce, re = U.check_fit(got, want, T, f"P={P} T={T} M={M}")
        print(f"P = {P}, T = {T}, M = {M} {np.dtype(dtype).name}: coefficients at most {ce:.2e} of the bound, rss {re:.2e}; device == host twin")
    again = [v.cpu().numpy() for v in TS.lstsq_series(_off(y), torch.from_numpy(a).to("cuda"))]
    assert all(np.array_equal(g, h, equal_nan=True) for g, h in zip(again, got))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_harmonic_fit_known_answer(dtype):
    """the tau scaling and the phase convention, through harmonic_fit itself; amp and phase within 8 ulp of numpy on the
    device's own coefficients"""
    from gan_danet_amd import timeseries as TS
    worst = 0.0
    for times in (None, 2002.0 + np.arange(181) / 12.0):
        period = 12.0 if times is None else 1.0
        y, ans, want = U.synth_harmonic(181, times, period)
        if dtype == np.float32:
            y = y.astype(np.float32)
        a, tau_scale = TS.harmonic_basis(np.arange(181.0) if times is None else times, period, 2, True)
        r = TS.harmonic_fit(_dev(y), times, period, 2, True)
        coef = TS.lstsq_series(_dev(y), a)[0].cpu().numpy()
        mean, slope, amp, phase, rms, n = (v.cpu().numpy() for v in r)
        assert np.array_equal(mean, coef[0]) and np.array_equal(slope, coef[1] * tau_scale) and np.all(n == 181)
        for k in range(2):
            ua = U.ulps(amp[k], np.hypot(coef[2 + 2 * k], coef[3 + 2 * k]))
            up = U.ulps(phase[k], np.arctan2(coef[3 + 2 * k], coef[2 + 2 * k]))
            worst = max(worst, float(ua.max()), float(up.max()))
            assert ua.max() <= 8 and up.max() <= 8
        if dtype == np.float64:
            cb = (181 + 48) * np.linalg.cond(a) ** 2 * U.U53 * np.linalg.norm(want, axis=0)
            assert np.all(np.linalg.norm(coef - want, axis=0) <= cb)
            assert np.allclose(slope, ans["slope"], rtol=0, atol=1e-13) and np.allclose(amp, ans["amp"], rtol=0, atol=1e-12)
            assert np.allclose(phase, ans["phase"], rtol=0, atol=1e-11) and np.all(rms <= 1e-13)
        else:
            assert np.allclose(amp, ans["amp"], rtol=0, atol=1e-6) and np.allclose(phase, ans["phase"], rtol=0, atol=1e-4)
    print(f"{np.dtype(dtype).name}: amp / phase at most {worst:.2f} ulp from numpy on the device's coefficients")
    lin = TS.harmonic_fit(_dev(y.reshape(181, 3, 1)), harmonics=0, trend=True)           # the per-pixel linear trend
    assert lin.amplitude.shape == (0, 3, 1) and lin.slope.shape == (3, 1) and lin.rms_resid.shape == (3, 1)
    flat = TS.harmonic_fit(_dev(y), harmonics=1, trend=False)
    assert flat.slope is None and flat.amplitude.shape == (1, 3)


@pytest.mark.parametrize("shape,f", [((3, 10, 15), (5, 5)), ((2, 4, 6), (2, 3)), ((1, 5, 5 * 67), (5, 5))])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_block_mean(shape, f, dtype):
    from gan_danet_amd import kern as K
    from gan_danet_amd import timeseries as TS
    x = U.block_case(shape, dtype)
    x[0, :f[0], :f[1]] = np.nan                                             # a block of all NaN
    w = np.cos(np.linspace(-1.2, 1.2, shape[1]))[:, None] * np.ones(shape[2])
    worst = 0.0
    for weights in (None, w):
        for min_count in (1, f[0] * f[1]):                                  # the second is above every block that lost a value
            got, cnt = TS.coarsen(_dev(x), f, None if weights is None else _dev(weights), min_count, return_count=True)
            got, cnt = got.cpu().numpy(), cnt.cpu().numpy()
            hm, hc = K.block_mean_host(x, f[0], f[1], weights, min_count)
            assert got.dtype == x.dtype and np.array_equal(got, hm, equal_nan=True) and np.array_equal(cnt, hc)
            assert np.isnan(got[0, 0, 0]) and cnt[0, 0, 0] == 0
            worst = max(worst, U.check_block(got, cnt, U.block_mean_oracle(x, f[0], f[1], weights, min_count), f[0], f[1], dtype))
            assert min_count == 1 or np.array_equal(np.isnan(got), cnt < min_count)
    same = TS.coarsen(_off(x), 1).cpu().numpy()                             # factor (1, 1): the input, bit for bit
    assert np.array_equal(same, x, equal_nan=True)
    print(f"{shape} by {f} {np.dtype(dtype).name}: at most {worst:.3f} of the bound; device == host twin")


def test_block_mean_errors_and_consistency():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import timeseries as TS
    x = torch.zeros(2, 10, 15, device="cuda")
    for bad in (lambda: TS.coarsen(x, 4), lambda: TS.coarsen(x, (5, 4)), lambda: TS.coarsen(x, 0), lambda: TS.coarsen(x, 2.5),
                lambda: TS.coarsen(x, 5, weights=torch.ones(10, 14, device="cuda", dtype=torch.float64)),
                lambda: TS.coarsen(x.int(), 5), lambda: TS.harmonic_fit(x, times=np.arange(3.0)), lambda: TS.harmonic_fit(x, harmonics=4),
                lambda: TS.lstsq_series(x, np.ones((2, 9))), lambda: TS.skill_maps(x, x.double()), lambda: TS.skill_maps(x, x[:, :5]),
                lambda: TS.skill_maps(x, x, mask=torch.ones(10, 14, device="cuda", dtype=torch.uint8)),
                lambda: TS.skill_maps(x, x, metrics=("r2",))):
        with pytest.raises(L.GandanetError):
            bad()
    rc = L.load().gd_block_mean(x.data_ptr(), 0, 2, 10, 15, 4, 5, None, 1, x.data_ptr(), None, None)
    assert rc == -1 and "does not divide" in L.last_error()
    # a cube built by np.repeat of a coarse cube comes back exactly (fp32 values: 25 of them add without rounding in fp64)
    for dtype in (np.float32, np.float64):
        coarse = U.pair(24, 6 * 9, np.float32)[0].reshape(24, 6, 9).astype(dtype)
        fine = np.repeat(np.repeat(coarse, 5, 1), 5, 2)
        maps = TS.consistency(_dev(fine), _dev(coarse), 5, metrics=("n", "rmse", "cc", "bias", "nse"))
        assert torch.equal(TS.coarsen(_dev(fine), (5, 5)), _dev(coarse))
        assert torch.all(maps["rmse"] == 0) and torch.all(maps["cc"] == 1) and torch.all(maps["n"] == 24) and torch.all(maps["nse"] == 1)
        assert maps["cc"].shape == (6, 9)


def _guarded(n, dtype=torch.float64):
    """(buffer of sentinels, its middle ``n`` elements)"""
    buf = torch.full((n + 128,), -7.0, device="cuda", dtype=dtype)
    return buf, buf[64:64 + n]


def _middle(buf, n):
    host = buf.cpu().numpy()
    assert np.all(host[:64] == -7) and np.all(host[64 + n:] == -7), "written outside the output"
    return host[64:64 + n]


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_launcher_edges(M):
    """the one-thread-per-item launcher around its 256-thread workgroup, T = 5: lstsq, skill, harmonic_finalize and
    block_mean write into the middle of sentinel buffers through the C entries; the sentinels stay, and the outputs are
    bit for bit those of the host twins (harmonic_finalize has none: its slope is exact and amp / phase are within the
    8 ulp of test_harmonic_fit_known_answer)"""
    from gan_danet_amd import _lib as L
    from gan_danet_amd import kern as K
    lib, st, T, P = K.lib(), K._stream(), 5, 2
    y, a = U.fit_series(P, T, M, np.float32)
    bufs, yd, ad = [_guarded(n) for n in (P * M, M, M)], _dev(y), _dev(a)      # inputs stay referenced until their results are read
    L.check(lib.gd_series_lstsq(yd.data_ptr(), L.FILTER_F32, T, M, ad.data_ptr(), P, *[v.data_ptr() for _, v in bufs], st), "gd_series_lstsq")
    for (buf, v), host in zip(bufs, K.series_lstsq_host(y, a)):
        assert np.array_equal(_middle(buf, v.numel()), host.reshape(-1), equal_nan=True), M

    p, t = U.pair(T, M)
    rec = K.series_stats_host(p, t)
    names = L.SKILL_MAPS
    (buf, v), recd = _guarded(len(names) * M), _dev(rec)
    L.check(lib.gd_series_skill(recd.data_ptr(), M, 0, K.skill_which(names), v.data_ptr(), st), "gd_series_skill")
    host = K.series_skill_host(rec, names)
    assert np.array_equal(_middle(buf, v.numel()), np.stack([host[nm] for nm in names]).reshape(-1), equal_nan=True), M

    rng = np.random.default_rng(M)
    coef, rss, n = rng.standard_normal((4, M)), rng.random(M), np.full(M, 5.0)
    bufs, ins = [_guarded(M) for _ in range(4)], [_dev(coef), _dev(rss), _dev(n)]
    L.check(lib.gd_harmonic_finalize(ins[0].data_ptr(), 4, M, 1, 1, 0.5, ins[1].data_ptr(), ins[2].data_ptr(), *[v.data_ptr() for _, v in bufs],
                                     st), "gd_harmonic_finalize")
    amp, phase, slope, rms = (_middle(buf, M) for buf, _ in bufs)
    assert np.array_equal(slope, coef[1] * 0.5)
    assert U.ulps(amp, np.hypot(coef[2], coef[3])).max() <= 8 and U.ulps(phase, np.arctan2(coef[3], coef[2])).max() <= 8
    assert U.ulps(rms, np.sqrt(rss / n)).max() <= 8

    for dtype, td in ((np.float64, torch.float64), (np.float32, torch.float32)):
        x = U.block_case((1, 2, 2 * M), dtype)
        (buf, v), (cbuf, c), xd = _guarded(M, td), _guarded(M, torch.int32), _dev(x)
        L.check(lib.gd_block_mean(xd.data_ptr(), int(dtype == np.float64), 1, 2, 2 * M, 2, 2, None, 1, v.data_ptr(), c.data_ptr(), st),
                "gd_block_mean")
        hm, hc = K.block_mean_host(x, 2, 2)
        assert np.array_equal(_middle(buf, M), hm.reshape(-1), equal_nan=True) and np.array_equal(_middle(cbuf, M), hc.reshape(-1)), M


def _arg_cases(K):
    """one device wrapper per analysis family that has a host twin: name -> (call(x), the shape of its main array); the other
    arguments are good ones on the device, so only the main array can be at fault"""
    f64 = dict(device="cuda", dtype=torch.float64)
    stl = dict(period=2, seasonal=3, trend=3, low_pass=3, seasonal_deg=1, trend_deg=1, low_pass_deg=1, inner_iter=2, outer_iter=1)
    mean, valid = torch.zeros(7, **f64), torch.ones(7, device="cuda", dtype=torch.uint8)
    clim = torch.ones(3, 2, 7, **f64)
    table = torch.linspace(-2.0, 2.0, 60, **f64).reshape(1, 3, 4, 5)
    return {
        "stl_decompose": (lambda x: K.stl_decompose(x, stl), (5, 7)),
        "series_stats": (lambda x: K.series_stats(x, x, torch.zeros(8, 7, **f64)), (5, 7)),
        "trend_test": (lambda x: K.trend_test(x, torch.arange(5, **f64)), (5, 7)),
        "ens_verify": (lambda x: K.ens_verify(x, torch.zeros(7, device="cuda", dtype=x.dtype), torch.zeros(K.L.ENSV_REC, **f64)), (5, 7)),
        "eof_gram": (lambda x: K.eof_gram(x, mean, valid), (5, 7)),
        "spec_prepare": (lambda x: K.spec_prepare(x), (3, 4, 5)),
        "drought_index": (lambda x: K.drought_index(x, clim), (5, 7)),
        "ccl_label": (lambda x: K.ccl_label(x, 0.0, 0x1FFF), (3, 4, 5)),
        "nbr_fraction": (lambda x: K.nbr_fraction(x, 0.0, 3), (3, 4, 5)),
        "qm_quantiles": (lambda x: K.qm_quantiles(x, [0.25, 0.5]), (5, 7)),
        "qm_apply": (lambda x: K.qm_apply(x, table, table), (3, 4, 5)),
    }


@pytest.mark.parametrize("name", ["stl_decompose", "series_stats", "trend_test", "ens_verify", "eof_gram", "spec_prepare", "drought_index",
                                  "ccl_label", "nbr_fraction", "qm_quantiles", "qm_apply"])
def test_device_wrappers_refuse_a_bad_main_array_before_any_launch(name):
    """a CPU tensor, a non-contiguous view, a wrong dtype and a wrong ndim each raise GandanetError in the wrapper, which
    returns before it reaches the C entry; the good array goes through"""
    from gan_danet_amd import kern as K
    call, shape = _arg_cases(K)[name]
    x = torch.linspace(-1.0, 1.0, int(np.prod(shape)), device="cuda", dtype=torch.float64).reshape(shape)
    call(x)
    torch.cuda.synchronize()
    view = x.transpose(0, 1).contiguous().transpose(0, 1)
    assert view.shape == x.shape and not view.is_contiguous() and not view[0].is_contiguous()
    bad = {"CPU tensor": x.cpu(), "non-contiguous view": view, "wrong dtype": x.to(torch.int32), "one dimension too few": x[0]}
    if name != "ens_verify":                                                      # (M, ...) members: any ndim from 2 on
        bad["one dimension too many"] = x[None]
    for what, arr in bad.items():
        with pytest.raises(K.L.GandanetError):
            call(arr)
            pytest.fail(f"{name} took a {what}")
