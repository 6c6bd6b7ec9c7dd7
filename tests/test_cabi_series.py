"""CPU: the per-pixel time-series entry points of the C ABI (include/gandanet.h, "Per-pixel time series") are declared and
bound, reject every bad argument before any launch, and the host twins -- plain loops over csrc/series_core.h, the
arithmetic the device kernels share -- hold the derived bounds of tests/series_util.py against its independent oracles
(exact rational records, np.linalg.lstsq, math.fsum block means).  Each test prints its largest error over its bound
(python -m pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import series_util as U

NAMES = ("gd_series_stats", "gd_series_stats_host", "gd_series_skill", "gd_series_skill_host", "gd_series_lstsq",
         "gd_series_lstsq_host", "gd_harmonic_finalize", "gd_block_mean", "gd_block_mean_host")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_series_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import build, timeseries
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    assert "Per-pixel time series" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
    assert f"#define GD_LSTSQ_MAX_P {L.LSTSQ_MAX_P}" in src
    for k, name in enumerate(L.SKILL_MAPS):
        assert f"GD_SKILL_{name.upper()} = {k}" in src
    assert f"GD_SKILL_MAPS = {len(L.SKILL_MAPS)}" in src and L.SKILL_MAPS == U.MAPS
    assert "series.hip" in build.SOURCES
    assert gan_danet_amd.timeseries is timeseries and gan_danet_amd.skill_maps is timeseries.skill_maps
    for name in ("SeriesSkill", "skill_maps", "taylor_stats", "lstsq_series", "harmonic_fit", "coarsen", "consistency"):
        assert getattr(gan_danet_amd, name) is getattr(timeseries, name)


def test_series_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the device pointers (never-dereferenced addresses) are
    not touched"""
    L, lib = _lib()
    a, b, c, d, e = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000

    def sweep(fns, order, good, rules):
        for host, fn in fns:
            for kw, word in rules:
                v = dict(good, **kw)
                args = [v[k] for k in order]
                rc = fn(*args) if host else fn(*args, None)
                assert rc == -1, (fn.__name__, kw, rc)
                assert word in L.last_error(), (fn.__name__, kw, L.last_error())

    sweep(((False, lib.gd_series_stats), (True, lib.gd_series_stats_host)),
          ("p", "t", "dtype", "T", "M", "mask", "flags", "rec", "acc"),
          dict(p=a, t=b, dtype=1, T=181, M=7, mask=None, flags=2, rec=c, acc=0),
          [(dict(p=None), "null"), (dict(t=None), "null"), (dict(rec=None), "null"), (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"),
           (dict(T=0), "<= 0"), (dict(M=0), "<= 0"), (dict(T=-1), "<= 0"), (dict(M=1 << 31), "too many"), (dict(flags=1), "flag"),
           (dict(flags=4), "flag"), (dict(p=a + 4), "aligned"), (dict(t=b + 2, dtype=0), "aligned"), (dict(rec=c + 4), "aligned")])
    sweep(((False, lib.gd_series_skill), (True, lib.gd_series_skill_host)), ("rec", "M", "ddof", "which", "out"),
          dict(rec=a, M=7, ddof=0, which=0xfff, out=b),
          [(dict(rec=None), "null"), (dict(out=None), "null"), (dict(M=0), "M <= 0"), (dict(ddof=2), "ddof"), (dict(ddof=-1), "ddof"),
           (dict(which=0), "map"), (dict(which=1 << 12), "map"), (dict(out=b + 4), "aligned")])
    sweep(((False, lib.gd_series_lstsq), (True, lib.gd_series_lstsq_host)), ("x", "dtype", "T", "M", "basis", "P", "coef", "rss", "n"),
          dict(x=a, dtype=1, T=181, M=7, basis=b, P=6, coef=c, rss=d, n=e),
          [(dict(x=None), "null"), (dict(basis=None), "null"), (dict(coef=None), "null"), (dict(dtype=3), "dtype"), (dict(T=0), "<= 0"),
           (dict(M=0), "<= 0"), (dict(P=0), "P outside"), (dict(P=9), "P outside"), (dict(M=1 << 31), "too many"),
           (dict(x=a + 4), "aligned"), (dict(basis=b + 4), "aligned"), (dict(rss=d + 4), "aligned"), (dict(n=e + 2), "aligned")])
    sweep(((False, lib.gd_block_mean), (True, lib.gd_block_mean_host)),
          ("x", "dtype", "planes", "H", "W", "fy", "fx", "w", "min_count", "out", "count"),
          dict(x=a, dtype=0, planes=3, H=10, W=15, fy=5, fx=5, w=None, min_count=1, out=b, count=c),
          [(dict(x=None), "null"), (dict(out=None), "null"), (dict(dtype=2), "dtype"), (dict(planes=0), "<= 0"), (dict(H=0), "<= 0"),
           (dict(fy=0), "factor"), (dict(fx=-1), "factor"), (dict(fy=4), "does not divide"), (dict(fx=4), "does not divide"),
           (dict(H=11), "does not divide"), (dict(min_count=-1), "min_count"), (dict(x=a + 2), "aligned"), (dict(w=d + 4), "aligned"),
           (dict(count=c + 2), "aligned")])
    sweep(((False, lib.gd_harmonic_finalize),), ("coef", "P", "M", "K", "trend", "ts", "rss", "n", "amp", "phase", "slope", "rms"),
          dict(coef=a, P=6, M=7, K=2, trend=1, ts=1.0, rss=b, n=c, amp=d, phase=e, slope=0x6000, rms=0x7000),
          [(dict(coef=None), "null"), (dict(M=0), "M <= 0"), (dict(K=4), "K outside"), (dict(K=-1), "K outside"), (dict(trend=2), "has_trend"),
           (dict(P=5), "1 + has_trend"), (dict(trend=0, P=5), "slope without"), (dict(rss=None), "rms needs"), (dict(amp=d + 4), "aligned")])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", U.TS)
def test_host_records_and_maps_against_the_oracle(T, dtype):
    """records within 4 T 2^-53 S of the exact ones, counts exact; the twelve maps (ddof 0 and 1) within 16 T 2^-53
    max(1, |value|) of the numpy formulas on the oracle's records; every M gives the same bits per series"""
    from gan_danet_amd import kern as K
    p, t = U.pair(T, U.M_MAX, dtype)
    rec = K.series_stats_host(p, t)
    cols = U.oracle_columns(U.M_MAX)
    want, scale = U.records_oracle(p, t, cols, key=np.dtype(dtype).name)
    err = np.abs(rec[:, cols] - want)
    bound = U.record_bound(T, scale)
    assert np.array_equal(rec[0], np.full(U.M_MAX, float(T)))
    assert np.all(err <= bound), (err / np.maximum(bound, 1e-300)).max()
    worst = float((err[1:] / np.maximum(bound[1:], 1e-300)).max())
    worst_map = 0.0
    for ddof in (0, 1):
        got = K.series_skill_host(rec[:, cols], U.MAPS, ddof)
        worst_map = max(worst_map, U.check_maps(got, U.skill_numpy(want, ddof), T, f"T={T} ddof={ddof}"))
    print(f"T = {T} {np.dtype(dtype).name}: records at most {worst:.3f} of the bound, maps {worst_map:.3f}")
    for M in U.MS[:-1]:
        pm, tm = U.pair(T, M, dtype)
        assert np.array_equal(K.series_stats_host(pm, tm), rec[:, :M]), M


def test_host_records_chunks_masks_and_nans():
    from gan_danet_amd import kern as K
    T, M = 181, 65
    p, t = (v.copy() for v in U.pair(T, M))
    p[:, 3] = np.nan                      # a series of all NaN
    t[1:, 4] = np.nan                     # one valid pair
    p[5:9, 5] = np.nan                    # NaN on one side only
    t[40, 6] = np.nan
    p[41, 6] = np.nan
    mask = np.ones(M, dtype=np.uint8)
    mask[[0, 31, M - 1]] = 0
    rec = K.series_stats_host(p, t, mask)
    cols = [1, 3, 4, 5, 6, 64 - 1]
    want, scale = U.records_oracle(p, t, cols)
    assert np.all(np.abs(rec[:, cols] - want) <= U.record_bound(T, scale))
    assert np.array_equal(rec[0, [3, 4, 5, 6]], [0, 1, T - 4, T - 2]) and np.all(rec[:, [0, 31, M - 1]] == 0)
    maps = K.series_skill_host(rec, U.MAPS)
    U.check_maps({k: v[cols] for k, v in maps.items()}, U.skill_numpy(want), T)
    assert all(np.isnan(v[[0, 3, 31]]).all() for k, v in maps.items() if k != "n") and np.all(maps["n"][[0, 3, 31]] == 0)
    assert np.isnan(maps["cc"][4]) and maps["rmse"][4] == abs(p[0, 4] - t[0, 4]) and np.isnan(K.series_skill_host(rec, ["std_p"], 1)["std_p"][4])
    # chunks of time steps give the bits of one call; a masked series keeps what it had
    for cuts in ([0, 1, T], list(range(0, T, (T + 2) // 3)) + [T]):
        part = None
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = K.series_stats_host(p[lo:hi], t[lo:hi], mask, rec=part)
        assert len(cuts) in (3, 4) and np.array_equal(part, rec, equal_nan=True), cuts
    # without SKIP_NAN a NaN propagates into what it touches, and the count is T
    raw = K.series_stats_host(p, t, skip_nan=False)
    assert np.all(raw[0] == T) and np.isnan(raw[[1, 3, 5, 6, 7], 5]).all() and np.isfinite(raw[[2, 4], 5]).all()
    assert np.array_equal(raw[:, 1], rec[:, 1])
    m = K.series_skill_host(raw, U.MAPS)
    assert all(np.isnan(m[k][5]) for k in ("mean_p", "bias", "rmse", "mae", "std_p", "cc", "nse", "kge", "crmsd")) and m["n"][5] == T


@pytest.mark.parametrize("P", [1, 2, 6, 8])
def test_host_fit_against_lstsq(P):
    from gan_danet_amd import kern as K
    for T, M, dtype in ((181, 65, np.float64), (181, 7, np.float32), (2 * P, 6, np.float64), (P, 3, np.float64)):
        y, a = U.fit_series(P, T, M, dtype)
        got = K.series_lstsq_host(y, a)
        want = U.lstsq_oracle(y, a)
        if M > 4 and T >= 2 * P:
            assert want[2][2] == P - 1 and want[2][3] == P and want[2][4] == 0 and np.nanmax(want[3]) < 1e3
            assert got[1][3] <= 1e-24 * np.abs(y[~np.isnan(y[:, 3]), 3]).max() ** 2      # exactly P samples: rss about 0
        ce, re = U.check_fit(got, want, T, f"P={P} T={T}")
        print(f"P = {P}, T = {T}, {np.dtype(dtype).name}: coefficients at most {ce:.2e} of the bound, rss {re:.2e}; "
              f"cond at most {np.nanmax(want[3]):.1f}")


def test_host_fit_known_answer_and_basis():
    """the tau scaling and the phase convention: a synthesised series comes back, through harmonic_basis"""
    from gan_danet_amd import kern as K
    from gan_danet_amd import timeseries as TS
    for times in (None, 2002.0 + np.arange(181) / 12.0):
        period = 12.0 if times is None else 1.0
        y, ans, want = U.synth_harmonic(181, times, period)
        a, tau_scale = TS.harmonic_basis(np.arange(181.0) if times is None else times, period, 2, True)
        assert a.shape == (181, 6) and abs(a[:, 1]).max() == 1.0 and np.linalg.cond(a) < 3.0
        coef, rss, n = K.series_lstsq_host(y, a)
        cb = (181 + 48) * np.linalg.cond(a) ** 2 * U.U53 * np.linalg.norm(want, axis=0)
        assert np.all(np.linalg.norm(coef - want, axis=0) <= cb) and np.all(n == 181)
        assert np.allclose(coef[1] * tau_scale, ans["slope"], rtol=0, atol=1e-13)
        assert np.allclose(np.hypot(coef[2], coef[3]), ans["amp"][0], rtol=0, atol=1e-12)
        assert np.allclose(np.arctan2(coef[5], coef[4]), ans["phase"][1], rtol=0, atol=1e-11)
    assert TS.harmonic_basis(np.arange(5.0), 12.0, 0, True)[0].shape == (5, 2)
    assert TS.harmonic_basis(np.arange(5.0), 12.0, 3, False)[0].shape == (5, 7)
    L, _ = _lib()
    for bad in (dict(harmonics=4), dict(harmonics=-1), dict(period=0.0)):
        with pytest.raises(L.GandanetError):
            TS.harmonic_basis(np.arange(5.0), **dict(dict(period=12.0, harmonics=2), **bad))


@pytest.mark.parametrize("shape,f", [((3, 10, 15), (5, 5)), ((2, 4, 6), (2, 3)), ((1, 5, 5 * 67), (5, 5))])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_block_mean(shape, f, dtype):
    from gan_danet_amd import kern as K
    x = U.block_case(shape, dtype)
    x[0, :f[0], :f[1]] = np.nan                                             # a block of all NaN
    w = np.cos(np.linspace(-1.2, 1.2, shape[1]))[:, None] * np.ones(shape[2])
    worst = 0.0
    for weights in (None, w):
        for min_count in (1, f[0] * f[1]):                                  # the second is above every block that lost a value
            got, cnt = K.block_mean_host(x, f[0], f[1], weights, min_count)
            want = U.block_mean_oracle(x, f[0], f[1], weights, min_count)
            assert got.dtype == x.dtype and cnt.dtype == np.int32 and np.isnan(got[0, 0, 0]) and cnt[0, 0, 0] == 0
            worst = max(worst, U.check_block(got, cnt, want, f[0], f[1], dtype, f"{shape} {f}"))
            assert min_count == 1 or np.array_equal(np.isnan(got), cnt < min_count)
    same, cnt = K.block_mean_host(x, 1, 1)
    assert np.array_equal(same, x, equal_nan=True) and np.array_equal(cnt, (~np.isnan(x)).astype(np.int32))
    print(f"{shape} by {f} {np.dtype(dtype).name}: at most {worst:.3f} of the bound")


def test_cpu_and_bad_tensors_are_refused():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import kern as K
    from gan_danet_amd import timeseries as TS
    x = torch.zeros(24, 4, 6, dtype=torch.float64)
    for call in (lambda: TS.skill_maps(x, x), lambda: TS.SeriesSkill((4, 6)).update(x, x), lambda: TS.taylor_stats(x, x),
                 lambda: TS.lstsq_series(x, np.ones((24, 1))), lambda: TS.harmonic_fit(x), lambda: TS.coarsen(x, 2),
                 lambda: TS.consistency(x, x[:, :2, :3], 2), lambda: TS.skill_maps(x.numpy(), x.numpy()),
                 lambda: TS.SeriesSkill((4, 6)).compute(), lambda: TS.SeriesSkill(()).records(), lambda: TS.SeriesSkill((0, 3))):
        with pytest.raises(L.GandanetError):
            call()
    with pytest.raises(L.GandanetError):
        K.skill_which(["rmse", "r2"])
    with pytest.raises(L.GandanetError):
        K.skill_which([])
    assert K.skill_which(U.MAPS) == 0xfff and K.skill_which(["cc", "n"]) == 0x101


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_host_twin_launcher_edges(M):
    """the host side of the per-item launcher, T = 5: gd_series_lstsq_host, gd_series_skill_host and gd_block_mean_host write
    through the C entries into the middle of buffers of sentinels, leave the sentinels alone, and a column's (a block's)
    bits are those the wrappers give on the 257-series input (the device side: tests/test_gpu_series.py::test_launcher_edges)"""
    from gan_danet_amd import kern as K
    L, lib = _lib()
    T, P, pad = 5, 2, 64

    def guarded(n, dtype=np.float64):
        return np.full(n + 2 * pad, 7, dtype=dtype)

    def ptr(buf):
        return buf[pad:].ctypes.data

    def middle(buf, n, shape):
        assert np.all(buf[:pad] == 7) and np.all(buf[pad + n:] == 7), "written outside the output"
        return buf[pad:pad + n].reshape(shape)

    for dtype in (np.float64, np.float32):
        dt = int(dtype == np.float64)
        yw, a = U.fit_series(P, T, 257, dtype)
        y = np.ascontiguousarray(yw[:, :M])
        cb, rb, nb = guarded(P * M), guarded(M), guarded(M)
        L.check(lib.gd_series_lstsq_host(y.ctypes.data, dt, T, M, a.ctypes.data, P, ptr(cb), ptr(rb), ptr(nb)), "gd_series_lstsq_host")
        coef, rss, n = K.series_lstsq_host(yw, a)
        assert np.array_equal(middle(cb, P * M, (P, M)), coef[:, :M], equal_nan=True)
        assert np.array_equal(middle(rb, M, (M,)), rss[:M], equal_nan=True) and np.array_equal(middle(nb, M, (M,)), n[:M])

        pw, tw = U.pair(T, 257, dtype)
        recw = K.series_stats_host(pw, tw)
        rec = np.ascontiguousarray(recw[:, :M])
        names = L.SKILL_MAPS
        sb = guarded(len(names) * M)
        L.check(lib.gd_series_skill_host(rec.ctypes.data, M, 0, K.skill_which(names), ptr(sb)), "gd_series_skill_host")
        want = K.series_skill_host(recw, names)
        got = middle(sb, len(names) * M, (len(names), M))
        assert all(np.array_equal(got[k], want[nm][:M], equal_nan=True) for k, nm in enumerate(names))

        xw = U.block_case((1, 2, 2 * 257), dtype)
        x = np.ascontiguousarray(xw[:, :, :2 * M])
        ob, kb = guarded(M, dtype), guarded(M, np.int32)
        L.check(lib.gd_block_mean_host(x.ctypes.data, dt, 1, 2, 2 * M, 2, 2, None, 1, ptr(ob), ptr(kb)), "gd_block_mean_host")
        hm, hc = K.block_mean_host(xw, 2, 2)
        assert np.array_equal(middle(ob, M, (1, 1, M)), hm[..., :M], equal_nan=True) and np.array_equal(middle(kb, M, (1, 1, M)), hc[..., :M])
