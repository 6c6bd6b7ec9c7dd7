"""CPU: the change-point entry points of the C ABI (include/gandanet.h, "Per-pixel change points") are declared and bound,
reject every bad argument before any launch, and the host twin -- plain C++ over csrc/changepoint_core.h -- matches the
numpy oracle of tests/changepoint_util.py: the integer planes (n, pt_k, pt_u, pt_index) are equal, the float planes lie
within the oracle's derived forward-error bound, the break indices are equal wherever the oracle's margin exceeds twice
that bound (asserted for every series with a planted break), integer-valued series agree with exact Fraction arithmetic,
and pt_p / cs_p are within P_RTOL = 4 x P_MEASURED (changepoint_util.py: 2.314e-16 measured on the device; the host twin's own
error against math.exp is 0) of math.exp applied to the twin's own K, n and q.  Each test prints its largest error over
its bound (python -m pytest -s)."""
import os

import numpy as np
import pytest
import torch

import changepoint_util as U

NAMES = ("gd_change_point", "gd_change_point_host")
TS = (2, 3, 4, 5, 9, 10, 11, 63, 64, 65, 129, 181)


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_changepoint_symbols_are_declared_and_bound():
    import re
    import gan_danet_amd
    from gan_danet_amd import build, changepoint, kern
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    assert "Per-pixel change points" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"int " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]), name          # matching argument counts
    assert hasattr(kern, "change_point") and hasattr(kern, "change_point_host")
    assert f"#define GD_CP_MAX_T {L.CP_MAX_T}" in src and L.CP_MAX_T == 2048
    flat = " ".join(src.split())
    for k, name in enumerate(L.CP_MAPS):
        assert f"GD_CP_{name.upper()} = {k}," in flat
    assert f"GD_CP_MAPS = {len(L.CP_MAPS)}" in src and L.CP_MAPS == U.MAPS
    assert f"GD_CP_PETTITT = {L.CP_PETTITT}, GD_CP_CUSUM = {L.CP_CUSUM}, GD_CP_STEP = {L.CP_STEP}, GD_CP_TREND = {L.CP_TREND}" in src
    assert (L.CP_PETTITT, L.CP_CUSUM, L.CP_STEP, L.CP_TREND) == (U.PETTITT, U.CUSUM, U.STEP, U.TREND)
    assert "changepoint.hip" in build.SOURCES
    assert gan_danet_amd.changepoint is changepoint and changepoint.ChangePoint._fields == U.MAPS
    for name in ("ChangePoint", "ChangePoints", "change_point", "change_points", "pettitt", "cusum", "segmented_fit"):
        assert getattr(gan_danet_amd, name) is getattr(changepoint, name)
    for fn in (changepoint.change_point, changepoint.segmented_fit, changepoint.change_points):
        assert "corrected for the selection" in " ".join(fn.__doc__.lower().split()), fn.__name__   # "not corrected" / "uncorrected"
    assert "asymptotic" in changepoint.change_point.__doc__.lower() and "asymptotic" in changepoint.cusum.__doc__.lower()


def test_changepoint_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses) are not
    touched"""
    L, lib = _lib()
    a, b, c, w = 0x1000, 0x2000, 0x3000, 0x4000
    order = ("x", "dtype", "T", "M", "times", "mask", "window", "min_seg", "flags", "out")
    good = dict(x=a, dtype=1, T=181, M=7, times=b, mask=None, window=w, min_seg=5, flags=15, out=c)
    rules = [(dict(x=None), "null"), (dict(times=None), "null"), (dict(out=None), "null"), (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"),
             (dict(T=1), "T outside"), (dict(T=0), "T outside"), (dict(T=2049), "T outside"), (dict(M=0), "M <= 0"), (dict(M=-3), "M <= 0"),
             (dict(M=1 << 31), "too many"), (dict(min_seg=1), "min_seg"), (dict(min_seg=0), "min_seg"), (dict(min_seg=-5), "min_seg"),
             (dict(min_seg=2049), "min_seg"), (dict(min_seg=(1 << 30) + 1), "min_seg"), (dict(min_seg=(1 << 30) + 2000), "min_seg"),
             (dict(min_seg=(1 << 31) - 1), "min_seg"),      # above GD_CP_MAX_T: n - 2 min_seg + 1 would leave the int range
             (dict(flags=16), "flag"), (dict(flags=-1), "flag"), (dict(flags=31), "flag"), (dict(x=a + 4), "aligned"),
             (dict(x=a + 2, dtype=0), "aligned"), (dict(times=b + 4), "aligned"), (dict(out=c + 4), "aligned"), (dict(window=w + 2), "aligned")]
    for host, fn in ((False, lib.gd_change_point), (True, lib.gd_change_point_host)):
        for kw, word in rules:
            v = dict(good, **kw)
            args = [v[k] for k in order]
            rc = fn(*args) if host else fn(*args, None)
            assert rc == -1, (fn.__name__, kw, rc)
            assert word in L.last_error(), (fn.__name__, kw, L.last_error())
    from gan_danet_amd import kern as K
    x = U.series(5, 3)
    for bad in ([0, 1, 1, 2, 3], [0, 1, 3, 2, 4], [0, 1, np.nan, 3, 4], [0, 1, 2, 3, np.inf]):
        with pytest.raises(L.GandanetError, match="times"):
            K.change_point_host(x, bad)
    with pytest.raises(L.GandanetError):
        K.change_point_host(x, np.arange(4.0))
    with pytest.raises(L.GandanetError):
        K.change_point_host(x.astype(np.int32), np.arange(5.0))
    with pytest.raises(L.GandanetError):
        K.change_point_host(x, np.arange(5.0), None, np.zeros(5, dtype=np.int32))      # a window of 2 M entries


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", TS)
def test_host_twin_against_the_oracle(T, dtype):
    """every kind of series (planted shift, slope break, monotone, all equal, integers 0..3, two-valued, an outlier of 1e12,
    noise), with and without NaN gaps (gaps: columns left with 0, 1, 2 min_seg - 1 and 2 min_seg samples; T = 3, 4, 9, 10
    are those counts without gaps), uniform and non-uniform times, min_seg 2 and 5"""
    worst = 0.0
    for gaps in (False, True):
        for min_seg in (2, 5):
            x = U.series(T, 65, dtype, gaps, min_seg=min_seg)
            t = U.times_of(T, uniform=not gaps)
            host, cols, val, err, margins = U.reference(("kinds", T, np.dtype(dtype).name, gaps, min_seg), x, t, min_seg, 15)
            worst = max(worst, U.assert_matches(host[:, cols], val, err, margins, 15, (T, gaps, min_seg)))
            assert U.p_error(host)[0] <= 1.0
            if gaps and T >= 2 * min_seg:
                assert list(host[0, 8:12]) == [0, 1, 2 * min_seg - 1, 2 * min_seg]
                assert np.isnan(host[1:3, 8:10]).all() and np.all(host[3, 8:10] == -1)          # Pettitt needs two samples
                assert np.all(host[[9, 16], 8:11] == -1) and np.isnan(host[10:16, 8:11]).all() and np.isnan(host[17:, 8:11]).all()
                assert host[9, 11] >= 0 and host[16, 11] >= 0 and np.isfinite(host[14, 11])      # exactly one candidate
                assert np.isnan(host[5, 8]) and host[7, 8] == -1 and np.isnan(host[5, 9])        # CUSUM: n = 0, and n = 1 (sd = 0)
    print(f"T = {T} {np.dtype(dtype).name}: host twin within the bound on every float plane, at most {worst:.3f} of it")


@pytest.mark.parametrize("T", [5, 11, 63, 64, 65, 129, 181])
def test_host_twin_planted_breaks_every_margin_holds(T):
    """real-valued series with a planted break: the oracle's margin between the best and the runner-up exceeds twice the
    bound for EVERY series (asserted, none left out), so the three break indices must be equal"""
    worst = 0.0
    for dtype in (np.float64, np.float32):
        for gaps in (False, True):
            for min_seg in ((2,) if T < 11 else (2, 5)):
                from gan_danet_amd import kern as K
                x = U.planted(T, 24, dtype, gaps)
                t = U.times_of(T, uniform=not gaps)
                host = K.change_point_host(x, t, None, None, min_seg, 15)
                val, err, margins = U.oracle(x, t, range(24), min_seg, 15)
                worst = max(worst, U.assert_matches(host, val, err, margins, 15, ("planted", T, gaps, min_seg), need_margin=True))
                assert U.p_error(host)[0] <= 1.0
                assert np.all(host[[3, 7]] >= 0) and np.all(host[[9, 16]][:, host[0] >= 2 * min_seg] >= 0)
    print(f"T = {T}: indices equal under asserted margins; floats at most {worst:.3f} of the bound")


def test_host_twin_integer_series_against_exact_fractions():
    """values 0..3, two-valued and all-equal series: the break of STEP and TREND is the exact minimiser (the twin's own
    index must be one whose exact rss is within the twin's rounding of the exact minimum, and THE exact one where that
    minimum is isolated), the rss planes are within a relative 1e-12 of the exact rss (n <= 65: n u is 7e-15); a tie in
    exact arithmetic that fp64 reproduces exactly (dyadic means) goes to the smallest k; all-equal data give the first
    candidate, rss = 0 and f NaN"""
    from gan_danet_amd import kern as K
    rng = np.random.default_rng(4)
    for T, min_seg in ((12, 2), (33, 5), (65, 5)):
        t = U.times_of(T)
        cols = [rng.integers(0, 4, T).astype(np.float64) for _ in range(4)] + [np.where(rng.random(T) < 0.5, 2.0, 5.0) for _ in range(2)]
        cols.append(np.full(T, 3.0))
        x = np.ascontiguousarray(np.stack(cols, 1))
        host = K.change_point_host(x, t, None, None, min_seg, U.STEP | U.TREND)
        for m in range(x.shape[1]):
            st, tr, ss, ls = U.exact_fits(x[:, m], t, min_seg)
            for fits, ki, kr, k0, whole in ((st, 9, 14, 13, ss), (tr, 16, 23, 22, ls)):
                best = min(r for _, r in fits)
                got_k, got_rss = int(host[ki, m]), host[kr, m]
                exact_at = dict(fits)[got_k]
                assert abs(got_rss - float(exact_at)) <= 1e-12 * float(exact_at) + 0.0, (T, m, ki, got_rss, float(exact_at))
                assert float(exact_at - best) <= 2e-12 * float(best), (T, m, ki)
                isolated = [k for k, r in fits if float(r - best) <= 4e-12 * float(best)]
                if len(isolated) == 1:
                    assert got_k == isolated[0]
                assert abs(host[k0, m] - float(whole)) <= 1e-12 * float(whole)
        last = x.shape[1] - 1                                                    # all equal: first candidate, rss 0, f NaN
        assert host[9, last] == min_seg - 1 == host[16, last] and host[14, last] == 0 == host[23, last]
        assert host[13, last] == 0 == host[22, last] and np.isnan(host[15, last]) and np.isnan(host[24, last])
    # an exact tie: means 0, 2 and 4 are dyadic, every rss is exact in fp64, k = 3 and k = 7 both give 32
    y = np.array([0, 0, 0, 0, 4, 4, 4, 4, 0, 0, 0, 0], dtype=np.float64)[:, None]
    host = K.change_point_host(y, np.arange(12.0), None, None, 2, U.STEP)
    st = U.exact_fits(y[:, 0], np.arange(12.0), 2)[0]
    assert [k for k, r in st if r == min(r for _, r in st)] == [3, 7]
    assert host[9, 0] == 3 and host[14, 0] == 32.0 and host[10, 0] == 0 and host[11, 0] == 2 and host[12, 0] == 2


def test_host_twin_windows_equal_slices_and_flags_leave_planes():
    """a window [a, b) gives, bit for bit, the result of the sliced array with the indices shifted by a; an empty or
    out-of-range window clamps; families not asked for keep the fill value"""
    from gan_danet_amd import kern as K
    T, M = 65, 24
    x = U.series(T, M, gaps=True, seed=2)
    t = U.times_of(T, uniform=False)
    index_planes = [U.IX[nm] for nm in ("pt_index", "cs_index", "st_index", "tr_index")]
    for a, b in ((0, T), (7, 50), (20, 31), (64, 65), (3, 3)):
        win = np.stack((np.full(M, a), np.full(M, b))).astype(np.int32)
        got = K.change_point_host(x, t, None, win, 5, 15)
        if a == b:
            assert np.all(got[0] == 0) and np.all(got[index_planes] == -1)
            continue
        if b - a < 2:
            assert np.all(got[0] <= 1)
            continue
        want = K.change_point_host(x[a:b], t[a:b], None, None, 5, 15).copy()
        for k in index_planes:
            want[k] = np.where(want[k] >= 0, want[k] + a, want[k])
        assert np.array_equal(got, want, equal_nan=True), (a, b)
    # per-series windows, clamped: (-5, 200) is the whole series, (40, 10) is empty at 40
    win = np.stack((np.full(M, -5), np.full(M, 200))).astype(np.int32)
    win[:, 1] = (40, 10)
    win[:, 2] = (10, 40)
    got = K.change_point_host(x, t, None, win, 5, 15)
    whole = K.change_point_host(x, t, None, None, 5, 15)
    assert np.array_equal(got[:, 3:], whole[:, 3:], equal_nan=True) and np.array_equal(got[:, 0], whole[:, 0], equal_nan=True)
    assert got[0, 1] == 0 and got[0, 2] == np.sum(~np.isnan(x[10:40, 2]))
    mask = np.ones(M, dtype=np.uint8)
    mask[[0, 5]] = 0
    for flags in (0, 1, 2, 4, 8, 5, 10, 15):
        got = K.change_point_host(x, t, mask, None, 5, flags, out=np.full((25, M), U.FILL))
        asked = U.planes_of(flags)
        for k in range(25):
            if k in asked:
                keep = np.ones(M, dtype=bool)
                keep[[0, 5]] = False
                assert np.array_equal(got[k, keep], whole[k, keep], equal_nan=True), (flags, k)
                assert got[0, 0] == 0 and (k == 0 or np.isnan(got[k, 0]) or got[k, 0] == -1)
            else:
                assert np.all(got[k] == U.FILL), (flags, k)


@pytest.mark.parametrize("method", ["pettitt", "step", "trend"])
def test_binary_segmentation_levels_against_numpy_recursion(method):
    """the level loop of change_points (torch ops) over the host twin, against a plain numpy recursion over the same twin"""
    from gan_danet_amd import changepoint as CP
    from gan_danet_amd import kern as K
    T, M, min_seg = 60, 12, 4
    rng = np.random.default_rng(11)
    x = 0.3 * rng.standard_normal((T, M))
    for m in range(M):
        for cut in sorted(rng.choice(np.arange(8, T - 8, 7), size=m % 4, replace=False)):
            x[cut + 1:, m] += 4.0 + m % 3
    t = np.arange(float(T))
    flags, index_map, stat_map = CP._METHODS[method]
    ki, ks = U.IX[index_map], U.IX[stat_map]
    alpha, min_f = 0.05, 30.0

    def run(xs, ms, win):
        return torch.from_numpy(K.change_point_host(xs.numpy(), t, None, win.numpy(), min_seg, flags))

    for max_breaks in (1, 2, 3, 7):
        count, index = CP._segmentation(run, torch.from_numpy(x), None, max_breaks, method, alpha, min_f)
        for m in range(M):
            def one(b, e):
                o = K.change_point_host(x[:, m:m + 1], t, None, np.array([[b], [e]], dtype=np.int32), min_seg, flags)
                return int(o[ki, 0]), float(o[ks, 0])
            accept = (lambda s: s < alpha) if method == "pettitt" else (lambda s: s >= min_f)
            score = (lambda s: -s) if method == "pettitt" else (lambda s: s)
            want = U.segmentation(one, T, max_breaks, accept, score)
            assert int(count[m]) == len(want) and list(index[:len(want), m]) == want and np.all(index[len(want):, m].numpy() == -1), (m, want)


def test_cpu_and_bad_arguments_are_refused():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import changepoint as CP
    x = torch.zeros(24, 4, 6, dtype=torch.float64)
    for call in (lambda: CP.change_point(x), lambda: CP.pettitt(x), lambda: CP.cusum(x), lambda: CP.segmented_fit(x), lambda: CP.change_points(x),
                 lambda: CP.change_point(x.numpy()), lambda: CP.segmented_fit(x, model="hinge"), lambda: CP._min_seg(1),
                 lambda: CP._min_seg(2049), lambda: CP._min_seg((1 << 30) + 1), lambda: CP._min_seg(True), lambda: CP._min_seg(5.0)):
        with pytest.raises(L.GandanetError):
            call()
