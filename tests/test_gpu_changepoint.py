"""GPU: gd_change_point (csrc/changepoint.hip) equals its host twin bit for bit on every plane but pt_p and cs_p, which stay
within P_RTOL = 4 x P_MEASURED of math.exp applied to the planes' own K, n and q (changepoint_util.py records the
measured 2.314e-16), and matches the numpy oracle as the CPU file does; results do not depend on M, on the run or on the
alignment of x; long series, masks, per-series windows; change_points returns the planted breaks.  Each test prints its
largest p error (python -m pytest -s)."""
import numpy as np
import pytest
import torch

import changepoint_util as U

pytestmark = pytest.mark.gpu
TS = (2, 3, 4, 5, 9, 10, 11, 63, 64, 65, 129, 181)
BITS = [k for k, nm in enumerate(U.MAPS) if nm not in U.PROB]


def _dev(x, t, mask=None, window=None, min_seg=5, flags=15, fill=None):
    from gan_danet_amd import kern as K
    d = torch.device("cuda:0")
    out = None if fill is None else torch.full((25, x.shape[1]), fill, device=d, dtype=torch.float64)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(d)
    return K.change_point(up(x), up(t), up(mask), up(window), min_seg, flags, out=out).cpu().numpy()


def _same_bits(got, want, flags, what):
    for k in U.planes_of(flags):
        if U.MAPS[k] in U.PROB:
            continue
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)) or np.array_equal(got[k], want[k], equal_nan=True), (what, U.MAPS[k])
        bad = ~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))
        assert not bad.any(), (what, U.MAPS[k], np.nonzero(bad)[0][:8])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", TS)
def test_device_equals_host_twin_and_oracle(T, dtype):
    """M = 65, the series kinds of the CPU file with and without gaps: all four families together and each alone (the other
    planes keep the fill value)"""
    worst = 0.0
    for gaps, min_seg in ((False, 5), (True, 2)):
        x = U.series(T, 65, dtype, gaps, min_seg=min_seg)
        t = U.times_of(T, uniform=not gaps)
        host, cols, val, err, margins = U.reference(("kinds", T, np.dtype(dtype).name, gaps, min_seg), x, t, min_seg, 15)
        got = _dev(x, t, None, None, min_seg, 15, fill=U.FILL)
        _same_bits(got, host, 15, (T, gaps))
        U.assert_matches(got[:, cols], val, err, margins, 15, (T, gaps, min_seg))
        w, rel = U.p_error(got)
        worst = max(worst, rel)
        print(f"T = {T} gaps = {gaps}: p relative error {rel:.3e}")
        assert w <= 1.0
        for flags in (1, 2, 4, 8):
            one = _dev(x, t, None, None, min_seg, flags, fill=U.FILL)
            asked = U.planes_of(flags)
            _same_bits(one, host, flags, (T, gaps, flags))
            assert U.p_error(one)[0] <= 1.0
            for k in range(25):
                assert k in asked or np.all(one[k] == U.FILL), (flags, k)
    print(f"T = {T} {np.dtype(dtype).name}: device == host twin on every plane but p; p relative error at most {worst:.3e}")


def test_independent_of_m_run_and_alignment():
    T = 65
    x = U.series(T, 257, gaps=True)
    t = U.times_of(T, uniform=False)
    full = _dev(x, t)
    assert np.array_equal(full.view(np.int64), _dev(x, t).view(np.int64))                 # two runs, the same bits
    for M in (65, 64, 63, 2, 1):
        part = _dev(np.ascontiguousarray(x[:, :M]), t)
        assert np.array_equal(part.view(np.int64), full[:, :M].view(np.int64)), M
    from gan_danet_amd import kern as K
    d = torch.device("cuda:0")
    for dt in (torch.float64, torch.float32):
        xs = torch.from_numpy(x[:, :65]).to(d).to(dt)
        base = K.change_point(xs.contiguous(), torch.from_numpy(t).to(d))
        buf = torch.empty(xs.numel() + 8, device=d, dtype=dt)
        off = [o for o in range(1, 8) if (buf.data_ptr() + o * buf.element_size() - buf.element_size()) % 16 == 0][0]
        view = buf[off:off + xs.numel()].view(T, 65)                                      # one element past a 16-byte boundary
        assert (view.data_ptr() - xs.element_size()) % 16 == 0
        view.copy_(xs)
        assert torch.equal(K.change_point(view, torch.from_numpy(t).to(d)).view(torch.int64), base.view(torch.int64))


def test_long_series():
    """T = 2048, M = 3: monotone (|U| reaches n^2 / 4 = 2^20, V sums over 2048 terms), integers 0..3, Gaussian with a planted
    shift -- against the host twin; T = 300, M = 5 against twin and oracle"""
    T = 2048
    rng = np.random.default_rng(8)
    x = np.stack((np.arange(T) * 0.5, rng.integers(0, 4, T).astype(np.float64), rng.standard_normal(T) + np.where(np.arange(T) > 1500, 8.0, 0.0)), 1)
    from gan_danet_amd import kern as K
    for dtype in (np.float64, np.float32):
        xx = np.ascontiguousarray(x.astype(dtype))
        t = U.times_of(T)
        host = K.change_point_host(xx, t, None, None, 5, 15)
        got = _dev(xx, t)
        _same_bits(got, host, 15, ("long", dtype))
        assert U.p_error(got)[0] <= 1.0
        assert got[1, 0] == 1024 * 1024 and got[2, 0] == -1024 * 1024 and got[3, 0] == 1023 and got[9, 2] == 1500
    x = U.planted(300, 5)
    t = U.times_of(300, uniform=False)
    got = _dev(x, t)
    _same_bits(got, K.change_point_host(x, t, None, None, 5, 15), 15, "T = 300")
    val, err, margins = U.oracle(x, t, range(5), 5, 15)
    U.assert_matches(got, val, err, margins, 15, "T = 300", need_margin=True)


def test_masks_and_windows():
    from gan_danet_amd import kern as K
    T, M = 64, 70
    x = U.series(T, M, gaps=True, seed=5)
    t = U.times_of(T)
    mask = np.ones(M, dtype=np.uint8)
    mask[[0, 31, 64, M - 1]] = 0
    rng = np.random.default_rng(1)
    win = np.stack((rng.integers(-3, 30, M), rng.integers(25, T + 4, M))).astype(np.int32)      # differ within one launch
    win[:, 5] = (40, 40)
    win[:, 6] = (50, 20)
    got = _dev(x, t, mask, win, 3)
    _same_bits(got, K.change_point_host(x, t, mask, win, 3, 15), 15, "mask and window")
    assert np.all(got[0, [0, 31, 64, M - 1, 5, 6]] == 0) and np.all(got[[3, 7, 9, 16]][:, [0, 31, 64, M - 1, 5, 6]] == -1)
    cols = [1, 2, 3, 4, 7, 33, 65, 68]
    val, err, margins = U.oracle(x, t, cols, 3, 15, mask, win)
    U.assert_matches(got[:, cols], val, err, margins, 15, "windows")


@pytest.mark.parametrize("method", ["pettitt", "step", "trend"])
def test_change_points_returns_the_planted_shifts(method):
    """a (40, 6, 7) cube: pixel p carries p % 4 upward shifts of 10, 30 and 90 noise sd at fixed steps: exactly those counts
    and indices, ascending and -1 padded.  The layout suits all three methods: the segment before the first of two shifts is
    as long as the two after it together (max |U_k| of a series with several shifts sits at a shift only then), and the
    growing heights keep a single line from fitting the staircase (the two-line F of equal steps is small).  alpha = 0.005
    is below the smallest pt_p a pure-noise segment of up to 15 samples can reach (0.011)."""
    import gan_danet_amd as gd
    T = 40
    plans = {0: [], 1: [19], 2: [19, 29], 3: [9, 19, 29]}
    rng = np.random.default_rng(3)
    x = 0.1 * rng.standard_normal((T, 6, 7))
    want = np.full((3, 6, 7), -1)
    for i in range(6):
        for j in range(7):
            cuts = plans[(i * 7 + j) % 4]
            for c, h in zip(cuts, (1.0, 3.0, 9.0)):
                x[c + 1:, i, j] += h
            want[:len(cuts), i, j] = cuts
    for dt in (torch.float64, torch.float32):
        res = gd.change_points(torch.from_numpy(x).to("cuda:0").to(dt), max_breaks=3, method=method, alpha=0.005, min_f=40.0, min_seg=4)
        assert res.count.dtype == torch.int64 and tuple(res.index.shape) == (3, 6, 7)
        assert np.array_equal(res.index.cpu().numpy(), want), method
        assert np.array_equal(res.count.cpu().numpy(), (want >= 0).sum(0)), method
    one = gd.change_point(torch.from_numpy(x).to("cuda:0"), window=(0, 20), min_seg=4)
    assert one.pt_index.shape == (6, 7) and one.n.max().item() == 20
    assert gd.pettitt(torch.from_numpy(x).to("cuda:0")).cs_q is None and gd.segmented_fit(torch.from_numpy(x).to("cuda:0"), "trend").st_f is None
