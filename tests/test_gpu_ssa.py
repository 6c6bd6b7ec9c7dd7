"""GPU: gd_ssa_decompose and gd_ssa_fill (csrc/ssa.hip) equal their host twins bit for bit on every output -- eig, all map
planes, rc, filled: nothing transcendental is involved, only sqrt and division -- over odd and even windows, the window and
series limits, pixel counts around a wave and across the launcher's chunk, both storages, both methods, with and without a
mask, degenerate series mixed in; results do not depend on the run or on how the pixels are split; the public module."""
import numpy as np
import pytest
import torch

import ssa_util as U

pytestmark = pytest.mark.gpu

# (T, M, pixels): every admissible pair of T in (3, 9, 65, 181) and M in (2, 3, 5, 24, 32, 33, 64); 1, 63, 64, 65 pixels
CASES = [(3, 2, 65), (9, 2, 1), (9, 3, 63), (9, 5, 64), (65, 2, 65), (65, 3, 12), (65, 5, 65), (65, 24, 12), (65, 32, 9), (65, 33, 9),
         (181, 2, 9), (181, 3, 9), (181, 5, 12), (181, 24, 12), (181, 32, 9), (181, 33, 9), (181, 64, 9)]


def _K():
    from gan_danet_amd import kern
    return kern


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), (what, np.argwhere(bad)[:6])


def _batch(T, P, dtype, gaps, seed=0):
    """P series: the kinds of ssa_util.series repeated with fresh noise, gaps (the GRACE pattern where T allows, else one step)
    on request, and from 9 pixels on the edge series: all NaN, one valid sample, constant, an infinity, every second sample
    missing, gaps at the first and the last step, a gap longer than most windows"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([U.series(T, np.float64, s) for s in range((P + 7) // 8)], 1)[:, :P] + 1e-3 * rng.standard_normal((T, P))
    if gaps:
        for m in range(P):
            if T >= 47:
                x[U.grace_gaps(T, m), m] = np.nan
            else:
                x[(m * 5 + 1) % T, m] = np.nan
    if P >= 9:
        x[:, 1] = np.nan
        x[1:, 2] = np.nan
        x[:, 3] = -2.5
        x[T // 2, 4] = -np.inf
        x[1::2, 5] = np.nan
        x[[0, T - 1], 6] = np.nan
        x[T // 3:T // 3 + min(T // 2, 40), 7] = np.nan
    return np.ascontiguousarray(x.astype(dtype))


def _mask(P, on):
    if not on:
        return None
    m = np.ones(P, dtype=np.uint8)
    m[6::7] = 0
    return m


@pytest.mark.parametrize("case", range(len(CASES)))
def test_device_equals_host_twin_bit_for_bit(case):
    K = _K()
    T, M, P = CASES[case]
    r = min(M, 16 if M < 32 else 4)
    dtypes = (np.float64, np.float32) if M < 32 else ((np.float64,) if case % 2 else (np.float32,))
    for dtype in dtypes:
        for method in U.METHODS:
            masked = (case + (method == "vg")) % 2 == 0
            mask = _mask(P, masked)
            x = _batch(T, P, dtype, gaps=False, seed=case)
            want = K.ssa_decompose_host(x, M, r, method, mask, True, True)
            got = K.ssa_decompose(_up(x), M, r, method, _up(mask), True, True)
            for g, w, nm in zip(got, want, ("eig", "maps", "rc", "evec")):
                _same(g, w, (T, M, P, np.dtype(dtype).name, method, nm))
            assert np.nanmax(want[1][U.IX["sweeps"]]) < _lib_const("SSA_MAX_SWEEPS")
            assert (want[1][U.IX["flags"]] == 0).sum() >= (1 if P < 9 else 2) - (1 if masked else 0)
            x = _batch(T, P, dtype, gaps=True, seed=case)
            rank, iters = (min(M, 4), 6) if M < 32 else (2, 2)
            want = K.ssa_fill_host(x, M, rank, method, mask, 1e-3, iters, max(2, min(2 * M, T // 2)))
            got = K.ssa_fill(_up(x), M, rank, method, _up(mask), 1e-3, iters, max(2, min(2 * M, T // 2)))
            for g, w, nm in zip(got, want, ("filled", "eig", "maps")):
                _same(g, w, (T, M, P, np.dtype(dtype).name, method, "fill", nm))
            assert np.isfinite(want[0]).any()


def _lib_const(name):
    from gan_danet_amd import _lib
    return getattr(_lib, name)


def test_chunks_runs_and_splits():
    """a pixel count that crosses the chunk of the launcher; the same call twice; a cube given in two pixel chunks"""
    K = _K()
    T, M, r = 9, 3, 3
    P = _lib_const("SSA_CHUNK") + 3
    x = _batch(T, P, np.float32, gaps=True, seed=5)
    want = K.ssa_fill_host(x, M, r, "bk", None, 1e-3, 4, 4)
    xd = _up(x)
    got = K.ssa_fill(xd, M, r, "bk", None, 1e-3, 4, 4)
    again = K.ssa_fill(xd, M, r, "bk", None, 1e-3, 4, 4)
    for g, a, w in zip(got, again, want):
        _same(g, w, "across the chunk")
        assert torch.equal(g.view(torch.int64), a.view(torch.int64))
    cut = _lib_const("SSA_CHUNK") - 61
    for lo, hi in ((0, cut), (cut, P)):
        part = K.ssa_fill(xd[:, lo:hi].contiguous(), M, r, "bk", None, 1e-3, 4, 4)
        for g, p in zip(got, part):
            assert torch.equal(g[..., lo:hi].contiguous().view(torch.int64), p.view(torch.int64)), (lo, hi)
    xc = _batch(65, 70, np.float64, gaps=False, seed=6)
    full = K.ssa_decompose(_up(xc), 24, 6, "vg", None, True)
    for lo, hi in ((0, 33), (33, 70)):
        part = K.ssa_decompose(_up(xc[:, lo:hi]), 24, 6, "vg", None, True)
        for g, p in zip(full, part):
            assert torch.equal(g[..., lo:hi].contiguous().view(torch.int64), p.view(torch.int64)), (lo, hi)


def test_overflowing_series_is_flagged_not_decomposed():
    """squares beyond the fp64 range: the trace of the solve is not finite, the series is flagged NONFINITE and its outputs are
    NaN, on the device as in the twin; its neighbours are untouched"""
    K = _K()
    T, M, r = 65, 5, 3
    x = _batch(T, 3, np.float64, gaps=False, seed=9)
    x[:, 1] *= 1e200
    want = K.ssa_decompose_host(x, M, r, "bk", None, True, True)
    got = K.ssa_decompose(_up(x), M, r, "bk", None, True, True)
    for g, w, nm in zip(got, want, ("eig", "maps", "rc", "evec")):
        _same(g, w, ("overflow", nm))
    assert list(want[1][U.IX["flags"]]) == [0, U.NONFINITE, 0]
    assert np.isnan(want[0][:, 1]).all() and np.isnan(want[2][:, :, 1]).all() and np.isnan(want[3][:, :, 1]).all()
    assert np.isfinite(want[2][:, :, [0, 2]]).all()
    x[5, :] = np.nan
    want = K.ssa_fill_host(x, M, r, "bk", None, 1e-3, 5)
    got = K.ssa_fill(_up(x), M, r, "bk", None, 1e-3, 5)
    for g, w, nm in zip(got, want, ("filled", "eig", "maps")):
        _same(g, w, ("overflow fill", nm))
    assert int(want[2][U.IX["flags"], 1]) == U.NONFINITE and np.isnan(want[0][:, 1]).all() and np.isfinite(want[0][:, [0, 2]]).all()


def test_groups_walk_the_pixels_in_chunks(monkeypatch):
    """the groups= path with more pixels than one pass holds (the pass size made small): eigenvalues, maps and group sums
    equal, bit for bit, those of a single pass; with a mask and a degenerate pixel in a later pass"""
    import gan_danet_amd as gd
    from gan_danet_amd import ssa as S
    T, M, r = 65, 12, 6
    x = _batch(T, 35, np.float64, gaps=False, seed=11)
    x[:, 20] = 4.0
    xd = _up(x).reshape(T, 5, 7)
    mask = torch.ones(5, 7, dtype=torch.bool, device="cuda:0")
    mask[3, 3] = False
    one = gd.ssa_decompose(xd, M, r, mask=mask, groups=[[0, 1], [2], [5, 4, 3]])
    monkeypatch.setattr(S, "_GROUP_CHUNK", 16)
    many = gd.ssa_decompose(xd, M, r, mask=mask, groups=[[0, 1], [2], [5, 4, 3]])
    for nm in ("eigenvalues", "groups", "trace", "mean", "sd", "n", "sweeps", "variance_fraction"):
        a, b = getattr(one, nm), getattr(many, nm)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), nm
    assert torch.equal(one.flags, many.flags) and int(one.flags[3, 3]) == U.MASKED and int(one.flags.reshape(-1)[20]) == U.CONSTANT
    assert bool(torch.isfinite(many.groups[:, :, 4, 6]).all())


def test_public_module():
    import gan_danet_amd as gd
    L = gd._lib
    T, M, r = 65, 12, 6
    rng = np.random.default_rng(2)
    for shape in ((T, 5, 7), (T, 2, 3, 4)):
        tail = shape[1:]
        t = np.arange(T).reshape((T,) + (1,) * len(tail))
        cube = 0.02 * t + np.sin(2 * np.pi * t / 12.0 + rng.random(tail) * 6) + 0.2 * rng.standard_normal(shape)
        for dt in (torch.float64, torch.float32):
            x = torch.from_numpy(cube).to("cuda:0").to(dt)
            res = gd.ssa_decompose(x, M, r, components=True)
            assert res.eigenvalues.shape == (r,) + tail and res.eigenvalues.dtype == torch.float64
            assert res.components.shape == (r, T) + tail and res.variance_fraction.shape == (r,) + tail
            assert res.flags.dtype == torch.int32 and res.flags.shape == tail and not res.flags.any()
            assert res.pairs(0.5).shape == (r - 1,) + tail and res.pairs(0.5).dtype == torch.bool and bool(res.pairs(0.5).any())
            assert gd.ssa_decompose(x, M, r).components is None
            grp = gd.ssa_decompose(x, M, r, groups=[[0], [1, 2], [5, 3]])
            assert grp.groups.shape == (3, T) + tail and grp.components is None
            c = res.components
            for g, want in zip(grp.groups, (c[0], c[1] + c[2], c[5] + c[3])):
                assert torch.equal(g.view(torch.int64), want.view(torch.int64))          # the order listed
            assert torch.equal(grp.eigenvalues, res.eigenvalues)
            assert torch.equal(res.reconstruct([1, 2]), c[1] + c[2] + res.mean)
            # all M components give the input back: (M^2 + 8 M) eps max|y| as in the CPU file, plus one rounding of the mean
            allc = gd.ssa_decompose(x, M, M, components=True)
            y = x.to(torch.float64)
            bound = ((M * M + 8 * M) * U.EPS * (y - allc.mean).abs().amax(0) + 2 * U.EPS * y.abs().amax(0))
            assert bool(((allc.reconstruct() - y).abs().amax(0) <= bound).all())
            gap = x.clone()
            gap[20:31, ..., 0] = float("nan")
            gap[3, ..., 1] = float("nan")
            f = gd.ssa_fill(gap, M, rank=4, filled64=dt == torch.float32)
            assert f.filled.dtype == dt and f.filled.shape == shape and (f.filled64 is None) == (dt == torch.float64)
            assert f.iterations.dtype == torch.int32 and f.converged.dtype == torch.bool and f.n_gaps.dtype == torch.int32
            assert f.eigenvalues.shape == (4,) + tail and f.n_gaps[..., 0].unique().tolist() == [11] and f.n_gaps[..., 2].max().item() == 0
            valid = ~torch.isnan(gap)
            assert torch.equal(f.filled[valid].view(torch.int32 if dt == torch.float32 else torch.int64),
                               x[valid].view(torch.int32 if dt == torch.float32 else torch.int64))
            assert bool(torch.isfinite(f.filled).all()) and bool((f.iterations[..., 0] > 0).all()) and bool((f.iterations[..., 2] == 0).all())
            assert bool(((f.filled - x)[20:31, ..., 0].abs() < 1.5).all())                  # close to the cycle it continues
    x = torch.from_numpy(cube).to("cuda:0")
    bad = (lambda: gd.ssa_decompose(x.cpu(), M), lambda: gd.ssa_fill(x.cpu(), M), lambda: gd.ssa_decompose(x, 1), lambda: gd.ssa_decompose(x, 65),
           lambda: gd.ssa_decompose(x, 40), lambda: gd.ssa_decompose(x, M, 0), lambda: gd.ssa_decompose(x, M, 17), lambda: gd.ssa_decompose(x, 4, 5),
           lambda: gd.ssa_decompose(x, M, method="svd"), lambda: gd.ssa_decompose(x, M, groups=[[0], []]), lambda: gd.ssa_decompose(x, M, groups=[[6]]),
           lambda: gd.ssa_decompose(x, M, groups=5), lambda: gd.ssa_decompose(x, M).reconstruct(), lambda: gd.ssa_decompose(x, M).pairs(0.0),
           lambda: gd.ssa_fill(x, M, rank=0), lambda: gd.ssa_fill(x, M, tol=0.0), lambda: gd.ssa_fill(x, M, tol=float("nan")),
           lambda: gd.ssa_fill(x, M, max_iter=0), lambda: gd.ssa_fill(x, M, max_iter=201), lambda: gd.ssa_fill(x, M, min_valid=1),
           lambda: gd.ssa_fill(x, M, method="toeplitz"), lambda: gd.ssa_fill(x, M, mask=torch.ones(3, device="cuda:0")),
           lambda: gd.ssa_fill(x.to(torch.float16), M), lambda: gd.ssa_fill(x, 2.0))
    for k, call in enumerate(bad):
        with pytest.raises(L.GandanetError):
            call()
            pytest.fail(f"bad argument {k} was accepted")


def test_filled_pixels_enter_eof_analysis():
    """pixels with a gap are invalid in eof_analysis; after ssa_fill they are valid and the analysis runs on the filled cube"""
    import gan_danet_amd as gd
    T, H, W = 48, 6, 8
    rng = np.random.default_rng(7)
    t = np.arange(T)[:, None, None]
    pattern = rng.standard_normal((H, W))
    cube = np.sin(2 * np.pi * t / 12.0) * pattern + 0.05 * t * rng.random((H, W)) + 0.1 * rng.standard_normal((T, H, W))
    x = torch.from_numpy(cube).to("cuda:0")
    x[20:25, 1, :] = float("nan")
    x[7, 4, 2] = float("nan")
    before = gd.eof_analysis(x, 2)
    assert not before.valid[1].any() and not before.valid[4, 2] and before.n_valid == H * W - W - 1
    f = gd.ssa_fill(x, 8, rank=4, max_iter=100)
    assert bool(f.converged.all()) and int(f.n_gaps.sum()) == 5 * W + 1
    after = gd.eof_analysis(f.filled, 2)
    assert bool(after.valid.all()) and after.n_valid == H * W and bool(torch.isfinite(after.eofs).all())
