"""CPU: the regionalisation entry points of the C ABI (include/gandanet.h, "Regionalisation") are declared and bound, reject bad
arguments with error codes, and their host twins (plain C++ over csrc/kmeans_core.h, no GPU) agree with the independent
long-double oracle of regions_util.py: labels and counts exactly (the blobs leave no pixel undecided), distances, centroids and
sums within the derived bounds, and to the bit on integer-valued data with planted ties.  Run with -s to see the largest observed
multiple of each bound.

Measured: the worst multiples over the grid were 0.869 (dist), 0.924 (dist2), both at T = 1 where the bound is three roundings,
0.300 (centroid), 0.326 (wsum), 0.401 (within); the file takes 10 s."""
import ctypes as C
import os

import numpy as np
import pytest

import regions_util as U

NAMES = ("gd_km_assign", "gd_km_assign_host", "gd_km_update_ws_bytes", "gd_km_update_min_ws_bytes", "gd_km_update", "gd_km_update_host",
         "gd_km_farthest", "gd_km_farthest_host")


def _K():
    from gan_danet_amd import kern
    return kern


def test_entries_are_declared_and_bound():
    K = _K()
    L, lib = K.L, K.lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
        decl = src[src.index(name + "("):]
        decl = decl[:decl.index(")")]
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]), name
    for macro, val in (("GD_KM_MAX_T", L.KM_MAX_T), ("GD_KM_MAX_K", L.KM_MAX_K), ("GD_KM_CHUNK", L.KM_CHUNK), ("GD_KM_SLAB", L.KM_SLAB)):
        assert f"#define {macro} {val}\n" in src, macro
    assert (L.KM_MAX_T, L.KM_MAX_K, L.KM_CHUNK, L.KM_SLAB) == (U.MAX_T, U.MAX_K, U.CHUNK, U.SLAB)
    assert K.km_update_workspace(181, 2500, 7) == (1 + 3) * (7 * 181 + 21) * 8 and K.km_update_min_workspace(181, 7) == 2 * (7 * 181 + 21) * 8


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", U.TS)
def test_twins_against_the_oracle(T, dtype):
    K = _K()
    worst = np.zeros(5)
    for M in U.MS:
        for Kc in U.KS:
            x, cent, _ = U.blobs(T, M, Kc, dtype)
            mask = U.mask_for(M) if M == 65 else None
            w = np.cos(np.linspace(-1.2, 1.2, M)) if M in (63, 257) else None
            got = K.km_assign_host(x, cent, mask=mask, second=True)
            want = U.assign(x, cent, mask=mask)
            r = U.check_assign(got, want, (T, M, Kc))
            up = K.km_update_host(x, got[0], got[1], cent, w)
            ru = U.check_update(up, U.update(x, want["label"], want["dist"], want["bound"], cent, w), (T, M, Kc))
            worst = np.maximum(worst, r + ru)
            assert K.km_assign_host(x, cent, mask=mask)[2:] == (None, None)
    print(f"\nT = {T} {np.dtype(dtype).name}: worst multiples of the bounds: dist {worst[0]:.3f} dist2 {worst[1]:.3f} "
          f"centroid {worst[2]:.3f} wsum {worst[3]:.3f} within {worst[4]:.3f}")


@pytest.mark.parametrize("normalize", ["center", "zscore"])
def test_shift_and_scale_against_the_oracle(normalize):
    K = _K()
    for T, M, Kc in ((65, 257, 9), (181, 65, 33)):
        x, _, lab = U.blobs(T, M, Kc, seed=3)
        x = x + 5.0
        shift = x.mean(axis=0)
        scale = 1.0 / x.std(axis=0) if normalize == "zscore" else None
        v = ((x - shift) * (1.0 if scale is None else scale))
        cent = np.stack([v[:, lab == k].mean(axis=1) if (lab == k).any() else v[:, 0] + 7.0 for k in range(Kc)]) + 0.003
        got = K.km_assign_host(x, cent, shift, scale, second=True)
        want = U.assign(x, cent, shift, scale)
        r = U.check_assign(got, want, (normalize, T, M, Kc))
        w = np.linspace(0.5, 1.5, M)
        ru = U.check_update(K.km_update_host(x, got[0], got[1], cent, w, shift, scale),
                            U.update(x, want["label"], want["dist"], want["bound"], cent, w, shift, scale), (normalize, T, M, Kc))
        print(f"\n{normalize} T = {T}: worst multiples: dist {r[0]:.3f} dist2 {r[1]:.3f} centroid {ru[0]:.3f} wsum {ru[1]:.3f} within {ru[2]:.3f}")


@pytest.mark.parametrize("M", (1025, 2500))
def test_update_across_slabs(M):
    """more than one slab of 1024 pixels: the slab sums are added in ascending order"""
    K = _K()
    x, cent, _ = U.blobs(33, M, 7)
    w = np.linspace(0.25, 1.75, M)
    got = K.km_assign_host(x, cent)
    want = U.assign(x, cent)
    U.check_assign(got, want, M, need_second=False)
    ru = U.check_update(K.km_update_host(x, got[0], got[1], cent, w), U.update(x, want["label"], want["dist"], want["bound"], cent, w), M)
    print(f"\nM = {M}: worst multiples: centroid {ru[0]:.3f} wsum {ru[1]:.3f} within {ru[2]:.3f}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_integer_data_is_exact_with_planted_ties(dtype):
    """small integers, dyadic shift / scale / weights: every operation is exact, so twin and oracle agree to the bit; centroid 3
    repeats centroid 1 and centroid 5 mirrors centroid 0 about pixel 4, so there are exact ties, which go to the lower index"""
    K = _K()
    rng = np.random.default_rng(5)
    T, M, Kc = 65, 130, 9
    x = rng.integers(-8, 9, size=(T, M)).astype(dtype)
    shift = rng.integers(-2, 3, size=M).astype(np.float64)
    scale = 2.0 ** rng.integers(-2, 3, size=M)
    cent = rng.integers(-4, 5, size=(Kc, T)).astype(np.float64) / 4.0
    cent[3] = cent[1]
    v4 = (x[:, 4].astype(np.float64) - shift[4]) * scale[4]
    cent[5] = 2.0 * v4 - cent[0]                                     # |v4 - c5| = |v4 - c0| term by term
    x[:, 7] = ((cent[1] / scale[7]) + shift[7]).astype(dtype)        # pixel 7 sits on centroids 1 and 3: distance 0 to both
    assert np.array_equal((x[:, 7].astype(np.float64) - shift[7]) * scale[7], cent[1])
    got = K.km_assign_host(x, cent, shift, scale, second=True)
    want = U.assign(x, cent, shift, scale)
    assert np.array_equal(got[0], want["label"]) and np.array_equal(got[2], want["label2"])
    assert np.array_equal(got[1], want["dist"].astype(np.float64)) and np.array_equal(got[3], want["dist2"].astype(np.float64))
    assert got[0][7] == 1 and got[2][7] == 3 and got[1][7] == 0.0 and got[3][7] == 0.0
    only = U.assign(x[:, 4:5], cent[[0, 5]], shift[4:5], scale[4:5])   # the mirrored pair alone: an exact tie, index 0 wins
    assert only["margin"][0] == 0 and only["label"][0] == 0
    assert K.km_assign_host(np.ascontiguousarray(x[:, 4:5]), cent[[0, 5]], shift[4:5], scale[4:5])[0][0] == 0
    assert K.km_assign_host(np.ascontiguousarray(x[:, 4:5]), cent[[5, 0]], shift[4:5], scale[4:5])[0][0] == 0
    w = 2.0 ** rng.integers(-1, 2, size=M)
    cnew, wsum, count, within = K.km_update_host(x, got[0], got[1], cent, w, shift, scale)
    o = U.update(x, want["label"], want["dist"], want["bound"], cent, w, shift, scale)
    assert np.array_equal(count, o["count"]) and np.array_equal(wsum, o["wsum"].astype(np.float64))
    assert np.array_equal(within, o["within"].astype(np.float64))
    v = U.sample(x, shift, scale)
    for k in range(Kc):
        mem = want["label"] == k
        if mem.any():                                                 # exact numerator and denominator, one fp64 division
            num = (v[:, mem] * w[mem].astype(U.LD)[None, :]).sum(axis=1).astype(np.float64)
            assert np.array_equal(cnew[k], num / np.float64(o["wsum"][k])), k
        else:
            assert np.array_equal(cnew[k], cent[k])


def test_nan_and_masked_series_touch_nothing():
    K = _K()
    x, cent, _ = U.blobs(24, 70, 4)
    base = K.km_assign_host(x, cent, second=True)
    bad = x.copy()
    bad[3, 5], bad[0, 11], bad[23, 64] = np.nan, np.inf, -np.inf
    mask = np.ones(70, dtype=np.uint8)
    mask[[0, 69]] = 0
    out = [5, 11, 64, 0, 69]
    got = K.km_assign_host(bad, cent, mask=mask, second=True)
    keep = np.setdiff1d(np.arange(70), out)
    for g, b in zip(got, base):
        assert np.array_equal(g[keep], b[keep])
    assert (got[0][out] == -1).all() and (got[2][out] == -1).all() and np.isnan(got[1][out]).all() and np.isnan(got[3][out]).all()
    w = np.linspace(1.0, 2.0, 70)
    a = K.km_update_host(bad, got[0], got[1], cent, w)
    b = K.km_update_host(np.ascontiguousarray(x[:, keep]), base[0][keep], base[1][keep], cent, w[keep])
    for p, q in zip(a, b):
        assert np.array_equal(p, q)                                   # fewer than one slab: the same additions in the same order
    assert int(a[2].sum()) == 65


def test_k_one_and_an_empty_cluster():
    K = _K()
    x, _, _ = U.blobs(12, 40, 1)
    cent = np.full((1, 12), 2.0)
    label, dist, label2, dist2 = K.km_assign_host(x, cent, second=True)
    assert (label == 0).all() and (label2 == -1).all() and np.isnan(dist2).all()
    cnew, wsum, count, within = K.km_update_host(x, label, dist, cent)
    assert count[0] == 40 and wsum[0] == 40.0
    cent3 = np.stack([x[:, :20].mean(axis=1), np.full(12, 1e3), x[:, 20:].mean(axis=1)])
    label, dist, _, _ = K.km_assign_host(x, cent3)
    assert not (label == 1).any()
    cnew, wsum, count, within = K.km_update_host(x, label, dist, cent3)
    assert count[1] == 0 and wsum[1] == 0.0 and within[1] == 0.0 and np.array_equal(cnew[1], cent3[1])
    # a cluster whose members all weigh nothing also keeps its centroid, and reports its count
    label[:] = 0
    w = np.zeros(40)
    cnew, wsum, count, within = K.km_update_host(x, label, dist, cent3, w)
    assert count[0] == 40 and wsum[0] == 0.0 and np.array_equal(cnew, cent3)


def test_weights_are_honoured():
    K = _K()
    x, cent, _ = U.blobs(6, 50, 3)
    label, dist, _, _ = K.km_assign_host(x, cent)
    w = np.zeros(50)
    w[[0, 1, 2, 30, 31, 32]] = 1.0                                    # only six pixels weigh: the means are theirs
    cnew, wsum, count, within = K.km_update_host(x, label, dist, cent, w)
    for k in range(3):
        mem = np.flatnonzero((label == k) & (w > 0))
        assert wsum[k] == len(mem) and count[k] == (label == k).sum()
        np.testing.assert_allclose(cnew[k], x[:, mem].mean(axis=1), rtol=1e-14)
        np.testing.assert_allclose(within[k], dist[mem].sum(), rtol=1e-14)


def test_result_for_a_series_does_not_depend_on_m():
    K = _K()
    x, cent, _ = U.blobs(65, 257, 9, np.float32)
    shift, scale = x.mean(axis=0).astype(np.float64), np.linspace(0.5, 2.0, 257)
    full = K.km_assign_host(x, cent, shift, scale, second=True)
    for cols in (np.arange(64, 129), np.array([256]), np.arange(0, 257, 3)):
        part = K.km_assign_host(np.ascontiguousarray(x[:, cols]), cent, shift[cols], scale[cols], second=True)
        for p, q in zip(part, full):
            assert np.array_equal(p, q[cols])


def test_farthest():
    K = _K()
    d = np.array([1.0, 5.0, np.nan, 5.0, np.inf, 2.0, 5.0, -np.inf])
    assert K.km_farthest_host(d)[0] == 1                              # the tie of 1, 3, 6 goes to the lowest; inf is not finite
    assert K.km_farthest_host(d, np.array([1], dtype=np.int32))[0] == 3
    assert K.km_farthest_host(d, np.array([6, 1, 3], dtype=np.int32))[0] == 5
    assert K.km_farthest_host(d, np.array([1, 3, 6, 5, 0], dtype=np.int32))[0] == -1
    assert K.km_farthest_host(np.full(9, np.nan))[0] == -1
    assert K.km_farthest_host(np.array([-3.0]))[0] == 0
    rng = np.random.default_rng(2)
    big = rng.integers(0, 50, size=5000).astype(np.float64)
    big[rng.integers(0, 5000, size=300)] = np.nan
    ex = []
    for _ in range(12):
        got = int(K.km_farthest_host(big, np.array(ex, dtype=np.int32) if ex else None)[0])
        assert got == U.farthest(big, ex)
        ex.append(got)
    with pytest.raises(K.L.GandanetError):
        K.km_farthest_host(big, np.arange(65, dtype=np.int32))


def test_argument_checks_return_error_codes():
    K = _K()
    lib = K.lib()
    x, cent = np.zeros((4, 8)), np.zeros((2, 4))
    lab, d = np.zeros(8, dtype=np.int32), np.zeros(8)
    ws, cnt = np.zeros(2), np.zeros(2, dtype=np.int64)
    p = lambda a: a.ctypes.data

    def assign(xp=p(x), dtype=1, T=4, M=8, cp=p(cent), Kc=2, lp=p(lab), dp=p(d), l2=None, d2=None):
        return lib.gd_km_assign_host(xp, dtype, T, M, cp, Kc, None, None, None, lp, dp, l2, d2)

    def update(xp=p(x), T=4, M=8, Kc=2, lp=p(lab), cp=p(cent), wp=None):
        return lib.gd_km_update_host(xp, 1, T, M, lp, p(d), wp, None, None, Kc, cp, p(ws), p(cnt), p(ws))

    assert assign() == 0 and update() == 0
    for bad in (dict(xp=None), dict(cp=None), dict(lp=None), dict(dp=None), dict(dtype=2), dict(T=0), dict(T=U.MAX_T + 1), dict(M=0), dict(M=-3),
                dict(Kc=0), dict(Kc=U.MAX_K + 1), dict(xp=p(x) + 4), dict(cp=p(cent) + 4), dict(lp=p(lab) + 2), dict(dp=p(d) + 4),
                dict(d2=p(d) + 4), dict(l2=p(lab) + 1)):
        assert assign(**bad) == -1 and K.L.last_error().startswith("gd_km_assign_host"), bad
    for bad in (dict(xp=None), dict(lp=None), dict(cp=None), dict(T=0), dict(T=U.MAX_T + 1), dict(M=0), dict(Kc=0), dict(Kc=U.MAX_K + 1),
                dict(xp=p(x) + 4), dict(wp=p(d) + 4), dict(lp=p(lab) + 2)):
        assert update(**bad) == -1 and K.L.last_error().startswith("gd_km_update_host"), bad
    idx = np.zeros(1, dtype=np.int32)
    assert lib.gd_km_farthest_host(p(d), 8, None, 0, p(idx)) == 0
    for args in ((None, 8, None, 0, p(idx)), (p(d), 0, None, 0, p(idx)), (p(d), 8, None, 1, p(idx)), (p(d), 8, p(lab), 65, p(idx)),
                 (p(d), 8, None, 0, None), (p(d) + 4, 8, None, 0, p(idx)), (p(d), 8, p(lab) + 2, 1, p(idx))):
        assert lib.gd_km_farthest_host(*args) == -1, args
    # the device entries make the same checks before any launch (no GPU is touched)
    assert lib.gd_km_assign(None, 1, 4, 8, p(cent), 2, None, None, None, p(lab), p(d), None, None, None) == -1
    assert lib.gd_km_assign(p(x), 1, 4, 8, p(cent), 65, None, None, None, p(lab), p(d), None, None, None) == -1
    assert lib.gd_km_update(p(x), 1, 4, 8, p(lab), p(d), None, None, None, 2, p(cent), p(ws), p(cnt), p(ws), None, 0, None) == -1
    assert lib.gd_km_update(p(x), 1, 4, 8, p(lab), p(d), None, None, None, 2, p(cent), p(ws), p(cnt), p(ws), p(x), 8, None) == -1
    assert "workspace" in K.L.last_error()
    assert lib.gd_km_farthest(p(d), 0, None, 0, p(idx), None) == -1
    assert lib.gd_km_update_ws_bytes(0, 8, 2) == 0 and lib.gd_km_update_min_ws_bytes(4, 65) == 0
    for bad in (dict(cent=np.zeros((2, 5))), dict(cent=np.zeros((65, 4))), dict(shift=np.zeros(7)), dict(mask=np.ones(9, dtype=np.uint8))):
        kw = dict(cent=cent)
        kw.update(bad)
        with pytest.raises(K.L.GandanetError):
            K.km_assign_host(x, **kw)
