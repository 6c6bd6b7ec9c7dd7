"""CPU: the dataset-preparation entry points of the C ABI (include/gandanet.h, "dataset preparation") are declared and
bound, every device entry point rejects bad arguments before any launch, gd_scale_from_moments_host reproduces sklearn's
StandardScaler attributes, split_indices reproduces sklearn's split, the host cosine table agrees with numpy, and the
public module refuses CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

NAMES = ("gd_channel_moments_ws_bytes", "gd_channel_moments", "gd_scale_from_moments_host", "gd_channel_affine",
         "gd_freq_cos_table_host", "gd_freq_augment_axis")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_prepare_symbols_are_declared_and_bound():
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    assert "Dataset preparation" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name


def test_prepare_argument_errors_before_any_launch():
    """negative code + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses)
    are not touched"""
    L, lib = _lib()
    p, q, r, s = 0x1000, 0x2000, 0x3000, 0x4000

    def bad(rc, word):
        assert rc < 0, rc
        assert word in L.last_error(), L.last_error()

    mom = lib.gd_channel_moments
    big = 1 << 30
    bad(mom(None, 0, 10, 3, q, r, big, None), "null")
    bad(mom(p, 0, 10, 3, None, r, big, None), "null")
    bad(mom(p, 0, 10, 3, q, None, big, None), "null")
    bad(mom(p, 2, 10, 3, q, r, big, None), "dtype")
    bad(mom(p, -1, 10, 3, q, r, big, None), "dtype")
    bad(mom(p, 0, 0, 3, q, r, big, None), "<= 0")
    bad(mom(p, 0, -4, 3, q, r, big, None), "<= 0")
    bad(mom(p, 0, 10, 0, q, r, big, None), "<= 0")
    bad(mom(p, 0, 10, -1, q, r, big, None), "<= 0")
    need = lib.gd_channel_moments_ws_bytes(5000, 3)
    assert need > 0 and need % 24 == 0
    bad(mom(p, 0, 5000, 3, q, r, need - 1, None), "workspace")
    bad(mom(p + 4, 1, 10, 3, q, r, big, None), "aligned")
    assert lib.gd_channel_moments_ws_bytes(0, 3) == 0 and lib.gd_channel_moments_ws_bytes(5, 0) == 0

    aff = lib.gd_channel_affine
    bad(aff(None, 0, q, 0, 10, 3, r, s, 0, 0, 0, None), "null")
    bad(aff(p, 0, None, 0, 10, 3, r, s, 0, 0, 0, None), "null")
    bad(aff(p, 0, q, 0, 10, 3, None, s, 0, 0, 0, None), "null")
    bad(aff(p, 0, q, 0, 10, 3, r, None, 0, 0, 0, None), "null")
    bad(aff(p, 0, p, 0, 10, 3, r, s, 0, 0, 0, None), "src == dst")
    bad(aff(p, 2, q, 0, 10, 3, r, s, 0, 0, 0, None), "dtype")
    bad(aff(p, 0, q, -1, 10, 3, r, s, 0, 0, 0, None), "dtype")
    bad(aff(p, 0, q, 0, 0, 3, r, s, 0, 0, 0, None), "<= 0")
    bad(aff(p, 0, q, 0, 10, 0, r, s, 0, 0, 0, None), "<= 0")
    bad(aff(p, 0, q, 0, 10, -2, r, s, 0, 0, 0, None), "<= 0")
    bad(aff(p, 0, q, 0, 10, 3, r, s, 2, 0, 0, None), "inverse")
    bad(aff(p, 0, q, 0, 10, 3, r, s, 0, 3, 3, None), "N * HW == M")
    bad(aff(p, 0, q, 0, 10, 3, r, s, 0, -1, 10, None), "N * HW == M")
    bad(aff(p, 0, q, 0, 10, 3, r, s, 0, 2, 0, None), "N * HW == M")
    bad(aff(p, 0, q + 4, 1, 10, 3, r, s, 0, 0, 0, None), "aligned")

    fq = lib.gd_freq_augment_axis
    bad(fq(None, q, 0, 2, 10, 3, r, 2, s, None), "null")
    bad(fq(p, None, 0, 2, 10, 3, r, 2, s, None), "null")
    bad(fq(p, q, 0, 2, 10, 3, None, 2, s, None), "null")
    bad(fq(p, q, 0, 2, 10, 3, r, 2, None, None), "null")
    bad(fq(p, p, 0, 2, 10, 3, r, 2, s, None), "src == dst")
    bad(fq(p, q, 2, 2, 10, 3, r, 2, s, None), "dtype")
    bad(fq(p, q, -1, 2, 10, 3, r, 2, s, None), "dtype")
    bad(fq(p, q, 0, 2, 0, 3, r, 1, s, None), "L <= 0")
    bad(fq(p, q, 0, 2, -3, 3, r, 1, s, None), "L <= 0")
    bad(fq(p, q, 0, 0, 10, 3, r, 2, s, None), "<= 0")
    bad(fq(p, q, 0, 2, 10, 0, r, 2, s, None), "<= 0")
    bad(fq(p, q, 0, 2, 10, 3, r, 0, s, None), "K1 < 1")
    bad(fq(p, q, 0, 2, 10, 3, r, -1, s, None), "K1 < 1")
    bad(fq(p, q, 0, 2, 10, 3, r, 11, s, None), "K1 > L")
    bad(fq(p, q, 0, 2, 100, 3, r, 34, s, None), "K1 > 33")
    cap = L.FREQ_MAX_TABLE_BYTES
    bad(fq(p, q, 0, 2, cap // (8 * 33) + 1, 3, r, 33, s, None), "over the cap")      # 33 * L * 8 bytes just over the cap
    bad(fq(p, q, 0, 2, cap // 8 + 1, 3, r, 1, s, None), "over the cap")
    bad(fq(p + 4, q, 1, 2, 10, 3, r, 2, s, None), "aligned")

    tab = lib.gd_freq_cos_table_host
    buf = (C.c_double * 64)()
    bad(tab(10, 2, None), "null")
    bad(tab(0, 1, buf), "L <= 0")
    bad(tab(10, 0, buf), "K1")
    bad(tab(5, 6, buf), "K1")
    bad(tab(100, 34, buf), "K1")

    sc = lib.gd_scale_from_moments_host
    d3, d1 = (C.c_double * 3)(4.0, 1.0, 2.0), (C.c_double * 1)()
    bad(sc(None, 1, d1, d1, d1), "null")
    bad(sc(d3, 1, None, d1, d1), "null")
    bad(sc(d3, 0, d1, d1, d1), "C <= 0")
    bad(sc((C.c_double * 3)(0.0, 0.0, 0.0), 1, d1, d1, d1), "without samples")


def _moments(x):
    """(count, mean, M2) per column of a 2-D fp64 array, two-pass in numpy"""
    mean = x.mean(axis=0)
    return np.stack([np.full(x.shape[1], float(x.shape[0])), mean, ((x - mean) ** 2).sum(axis=0)], axis=1)


SCALE_CASES = {
    "plain": lambda rs: rs.randn(400, 5) * np.array([1.0, 3.0, 0.01, 50.0, 2.0]) + np.array([0.0, -2.0, 7.0, 100.0, 1e-3]),
    "constant_channel": lambda rs: np.concatenate([rs.randn(300, 2), np.full((300, 1), 3.25), np.zeros((300, 1))], axis=1),
    "mean_1e4_std_1e-3": lambda rs: np.concatenate([1e4 + 1e-3 * rs.randn(1000, 1), rs.randn(1000, 1)], axis=1),
    "one_row": lambda rs: rs.randn(1, 4) * 10.0,
}


@pytest.mark.parametrize("case", sorted(SCALE_CASES))
def test_scale_from_moments_host_against_sklearn(case):
    from sklearn.preprocessing import StandardScaler
    from gan_danet_amd import kern as K
    x = SCALE_CASES[case](np.random.RandomState(5))
    ref = StandardScaler().fit(x)
    mean, var, scale = K.scale_from_moments_host(_moments(x))

    def ulps(got, want):
        return float(np.max(np.abs(got - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny))))

    u_mean, u_scale = ulps(mean, ref.mean_), ulps(scale, ref.scale_)
    print(f"{case}: mean_ {u_mean} ulp, scale_ {u_scale} ulp from sklearn; scale_ = {scale}")
    assert mean.dtype == var.dtype == scale.dtype == np.float64
    assert u_mean <= 4 and u_scale <= 4
    assert np.array_equal(scale == 1.0, ref.scale_ == 1.0)          # the same channels are called constant
    if case == "constant_channel":
        assert scale[2] == 1.0 and scale[3] == 1.0 and var[2] == 0.0
    if case == "one_row":
        assert np.all(scale == 1.0) and np.all(var == 0.0)
    if case == "mean_1e4_std_1e-3":
        assert 0.9e-3 < scale[0] < 1.1e-3                          # far above sklearn's constant threshold


@pytest.mark.parametrize("n", [5, 181, 543])
@pytest.mark.parametrize("seed", [42, 7])
def test_split_indices_equal_sklearn(n, seed):
    from sklearn.model_selection import train_test_split
    from gan_danet_amd import prepare
    want_train, want_test = train_test_split(np.arange(n), test_size=0.2, random_state=seed)
    train, test = prepare.split_indices(n, 0.2, seed)
    assert np.array_equal(train, want_train) and np.array_equal(test, want_test)


@pytest.mark.parametrize("n,k1", [(181, 13), (5, 5), (300, 33), (1, 1), (25, 13), (7919, 33)])
def test_cos_table_host(n, k1):
    from gan_danet_amd import kern as K
    got = K.freq_cos_table_host(n, k1)
    k, t = np.arange(k1, dtype=np.int64)[:, None], np.arange(n, dtype=np.int64)[None, :]
    want = np.cos(2 * np.pi * ((k * t) % n) / n) / n
    ulps = np.max(np.abs(got - want) / np.spacing(np.abs(want)))
    print(f"cosine table L = {n}, K1 = {k1}: max {ulps} ulp from numpy")
    assert got.shape == (k1, n) and got.dtype == np.float64
    assert ulps <= 1.0


def test_used_bins():
    from gan_danet_amd import prepare
    assert prepare.used_bins(12, 181) == 13 and prepare.used_bins(12, 5) == 5 and prepare.used_bins(2, 1) == 1
    assert prepare.used_bins(0, 40) == 1
    with pytest.raises(ValueError):
        prepare.used_bins(-1, 10)


def test_cpu_tensors_are_refused():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import prepare
    x = torch.zeros(6, 4, 5, 3, dtype=torch.float64)
    sc = prepare.ChannelScaler.from_sklearn([type("S", (), dict(mean_=[0.0], var_=[1.0], scale_=[1.0], n_samples_seen_=4))()
                                             for _ in range(3)])
    assert sc.mean_.shape == (3,) and sc.n_samples_seen_ == 4
    calls = [lambda: prepare.ChannelScaler().fit(x), lambda: prepare.ChannelScaler().fit(x, channel_axis=None),
             lambda: sc.transform(x), lambda: sc.inverse_transform(x),
             lambda: prepare.frequency_domain_augmentation(x, 12),
             lambda: prepare.augment_dataset(x[..., 0], x[..., 0], x[..., 1], x[..., 1], x),
             lambda: prepare.train_test_split(x, x)]
    for call in calls:
        with pytest.raises(L.GandanetError):
            call()
    import gan_danet_amd
    assert gan_danet_amd.prepare is prepare
