"""GPU: the neighbourhood-verification kernels (csrc/neighborhood.hip) equal their host twins bit for bit -- sums, base, maps
and the fraction field, in both normalisations, on every case of tests/neighborhood_util.py -- equal the oracle's integers
directly in window mode, give the same bits on a second run and with a workspace of a single step (T walked in chunks), and
the public interface (fractions_skill_score, fss_cross_grid, drought_fss, useful_scale, the refusals) holds together."""
import numpy as np
import pytest
import torch

import neighborhood_util as U
from gpu_util import DEV

pytestmark = pytest.mark.gpu


def device_fss(K, case, dtype, below, normalize, planes=None):
    f, o = (torch.from_numpy(x).to(DEV) for x in case.cubes(dtype))
    mask = torch.from_numpy(case.mask).to(DEV).reshape(-1) if case.mask is not None else None
    sums, base, maps = K.nbr_fss(f, o, case.thr_f, case.thr_o, case.scales, below, normalize, True, mask, planes=planes)
    kind = np.float64 if normalize == "valid" else np.uint64
    return sums.cpu().numpy().view(kind), base.cpu().numpy().view(np.uint64), maps.cpu().numpy().view(kind)


@pytest.mark.parametrize("case,dtype,below", U.TWINS, ids=U.twin_id)
def test_device_equals_host_twin_and_oracle(case, dtype, below):
    from gan_danet_amd import kern as K
    want = U.oracle(case.name, below)
    f, o = case.cubes(dtype)
    T = f.shape[0]
    for normalize in ("window", "valid"):
        host = K.nbr_fss_host(f, o, case.thr_f, case.thr_o, case.scales, below, normalize, True, case.mask)
        dev = device_fss(K, case, dtype, below, normalize)
        for nm, h, d in zip(("sums", "base", "maps"), host, dev):
            assert U.same_bits(h, d), (case, normalize, nm)
        for nm, d, e in zip(("sums", "base", "maps"), dev, device_fss(K, case, dtype, below, normalize)):
            assert U.same_bits(d, e), (case, normalize, nm, "second run")
        if T > 1:      # a workspace of one step: T chunks
            for nm, d, e in zip(("sums", "base", "maps"), dev, device_fss(K, case, dtype, below, normalize, planes=1)):
                assert U.same_bits(d, e), (case, normalize, nm, "one step in flight")
        sums, base, maps = dev
        if normalize == "window":
            assert np.array_equal(sums, want.sums_w) and np.array_equal(base, want.base), (case, "oracle")
            # maps summed over the pixels are sums summed over time, exactly
            assert np.array_equal(maps.sum(axis=(2, 3)), sums.sum(axis=0)), case
        else:
            worst = U.worst_over_bound(sums, want.sums_v, want.bound_v)
            # both sides add the same non-negative terms, T * (valid pixels) of them at the most, in some order
            n_terms = int(want.base[..., 2].max()) * T
            total = maps.sum(axis=(2, 3))
            worst_m = U.worst_over_bound(total, sums.sum(axis=0), 2 * U.sum_bound(np.abs(total), n_terms))
            print(f"{case} {np.dtype(dtype).name} below={below}: valid-mode sums at most {worst:.3f} of the bound against fsum, "
                  f"maps over pixels against sums over time {worst_m:.3f}")
            assert worst <= 1.0 and worst_m <= 1.0


@pytest.mark.parametrize("normalize", ["window", "valid"])
@pytest.mark.parametrize("case", U.CASES, ids=repr)
def test_fraction_field(case, normalize):
    from gan_danet_amd import kern as K
    from gan_danet_amd import neighborhood as N
    mask = torch.from_numpy(case.mask).to(DEV) if case.mask is not None else None
    for dtype in U.DTYPES:
        f, _ = case.cubes(dtype)
        x = torch.from_numpy(f).to(DEV)
        for k, s, below in ((0, 1, True), (case.thr_f.shape[1] - 1, 4, True), (0, 5, False), (0, 0, True)):
            host = K.nbr_fraction_host(f, case.thr_f[:, k], case.scales[s], below, normalize, case.mask)
            got = N.neighborhood_fraction(x, case.thr_f[:, k], case.scales[s], below, mask, normalize)
            assert got.dtype == torch.float64 and U.same_bits(got.cpu().numpy(), host), (case, dtype, k, s, below)
            one = K.nbr_fraction(x, case.thr_f[:, k], case.scales[s], below, normalize, None if mask is None else mask.reshape(-1), planes=1)
            assert U.same_bits(one.cpu().numpy(), host), (case, dtype, k, s, below, "one step in flight")
    assert U.same_bits(host, U.fraction_oracle(case, 0, 0, True, normalize))


def test_public_interface_on_the_full_case():
    from gan_danet_amd import neighborhood as N
    case = U.BY_NAME["full"]
    want = U.oracle("full", True)
    f, o = (torch.from_numpy(x).to(DEV) for x in case.cubes(np.float32))
    mask = torch.from_numpy(case.mask).to(DEV)
    res = N.fractions_skill_score(f, o, case.thr_f, case.scales, thresholds_observed=case.thr_o, mask=mask, maps=True)
    assert res.sums.dtype == np.uint64 and np.array_equal(res.sums, want.sums_w) and np.array_equal(res.base, want.base)
    a, b, c = (want.sums_w[..., i].astype(object) for i in range(3))
    assert np.array_equal(res.fss, np.array(1.0 - (a / (b + c)).astype(np.float64)))
    pa, pb, pc = (x.sum(axis=0) for x in (a, b, c))
    assert np.array_equal(res.pooled, np.array(1.0 - (pa / (pb + pc)).astype(np.float64)))
    tot = want.base.astype(np.int64).sum(axis=0)
    assert np.array_equal(res.base_rate_forecast, tot[:, 0] / tot[:, 2]) and np.array_equal(res.base_rate_observed, tot[:, 1] / tot[:, 2])
    assert np.array_equal(res.frequency_bias, tot[:, 0] / tot[:, 1]) and np.array_equal(res.fss_random, res.base_rate_observed)
    assert np.array_equal(res.fss_uniform, 0.5 + res.base_rate_observed / 2)
    m = res.fss_map(1, 2).cpu().numpy()
    tw = want.terms_w[:, 1, 2].sum(axis=0)
    den = tw[..., 1] + tw[..., 2]
    assert m.shape == case.f.shape[1:] and np.array_equal(np.isnan(m), den == 0)
    assert np.array_equal(m[den > 0], 1.0 - tw[..., 0][den > 0] / den[den > 0])
    # thresholds as a plain list hold at every step and for both fields
    lst = N.fractions_skill_score(f, o, (-0.5, 0.3), (1, 5), below=False, normalize="valid")
    tab = N.fractions_skill_score(f, o, np.array([[-0.5, 0.3]] * 4), (1, 5), thresholds_observed=[-0.5, 0.3], below=False, normalize="valid")
    assert lst.sums.dtype == np.float64 and U.same_bits(lst.sums, tab.sums) and U.same_bits(lst.base, tab.base) and lst.maps is None
    with pytest.raises(N.L.GandanetError):
        lst.fss_map(0, 0)


def test_cross_grid_and_drought_wrappers():
    from gan_danet_amd import neighborhood as N
    from gan_danet_amd.drought import DSI_CLASSES
    rng = np.random.default_rng(21)
    lo = torch.from_numpy(rng.normal(size=(2, 8, 10))).to(DEV)
    hi = torch.from_numpy(rng.normal(size=(2, 40, 50))).to(DEV)
    fine = lo.repeat_interleave(5, dim=1).repeat_interleave(5, dim=2)
    assert fine.shape == hi.shape and bool((fine[:, 7, 13] == lo[:, 1, 2]).all())
    scales = (1, 5, 15, 101)
    for hi_first in (True, False):
        got = N.fss_cross_grid(hi, lo, 5, (-0.5, 0.2), scales, hi_is_forecast=hi_first, normalize="window")
        want = N.fractions_skill_score(hi, fine, (-0.5, 0.2), scales) if hi_first else N.fractions_skill_score(fine, hi, (-0.5, 0.2), scales)
        assert U.same_bits(got.sums, want.sums) and U.same_bits(got.base, want.base) and got.scales == scales
    a, b = hi, hi + 0.5 * torch.from_numpy(rng.normal(size=(2, 40, 50))).to(DEV)
    got = N.drought_fss(a, b, scales=scales)
    want = N.fractions_skill_score(a, b, DSI_CLASSES, scales, below=True)
    assert got.sums.shape == (2, 5, 4, 3) and U.same_bits(got.sums, want.sums) and U.same_bits(got.base, want.base)
    assert np.array_equal(got.thresholds, np.array([DSI_CLASSES] * 2))
    for bad in (lambda: N.fss_cross_grid(hi, lo, 4, (-0.5,)), lambda: N.fss_cross_grid(hi, lo, 0, (-0.5,)),
                lambda: N.fss_cross_grid(hi, lo.cpu(), 5, (-0.5,))):
        with pytest.raises(N.L.GandanetError):
            bad()


def test_useful_scale_on_the_displaced_pixel():
    from gan_danet_amd import neighborhood as N
    d = 4
    f, o, thr, scales = U.displaced(d)
    res = N.fractions_skill_score(torch.from_numpy(f).to(DEV), torch.from_numpy(o).to(DEV), thr, scales)
    for s, n in enumerate(scales):
        assert res.sums[0, 0, s].tolist() == [2 * n * min(d, n), n * n, n * n], n
    # FSS = 1 - min(d, n) / n: 0, 0, 1/5, 3/7, 5/9, 7/11 against 0.5 + f_o / 2 just above one half
    assert np.array_equal(res.pooled[0], np.array([1.0 - min(d, n) / n for n in scales]))
    assert res.useful_scale(0) == 9
    assert N.FSSResult(res.sums[:, :, :4], res.base, scales[:4], res.thresholds, res.thresholds, "window", None).useful_scale(0) is None
    same = N.fractions_skill_score(torch.from_numpy(f).to(DEV), torch.from_numpy(f).to(DEV), thr, scales)
    assert np.all(same.fss == 1.0) and same.useful_scale(0) == 1


def test_refusals_on_the_device():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import neighborhood as N
    x = torch.zeros((2, 5, 6), device=DEV, dtype=torch.float64)
    thr9, sc33 = tuple(-0.1 * k for k in range(9)), tuple(range(1, 67, 2))
    for call in (lambda: N.fractions_skill_score(x.cpu(), x, (-0.5,), (1, 3)), lambda: N.fractions_skill_score(x, x.cpu(), (-0.5,), (1, 3)),
                 lambda: N.fractions_skill_score(x, x[:, :4], (-0.5,), (1, 3)), lambda: N.fractions_skill_score(x, x[:1], (-0.5,), (1, 3)),
                 lambda: N.fractions_skill_score(x, x.float(), (-0.5,), (1, 3)), lambda: N.fractions_skill_score(x.int(), x.int(), (-0.5,), (1, 3)),
                 lambda: N.fractions_skill_score(x, x, (-0.5,), (1, 4)), lambda: N.fractions_skill_score(x, x, (-0.5,), (0,)),
                 lambda: N.fractions_skill_score(x, x, (-0.5,), (-3,)), lambda: N.fractions_skill_score(x, x, (-0.5,), ()),
                 lambda: N.fractions_skill_score(x, x, thr9, (1, 3)), lambda: N.fractions_skill_score(x, x, (), (1, 3)),
                 lambda: N.fractions_skill_score(x, x, (-0.5,), sc33), lambda: N.fractions_skill_score(x, x, (float("nan"),), (1, 3)),
                 lambda: N.fractions_skill_score(x, x, (-0.5,), (1, 3), normalize="padded"),
                 lambda: N.fractions_skill_score(x, x, (-0.5,), (1, 3), thresholds_observed=(-0.5, 0.1)),
                 lambda: N.fractions_skill_score(x, x, np.zeros((3, 1)), (1, 3)),
                 lambda: N.fractions_skill_score(x, x, (-0.5,), (1, 3), mask=torch.ones(5, 5, device=DEV, dtype=torch.uint8)),
                 lambda: N.neighborhood_fraction(x, -0.5, 4), lambda: N.neighborhood_fraction(x[0], -0.5, 3),
                 lambda: N.neighborhood_fraction(x, (-0.5, 0.1, 0.2), 3)):
        with pytest.raises(L.GandanetError):
            call()
