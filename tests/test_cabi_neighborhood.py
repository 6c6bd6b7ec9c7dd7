"""CPU: the neighbourhood-verification entry points of the C ABI (include/gandanet.h, "Neighbourhood verification") are
declared, bound and re-exported, refuse every bad argument before any launch, and the host twins -- plain C++ over
csrc/neighborhood_core.h -- give the oracle of tests/neighborhood_util.py: the integer records exactly, the fp64 sums of
normalize="valid" inside the summation bound derived there, the fraction field bit for bit, and the closed forms.  Each test
prints its largest error over its bound (pytest -s)."""
import os

import numpy as np
import pytest
import torch

import neighborhood_util as U

NAMES = ("gd_nbr_fss", "gd_nbr_fraction")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_neighborhood_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import build, kern, neighborhood
    L, lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gandanet.h")).read()
    assert "Neighbourhood verification (neighborhood.hip, csrc/neighborhood_core.h)" in src
    for name in NAMES:
        for nm in (name, name + "_host"):
            assert nm + "(" in src and nm in L.SIGNATURES and hasattr(lib, nm) and hasattr(kern, nm[3:]), nm
    assert "gd_nbr_ws_bytes(" in src and "gd_nbr_ws_bytes" in L.SIGNATURES and hasattr(kern, "nbr_ws_bytes")
    for nm, v in (("MAX_HW", L.NBR_MAX_HW), ("MAX_K", L.NBR_MAX_K), ("MAX_S", L.NBR_MAX_S)):
        assert f"#define GD_NBR_{nm} {v}" in src, nm
    assert (L.NBR_MAX_HW, L.NBR_MAX_K, L.NBR_MAX_S) == (1 << 20, 8, 32)
    assert f"GD_NBR_WINDOW = {L.NBR_NORMALIZE['window']}" in src and f"GD_NBR_VALID = {L.NBR_NORMALIZE['valid']}" in src
    assert "neighborhood.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "neighborhood_core.h"))
    assert gan_danet_amd.neighborhood is neighborhood
    for name in ("FSSResult", "fractions_skill_score", "neighborhood_fraction", "fss_cross_grid", "drought_fss"):
        assert getattr(gan_danet_amd, name) is getattr(neighborhood, name)
    # the workspace: the tables of (H + 1) (W + 1) 8-byte words per step and threshold at the least, linear in the steps
    one = lib.gd_nbr_ws_bytes(440, 900, 5, 1)
    assert one >= 5 * 441 * 901 * 8 and lib.gd_nbr_ws_bytes(440, 900, 5, 7) == 7 * one
    for bad in ((0, 9, 1, 1), (1025, 1024, 1, 1), (1 << 40, 1 << 40, 1, 1), (9, 9, 0, 1), (9, 9, 9, 1), (9, 9, 1, 0)):
        assert lib.gd_nbr_ws_bytes(*bad) == 0, bad
    for word in ("percentile", "upscaled", "eriodic longitude", "even windows", "2^20"):
        assert word in neighborhood.__doc__, word


def _refused(L, fn, order, good, rules, host, drop=("ws", "ws_bytes")):
    for kw, word in rules:
        v = dict(good, **kw)
        args = [v[k] for k in order if not (host and k in drop)]
        rc = fn(*args) if host else fn(*args, None)
        assert rc == -1, (fn.__name__, kw, rc)
        assert word in L.last_error(), (fn.__name__, kw, L.last_error())


def test_neighborhood_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the cube pointers (never-dereferenced addresses) are not
    touched; the threshold tables and the scales are real host arrays, as the interface has them"""
    L, lib = _lib()
    a, b, c, d, e, g = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    T, K = 3, 2
    thr = np.array([[-0.5, 0.3]] * T)
    nan_thr = thr.copy()
    nan_thr[2, 1] = np.nan
    sc = np.array([1, 3, 9], dtype=np.int32)
    wide = np.arange(1, 2 * 33 + 1, 2, dtype=np.int32)
    thr9 = np.zeros((T, 9))
    ptr = lambda arr: arr.ctypes.data
    cube = [(dict(T=0), "<= 0"), (dict(H=0), "<= 0"), (dict(W=-7), "<= 0"), (dict(H=1025, W=1024), "2^20"), (dict(H=1 << 21, W=1), "2^20"),
            (dict(H=1 << 40, W=1 << 40), "2^20"), (dict(T=2048, H=1024, W=1024), "2^31"), (dict(T=1 << 31, H=1, W=1), "2^31"),
            (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(below=2), "below"), (dict(normalize=2), "normalize"),
            (dict(normalize=-1), "normalize")]
    for host in (False, True):
        sfx = "_host" if host else ""
        order = ("f", "o", "dtype", "T", "H", "W", "mask", "thr_f", "thr_o", "K", "below", "scales", "S", "normalize", "sums", "base", "maps",
                 "ws", "ws_bytes")
        good = dict(f=a, o=b, dtype=1, T=T, H=17, W=65, mask=None, thr_f=ptr(thr), thr_o=ptr(thr), K=K, below=1, scales=ptr(sc), S=3,
                    normalize=0, sums=c, base=d, maps=None, ws=e, ws_bytes=1 << 30)
        rules = [(dict(f=None), "null"), (dict(o=None), "null"), (dict(thr_f=None), "null"), (dict(thr_o=None), "null"),
                 (dict(scales=None), "null"), (dict(sums=None), "null"), (dict(base=None), "null"),
                 (dict(K=0), "K outside"), (dict(K=9, thr_f=ptr(thr9), thr_o=ptr(thr9)), "K outside"), (dict(S=0), "S outside"),
                 (dict(S=33, scales=ptr(wide)), "S outside"), (dict(scales=ptr(np.array([1, 4, 9], dtype=np.int32))), "scale"),
                 (dict(scales=ptr(np.array([1, 3, 0], dtype=np.int32))), "scale"), (dict(scales=ptr(np.array([-3, 3, 5], dtype=np.int32))), "scale"),
                 (dict(thr_f=ptr(nan_thr)), "NaN"), (dict(thr_o=ptr(nan_thr)), "NaN"), (dict(f=a + 4), "aligned"),
                 (dict(o=b + 2, dtype=0), "aligned"), (dict(sums=c + 4), "aligned"), (dict(base=d + 2), "aligned"), (dict(maps=g + 1), "aligned")]
        small = lib.gd_nbr_ws_bytes(17, 65, K, 1) - 1
        dev = [(dict(ws=None), "workspace"), (dict(ws=e + 4), "workspace"), (dict(ws_bytes=small), "workspace"), (dict(ws_bytes=0), "workspace")]
        _refused(L, getattr(lib, "gd_nbr_fss" + sfx), order, good, rules + cube + ([] if host else dev), host)

        order = ("x", "dtype", "T", "H", "W", "mask", "thr", "below", "scale", "normalize", "out", "ws", "ws_bytes")
        one = np.array([-0.5, 0.1, 0.3])
        good = dict(x=a, dtype=1, T=T, H=17, W=65, mask=None, thr=ptr(one), below=1, scale=5, normalize=0, out=c, ws=e, ws_bytes=1 << 30)
        rules = [(dict(x=None), "null"), (dict(thr=None), "null"), (dict(out=None), "null"), (dict(scale=4), "scale"), (dict(scale=0), "scale"),
                 (dict(scale=-1), "scale"), (dict(thr=ptr(np.array([0.0, np.nan, 0.0]))), "NaN"), (dict(x=a + 4), "aligned"),
                 (dict(out=c + 4), "aligned")]
        small = lib.gd_nbr_ws_bytes(17, 65, 1, 1) - 1
        dev = [(dict(ws=None), "workspace"), (dict(ws_bytes=small), "workspace")]
        _refused(L, getattr(lib, "gd_nbr_fraction" + sfx), order, good, rules + cube + ([] if host else dev), host)


def test_the_cases_and_the_oracle_have_their_properties():
    U.check_case_properties()
    U.check_box_forms_agree()


@pytest.mark.parametrize("case,dtype,below", U.TWINS, ids=U.twin_id)
def test_host_twin_against_the_oracle(case, dtype, below):
    from gan_danet_amd import kern as K
    want = U.oracle(case.name, below)
    f, o = case.cubes(dtype)
    sums, base, maps = K.nbr_fss_host(f, o, case.thr_f, case.thr_o, case.scales, below, "window", True, case.mask)
    assert sums.dtype == np.uint64 and np.array_equal(sums, want.sums_w), case
    assert base.dtype == np.uint64 and np.array_equal(base, want.base), case
    assert np.array_equal(maps.astype(np.int64), want.terms_w.sum(axis=0)), case
    vsums, vbase, vmaps = K.nbr_fss_host(f, o, case.thr_f, case.thr_o, case.scales, below, "valid", True, case.mask)
    assert vsums.dtype == np.float64 and np.array_equal(vbase, want.base)
    worst = U.worst_over_bound(vsums, want.sums_v, want.bound_v)
    # a map adds the T terms of a pixel in ascending t: T - 1 roundings of non-negative terms
    T = f.shape[0]
    msum = want.terms_v.sum(axis=0)
    worst_m = U.worst_over_bound(vmaps, msum, 2 * T * U.U64 * msum)
    print(f"{case} {np.dtype(dtype).name} below={below}: integer records exact; valid-mode sums at most {worst:.3f} of the bound, "
          f"maps {worst_m:.3f}")
    assert worst <= 1.0 and worst_m <= 1.0


@pytest.mark.parametrize("normalize", ["window", "valid"])
@pytest.mark.parametrize("case", U.CASES, ids=repr)
def test_host_fraction_field_is_one_exact_division(case, normalize):
    from gan_danet_amd import kern as K
    for dtype in U.DTYPES:
        f, _ = case.cubes(dtype)
        for k, s, below in ((0, 1, True), (case.thr_f.shape[1] - 1, 4, True), (0, 5, False), (0, 0, True)):
            got = K.nbr_fraction_host(f, case.thr_f[:, k], case.scales[s], below, normalize, case.mask)
            assert U.same_bits(got, U.fraction_oracle(case, k, s, below, normalize)), (case, dtype, k, s, below)


def _result(sums, base, scales, thr, normalize="window"):
    from gan_danet_amd import neighborhood as N
    from gan_danet_amd import kern as K
    t = K._nbr_thresholds(thr, sums.shape[0], "thr")
    return N.FSSResult(sums, base, scales, t, t, normalize, None)


def test_closed_forms_on_the_host():
    from gan_danet_amd import kern as K
    # identical fields: FSS = 1 at every scale, in both normalisations
    case = U.BY_NAME["carry"]
    for normalize in ("window", "valid"):
        sums, base, _ = K.nbr_fss_host(case.f, case.f, case.thr_f, case.thr_f, case.scales, True, normalize)
        assert np.all(sums[..., 0] == 0) and np.all(base[..., 0] == base[..., 1]) and np.all(sums[..., 1] > 0)
        assert np.all(_result(sums, base, case.scales, case.thr_f, normalize).fss == 1.0)
    # one event pixel in each field d columns apart: A = 2 n min(d, n), B = C = n^2, so FSS = 1 - min(d, n) / n
    d = 4
    f, o, thr, scales = U.displaced(d)
    sums, base, _ = K.nbr_fss_host(f, o, thr, thr, scales)
    for s, n in enumerate(scales):
        assert sums[0, 0, s].tolist() == [2 * n * min(d, n), n * n, n * n], n
    res = _result(sums, base, scales, thr)
    assert base[0, 0].tolist() == [1, 1, 41 * 61] and np.all(res.fss[0, 0, :2] == 0.0)
    assert np.array_equal(res.fss[0, 0], np.array([1.0 - (2 * n * min(d, n)) / (2 * n * n) for n in scales]))
    assert res.frequency_bias[0] == 1.0 and res.fss_random[0] == 1 / (41 * 61) and res.fss_uniform[0] == 0.5 + 1 / (41 * 61) / 2
    assert res.useful_scale(0) == 9 and np.array_equal(res.pooled, res.fss[0])
    # valid mode, whole-domain window: every centre sees f_f and f_o, so FSS = 2 f_f f_o / (f_f^2 + f_o^2).  35 equal terms
    # go through at most 6 levels of the block sum in the numerator and in the denominator, then one addition, one
    # division and one subtraction: 16 u = 8 ulp of 1 at the most on a ratio <= 1
    case = U.BY_NAME["sub-wave"]
    sums, base, _ = K.nbr_fss_host(case.f, case.o, case.thr_f, case.thr_o, case.scales[-1:], True, "valid")
    res = _result(sums, base, case.scales[-1:], case.thr_f, "valid")
    worst = 0.0
    for t in range(base.shape[0]):
        for k in range(base.shape[1]):
            ff, fo = float(base[t, k, 0]) / float(base[t, k, 2]), float(base[t, k, 1]) / float(base[t, k, 2])
            assert ff > 0 and fo > 0
            worst = max(worst, abs(res.fss[t, k, 0] - 2 * ff * fo / (ff * ff + fo * fo)))
    print(f"valid-mode asymptote: at most {worst / 2.0 ** -52:.2f} ulp of 1 off (bound 8)")
    assert worst <= 8 * 2.0 ** -52
    # an all-invalid step: NaN score, zero base record; the other step is untouched
    f2 = np.stack([np.full((5, 7), np.nan), case.f[1]])
    o2 = np.stack([case.o[0], case.o[1]])
    for normalize in ("window", "valid"):
        sums, base, _ = K.nbr_fss_host(f2, o2, case.thr_f[:2], case.thr_o[:2], case.scales, True, normalize)
        res = _result(sums, base, case.scales, case.thr_f[:2], normalize)
        assert not base[0].any() and not sums[0].any() and np.isnan(res.fss[0]).all() and not np.isnan(res.fss[1]).any()
        assert np.array_equal(res.pooled, res.fss[1])
    sums, base, _ = K.nbr_fss_host(case.f, case.o, case.thr_f, case.thr_o, case.scales, mask=np.zeros((5, 7), dtype=np.uint8))
    assert not base.any() and not sums.any()


def test_cpu_and_bad_arguments_are_refused():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import neighborhood as N
    x = torch.zeros(2, 5, 6, dtype=torch.float64)
    for call in (lambda: N.fractions_skill_score(x, x, (-0.5,), (1, 3)), lambda: N.neighborhood_fraction(x, -0.5, 3),
                 lambda: N.fss_cross_grid(x, x, 1, (-0.5,), (1, 3)), lambda: N.drought_fss(x, x), lambda: N.drought_fss(x.numpy(), x.numpy()),
                 lambda: N.neighborhood_fraction(x.numpy(), -0.5, 3)):
        with pytest.raises(L.GandanetError):
            call()
