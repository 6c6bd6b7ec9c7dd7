"""CPU: the ensemble-verification entry points of the C ABI (include/gandanet.h, "Ensemble verification") are declared and
bound, reject every bad argument before any launch, the host twin -- plain C++ over csrc/ensverify_core.h with std::sort --
agrees with the numpy oracle of tests/ensverify_util.py (exactly on ranks and counts, inside the derived bounds elsewhere,
and against exact rationals on the small cases), and gd_ens_verify_merge_host adds records and derives the metrics.  Each
test prints its largest error over its bound (python -m pytest -s)."""
import math
import os

import numpy as np
import pytest

import ensverify_util as U

NAMES = ("gd_ens_verify_ws_bytes", "gd_ens_verify", "gd_ens_verify_host", "gd_ens_verify_merge_host")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import build, kern, verification
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    assert "Ensemble verification" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
    for fn in ("ens_verify", "ens_verify_host", "ens_verify_merge_host"):
        assert hasattr(kern, fn)
    assert f"GD_ENSV_F64 = {L.ENSV_F64}, GD_ENSV_FAIR = {L.ENSV_FAIR}" in src and f"#define GD_ENSV_MAX_M {L.ENSV_MAX_M}" in src
    for k, name in enumerate(L.ENSV_FIELDS):
        assert f"GD_ENSV_{name.upper()} = {k}" in src
    assert f"GD_ENSV_COVER = {L.ENSV_COVER}, GD_ENSV_HIST = {L.ENSV_HIST}, GD_ENSV_BINS = {L.ENSV_BINS}, GD_ENSV_REC = {L.ENSV_REC}" in src
    assert (L.ENSV_COVER, L.ENSV_HIST, L.ENSV_BINS, L.ENSV_REC) == (U.COVER, U.HIST, U.BINS, U.REC)
    for k, name in enumerate(L.ENSV_METRIC_NAMES):
        assert f"GD_ENSV_M_{name.upper()} = {k}" in src
    assert f"GD_ENSV_METRICS = {L.ENSV_METRICS}" in src and L.ENSV_METRICS == L.ENSV_M_HIST + L.ENSV_BINS
    assert "ensverify.hip" in build.SOURCES
    assert gan_danet_amd.verification is verification
    for name in ("EnsembleVerification", "ensemble_scores"):
        assert getattr(gan_danet_amd, name) is getattr(verification, name)
    assert lib.gd_ens_verify_ws_bytes(0) == 0 and lib.gd_ens_verify_ws_bytes(1) == lib.gd_ens_verify_ws_bytes(1 << 30) > 0


def test_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses) are not
    touched"""
    L, lib = _lib()
    a, b, c, d = 0x1000, 0x2000, 0x3000, 0x40000
    order = ("x", "M", "stride", "y", "planes", "hw", "mask", "scale", "flags", "rec", "crps", "err", "spread", "rank")
    good = dict(x=a, M=5, stride=400, y=b, planes=3, hw=128, mask=None, scale=509.7, flags=3, rec=c, crps=None, err=None, spread=None,
                rank=None)
    rules = [(dict(x=None), "null"), (dict(y=None), "null"), (dict(rec=None), "null"), (dict(M=0), "M outside"), (dict(M=33), "M outside"),
             (dict(M=-1), "M outside"), (dict(stride=383), "stride"), (dict(planes=0), "n <= 0"), (dict(hw=-4), "n <= 0"),
             (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"),
             (dict(flags=4), "flag"), (dict(flags=-1), "flag"), (dict(M=1, flags=2), "fair"), (dict(x=a + 4), "aligned"),
             (dict(x=a + 2, flags=0), "aligned"), (dict(y=b + 4), "aligned"), (dict(rec=c + 4), "aligned"), (dict(crps=a + 4), "aligned"),
             (dict(err=a + 2, flags=0), "aligned"), (dict(spread=a + 4), "aligned")]
    ws_bytes = lib.gd_ens_verify_ws_bytes(384)
    for host, fn in ((False, lib.gd_ens_verify), (True, lib.gd_ens_verify_host)):
        for kw, word in rules:
            v = dict(good, **kw)
            args = [v[k] for k in order]
            rc = fn(*args) if host else fn(*args, d, ws_bytes, None)
            assert rc == -1, (fn.__name__, kw, rc)
            assert word in L.last_error(), (fn.__name__, kw, L.last_error())
    args = [good[k] for k in order]
    for tail, word in (((None, ws_bytes, None), "null"), ((d + 4, ws_bytes, None), "aligned"), ((d, ws_bytes - 1, None), "workspace")):
        assert lib.gd_ens_verify(*args, *tail) == -1 and word in L.last_error(), (tail, L.last_error())
    met = (np.zeros(1), np.zeros(L.ENSV_METRICS))
    assert lib.gd_ens_verify_merge_host(None, 1, 5, None, met[1].ctypes.data_as(L.C.POINTER(L.C.c_double))) == -1 and "no pointer" in L.last_error()
    assert lib.gd_ens_verify_merge_host(None, 0, 5, None, None) == -1 and "null" in L.last_error()
    assert lib.gd_ens_verify_merge_host(None, 0, 0, None, met[1].ctypes.data_as(L.C.POINTER(L.C.c_double))) == -1 and "M outside" in L.last_error()
    from gan_danet_amd import kern as K
    with pytest.raises(L.GandanetError):
        K.ens_verify_host(np.zeros((2, 3), np.int32), np.zeros(3))
    with pytest.raises(L.GandanetError):
        K.ens_verify_host(np.zeros((33, 3)), np.zeros(3))
    with pytest.raises(L.GandanetError):
        K.ens_verify_host(np.zeros((2, 6)), np.zeros(6), mask=np.ones(4, np.uint8))
    with pytest.raises(L.GandanetError, match="fair"):
        K.ens_verify_host(np.zeros((1, 6)), np.zeros(6), fair=True)


# the integer kind runs at even M only (ensverify_util.even_m)
CASES = [(kind, U.even_m(M) if kind == "ints" else M, planes, hw) for kind in U.KINDS
         for M, planes, hw in ((1, 1, 65), (2, 2, 63), (3, 3, 64), (7, 1, 257), (8, 2, 65), (9, 1, 63), (31, 1, 64), (32, 2, 257))]


def _host_case(kind, M, planes, hw, dtype, mask=None, scale=1.0, fair=False, nans=False, seed=0, exact=False):
    from gan_danet_amd import kern as K
    x, y = U.make(kind, M, planes, hw, dtype, seed=seed, nans=nans)
    ref = U.oracle(x, y, mask, scale, fair)
    rec, maps = K.ens_verify_host(x, y, mask, scale, fair)
    what = f"{kind} M={M} {planes}x{hw} {np.dtype(dtype).name}"
    worst = U.check_maps(maps, ref, dtype, what)
    worst.update(U.check_rec(rec, ref, what))
    # sum crps_gauss: the host's erf / exp against math.erf / math.exp on the twin's own err and spread in fp64 storage
    if dtype == np.float64:
        worst["gauss"] = U.check_gauss_sum(rec[U.CRPS_GAUSS], maps["err"], maps["spread"], ref["valid"], scale, what)
    if exact and not nans:
        ex = U.crps_exact(x, y, fair)
        got = maps["crps"].reshape(-1).astype(np.float64)
        A_P = (ref["tol"]["crps"] / ((M + 3) * U.U)).reshape(-1)          # (A + P) * scale
        r = max(abs(float(Fraction_of(g) - e * Fraction_of(scale))) / max(w * U.U, 1e-300) for g, e, w in zip(got, ex, A_P)
                if w > 0) if (A_P > 0).any() else 0.0
        assert r <= M + 3, f"{what}: CRPS {r:.3g} u (A + P) from the exact rationals"
        worst["crps_exact_u"] = r
    print(what, {k: f"{v:.3g}" for k, v in worst.items()})
    return rec, maps, ref


def Fraction_of(v):
    from fractions import Fraction
    return Fraction(float(v))


@pytest.mark.parametrize("kind,M,planes,hw", CASES)
def test_host_twin_against_the_oracle(kind, M, planes, hw):
    dtype = np.float64 if kind == "near" or (M + hw) % 2 else np.float32
    _host_case(kind, M, planes, hw, dtype)


@pytest.mark.parametrize("M", [2, 6, 8, 32])
@pytest.mark.parametrize("kind", ["gauss", "ints", "near", "outlier"])
def test_host_twin_against_exact_rationals(kind, M):
    """fp64 storage, so the crps map is the computed value itself"""
    _host_case(kind, M, 1, 200, np.float64, exact=True, fair=(M == 6))


def test_host_twin_nan_mask_scale_fair():
    hw = 257
    mask = (np.random.default_rng(5).random(hw) < 0.7).astype(np.uint8)
    for dtype in (np.float32, np.float64):
        _host_case("gauss", 5, 3, hw, dtype, mask=mask, scale=509.7, fair=True, nans=True)
        _host_case("ints", 4, 2, hw, dtype, mask=mask, scale=509.7, nans=True)
        _host_case("ints", 6, 1, hw, dtype, fair=True)
    rec, maps, ref = _host_case("gauss", 3, 2, 64, np.float32, mask=np.zeros(64, np.uint8))
    assert rec[U.N] == 0 and not rec.any() and np.isnan(maps["crps"]).all() and (maps["rank"] == 255).all()


def test_special_kinds_have_their_exact_values():
    from gan_danet_amd import kern as K
    for M in (1, 2, 3, 7, 32):
        x, y = U.make("identical", M, 1, 130, np.float32)
        rec, maps = K.ens_verify_host(x, y)
        e = x[0].astype(np.float64) - y
        assert np.array_equal(maps["spread"], np.zeros_like(y)) and np.array_equal(maps["err"], e.astype(np.float32))
        assert np.array_equal(maps["crps"], np.abs(e).astype(np.float32))
        assert rec[U.CRPS] == rec[U.CRPS_GAUSS] == rec[U.ABS_E] == np.abs(e).sum()           # eighths: every sum is exact
        assert (rec[U.COVER:U.COVER + 4] == (e == 0).sum()).all() and rec[U.TIED] == (e == 0).sum()
        x, y = U.make("equal_truth", M, 1, 130, np.float32)
        rec, maps = K.ens_verify_host(x, y)
        assert (maps["rank"] == M // 2).all() and rec[U.HIST + M // 2] == 130 and rec[U.TIED] == 130
        assert not rec[U.CRPS:U.S2 + 1].any() and (rec[U.COVER:U.COVER + 4] == 130).all()
        assert not maps["crps"].any() and not maps["err"].any() and not maps["spread"].any()


def test_merge_host():
    from gan_danet_amd import kern as K
    L, _ = _lib()
    M = 5
    x, y = U.make("gauss", M, 6, 257, np.float64, seed=1, nans=True)
    ref = U.oracle(x, y)
    whole, _ = K.ens_verify_host(x, y, maps=False)
    zero = np.zeros(U.REC)
    merged, met = K.ens_verify_merge_host([zero, whole, zero], M)
    assert np.array_equal(merged, whole)
    for cuts in ((0, 2, 6), (0, 1, 4, 6)):
        parts = [K.ens_verify_host(x[:, a:b], y[a:b], maps=False)[0] for a, b in zip(cuts[:-1], cuts[1:])]
        got, _ = K.ens_verify_merge_host(parts, M)
        U.check_rec(np.asarray(got), ref, f"cut {cuts}")
        for f in (U.CRPS, U.ABS_E, U.E2, U.S2):
            assert abs(got[f] - whole[f]) <= 2 * ref["rec_tol"][f]
    want = U.metrics_np(np.asarray(merged), M)
    for k in ("crps", "crps_gauss", "mae", "rmse", "spread", "spread_skill", "reliability", "tied"):
        assert math.isclose(met[k], want[k], rel_tol=4 * U.U, abs_tol=0.0), k
    assert np.allclose(list(met["coverage"].values()), want["coverage"], rtol=4 * U.U, atol=0)
    assert tuple(met["coverage"]) == L.ENSV_LEVELS and len(met["rank_hist"]) == M + 1
    assert np.allclose(met["rank_hist"], want["rank_hist"], rtol=4 * U.U, atol=0) and abs(sum(met["rank_hist"]) - 1) < 1e-12
    assert met["n"] == ref["n"] and met["rank_counts"] == list(ref["rec"][U.HIST:U.HIST + M + 1])
    for recs in ([], [zero]):
        _, empty = K.ens_verify_merge_host(recs, M)
        assert empty["n"] == 0 and all(math.isnan(empty[k]) for k in L.ENSV_METRIC_NAMES + ("reliability", "tied"))
        assert all(math.isnan(v) for v in empty["rank_hist"]) and all(math.isnan(v) for v in empty["coverage"].values())
    one = K.ens_verify_merge_host([K.ens_verify_host(x[:1], y, maps=False)[0]], 1)[1]
    assert math.isnan(one["spread_skill"]) and one["spread"] == 0.0 and one["crps"] == one["mae"]
