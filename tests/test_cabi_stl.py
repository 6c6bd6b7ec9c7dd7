"""CPU: the STL entry points of the C ABI (include/gandanet.h, "STL decomposition") are declared and bound, reject every
bad argument before any launch, and gd_stl_decompose_host -- plain loops over csrc/stl_core.h, the arithmetic the device
kernel shares -- agrees with the independent oracle of tests/stl_util.py and with the closed form (a line plus a zero-mean
periodic term comes back exactly) to 1e-12 max|y| per element.  statsmodels is not involved anywhere: it is not installed.

Largest |host - oracle| over the case list, trend / seasonal / resid: 2.4e-15 (the robust case, max|y| = 15.6; bound
1.6e-11); non-robust cases 8.9e-16 at most.  Largest |host - closed form|: 2.5e-14 at T = 181 (bound 2.5e-12)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stl_util as U

NAMES = ("gd_stl_decompose", "gd_stl_decompose_host")
CASES = U.cases()


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_stl_symbols_are_declared_and_bound():
    from gan_danet_amd import build
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    assert "STL decomposition" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
    assert f"#define GD_STL_MAX_T {L.STL_MAX_T}" in src
    assert "stl.hip" in build.SOURCES


def test_stl_argument_errors_before_any_launch():
    """negative code + gd_last_error with no GPU: validation comes first, so the device pointers (never-dereferenced
    addresses) are not touched"""
    L, lib = _lib()
    x, a, b, c, d = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    good = dict(x=x, dtype=1, T=181, M=7, period=12, seasonal=13, trend=21, low_pass=13, sd=1, td=1, ld=1, ni=5, no=0, a=a, b=b, c=c, d=d)

    def call(fn, host, **kw):
        v = dict(good, **kw)
        args = [v[k] for k in ("x", "dtype", "T", "M", "period", "seasonal", "trend", "low_pass", "sd", "td", "ld", "ni", "no", "a", "b",
                               "c", "d")]
        return fn(*args) if host else fn(*args, None)

    rules = [(dict(x=None), "null"), (dict(a=None), "null"), (dict(b=None), "null"), (dict(c=None), "null"),
             (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(T=0), "<= 0"), (dict(M=0), "<= 0"), (dict(M=-3), "<= 0"),
             (dict(period=1), "period < 2"), (dict(period=0), "period < 2"),
             (dict(seasonal=12), "seasonal"), (dict(seasonal=1), "seasonal"), (dict(seasonal=-3), "seasonal"),
             (dict(trend=20), "trend must be an odd"), (dict(trend=1), "trend must be an odd"),
             (dict(low_pass=14), "low_pass must be an odd"), (dict(low_pass=1), "low_pass must be an odd"),
             (dict(trend=11), "trend must be larger"), (dict(period=21, T=100, low_pass=23), "trend must be larger"),
             (dict(low_pass=11), "low_pass must be larger"), (dict(period=13, low_pass=13), "low_pass must be larger"),
             (dict(sd=2), "degree"), (dict(td=-1), "degree"), (dict(ld=3), "degree"),
             (dict(ni=0), "inner_iter"), (dict(no=-1), "outer_iter"),
             (dict(T=23), "T < 2 * period"), (dict(T=L.STL_MAX_T + 1), "GD_STL_MAX_T"), (dict(T=1 << 40), "GD_STL_MAX_T"),
             (dict(M=1 << 31), "too many"),
             (dict(x=x + 4), "aligned"), (dict(a=a + 4), "aligned"), (dict(b=b + 2), "aligned"), (dict(c=c + 4), "aligned"),
             (dict(d=d + 4), "aligned"), (dict(dtype=0, x=x + 2), "aligned")]
    for host, fn in ((False, lib.gd_stl_decompose), (True, lib.gd_stl_decompose_host)):
        for kw, word in rules:
            rc = call(fn, host, **kw)
            assert rc < 0, (host, kw, rc)
            assert word in L.last_error(), (host, kw, L.last_error())
    # the weights are optional, and the largest T passes the checks of the host entry (which then runs)
    y = np.zeros((L.STL_MAX_T, 1))
    outs = [np.empty_like(y) for _ in range(3)]
    assert lib.gd_stl_decompose_host(y.ctypes.data, 1, L.STL_MAX_T, 1, 12, 13, 21, 13, 1, 1, 1, 1, 0, *[o.ctypes.data for o in outs], None) == 0
    assert all(np.array_equal(o, y) for o in outs)


@pytest.mark.parametrize("period,seasonal,want", [(12, 13, (21, 13)), (7, 7, (15, 9)), (2, 7, (5, 3))])
def test_default_windows(period, seasonal, want):
    from gan_danet_amd import stl
    assert stl.default_windows(period, seasonal) == want
    p = stl.resolve(4 * period, period, seasonal)
    assert (p["trend"], p["low_pass"], p["inner_iter"], p["outer_iter"]) == want + (5, 0)
    p = stl.resolve(4 * period, period, seasonal, robust=True)
    assert (p["inner_iter"], p["outer_iter"]) == (2, 15)
    assert p == U.params(period=period, seasonal=seasonal, robust=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_entry_against_the_oracle_and_the_closed_form(name):
    from gan_danet_amd import kern as K
    from gan_danet_amd import stl
    y, kw, closed = CASES[name]
    p = U.params(**kw)
    assert p == stl.resolve(y.shape[0], **kw) and y.shape[1] <= 5
    U.STATS["not_ok"] = 0
    U._CACHE.clear()
    want = U.oracle(y, **p)
    not_ok = U.STATS["not_ok"]
    got = K.stl_decompose_host(y, p)
    tol = U.TOL * np.abs(y).max()
    err = [float(np.abs(g - w).max()) for g, w in zip(got[:3], want[:3])]
    print(f"{name}: |host - oracle| trend {err[0]:.2e} seasonal {err[1]:.2e} resid {err[2]:.2e} (bound {tol:.2e}), "
          f"{not_ok} est calls not ok")
    assert max(err) <= tol
    assert np.all(np.abs(got[3] - want[3]) <= U.weight_bound(y, want[4]))
    if closed is not None:
        cerr = [float(np.abs(got[i] - closed[i]).max()) for i in range(2)]
        print(f"{name}: |host - closed form| trend {cerr[0]:.2e} seasonal {cerr[1]:.2e}")
        assert max(cerr) <= tol and float(np.abs(got[2]).max()) <= tol
    if p["outer_iter"] == 0:
        assert np.all(got[3] == 1.0)
    if name == "not_ok":
        assert not_ok > 0
    else:
        assert not_ok == 0
    if name == "robust":
        assert np.all(got[3][list(U.OUTLIERS), 1] == 0.0) and np.all(want[3][list(U.OUTLIERS), 1] == 0.0)
        moved = float(np.abs(got[0][:, 1] - got[0][:, 0]).max())
        plain = K.stl_decompose_host(y, U.params())[0]
        assert moved < 0.1 and float(np.abs(plain[:, 1] - plain[:, 0]).max()) > 1.0   # 0.045 against 1.30 without the weights


def test_host_entry_fp32_and_linearity():
    from gan_danet_amd import kern as K
    p = U.params()
    y = U.noisy(181, 12, 2)
    y32 = y.astype(np.float32)
    want = U.oracle(y32.astype(np.float64), **p)
    got = K.stl_decompose_host(y32, p)
    for g, w in zip(got[:3], want[:3]):
        assert g.dtype == np.float32 and np.all(np.abs(g.astype(np.float64) - w.astype(np.float32)) <= U.ulp32(w))
    assert np.all(got[3] == 1.0)
    y1, y2 = U.noisy(181, 12, 2, seed=3), U.noisy(181, 12, 2, seed=4)
    mix, a, b = (K.stl_decompose_host(v, p) for v in (2.5 * y1 - 0.75 * y2, y1, y2))
    tol = U.TOL * np.abs(2.5 * y1 - 0.75 * y2).max()
    for i in range(3):
        assert float(np.abs(mix[i] - (2.5 * a[i] - 0.75 * b[i])).max()) <= tol


def test_cpu_and_bad_tensors_are_refused():
    import gan_danet_amd
    from gan_danet_amd import _lib as L
    from gan_danet_amd import stl
    assert gan_danet_amd.stl is stl and gan_danet_amd.stl_decompose is stl.stl_decompose
    assert gan_danet_amd.detrend_and_compare is stl.detrend_and_compare
    x = torch.zeros(181, 2, 3, dtype=torch.float64)
    for call in (lambda: stl.stl_decompose(x), lambda: stl.detrend_and_compare(x), lambda: stl.stl_decompose(x.numpy())):
        with pytest.raises(L.GandanetError):
            call()
    for kw in (dict(period=1), dict(seasonal=12), dict(trend=20), dict(trend=11), dict(low_pass=12), dict(low_pass=11),
               dict(seasonal_deg=2), dict(inner_iter=0), dict(outer_iter=-1), dict(period=100), dict(seasonal=13.5)):
        with pytest.raises(L.GandanetError):
            stl.resolve(181, **kw)
    with pytest.raises(L.GandanetError):
        stl.resolve(L.STL_MAX_T + 1)
