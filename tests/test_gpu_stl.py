"""GPU: the device STL (gan_danet_amd/stl.py, csrc/stl.hip) against the independent fp64 oracle of tests/stl_util.py, the
closed form (a line plus a zero-mean periodic term comes back exactly) and the host entry gd_stl_decompose_host, to
1e-12 max|y| per element (fp32 tensors: one fp32 ulp of the oracle's result rounded to fp32).  The oracle takes 0.04 s per
series of 181 samples, so the M = 67 and M = 300 runs are compared with it on the columns around the workgroup boundaries
and at both ends, and with the host entry -- itself held to the oracle on the CPU -- on every column.  statsmodels is not
involved anywhere: it is not installed, and nothing here claims agreement with a run of it.

Largest errors observed on an MI355X (each test prints its own, python -m pytest -s): the device equals the host entry
bit for bit in every case, T = 2048 included; |device - oracle| 8.9e-16 at T = 181 defaults (bound 4.4e-12 to 6.0e-12),
at most 4.4e-16 on the short series, 2.4e-15 robust (bound 1.6e-11; weights 8.2e-15), 1.8e-15 on the not-ok case
(weights 1.3e-14); |device - closed form| 2.5e-14 at T = 181 (bound 2.5e-12); linearity defect 5.1e-15; fp32 0 ulp."""
import numpy as np
import pytest
import torch

import stl_util as U

pytestmark = pytest.mark.gpu

CASES = U.cases()
BIG = U.noisy(181, 12, 300, seed=5)
# S = 4 series per workgroup at T = 181: columns around the first and last group boundaries, and both ends
ORACLE_COLUMNS = {1: [0], 5: [0, 1, 2, 3, 4], 67: [0, 3, 4, 5, 63, 64, 66], 300: [0, 4, 151, 296, 299]}


def _dev(y, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(y)).to(device="cuda", dtype=dtype)


def _run(y, **kw):
    from gan_danet_amd import stl
    r = stl.stl_decompose(_dev(y), **kw)
    return [t.cpu().numpy() for t in r]


def _errs(got, want):
    return [float(np.abs(g - w).max()) for g, w in zip(got[:3], want[:3])]


@pytest.fixture(scope="module")
def big_runs():
    """the default decomposition of the first M columns of BIG, M = 1, 5, 67, 300 (the last as a (181, 3, 100) tensor)"""
    out = {}
    for m in (1, 5, 67, 300):
        y = BIG[:, :m]
        got = _run(y.reshape(181, 3, 100) if m == 300 else y)
        assert all(g.shape == ((181, 3, 100) if m == 300 else (181, m)) and g.dtype == np.float64 for g in got)
        out[m] = [g.reshape(181, m) for g in got]
    return out


@pytest.mark.parametrize("m", [1, 5, 67, 300])
def test_defaults_at_t181(big_runs, m):
    """fewer series than a workgroup holds, a ragged last group, several workgroups; 181 = 15 * 12 + 1, so the
    cycle-subseries have two lengths"""
    from gan_danet_amd import kern as K
    p = U.params()
    y, got = BIG[:, :m], big_runs[m]
    tol = U.TOL * np.abs(y).max()
    host = K.stl_decompose_host(y, p)
    cols = ORACLE_COLUMNS[m]
    want = U.oracle(y, cols, **p)
    eh, eo = _errs(got, host), _errs([g[:, cols] for g in got], want)
    print(f"M = {m}: |device - host| {max(eh):.2e} over {m} series, |device - oracle| {max(eo):.2e} over {len(cols)} (bound {tol:.2e})")
    assert max(eh) <= tol and max(eo) <= tol
    assert np.all(got[3] == 1.0)


def test_a_series_does_not_depend_on_its_neighbours(big_runs):
    for m in (1, 5, 67):
        for a, b in zip(big_runs[m], big_runs[300]):
            assert np.array_equal(a, b[:, :m]), m                   # bit for bit, whatever the column's place in its group
    again = _run(BIG.reshape(181, 3, 100))
    for a, b in zip(again, big_runs[300]):
        assert np.array_equal(a.reshape(181, 300), b)
    # the last column alone (first of its group) against its place at the end of a ragged group
    alone = _run(BIG[:, 66:67])
    for a, b in zip(alone, big_runs[67]):
        assert np.array_equal(a[:, 0], b[:, 66])


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_list(name):
    from gan_danet_amd import kern as K
    y, kw, closed = CASES[name]
    p = U.params(**kw)
    U.STATS["not_ok"] = 0
    U._CACHE.clear()
    want = U.oracle(y, **p)
    not_ok = U.STATS["not_ok"]
    got = _run(y, **kw)
    host = K.stl_decompose_host(y, p)
    tol = U.TOL * np.abs(y).max()
    eo, eh = _errs(got, want), _errs(got, host)
    ew = float(np.abs(got[3] - want[3]).max())
    print(f"{name}: |device - oracle| {max(eo):.2e}, |device - host| {max(eh):.2e} (bound {tol:.2e}); weights {ew:.2e}; "
          f"{not_ok} est calls not ok")
    assert max(eo) <= tol and max(eh) <= tol
    assert np.all(np.abs(got[3] - want[3]) <= U.weight_bound(y, want[4]))
    if closed is not None:
        ec = [float(np.abs(got[i] - closed[i]).max()) for i in range(2)]
        print(f"{name}: |device - closed form| trend {ec[0]:.2e} seasonal {ec[1]:.2e}")
        assert max(ec) <= tol and float(np.abs(got[2]).max()) <= tol
    assert (not_ok > 0) == (name == "not_ok")
    if name == "robust":
        # three outliers of +15 move the plain trend by 1.30 and the robust trend by 0.045
        assert np.all(got[3][list(U.OUTLIERS), 1] == 0.0)
        plain = _run(y)[0]
        moved, moved_plain = float(np.abs(got[0][:, 1] - got[0][:, 0]).max()), float(np.abs(plain[:, 1] - plain[:, 0]).max())
        print(f"robust: the outliers move the trend by {moved:.3f}, {moved_plain:.3f} without the weights")
        assert moved < 0.1 and moved_plain > 1.0


def test_fp32_at_t181():
    from gan_danet_amd import kern as K
    from gan_danet_amd import stl
    y32 = BIG[:, :67].astype(np.float32)
    r = stl.stl_decompose(_dev(y32, torch.float32))
    got = [t.cpu().numpy() for t in r]
    assert all(g.dtype == np.float32 and g.shape == (181, 67) for g in got)
    cols = ORACLE_COLUMNS[67]
    want = U.oracle(y32.astype(np.float64), cols, **U.params())
    host = K.stl_decompose_host(y32, U.params())
    worst = 0.0
    for g, w, h in zip(got[:3], want[:3], host[:3]):
        d = np.abs(g[:, cols].astype(np.float64) - w.astype(np.float32).astype(np.float64)) / U.ulp32(w)
        worst = max(worst, float(d.max()))
        assert np.all(d <= 1.0)
        assert np.all(np.abs(g.astype(np.float64) - h.astype(np.float64)) <= U.ulp32(h))
    print(f"fp32: at most {worst:.2f} ulp from the oracle's result rounded to fp32")
    assert np.all(got[3] == 1.0)


def test_longest_series_against_the_host_entry():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import kern as K
    from gan_danet_amd import stl
    t_len = L.STL_MAX_T
    y = U.noisy(t_len, 12, 3, seed=7)
    got = _run(y)
    host = K.stl_decompose_host(y, U.params())
    tol = U.TOL * np.abs(y).max()
    eh = _errs(got, host)
    print(f"T = {t_len}: |device - host| {max(eh):.2e} (bound {tol:.2e})")
    assert max(eh) <= tol
    with pytest.raises(L.GandanetError):
        stl.stl_decompose(torch.zeros(t_len + 1, 2, device="cuda", dtype=torch.float64))


def test_detrend_and_compare():
    from gan_danet_amd import stl
    data = _dev(U.noisy(181, 12, 24, seed=9).reshape(181, 4, 6))
    trend, detrended, reconstructed, max_difference = stl.detrend_and_compare(data)
    assert trend.shape == data.shape and trend.dtype == data.dtype and isinstance(max_difference, float)
    assert torch.equal(detrended, data - trend) and torch.equal(detrended + trend, reconstructed)
    assert max_difference == float(np.max(np.abs(data.cpu().numpy() - reconstructed.cpu().numpy())))
    assert torch.equal(trend, stl.stl_decompose(data).trend)


def test_linearity():
    y1, y2 = U.noisy(181, 12, 5, seed=3), U.noisy(181, 12, 5, seed=4)
    mix, a, b = (_run(v) for v in (2.5 * y1 - 0.75 * y2, y1, y2))
    tol = U.TOL * np.abs(2.5 * y1 - 0.75 * y2).max()
    defect = [float(np.abs(mix[i] - (2.5 * a[i] - 0.75 * b[i])).max()) for i in range(3)]
    print(f"linearity defect {max(defect):.2e} (bound {tol:.2e})")
    assert max(defect) <= tol


def test_bad_tensors_raise():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import stl
    for bad in (torch.zeros(181, 3, dtype=torch.float64), torch.zeros(181, 3, device="cuda", dtype=torch.int32),
                torch.zeros(23, 3, device="cuda", dtype=torch.float64), torch.zeros(181, 0, device="cuda")):
        with pytest.raises(L.GandanetError):
            stl.stl_decompose(bad)
    y = _dev(BIG[:, :2])
    t1 = stl.stl_decompose(y[:, 0]).trend                               # a (T,) view, not contiguous
    assert t1.shape == (181,) and torch.equal(t1, stl.stl_decompose(y).trend[:, 0])
