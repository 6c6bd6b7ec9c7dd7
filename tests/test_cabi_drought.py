"""CPU: the drought entry points of the C ABI (include/gandanet.h, "Drought analysis") are declared, bound and
re-exported, reject every bad argument before any launch, and the host twins -- plain C++ over csrc/drought_core.h -- hold
the bounds of tests/drought_util.py against its independent oracles (exact rationals, longdouble, scipy's rankdata,
itertools.groupby) over every shape of the GPU test.  The properties the test data must have (an event, a run that fails
min_duration, a tie) are asserted here on the oracle's own output.  Each test prints its largest error over its bound
(python -m pytest -s)."""
import os

import numpy as np
import pytest
import torch

import drought_util as U

NAMES = ("gd_drought_clim", "gd_drought_index", "gd_drought_rank", "gd_drought_events", "gd_drought_exceed")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_drought_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import build, drought, kern
    L, lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gandanet.h")).read()
    assert "Drought analysis (drought.hip, csrc/drought_core.h)" in src
    for name in NAMES:
        for nm in (name, name + "_host"):
            assert nm + "(" in src and nm in L.SIGNATURES and hasattr(lib, nm), nm
            assert hasattr(kern, nm[3:]), nm
    assert f"#define GD_DROUGHT_MAX_T {L.DROUGHT_MAX_T}" in src and L.DROUGHT_MAX_T == 2048
    assert f"#define GD_DROUGHT_MAX_PERIOD {L.DROUGHT_MAX_PERIOD}" in src and L.DROUGHT_MAX_PERIOD == 366
    assert f"#define GD_DROUGHT_MAX_N {L.DROUGHT_MAX_N}" in src and L.DROUGHT_MAX_N == 257
    assert f"GD_DROUGHT_ANOMALY = {L.DROUGHT_ANOMALY}, GD_DROUGHT_STANDARDIZED = {L.DROUGHT_STANDARDIZED}" in src
    for k, name in enumerate(L.DROUGHT_EV_MAPS):
        assert f"GD_DROUGHT_EV_{name.upper()} = {k}" in src
    assert f"GD_DROUGHT_EV_MAPS = {len(L.DROUGHT_EV_MAPS)}" in src and L.DROUGHT_EV_MAPS == U.EV_MAPS == drought.MAPS
    assert "drought.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "drought_core.h"))
    assert gan_danet_amd.drought is drought
    for name in ("DroughtClimatology", "DroughtEvents", "climatology", "drought_index", "drought_events", "drought_area", "DSI_CLASSES",
                 "compare_events"):
        assert getattr(gan_danet_amd, name) is getattr(drought, name)
    assert drought.DSI_CLASSES == (-0.5, -0.8, -1.3, -1.6, -2.0)


def _refused(L, fn, order, good, rules, host, tail=(None,)):
    for kw, word in rules:
        v = dict(good, **kw)
        args = [v[k] for k in order]
        rc = fn(*args) if host else fn(*args, *tail)
        assert rc == -1, (fn.__name__, kw, rc)
        assert word in L.last_error(), (fn.__name__, kw, L.last_error())


def test_drought_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses) are not
    touched"""
    L, lib = _lib()
    a, b, c = 0x1000, 0x2000, 0x3000
    cube = [(dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(T=0), "T outside"), (dict(T=-4), "T outside"),
            (dict(T=2049), "T outside"), (dict(M=0), "M <= 0"), (dict(M=-3), "M <= 0"), (dict(M=1 << 31), "too many"),
            (dict(x=a + 4), "aligned"), (dict(x=a + 2, dtype=0), "aligned")]
    calendar = [(dict(period=0), "period"), (dict(period=367), "period"), (dict(period=-12), "period"), (dict(phase=-1), "phase"),
                (dict(phase=12), "phase")]
    baseline = [(dict(b0=5, b1=5), "baseline"), (dict(b0=9, b1=4), "baseline"), (dict(b0=-1), "baseline"), (dict(b1=182), "baseline")]
    for host in (False, True):
        sfx = "_host" if host else ""
        order = ("x", "dtype", "T", "M", "period", "phase", "b0", "b1", "mask", "clim")
        good = dict(x=a, dtype=1, T=181, M=7, period=12, phase=0, b0=0, b1=181, mask=None, clim=b)
        rules = [(dict(x=None), "null"), (dict(clim=None), "null"), (dict(clim=b + 4), "aligned")] + cube + calendar + baseline
        _refused(L, getattr(lib, "gd_drought_clim" + sfx), order, good, rules, host)

        order = ("x", "dtype", "T", "M", "clim", "period", "phase", "kind", "ddof", "mask", "out")
        good = dict(x=a, dtype=1, T=181, M=7, clim=b, period=12, phase=0, kind=1, ddof=0, mask=None, out=c)
        rules = [(dict(x=None), "null"), (dict(clim=None), "null"), (dict(out=None), "null"), (dict(kind=2), "kind"), (dict(kind=-1), "kind"),
                 (dict(ddof=2), "ddof"), (dict(ddof=-1), "ddof"), (dict(clim=b + 4), "aligned"), (dict(out=c + 4), "aligned")]
        _refused(L, getattr(lib, "gd_drought_index" + sfx), order, good, rules + cube + calendar, host)

        order = ("x", "dtype", "T", "M", "period", "phase", "b0", "b1", "mask", "table", "nmax", "out")
        good = dict(x=a, dtype=1, T=181, M=7, period=12, phase=0, b0=0, b1=181, mask=None, table=b, nmax=17, out=c)
        rules = [(dict(x=None), "null"), (dict(table=None), "null"), (dict(out=None), "null"), (dict(nmax=0), "nmax outside"),
                 (dict(nmax=258), "nmax outside"), (dict(nmax=16), "too small"), (dict(period=1, T=2048, b1=2048, nmax=257), "too small"),
                 (dict(table=b + 4), "aligned"), (dict(out=c + 4), "aligned")]
        _refused(L, getattr(lib, "gd_drought_rank" + sfx), order, good, rules + cube + calendar + baseline, host)

        order = ("x", "dtype", "T", "M", "threshold", "min_duration", "which", "mask", "maps", "in_event")
        good = dict(x=a, dtype=1, T=181, M=7, threshold=-0.8, min_duration=3, which=0xFFF, mask=None, maps=b, in_event=None)
        rules = [(dict(x=None), "null"), (dict(maps=None), "null"), (dict(threshold=float("nan")), "threshold"),
                 (dict(min_duration=0), "min_duration"), (dict(min_duration=-2), "min_duration"), (dict(which=0), "no map"),
                 (dict(which=1 << 12), "no map"), (dict(which=-1), "no map"), (dict(maps=b + 4), "aligned")]
        _refused(L, getattr(lib, "gd_drought_events" + sfx), order, good, rules + cube, host)

        order = ("x", "dtype", "n", "threshold", "out")
        good = dict(x=a, dtype=1, n=100, threshold=-0.8, out=c)
        rules = [(dict(x=None), "null"), (dict(out=None), "null"), (dict(dtype=2), "dtype"), (dict(n=0), "n <= 0"), (dict(n=-1), "n <= 0"),
                 (dict(threshold=float("nan")), "threshold"), (dict(x=a + 4), "aligned"), (dict(out=c + 2, dtype=0), "aligned")]
        _refused(L, getattr(lib, "gd_drought_exceed" + sfx), order, good, rules, host)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", U.CASES, ids=lambda c: f"T{c[0]}-p{c[1]}")
def test_host_twins_against_the_oracles(case, dtype):
    """every M of the GPU test: a column's bits do not depend on M; the oracle's columns of the widest cube hold every
    bound, with and without a mask"""
    from gan_danet_amd import drought as D
    from gan_danet_amd import kern as K
    T, period, phase, baseline = case
    b0, b1 = (0, T) if baseline is None else baseline
    nmax = U.nmax_of(T, period, baseline)
    tables = {kind: D.rank_table(kind, nmax) for kind in ("percentile", "empirical")}
    for kind in tables:
        assert np.array_equal(tables[kind], U.table_oracle(kind, nmax))
    wide = {}
    for M in reversed(U.MS):
        x = U.series(T, M, dtype)
        got = {"clim": K.drought_clim_host(x, period, phase, b0, b1)}
        for kind, code in (("anomaly", 0), ("standardized", 1)):
            for ddof in (0, 1):
                got[kind, ddof] = K.drought_index_host(x, got["clim"], phase, code, ddof)
        for kind in tables:
            got[kind] = K.drought_rank_host(x, tables[kind], period, phase, b0, b1)
        for md in U.durations(T):
            got["events", md] = K.drought_events_host(x, U.THRESHOLD, md, want_steps=True)
        got["exceed"] = K.drought_exceed_host(x, U.THRESHOLD)
        if not wide:
            wide = got
            continue
        for key, val in got.items():
            if key[0] == "events":
                assert all(np.array_equal(val[0][nm], wide[key][0][nm][:M], equal_nan=True) for nm in U.EV_MAPS), (key, M)
                assert np.array_equal(val[1], wide[key][1][:, :M]), (key, M)
            else:
                assert np.array_equal(val, wide[key][..., :M], equal_nan=True), (key, M)
    M = U.M_MAX
    x = U.series(T, M, dtype)
    cols = U.oracle_columns(M)
    wm, wm2 = U.check_clim(wide["clim"], cols, U.clim_oracle(dtype, T, period, phase, baseline, cols))
    wi = max(U.check_index(wide[kind, ddof], dtype, T, period, phase, baseline, kind, ddof, cols)
             for kind in ("anomaly", "standardized") for ddof in (0, 1))
    ties = 0
    for kind in tables:
        want, ties = U.rank_want(dtype, T, period, phase, baseline, tables[kind], cols)
        for c in cols:
            assert np.array_equal(wide[kind][:, c], want[c], equal_nan=True), (kind, c)
    # a tie needs two samples in one slot's comparison set
    if nmax > 2:
        assert ties > 0
    else:
        assert max(len(s) for s in U.slot_steps(T, period, phase, b0, b1)) == 1
    n_events = n_fail = 0
    ws = 0.0
    everything = range(M)
    for md in U.durations(T):
        maps, steps = wide["events", md]
        ne, nf, w = U.check_events(maps, steps, x, U.THRESHOLD, md, everything)
        n_events, n_fail, ws = n_events + ne, n_fail + nf, max(ws, w)
        if T >= 3 and md == 3:
            assert ne > 0 and nf > 0                     # the default duration alone meets both
    assert n_events > 0 and n_fail > 0
    assert np.any(x == U.THRESHOLD)                      # samples exactly on the threshold
    assert np.array_equal(wide["exceed"], U.exceed_oracle(x, U.THRESHOLD), equal_nan=True)
    # the constant series has no variance: anomaly 0, standardized NaN; the empty one is NaN everywhere
    assert np.all(wide["anomaly", 0][:, 4] == 0) and np.isnan(wide["standardized", 0][:, 4]).all()
    assert all(np.isnan(wide[k][:, 3]).all() for k in (("anomaly", 0), ("standardized", 1), "percentile", "empirical"))
    # with a mask
    mask = U.mask_of(M)
    off = set(np.flatnonzero(mask == 0))
    mc = sorted(set(cols) | off)
    rec = K.drought_clim_host(x, period, phase, b0, b1, mask)
    U.check_clim(rec, mc, U.clim_oracle(dtype, T, period, phase, baseline, mc), off)
    keep = mask != 0
    assert np.array_equal(rec[:, :, keep], wide["clim"][:, :, keep], equal_nan=True)
    for kind, code in (("anomaly", 0), ("standardized", 1)):
        z = K.drought_index_host(x, wide["clim"], phase, code, 0, mask)                 # the mask of the index itself
        z2 = K.drought_index_host(x, rec, phase, code, 0)                               # a masked climatology
        assert np.array_equal(z, z2, equal_nan=True) and np.isnan(z[:, ~keep]).all()
        assert np.array_equal(z[:, keep], wide[kind, 0][:, keep], equal_nan=True)
    r = K.drought_rank_host(x, tables["empirical"], period, phase, b0, b1, mask)
    assert np.isnan(r[:, ~keep]).all() and np.array_equal(r[:, keep], wide["empirical"][:, keep], equal_nan=True)
    maps, steps = K.drought_events_host(x, U.THRESHOLD, 3, mask=mask, want_steps=True)
    U.check_events(maps, steps, x, U.THRESHOLD, 3, mc, off)
    print(f"T = {T} period {period} {np.dtype(dtype).name}: mean at most {wm:.3f} of its bound, M2 {wm2:.3f}, index {wi:.3f}, "
          f"severity {ws:.3f}; ranks, counts, starts and steps exact; {n_events} events, {n_fail} short runs, {ties} tied samples")


def test_events_on_an_index_that_is_not_quantised():
    """run theory on the standardised index itself at the D1 threshold -0.8: severities are rounded sums here"""
    from gan_danet_amd import kern as K
    T, M = 181, 257
    x = U.series(T, M)
    z = K.drought_index_host(x, K.drought_clim_host(x), 0, 1, 0)
    maps, steps = K.drought_events_host(z, -0.8, 3, want_steps=True)
    ne, nf, w = U.check_events(maps, steps, z, -0.8, 3, range(M))
    assert ne > 0 and nf > 0
    some, _ = K.drought_events_host(z, -0.8, 3, maps=("peak", "n_events"))
    assert list(some) == ["n_events", "peak"] and np.array_equal(some["peak"], maps["peak"], equal_nan=True)
    print(f"{ne} events, {nf} short runs: severities at most {w:.3f} of the bound")


def test_cpu_and_bad_arguments_are_refused():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import drought as D
    x = torch.zeros(24, 4, 6, dtype=torch.float64)
    e = torch.zeros(24, 4, 6, dtype=torch.uint8)
    for call in (lambda: D.climatology(x), lambda: D.drought_index(x), lambda: D.drought_index(x, "empirical"), lambda: D.drought_events(x),
                 lambda: D.drought_area(x), lambda: D.compare_events(e, e), lambda: D.climatology(x.numpy()),
                 lambda: D.rank_table("gringorten", 4), lambda: D.rank_table("percentile", 258), lambda: D.rank_table("percentile", 0)):
        with pytest.raises(L.GandanetError):
            call()
    t = D.rank_table("percentile", 3)
    assert t[0] == (1 - 0.44) / 1.12 and t[(3 - 1) ** 2 + 4] == (3 - 0.44) / 3.12 and D.rank_table("empirical", 1)[0] == 0.0


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_host_twin_launcher_edges(M):
    """the host side of the per-item launcher, T = 5, period 2: every host twin writes through the C entry into the middle of
    a buffer of sentinels, leaves the sentinels alone, and a column's bits are those of the 257-series cube (the device
    side of the same sizes: tests/test_gpu_drought.py::test_launcher_edges)"""
    from gan_danet_amd import drought as D
    from gan_danet_amd import kern as K
    L, lib = _lib()
    T, period, pad = 5, 2, 64
    nmax = U.nmax_of(T, period, None)
    table = np.ascontiguousarray(D.rank_table("empirical", nmax)).reshape(-1)

    def guarded(n, dtype):
        return np.full(n + 2 * pad, 7, dtype=dtype)

    def middle(buf, n, shape):
        assert np.all(buf[:pad] == 7) and np.all(buf[pad + n:] == 7), "written outside the output"
        return buf[pad:pad + n].reshape(shape)

    for dtype in (np.float64, np.float32):
        wide, x = U.series(T, 257, dtype), U.series(T, M, dtype)
        dt, ptr = int(dtype == np.float64), lambda b: b[pad:].ctypes.data
        cb = guarded(3 * period * M, np.float64)
        L.check(lib.gd_drought_clim_host(x.ctypes.data, dt, T, M, period, 0, 0, T, None, ptr(cb)), "gd_drought_clim_host")
        clim = middle(cb, 3 * period * M, (3, period, M))
        assert np.array_equal(clim, K.drought_clim_host(wide, period)[..., :M], equal_nan=True)
        ib, rb, xb = guarded(T * M, dtype), guarded(T * M, dtype), guarded(T * M, dtype)
        L.check(lib.gd_drought_index_host(x.ctypes.data, dt, T, M, clim.ctypes.data, period, 0, 1, 0, None, ptr(ib)), "gd_drought_index_host")
        L.check(lib.gd_drought_rank_host(x.ctypes.data, dt, T, M, period, 0, 0, T, None, table.ctypes.data, nmax, ptr(rb)),
                "gd_drought_rank_host")
        L.check(lib.gd_drought_exceed_host(x.ctypes.data, dt, T * M, U.THRESHOLD, ptr(xb)), "gd_drought_exceed_host")
        wclim = K.drought_clim_host(wide, period)
        assert np.array_equal(middle(ib, T * M, (T, M)), K.drought_index_host(wide, wclim)[:, :M], equal_nan=True)
        assert np.array_equal(middle(rb, T * M, (T, M)), K.drought_rank_host(wide, table, period)[:, :M], equal_nan=True)
        assert np.array_equal(middle(xb, T * M, (T, M)), K.drought_exceed_host(wide, U.THRESHOLD)[:, :M], equal_nan=True)
        mb, sb = guarded(len(U.EV_MAPS) * M, np.float64), guarded(T * M, np.uint8)
        which = K.drought_which(U.EV_MAPS)
        L.check(lib.gd_drought_events_host(x.ctypes.data, dt, T, M, U.THRESHOLD, 2, which, None, ptr(mb), ptr(sb)), "gd_drought_events_host")
        maps, steps = K.drought_events_host(wide, U.THRESHOLD, 2, want_steps=True)
        got = middle(mb, len(U.EV_MAPS) * M, (len(U.EV_MAPS), M))
        assert all(np.array_equal(got[k], maps[nm][:M], equal_nan=True) for k, nm in enumerate(U.EV_MAPS))
        assert np.array_equal(middle(sb, T * M, (T, M)), steps[:, :M])
