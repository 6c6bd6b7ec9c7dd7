"""GPU: the drought module (gan_danet_amd/drought.py, csrc/drought.hip) against the host twins bit for bit -- climatology,
both parametric indices, both rank indices, every event map, in_event and the indicator: they share csrc/drought_core.h --
and against the independent oracles of tests/drought_util.py within its derived bounds on the oracle's columns (the host
twins are held to them on every column on the CPU, tests/test_cabi_drought.py).  M lies on both sides of a wave, of the
workgroup and of the vector width; a column's bits do not depend on M nor on the alignment of the input; sentinels around
every output show that nothing is written outside it.  Each test prints its largest error over its bound
(python -m pytest -s).

Largest figures observed on an MI355X, as fractions of the bounds of tests/drought_util.py: mean 0.056, M2 0.045, fp64
indices 0.099, fp32 indices 0.994 (the rounding to fp32 is the bound's largest term), severities 0 (the quantised data sums
exactly), weighted area fractions 0.123.  The device equalled the host twin bit for bit in every case."""
import math

import numpy as np
import pytest
import torch

import drought_util as U

pytestmark = pytest.mark.gpu

PAD = 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _off(a):
    """a copy of ``a`` on the device whose first element lies one element past a 16-byte boundary"""
    buf = torch.empty(a.size + 1, device="cuda", dtype=torch.from_numpy(a[:0].reshape(-1)).dtype)
    v = buf[1:].view(a.shape)
    v.copy_(_dev(a))
    assert v.data_ptr() % 16 == a.itemsize
    return v


class Guarded:
    """an output of ``shape`` in the middle of a buffer of sentinels"""

    def __init__(self, shape, dtype):
        self.n = math.prod(shape)
        self.fill = 7 if dtype == torch.uint8 else -7.0
        self.buf = torch.full((self.n + 2 * PAD,), self.fill, device="cuda", dtype=dtype)
        self.out = self.buf[PAD:PAD + self.n].view(shape)

    def get(self):
        host = self.buf.cpu().numpy()
        assert np.all(host[:PAD] == self.fill) and np.all(host[PAD + self.n:] == self.fill), "written outside the output"
        return host[PAD:PAD + self.n].reshape(tuple(self.out.shape))


def _device(x, xd, case, tables, mask=None, durations=None):
    """every entry point on the device cube ``xd`` into guarded outputs: the dict of test_cabi_drought's host loop"""
    from gan_danet_amd import kern as K
    T, period, phase, baseline = case
    b0, b1 = (0, T) if baseline is None else baseline
    M = x.shape[1]
    td = xd.dtype
    md = None if mask is None else _dev(mask)
    got = {}
    g = Guarded((3, period, M), torch.float64)
    clim = K.drought_clim(xd, period, phase, b0, b1, md, out=g.out)
    got["clim"] = g.get()
    for kind, code in (("anomaly", 0), ("standardized", 1)):
        for ddof in (0, 1):
            g = Guarded((T, M), td)
            K.drought_index(xd, clim, phase, code, ddof, md, out=g.out)
            got[kind, ddof] = g.get()
    for kind, table in tables.items():
        g = Guarded((T, M), td)
        K.drought_rank(xd, _dev(table.copy()), period, phase, b0, b1, md, out=g.out)
        got[kind] = g.get()
    for d in durations or U.durations(T):
        g, s = Guarded((len(U.EV_MAPS), M), torch.float64), Guarded((T, M), torch.uint8)
        K.drought_events(xd, U.THRESHOLD, d, mask=md, out=g.out, in_event=s.out)
        got["events", d] = (dict(zip(U.EV_MAPS, g.get())), s.get())
    g = Guarded((T, M), td)
    K.drought_exceed(xd, U.THRESHOLD, out=g.out)
    got["exceed"] = g.get()
    return got


def _host(x, case, tables, mask=None, durations=None):
    from gan_danet_amd import kern as K
    T, period, phase, baseline = case
    b0, b1 = (0, T) if baseline is None else baseline
    got = {"clim": K.drought_clim_host(x, period, phase, b0, b1, mask)}
    for kind, code in (("anomaly", 0), ("standardized", 1)):
        for ddof in (0, 1):
            got[kind, ddof] = K.drought_index_host(x, got["clim"], phase, code, ddof, mask)
    for kind, table in tables.items():
        got[kind] = K.drought_rank_host(x, table, period, phase, b0, b1, mask)
    for d in durations or U.durations(T):
        got["events", d] = K.drought_events_host(x, U.THRESHOLD, d, mask=mask, want_steps=True)
    got["exceed"] = K.drought_exceed_host(x, U.THRESHOLD)
    return got


def _same(a, b, where, cut=None):
    assert a.keys() == b.keys()
    for key, val in a.items():
        ref = b[key]
        if key[0] == "events":
            for nm in U.EV_MAPS:
                assert np.array_equal(val[0][nm], ref[0][nm][:cut], equal_nan=True), (where, key, nm)
            assert np.array_equal(val[1], ref[1][:, :cut]), (where, key, "in_event")
        else:
            assert val.dtype == ref.dtype and np.array_equal(val, ref[..., :cut], equal_nan=True), (where, key)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", U.CASES, ids=lambda c: f"T{c[0]}-p{c[1]}")
def test_device_against_host_twin_and_oracles(case, dtype):
    from gan_danet_amd import drought as D
    T, period, phase, baseline = case
    nmax = U.nmax_of(T, period, baseline)
    tables = {kind: D.rank_table(kind, nmax) for kind in ("percentile", "empirical")}
    wide = None
    for M in reversed(U.MS):
        x = U.series(T, M, dtype)
        got = _device(x, _dev(x), case, tables)
        _same(got, _host(x, case, tables), f"M={M} device vs host twin")
        wide = got if wide is None else wide
        _same(got, wide, f"M={M} vs M={U.M_MAX}", cut=M)                                  # a column's bits do not depend on M
        if M in (65, 1025):
            _same(_device(x, _off(x), case, tables), got, f"M={M} one element past a 16-byte boundary")
            mask = U.mask_of(M)
            masked = _device(x, _dev(x), case, tables, mask, durations=(3,))
            _same(masked, _host(x, case, tables, mask, durations=(3,)), f"M={M} masked, device vs host twin")
            off = np.flatnonzero(mask == 0)
            assert np.all(masked["clim"][0][:, off] == 0) and np.isnan(masked["clim"][1:][:, :, off]).all()
            assert np.isnan(masked["empirical"][:, off]).all() and np.isnan(masked["standardized", 0][:, off]).all()
            assert not masked["events", 3][1][:, off].any() and np.all(masked["events", 3][0]["n_valid"][off] == 0)
    M = U.M_MAX
    x = U.series(T, M, dtype)
    cols = U.oracle_columns(M)
    wm, wm2 = U.check_clim(wide["clim"], cols, U.clim_oracle(dtype, T, period, phase, baseline, cols))
    wi = max(U.check_index(wide[kind, ddof], dtype, T, period, phase, baseline, kind, ddof, cols)
             for kind in ("anomaly", "standardized") for ddof in (0, 1))
    for kind in tables:
        want, _ = U.rank_want(dtype, T, period, phase, baseline, tables[kind], cols)
        for c in cols:
            assert np.array_equal(wide[kind][:, c], want[c], equal_nan=True), (kind, c)
    ws = 0.0
    for d in U.durations(T):
        maps, steps = wide["events", d]
        ws = max(ws, U.check_events(maps, steps, x, U.THRESHOLD, d, cols)[2])
    assert np.array_equal(wide["exceed"], U.exceed_oracle(x, U.THRESHOLD), equal_nan=True)
    print(f"T = {T} period {period} {np.dtype(dtype).name}: device == host twin on every column; mean at most {wm:.3f} of its bound, "
          f"M2 {wm2:.3f}, index {wi:.3f}, severity {ws:.3f}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_python_surface(dtype):
    """(T, H, W) cubes through gan_danet_amd.drought: the kernels' outputs reshaped, a bool mask of the step's shape, a
    climatology of one cube applied to another, events on the standardised index at the default threshold"""
    from gan_danet_amd import drought as D
    from gan_danet_amd import kern as K
    T, H, W = 25, 5, 13
    x = U.series(T, H * W, dtype)
    xd = _dev(x.reshape(T, H, W))
    mask = U.mask_of(H * W).reshape(H, W).astype(bool)
    clim = D.climatology(xd, 12, 3, (3, 20), _dev(mask))
    assert (clim.period, clim.phase, clim.baseline) == (12, 3, (3, 20)) and clim.n.shape == (12, H, W)
    rec = K.drought_clim_host(x, 12, 3, 3, 20, mask.reshape(-1))
    assert np.array_equal(clim.rec.cpu().numpy().reshape(3, 12, -1), rec, equal_nan=True)
    assert np.array_equal(clim.mean.cpu().numpy().reshape(12, -1), rec[1], equal_nan=True)
    with np.errstate(all="ignore"):
        want = np.where(rec[0] - 1 > 0, np.sqrt(rec[2] / (rec[0] - 1)), np.nan)
    assert np.allclose(clim.std(1).cpu().numpy().reshape(12, -1), want, rtol=4e-16, atol=0, equal_nan=True)
    for kind, code in (("anomaly", 0), ("standardized", 1)):
        z = D.drought_index(xd, kind, period=12, phase=3, baseline=(3, 20), ddof=1, mask=_dev(mask))
        assert z.shape == xd.shape and z.dtype == xd.dtype
        assert np.array_equal(z.cpu().numpy().reshape(T, -1), K.drought_index_host(x, rec, 3, code, 1), equal_nan=True)
        assert torch.equal(torch.nan_to_num(D.drought_index(xd, kind, clim=clim, ddof=1), nan=9.0), torch.nan_to_num(z, nan=9.0))
    for kind in ("percentile", "empirical"):
        z = D.drought_index(xd, kind, period=12, phase=3, baseline=(3, 20))
        want = K.drought_rank_host(x, D.rank_table(kind, 3), 12, 3, 3, 20)
        assert z.dtype == xd.dtype and np.array_equal(z.cpu().numpy().reshape(T, -1), want, equal_nan=True)
    p = D.drought_index(xd, "percentile").cpu().numpy()
    assert np.nanmin(p) > 0 and np.nanmax(p) < 1
    dsi = D.drought_index(xd)                                                            # the GRACE-DSI over the whole record
    ev = D.drought_events(dsi, return_steps=True)
    assert (ev.threshold, ev.min_duration) == (-0.8, 3) and ev.in_event.shape == dsi.shape and ev.in_event.dtype == torch.uint8
    maps, steps = K.drought_events_host(dsi.cpu().numpy().reshape(T, -1), -0.8, 3, want_steps=True)
    for name in U.EV_MAPS:
        assert np.array_equal(getattr(ev, name).cpu().numpy().reshape(-1), maps[name], equal_nan=True), name
    assert np.array_equal(ev.in_event.cpu().numpy().reshape(T, -1), steps) and ev["n_events"].shape == (H, W)
    few = D.drought_events(dsi, maps=("peak", "n_events"))
    assert set(few.maps) == {"peak", "n_events"} and few.max_duration is None and few.in_event is None
    assert torch.equal(few.n_events, ev.n_events)
    L = K.L
    for call in (lambda: D.drought_index(xd, "spi"), lambda: D.drought_index(xd, "empirical", clim=clim), lambda: D.climatology(xd, 0),
                 lambda: D.climatology(xd, 12, 12), lambda: D.climatology(xd, 12, 0, (5, 5)), lambda: D.drought_events(dsi, min_duration=0),
                 lambda: D.drought_events(dsi, maps=("depth",)), lambda: D.drought_index(xd, ddof=2),
                 lambda: D.drought_index(_dev(np.zeros((600, 2))), "percentile", period=2)):
        with pytest.raises(L.GandanetError):
            call()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_drought_area_two_zones(dtype):
    """a two-zone ZoneMap on a 5 x 7 grid against numpy: unweighted fractions are count / count exactly, weighted ones hold
    the bound of gd_zone_mean's own test"""
    import basins_util as B
    from gan_danet_amd import drought as D
    from gan_danet_amd.basins import ZoneMap
    T, H, W = 25, 5, 7
    x = U.series(T, H * W, dtype).reshape(T, H, W)
    masks = [np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)]
    masks[0][:3, :4] = True
    masks[1][2:, 2:] = True                                                              # the zones overlap, and leave pixels out
    zm = ZoneMap(_dev(B.bits_of(masks)[None]), ["a", "b"], _dev(np.arange(W, dtype=np.float64)), _dev(np.arange(H, dtype=np.float64)))
    ks = (-0.5, 0.0, -1.25)
    frac, count = D.drought_area(_dev(x), ks, zm)
    assert frac.shape == (T, 2, 3) and frac.dtype == torch.float64 and count.shape == (T, 2) and count.dtype == torch.int64
    frac, count = frac.cpu().numpy(), count.cpu().numpy()
    weights = np.cos(np.deg2rad(np.linspace(10.0, 50.0, H)))[:, None] * np.ones((1, W))
    wfrac, wcount = (v.cpu().numpy() for v in D.drought_area(_dev(x), ks, zm, _dev(weights)))
    assert np.array_equal(wcount, count)
    worst = 0.0
    for t in range(T):
        for z, m in enumerate(masks):
            valid = m & ~np.isnan(x[t])
            assert count[t, z] == valid.sum() > 0
            for k, thr in enumerate(ks):
                assert frac[t, z, k] == float((valid & (x[t] <= thr)).sum()) / float(valid.sum()), (t, z, k)
    for k, thr in enumerate(ks):
        want, cnt, mabs = B.zone_mean_ref(U.exceed_oracle(x, thr).astype(np.float64), masks, weights)
        err, bound = np.abs(wfrac[:, :, k] - want), cnt * 2.0 ** -52 * mabs
        assert np.all(err <= bound)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    # without a zone map the domain is the one zone; the five DSI classes by default
    frac1, count1 = D.drought_area(_dev(x))
    assert frac1.shape == (T, 1, 5) and count1.shape == (T, 1)
    for t in range(T):
        valid = ~np.isnan(x[t])
        assert count1[t, 0].item() == valid.sum()
        assert frac1[t, 0, 1].item() == float((valid & (x[t] <= -0.8)).sum()) / float(valid.sum())
    print(f"{np.dtype(dtype).name}: unweighted fractions exact; weighted at most {worst:.3f} of the bound")


def test_compare_events_by_hand():
    from gan_danet_amd import drought as D
    a = np.array([[1, 0, 1], [1, 0, 0], [0, 0, 1], [1, 1, 1]], dtype=np.uint8)           # (T = 4, 3 pixels): the reference
    b = np.array([[1, 1, 0], [0, 0, 0], [0, 1, 1], [1, 1, 1]], dtype=np.uint8)
    r = D.compare_events(_dev(a), _dev(b))
    assert r.hits.tolist() == [2, 1, 2] and r.misses.tolist() == [1, 0, 1] and r.false_alarms.tolist() == [0, 2, 0]
    r2 = D.compare_events(_dev(a.reshape(4, 1, 3)), _dev(b.reshape(4, 1, 3)))
    assert r2.hits.shape == (1, 3) and r2.hits.dtype == torch.int64 and r2.false_alarms.tolist() == [[0, 2, 0]]
    with pytest.raises(D.L.GandanetError):
        D.compare_events(_dev(a), _dev(b[:3]))


@pytest.mark.parametrize("M", [255, 256])
def test_launcher_edges(M):
    """every entry with T = 5, period 2 at the series counts on either side of a whole 256-thread workgroup (1 and 257 are
    in U.MS): guarded outputs (the sentinels around them stay intact), bit for bit the host twins"""
    from gan_danet_amd import drought as D
    case = (5, 2, 0, None)
    tables = {"empirical": D.rank_table("empirical", U.nmax_of(5, 2, None))}
    for dtype in (np.float64, np.float32):
        x = U.series(5, M, dtype)
        _same(_device(x, _dev(x), case, tables, durations=(2,)), _host(x, case, tables, durations=(2,)), f"M={M} T=5 period 2")


def test_exceed_grid_stride_beyond_the_cap():
    """gd_drought_exceed with more elements than its capped grid has threads (65536 workgroups of 256): n = 2^24 + 257
    fp32, so the first 257 threads take a second element; guarded output, bit for bit the host twin.  This is
    drought_exceed_kernel, which kept a kernel of its own; the grid-stride form of gd_item_kernel (gd_block_mean, capped at
    2^20 workgroups) would need more than 2^28 outputs for a second trip, which does not fit a test, so that step of the
    shared launcher is run by no test (tests/test_gpu_series.py::test_launcher_edges covers its first trip)"""
    from gan_danet_amd import kern as K
    n = (1 << 24) + 257
    x = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    x[::1001] = np.nan
    g = Guarded((n,), torch.float32)
    K.drought_exceed(_dev(x), U.THRESHOLD, out=g.out)
    assert np.array_equal(g.get(), K.drought_exceed_host(x, U.THRESHOLD), equal_nan=True)
