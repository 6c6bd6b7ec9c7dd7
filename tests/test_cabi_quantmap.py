"""CPU: the bias-correction entry points of the C ABI (include/gandanet.h, "Bias correction") are declared, bound and
re-exported, reject every bad argument before any launch, and the host twins -- plain C++ over csrc/quantmap_core.h --
EQUAL the numpy oracle of tests/quantmap_util.py (np.nanquantile, np.interp) bit for bit: the quantile nodes on every
case of QUANT_CASES down every route that takes it, the fit both pairwise and not, and both kinds and both
extrapolations of the apply on APPLY_CASES.  Two properties: eqm sends the model's nodes to the observation's nodes
exactly, and qdm of a shifted cube is eqm's answer shifted, within the bound quantmap_util derives."""
import os

import numpy as np
import pytest
import torch

import quantmap_util as U

NAMES = ("gd_qm_quantiles", "gd_qm_apply")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_quantmap_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import biascorrect, build, kern
    L, lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gandanet.h")).read()
    assert "Bias correction (quantmap.hip, csrc/quantmap_core.h)" in src
    for name in NAMES:
        for nm in (name, name + "_host"):
            assert nm + "(" in src and nm in L.SIGNATURES and hasattr(lib, nm), nm
            assert hasattr(kern, nm[3:]), nm
    for k, v in (("MAX_T", 2048), ("MAX_N", 2048), ("MAX_Q", 256), ("MAX_PERIOD", 366), ("MAX_F", 16), ("SMALL_N", 32)):
        assert f"#define GD_QM_{k} {v}" in src and getattr(L, "QM_" + k) == v
    assert f"GD_QM_LAYOUT_QSM = {L.QM_LAYOUT_QSM}, GD_QM_LAYOUT_SQM = {L.QM_LAYOUT_SQM}" in src
    for table, fmt in ((L.QM_ROUTES, "GD_QM_ROUTE_{}"), (L.QM_KINDS, "GD_QM_{}"), (L.QM_EXTRAPOLATE, "GD_QM_{}")):
        for name, code in table.items():
            assert f"{fmt.format(name.upper())} = {code}" in src, name
    assert "quantmap.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "quantmap_core.h"))
    assert gan_danet_amd.biascorrect is biascorrect
    for name in ("QuantileMap", "series_quantiles"):
        assert getattr(gan_danet_amd, name) is getattr(biascorrect, name)


def _refused(L, fn, order, good, rules, host):
    for kw, word in rules:
        v = dict(good, **kw)
        args = [v[k] for k in order]
        rc = fn(*args) if host else fn(*args, None)
        assert rc == -1, (fn.__name__, kw, rc)
        assert word in L.last_error(), (fn.__name__, kw, L.last_error())


def test_quantmap_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses) are not
    touched"""
    L, lib = _lib()
    a, b, c, d = 0x1000, 0x2000, 0x3000, 0x4000
    for host in (False, True):
        sfx = "_host" if host else ""
        order = ("x", "x2", "dtype", "T", "M", "q", "Q", "period", "phase", "b0", "b1", "mask", "min_samples", "layout", "route", "quant", "n")
        good = dict(x=a, x2=None, dtype=1, T=181, M=7, q=b, Q=5, period=12, phase=0, b0=0, b1=181, mask=None, min_samples=1, layout=0,
                    route=0, quant=c, n=d)
        rules = [(dict(x=None), "null"), (dict(q=None), "null"), (dict(quant=None), "null"), (dict(n=None), "null"),
                 (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(T=0), "T outside"), (dict(T=2049), "T outside"),
                 (dict(M=0), "M <= 0"), (dict(M=1 << 31), "too many"), (dict(Q=0), "Q outside"), (dict(Q=257), "Q outside"),
                 (dict(period=0), "period"), (dict(period=367), "period"), (dict(phase=-1), "phase"), (dict(phase=12), "phase"),
                 (dict(b0=5, b1=5), "baseline"), (dict(b0=9, b1=4), "baseline"), (dict(b0=-1), "baseline"), (dict(b1=182), "baseline"),
                 (dict(min_samples=-1), "min_samples"), (dict(layout=2), "layout"), (dict(route=3), "route"), (dict(route=-1), "route"),
                 (dict(route=1, period=1), "register route"), (dict(x=a + 4), "aligned"), (dict(x2=a + 2, dtype=0), "aligned"),
                 (dict(q=b + 4), "aligned"), (dict(quant=c + 4), "aligned"), (dict(n=d + 2), "aligned")]
        _refused(L, getattr(lib, "gd_qm_quantiles" + sfx), order, good, rules, host)
        order = ("x", "dtype", "T", "H", "W", "f", "model_q", "obs_q", "own_q", "p", "Q", "period", "phase", "kind", "extrapolate", "out")
        good = dict(x=a, dtype=1, T=20, H=4, W=6, f=2, model_q=b, obs_q=c, own_q=None, p=None, Q=11, period=12, phase=3, kind=0,
                    extrapolate=0, out=d)
        rules = [(dict(x=None), "null"), (dict(model_q=None), "null"), (dict(obs_q=None), "null"), (dict(out=None), "null"),
                 (dict(dtype=2), "dtype"), (dict(T=0), "empty"), (dict(H=0), "empty"), (dict(W=-1), "empty"), (dict(f=0), "f outside"),
                 (dict(f=17), "f outside"), (dict(Q=1), "Q outside"), (dict(Q=257), "Q outside"), (dict(period=0), "period"),
                 (dict(period=367), "period"), (dict(phase=12), "phase"), (dict(phase=-1), "phase"), (dict(H=1 << 16, W=1 << 16), "too many"),
                 (dict(kind=2), "kind"), (dict(extrapolate=2), "extrapolate"), (dict(kind=1), "qdm needs"), (dict(kind=1, own_q=b), "qdm needs"),
                 (dict(x=a + 4), "aligned"), (dict(out=d + 2, dtype=0), "aligned"), (dict(model_q=b + 4), "aligned"),
                 (dict(kind=1, own_q=b, p=c + 4), "aligned")]
        _refused(L, getattr(lib, "gd_qm_apply" + sfx), order, good, rules, host)
    # the twin reads q, which is on the host there
    x, quant, n = np.zeros((4, 2)), np.zeros((1, 1, 2)), np.zeros((1, 2), dtype=np.int32)
    for bad in (np.nan, -0.1, 1.5):
        q = np.array([bad])
        rc = lib.gd_qm_quantiles_host(x.ctypes.data, None, 1, 4, 2, q.ctypes.data, 1, 1, 0, 0, 4, None, 1, 0, 0, quant.ctypes.data, n.ctypes.data)
        assert rc == -1 and "probability" in L.last_error()


def test_quantmap_wrappers_refuse_malformed_arguments():
    """every limit and every malformed argument raises GandanetError: the module and the kern wrappers check the host-side
    arguments before they look for a device, so this runs without one"""
    import gan_danet_amd as gd
    from gan_danet_amd import kern as K
    E = K.L.GandanetError
    cpu = torch.zeros(8, 2, 3, dtype=torch.float64)
    for fn in (lambda: gd.series_quantiles(cpu, [0.5]), lambda: gd.QuantileMap.fit(cpu, cpu),
               lambda: gd.series_quantiles(np.zeros((8, 2)), [0.5])):
        with pytest.raises(E, match="GPU tensor"):
            fn()
    for q in ([], [float("nan")], [-0.01], [1.01], np.linspace(0, 1, 257), [[0.5]], "half", None):
        with pytest.raises(E):
            K.qm_probs(q, "test")
    for nq in (1, 257, 0, -3, 2.5, True):
        with pytest.raises(E, match="n_quantiles"):
            K.qm_nodes(nq)
    assert U.same(K.qm_nodes(51), U.nodes(51)) and K.qm_probs(0.5, "test").shape == (1,)
    for args, word in (((2049, 1, 0, 0, 2049, 1), "T <="), ((10, 0, 0, 0, 10, 1), "period"), ((10, 367, 0, 0, 10, 1), "period"),
                       ((10, 4, 4, 0, 10, 1), "phase"), ((10, 4, -1, 0, 10, 1), "phase"), ((10, 4, 0, 5, 5, 1), "baseline"),
                       ((10, 4, 0, 0, 11, 1), "baseline"), ((10, 4, 0, 0, 10, -1), "min_samples")):
        with pytest.raises(E, match=word):
            K._qm_calendar("test", *args)
    with pytest.raises(E, match="route"):
        K._qm_route("medium")
    with pytest.raises(E, match="f <= 16"):
        K._qm_factor((3, 34, 51), 2, 3, "test")
    for shape in ((3, 7, 9), (3, 6, 10), (3, 6), (0, 6, 9), (3, 1, 9)):
        with pytest.raises(E):
            K._qm_factor(shape, 2, 3, "test")
    assert K._qm_factor((3, 6, 9), 2, 3, "test") == 3 and K._qm_factor((1, 32, 48), 2, 3, "test") == 16
    with pytest.raises(E, match="kind"):
        K._qm_codes("cdf", "constant", 0, 12, "test")
    with pytest.raises(E, match="extrapolate"):
        K._qm_codes("eqm", "linear", 0, 12, "test")
    t = np.zeros((12, 5, 2, 3))
    for mq, oq in ((t, t[:, :, :1]), (t[0], t[0]), (np.zeros((367, 2, 1, 1)), np.zeros((367, 2, 1, 1))), (t[:, :1], t[:, :1]),
                   (np.zeros((1, 257, 1, 1)), np.zeros((1, 257, 1, 1)))):
        with pytest.raises(E):
            K.qm_apply_host(np.zeros((4, 2, 3)), mq, oq)
    with pytest.raises(E, match="qdm"):
        K.qm_apply_host(np.zeros((4, 2, 3)), t, t, "qdm")
    with pytest.raises(E, match="own_q"):
        K.qm_apply_host(np.zeros((4, 2, 3)), t, t, "qdm", own_q=np.zeros((12, 5, 4, 3)), p=U.nodes(5))
    with pytest.raises(E):
        K.qm_quantiles_host(np.zeros((2049, 1)), [0.5])
    with pytest.raises(E):
        K.qm_quantiles_host(np.zeros((4, 2)), [0.5], x2=np.zeros((4, 3)))
    with pytest.raises(E):
        K.qm_quantiles_host(np.zeros((4, 2)), [0.5], x2=np.zeros((4, 2), dtype=np.float32))
    with pytest.raises(E):
        K.qm_quantiles_host(np.zeros((66, 2)), [0.5], _route="small")
    with pytest.raises(E):
        gd.QuantileMap.load_state_dict({"model_q": torch.zeros(1)})


def _routes(x, kw):
    T = x.shape[0]
    b0, b1 = (0, T) if kw["baseline"] is None else kw["baseline"]
    steps = -(-(b1 - b0) // kw["period"])
    return b0, b1, ("auto", "long") + (("small",) if steps <= 32 else ())


@pytest.mark.parametrize("name", sorted(U.QUANT_CASES))
def test_quantile_twin_equals_numpy(name):
    from gan_danet_amd import kern as K
    x, kw = U.quant_case(name)
    ref, n = U.quantiles(x, U.Q_LIST, **kw)
    b0, b1, routes = _routes(x, kw)
    assert np.isfinite(ref).any()
    for route in routes:
        for layout in (K.L.QM_LAYOUT_QSM, K.L.QM_LAYOUT_SQM):
            got, gn = K.qm_quantiles_host(x, U.Q_LIST, kw["period"], kw["phase"], b0, b1, kw["mask"], None, kw["min_samples"], layout, route)
            if layout == K.L.QM_LAYOUT_SQM:
                got = got.transpose(1, 0, 2)
            assert U.same(np.ascontiguousarray(got), ref) and U.same(gn, n), (name, route, layout)


def test_quantile_cases_hold_what_they_are_for():
    """asserted on the oracle's own output: an empty sample, a masked pixel, a slot below min_samples, tied nodes, a constant
    series, both sides of the route boundary"""
    ref, n = U.quantiles(*_xkw("months_f64"))
    assert np.all(n[:, 1] == 0) and np.all(np.isnan(ref[:, :, 1])) and np.all(n[:, 4] == 0) and np.all(np.isnan(ref[:, :, 4]))
    assert np.all(ref[:, :, 2] == 1.75) and set(np.unique(n)) >= {0, 1, 2, 3, 4}
    ref, n = U.quantiles(*_xkw("months_min4"))
    assert np.all(n[0] == 4) and np.all(n[1:] == 3) and np.isfinite(ref[:, 0]).all() and np.isnan(ref[:, 1:]).all()
    ref, n = U.quantiles(*_xkw("ties"))
    assert np.any((ref[0] == ref[1]) & (n >= 3)) and np.any(ref[0] < ref[2])
    for name, steps in (("slot_32", 32), ("slot_33", 33), ("slot_16", 16), ("long_150_f32", None), ("series_2048", 2048)):
        _, n = U.quantiles(*_xkw(name))
        assert steps is None or np.all(n == steps)
    _, n = U.quantiles(*_xkw("baseline_phase"))
    assert n.max() <= 3 and n.sum() < 25 * 70


def _xkw(name):
    x, kw = U.quant_case(name)
    return x, U.Q_LIST, kw["period"], kw["phase"], kw["baseline"], kw["mask"], None, kw["min_samples"]


def _fit_host(model, obs, kw):
    from gan_danet_amd import kern as K
    T = model.shape[0]
    m2, o2 = model.reshape(T, -1), obs.reshape(T, -1)
    p = U.nodes(kw["Q"])
    args = dict(period=kw["period"], phase=kw["phase"], min_samples=kw["min_samples"], layout=K.L.QM_LAYOUT_SQM)
    mq, nm = K.qm_quantiles_host(m2, p, x2=o2 if kw["pairwise"] else None, **args)
    oq, no = K.qm_quantiles_host(o2, p, x2=m2 if kw["pairwise"] else None, **args)
    return mq, oq, nm, no


@pytest.mark.parametrize("name", sorted(U.APPLY_CASES))
def test_fit_and_apply_twins_equal_numpy(name):
    from gan_danet_amd import kern as K
    model, obs, x, kw, t0 = U.apply_case(name)
    T, H, W = model.shape
    Q, period = kw["Q"], kw["period"]
    ref = U.fit(model.reshape(T, -1), obs.reshape(T, -1), **kw)
    got = _fit_host(model, obs, kw)
    for g, r in zip(got, ref):
        assert U.same(g, r)
    assert U.same(ref[2], ref[3]) == kw["pairwise"] and np.isnan(ref[0]).any() and np.isfinite(ref[0]).any()
    mq, oq = ref[0].reshape(period, Q, H, W), ref[1].reshape(period, Q, H, W)
    ph = (t0 + kw["phase"]) % period
    p = U.nodes(Q)
    own, _ = K.qm_quantiles_host(x.reshape(x.shape[0], -1), p, period, ph, layout=K.L.QM_LAYOUT_SQM)
    own = own.reshape((period, Q) + x.shape[1:])
    outs = {}
    for kind in ("eqm", "qdm"):
        for ex in ("constant", "clip"):
            want = U.apply(x, mq, oq, kind, ex, kw["phase"], t0)
            outs[kind, ex] = K.qm_apply_host(x, mq, oq, kind, ex, ph, own if kind == "qdm" else None, p if kind == "qdm" else None)
            assert outs[kind, ex].dtype == x.dtype and U.same(outs[kind, ex], want), (name, kind, ex)
            assert np.isnan(want).any() and np.isfinite(want).any()
    # the cases hold values outside the tables (the extrapolations differ there) and exactly on their end nodes
    f = x.shape[1] // H
    assert not U.same(outs["eqm", "constant"], outs["eqm", "clip"]) and U.same(outs["qdm", "constant"], outs["qdm", "clip"])
    if x.dtype == np.float64:
        s = (t0 + kw["phase"]) % period
        on = (x[0, 0::f, 0::f] == mq[s, 0]) & (mq[s, 1] > mq[s, 0])   # tied first nodes: numpy answers with the last of them
        assert on.any() and U.same(outs["eqm", "clip"][0, 0::f, 0::f][on], oq[s, 0][on])


def test_eqm_sends_model_nodes_to_obs_nodes():
    """strictly increasing tables: apply(model_q[j], "eqm") is obs_q[j] exactly, for both extrapolations"""
    from gan_danet_amd import kern as K
    rng = np.random.default_rng(7)
    period, Q, H, W, phase = 3, 9, 4, 5, 2
    mq = np.cumsum(rng.random((period, Q, H, W)) + 1e-3, axis=1) - 4.0
    oq = np.cumsum(rng.random((period, Q, H, W)) + 1e-3, axis=1) * 1.7
    x = np.empty((Q * period, H, W))
    want = np.empty_like(x)
    for t in range(Q * period):
        x[t], want[t] = mq[(t + phase) % period, t // period], oq[(t + phase) % period, t // period]
    for ex in ("constant", "clip"):
        assert U.same(K.qm_apply_host(x, mq, oq, "eqm", ex, phase), want)
        assert U.same(U.apply(x, mq, oq, "eqm", ex, phase), want)


def test_qdm_of_a_shifted_cube_is_eqm_shifted():
    """x = z + c through a map fitted on (z, o): its own table is the model table shifted by c, so qdm(x) = eqm(z) + c up
    to the rounding of three interpolations (quantmap_util.shift_bound)"""
    from gan_danet_amd import kern as K
    T, H, W, period, Q, c = 120, 3, 4, 4, 11, 2.625
    z = U.cube(T, H * W, 11).reshape(T, H, W)
    o = (U.cube(T, H * W, 12) * 1.4 + 0.3).reshape(T, H, W)
    kw = dict(Q=Q, period=period, phase=0, pairwise=True, min_samples=2)
    mq, oq, _, _ = (t.reshape((period, -1, H, W)) for t in U.fit(z.reshape(T, -1), o.reshape(T, -1), **kw))
    x = z + c
    A = max(np.abs(z).max(), np.abs(o).max(), np.abs(x).max()) + abs(c)
    dm, do = np.diff(mq, axis=1), np.diff(oq, axis=1)
    assert dm.min() >= 1e6 * U.U64 * A                       # the bound's precondition, on the oracle's tables
    S = float((do / dm).max())
    p = U.nodes(Q)
    own, _ = K.qm_quantiles_host(x.reshape(T, -1), p, period, 0, layout=K.L.QM_LAYOUT_SQM)
    own = own.reshape(period, Q, H, W)
    assert np.abs(own - (mq + c)).max() <= 17 * U.U64 * A    # "the same table shifted", to the rounding the bound allows it
    qdm = K.qm_apply_host(x, mq, oq, "qdm", "constant", 0, own, p)
    eqm = K.qm_apply_host(z, mq, oq, "eqm", "constant", 0)
    err, bound = np.abs(qdm - (eqm + c)).max(), U.shift_bound(A, S, Q)
    print(f"qdm shift: max err {err:.3e}, bound {bound:.3e} (S = {S:.3g}, A = {A:.3g})")
    assert np.isfinite(qdm).all() and err <= bound
    assert np.abs(qdm - x).max() > 0.1                       # and the correction is no identity
