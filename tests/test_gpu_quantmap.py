"""GPU: the bias-correction module (gan_danet_amd/biascorrect.py, csrc/quantmap.hip) against the host twins bit for bit on
every output of every case of tests/quantmap_util.py -- they share csrc/quantmap_core.h, and the twins equal numpy bit for
bit on the CPU (tests/test_cabi_quantmap.py).  The device equals itself on a second run and with a second launch in flight
on another stream; the register route and the LDS route give the same bits on a 32-sample slot; sentinels around the outputs
show that nothing is written outside them.  series_quantiles against torch.nanquantile is a sanity check at fp64 rounding
level only.  QuantileMap round-trips through its state_dict, and assemble_product without the keyword keeps its bits and
with a map equals the chain done by hand.

Observed on an MI355X: the device equalled the host twin bit for bit in every case, down both routes and in both layouts."""
import numpy as np
import pytest
import torch

import quantmap_util as U

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _host_quantiles(x, kw, route="auto"):
    from gan_danet_amd import kern as K
    T = x.shape[0]
    b0, b1 = (0, T) if kw["baseline"] is None else kw["baseline"]
    return K.qm_quantiles_host(x, U.Q_LIST, kw["period"], kw["phase"], b0, b1, kw["mask"], None, kw["min_samples"], _route=route)


@pytest.mark.parametrize("name", sorted(U.QUANT_CASES))
def test_quantiles_device_equals_twin(name):
    from gan_danet_amd import kern as K
    x, kw = U.quant_case(name)
    T = x.shape[0]
    b0, b1 = (0, T) if kw["baseline"] is None else kw["baseline"]
    want, wn = _host_quantiles(x, kw)
    xd, md = _dev(x), None if kw["mask"] is None else _dev(kw["mask"])
    routes = ("auto", "long") + (("small",) if -(-(b1 - b0) // kw["period"]) <= 32 else ())
    for route in routes:
        for layout in (K.L.QM_LAYOUT_QSM, K.L.QM_LAYOUT_SQM):
            got, gn = K.qm_quantiles(xd, U.Q_LIST, kw["period"], kw["phase"], b0, b1, md, None, kw["min_samples"], layout, route)
            got = got.cpu().numpy()
            if layout == K.L.QM_LAYOUT_SQM:
                got = np.ascontiguousarray(got.transpose(1, 0, 2))
            assert U.same(got, want) and U.same(gn.cpu().numpy(), wn), (name, route, layout)


def test_both_sort_routes_give_the_same_bits_on_a_32_sample_slot():
    from gan_danet_amd import kern as K
    x, kw = U.quant_case("slot_32")
    xd = _dev(x)
    small, ns = K.qm_quantiles(xd, U.Q_LIST, kw["period"], kw["phase"], _route="small")
    long_, nl = K.qm_quantiles(xd, U.Q_LIST, kw["period"], kw["phase"], _route="long")
    assert torch.all(ns == 32) and torch.equal(ns, nl)
    assert U.same(small.cpu().numpy(), long_.cpu().numpy())
    with pytest.raises(K.L.GandanetError, match="register route"):
        K.qm_quantiles(_dev(U.quant_case("slot_33")[0]), U.Q_LIST, 2, 1, _route="small")


def test_series_quantiles_interface_and_torch_sanity():
    import gan_danet_amd as gd
    x, kw = U.quant_case("months_f64")
    want, wn = _host_quantiles(x, kw)
    xd = _dev(x).reshape(37, 5, 67)
    q, n = gd.series_quantiles(xd, U.Q_LIST, period=12, mask=_dev(kw["mask"]).reshape(5, 67))
    assert q.shape == (len(U.Q_LIST), 12, 5, 67) and q.dtype == torch.float64 and n.shape == (12, 5, 67) and n.dtype == torch.int32
    assert U.same(q.cpu().numpy().reshape(want.shape), want) and U.same(n.cpu().numpy().reshape(wn.shape), wn)
    # a (T,) series, period 1, against torch.nanquantile: a sanity check at rounding level (the bit claim is the twin's)
    x1 = _dev(U.quant_case("series_2048")[0][:, 0])
    q1, n1 = gd.series_quantiles(x1, U.Q_LIST)
    assert q1.shape == (len(U.Q_LIST), 1) and int(n1) == 2048
    ref = torch.nanquantile(x1, torch.tensor(U.Q_LIST, device="cuda", dtype=torch.float64))
    assert torch.allclose(q1[:, 0], ref, rtol=0.0, atol=16 * 2.0 ** -53 * float(x1.abs().max()))
    xs = _dev(U.quant_case("long_150")[0])
    qs, _ = gd.series_quantiles(xs, [0.25, 0.5])
    ref = torch.nanquantile(xs, torch.tensor([0.25, 0.5], device="cuda", dtype=torch.float64), dim=0)
    assert torch.allclose(qs[:, 0], ref, rtol=0.0, atol=16 * 2.0 ** -53 * 16.0, equal_nan=True)
    for bad in ([1.5], [float("nan")], []):
        with pytest.raises(gd.kern.L.GandanetError):
            gd.series_quantiles(xd, bad)
    with pytest.raises(gd.kern.L.GandanetError):
        gd.series_quantiles(torch.zeros(2049, 2, device="cuda"), [0.5])


def _fit_and_tables(name):
    import gan_danet_amd as gd
    model, obs, x, kw, t0 = U.apply_case(name)
    qm = gd.QuantileMap.fit(_dev(model), _dev(obs), n_quantiles=kw["Q"], period=kw["period"], phase=kw["phase"], pairwise=kw["pairwise"],
                            min_samples=kw["min_samples"])
    return qm, model, obs, x, kw, t0


@pytest.mark.parametrize("name", sorted(U.APPLY_CASES))
def test_fit_and_apply_device_equal_twin(name):
    from gan_danet_amd import kern as K
    qm, model, obs, x, kw, t0 = _fit_and_tables(name)
    T, H, W = model.shape
    Q, period = kw["Q"], kw["period"]
    m2, o2, p = model.reshape(T, -1), obs.reshape(T, -1), U.nodes(Q)
    args = dict(period=period, phase=kw["phase"], min_samples=kw["min_samples"], layout=K.L.QM_LAYOUT_SQM)
    mq, nm = K.qm_quantiles_host(m2, p, x2=o2 if kw["pairwise"] else None, **args)
    oq, no = K.qm_quantiles_host(o2, p, x2=m2 if kw["pairwise"] else None, **args)
    mq, oq = mq.reshape(period, Q, H, W), oq.reshape(period, Q, H, W)
    assert qm.model_q.shape == (period, Q, H, W) and qm.n_model.dtype == torch.int32
    assert U.same(qm.model_q.cpu().numpy(), mq) and U.same(qm.obs_q.cpu().numpy(), oq)
    assert U.same(qm.n_model.cpu().numpy().reshape(nm.shape), nm) and U.same(qm.n_obs.cpu().numpy().reshape(no.shape), no)
    if kw["pairwise"]:
        assert qm.n is qm.n_model
    else:
        with pytest.raises(AttributeError):
            qm.n
    ph = (t0 + kw["phase"]) % period
    own, _ = K.qm_quantiles_host(x.reshape(x.shape[0], -1), p, period, ph, layout=K.L.QM_LAYOUT_SQM)
    own = own.reshape((period, Q) + x.shape[1:])
    xd = _dev(x)
    pad = 64
    for kind in ("eqm", "qdm"):
        for ex in ("constant", "clip"):
            want = K.qm_apply_host(x, mq, oq, kind, ex, ph, own if kind == "qdm" else None, p if kind == "qdm" else None)
            buf = torch.full((x.size + 2 * pad,), -7.0, device="cuda", dtype=xd.dtype)
            out = buf[pad:pad + x.size].view(x.shape)
            got = qm.apply(xd, kind, ex, t0=t0, out=out)
            assert got.data_ptr() == out.data_ptr() and got.dtype == xd.dtype
            host = buf.cpu().numpy()
            assert np.all(host[:pad] == -7.0) and np.all(host[pad + x.size:] == -7.0), "written outside the output"
            assert U.same(host[pad:pad + x.size].reshape(x.shape), want), (name, kind, ex)
            assert U.same(qm.apply(xd, kind, ex, t0=t0).cpu().numpy(), want)       # a second run, a new output


def test_same_bits_with_a_second_launch_in_flight():
    """the entries run on the caller's stream and share nothing: two streams at once give the bits of one"""
    from gan_danet_amd import kern as K
    qm, model, obs, x, kw, t0 = _fit_and_tables("f3")
    xa, kwa = U.quant_case("months_f64")
    xb, kwb = U.quant_case("long_150")
    xad, xbd, xd = _dev(xa), _dev(xb), _dev(x)
    ref_a = K.qm_quantiles(xad, U.Q_LIST, 12)[0]
    ref_b = K.qm_quantiles(xbd, U.Q_LIST, 1)[0]
    ref_e, ref_q = qm.apply(xd, "eqm", t0=t0), qm.apply(xd, "qdm", t0=t0)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a, e = K.qm_quantiles(xad, U.Q_LIST, 12)[0], qm.apply(xd, "eqm", t0=t0)
    with torch.cuda.stream(s2):
        b, q = K.qm_quantiles(xbd, U.Q_LIST, 1)[0], qm.apply(xd, "qdm", t0=t0)
    torch.cuda.synchronize()
    for got, ref in ((a, ref_a), (b, ref_b), (e, ref_e), (q, ref_q)):
        assert U.same(got.cpu().numpy(), ref.cpu().numpy())


def test_state_dict_round_trip():
    import gan_danet_amd as gd
    qm, model, obs, x, kw, t0 = _fit_and_tables("f1_own_nans")
    sd = {k: v.cpu() for k, v in qm.state_dict().items()}
    assert all(isinstance(v, torch.Tensor) for v in sd.values())
    back = gd.QuantileMap.load_state_dict(sd, device="cuda")
    assert (back.period, back.phase, back.pairwise, back.min_samples, back.baseline) == (qm.period, qm.phase, qm.pairwise, qm.min_samples,
                                                                                        qm.baseline)
    for k in ("model_q", "obs_q", "n_model", "n_obs"):
        assert U.same(getattr(back, k).cpu().numpy(), getattr(qm, k).cpu().numpy())
    xd = _dev(x)
    for kind in ("eqm", "qdm"):
        assert U.same(back.apply(xd, kind).cpu().numpy(), qm.apply(xd, kind).cpu().numpy())
    with pytest.raises(gd.kern.L.GandanetError):
        gd.QuantileMap.load_state_dict(sd)                       # host tensors and no device
    with pytest.raises(gd.kern.L.GandanetError):
        qm.apply(xd.cpu())
    with pytest.raises(gd.kern.L.GandanetError):
        qm.apply(xd, "cdf")
    with pytest.raises(gd.kern.L.GandanetError):
        qm.apply(xd[:, :, :4].contiguous())


def test_assemble_product_with_and_without_a_map():
    import gan_danet_amd as gd
    from gan_danet_amd import inference
    rng = np.random.default_rng(3)
    T, H, W, f = 14, 4, 6, 5
    res = _dev(rng.standard_normal((T, H * f, W * f)).astype(np.float32))
    trend = _dev(rng.standard_normal((T, H, W)))
    bias = _dev(rng.standard_normal((T, H * 4, W * 4)) * 0.1)
    mask = _dev((rng.random((H * f, W * f)) > 0.2).astype(np.uint8))
    kw = dict(mask=mask, bias=bias)
    base = inference.assemble_product(res, trend, 2.5, 0.75, **kw)
    none = inference.assemble_product(res, trend, 2.5, 0.75, quantile_map=None, quantile_kind="qdm", **kw)
    for k in ("product", "series"):
        assert U.same(base[k].cpu().numpy(), none[k].cpu().numpy())
    # a map on the coarse grid, fitted as the documented recipe does
    raw = inference.restore_units(res, gd.spline.zoom(trend, (1, 5, 5), order=3), 2.5, 0.75, 10.0)
    grace = _dev(rng.standard_normal((T, H, W)) * 30.0 + 4.0)
    qm = gd.QuantileMap.fit(gd.timeseries.coarsen(raw, (f, f)), grace, n_quantiles=7, period=4)
    for kind in ("eqm", "qdm"):
        out = inference.assemble_product(res, trend, 2.5, 0.75, quantile_map=qm, quantile_kind=kind, **kw)
        hand = qm.apply(raw, kind)
        hand[:, mask == 0] = float("nan")
        series = torch.nanmean(hand.reshape(T, -1), dim=1)
        # two fp64 sums of at most H W values in different orders: each within n u max|v| of the exact sum
        tol = 2.0 * 2.0 ** -53 * hand.shape[1] * hand.shape[2] * float(torch.nan_to_num(hand).abs().max())
        hand = hand + gd.spline.zoom(bias, (1, 1.25, 1.25), order=3)
        assert U.same(out["product"].cpu().numpy(), hand.cpu().numpy())
        assert torch.allclose(out["series"], series, rtol=0.0, atol=tol)
        assert not U.same(out["product"].cpu().numpy(), base["product"].cpu().numpy())
