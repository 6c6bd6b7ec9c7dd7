"""GPU: the connected-component kernels (csrc/ccl.hip) equal their host twins bit for bit -- labels, K and every table
and track field -- on every case and structure of tests/clusters_util.py, equal scipy.ndimage.label directly, give the same
bits on a second run and with the LDS tile stage skipped, and drought_clusters agrees with drought_events' in_event cube
and with the per-step patch filter recipe done with scipy."""
import numpy as np
import pytest
import torch

import clusters_util as U
from gpu_util import DEV

pytestmark = pytest.mark.gpu


def device_pipeline(K, C, case, s, weights=None, tiles=True):
    """the device entries end to end, as numpy: (parent, labels, K, bounds, offsets, tracks, index, totals)"""
    values = case.x.dtype != np.uint8
    x = torch.from_numpy(case.x).to(DEV)
    mask = torch.from_numpy(case.mask).to(DEV).reshape(-1) if values and case.mask is not None else None
    thr = case.threshold if values else 0.0
    parent = K.ccl_label(x, thr, C.structure_word(s), mask, tiles)
    if case.min_size > 1:
        K.ccl_filter(parent, case.min_size)
    labels, count = K.ccl_relabel(parent)
    k = int(count.item())
    if k == 0:
        return parent.cpu().numpy(), labels.cpu().numpy(), 0, None, None, None, None, None
    bounds = K.ccl_bounds(labels, k)
    offsets = K.ccl_offsets(bounds)
    w = torch.from_numpy(weights).to(DEV) if weights is not None else None
    tracks, index = K.ccl_tracks(x if values else None, labels, bounds, offsets, int(offsets[-1].item()), thr, w, values)
    totals = K.ccl_totals(tracks, bounds, offsets)
    return tuple(v.cpu().numpy() if isinstance(v, torch.Tensor) else v for v in (parent, labels, k, bounds, offsets, tracks, index, totals))


def same_bits(a, b):
    if a is None or b is None or isinstance(a, int):
        return a is b or a == b
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", U.CASES, ids=repr)
def test_device_equals_host_twin_and_scipy(case):
    from gan_danet_amd import clusters as C
    from gan_danet_amd import kern as K
    names = ("parent", "labels", "K", "bounds", "offsets", "tracks", "index", "totals")
    for s in U.STRUCTURES:
        want, kw = U.labels_oracle(case, s)
        weights = U.weights_of(case.x.shape) if isinstance(s, int) else None
        host = U.host_pipeline(K, case, s, weights)
        dev = device_pipeline(K, C, case, s, weights)
        assert dev[2] == kw and np.array_equal(dev[1], want), (case, U.structure_id(s), "scipy")
        for nm, h, d in zip(names, host, dev):
            assert same_bits(h, d), (case, U.structure_id(s), nm)
        again = device_pipeline(K, C, case, s, weights)
        for nm, d, e in zip(names, dev, again):
            assert same_bits(d, e), (case, U.structure_id(s), nm, "second run")
        flat = device_pipeline(K, C, case, s, weights, tiles=False)
        assert same_bits(dev[0], flat[0]) and same_bits(dev[1], flat[1]), (case, U.structure_id(s), "without the tile stage")


@pytest.mark.parametrize("name", ["random0.35", "index-f64", "index-f32", "small-clusters", "empty"])
def test_public_interface(name):
    from gan_danet_amd import clusters as C
    case = {c.name: c for c in U.CASES}[name]
    values = case.x.dtype != np.uint8
    x = torch.from_numpy(case.x).to(DEV)
    mask = torch.from_numpy(case.mask).to(DEV) if case.mask is not None else None
    w = torch.from_numpy(U.weights_of(case.x.shape)).to(DEV)
    for s in U.STRUCTURES:
        want, kw = U.labels_oracle(case, s)
        labels, k = C.label_components(x, case.threshold, s, case.min_size, mask)
        assert k == kw and labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want), (case, U.structure_id(s))
        for weights in (None, w):
            cl = C.drought_clusters(x, case.threshold if values else 0.0, s, case.min_size, weights=weights, mask=mask)
            assert cl.n == kw and np.array_equal(cl.labels.cpu().numpy(), want)
            series = cl.area_series()
            assert tuple(series.shape) == (case.x.shape[0], kw) and series.dtype == torch.float64
            if kw == 0:
                assert cl.volume.numel() == 0 and cl.tracks.shape == (0, 6)
                continue
            bounds = U.bounds_oracle(want, kw)
            assert np.array_equal(cl.voxels.cpu().numpy(), bounds[:, 0]) and np.array_equal(cl.bbox.cpu().numpy(), bounds[:, 1:])
            assert np.array_equal(cl.duration.cpu().numpy(), bounds[:, 2] - bounds[:, 1] + 1)
            assert np.array_equal(cl.start.cpu().numpy(), bounds[:, 1]) and np.array_equal(cl.end.cpu().numpy(), bounds[:, 2])
            wn = None if weights is None else weights.cpu().numpy()
            U.check_tracks(case, want, cl.bounds.cpu().numpy(), cl.offsets.cpu().numpy(), cl.tracks.cpu().numpy(), cl.index.cpu().numpy(),
                           wn, values)
            U.check_totals(cl.bounds.cpu().numpy(), cl.offsets.cpu().numpy(), cl.tracks.cpu().numpy(), cl.totals.cpu().numpy(), values)
            if weights is None:
                # the unweighted area is the pixel count: exact, and its sum over the clusters is the labelled pixels of the step
                assert np.array_equal(series.sum(1).cpu().numpy(), (want > 0).sum((1, 2)).astype(np.float64))
                assert np.array_equal(cl.volume.cpu().numpy(), bounds[:, 0].astype(np.float64))
            k0 = kw // 2
            tr = cl.track(k0)
            assert np.array_equal(tr["step"].cpu().numpy(), np.arange(bounds[k0, 1], bounds[k0, 2] + 1))
            assert np.array_equal(tr["area"].cpu().numpy(), series[bounds[k0, 1]:bounds[k0, 2] + 1, k0].cpu().numpy())
            assert set(tr) == {"step", "count", "area", "severity", "centroid_h", "centroid_w", "min"}
            assert bool((series[:bounds[k0, 1], k0] == 0).all()) and bool((series[bounds[k0, 2] + 1:, k0] == 0).all())


@pytest.mark.parametrize("name", ["random0.35", "index-f64", "index-f32"])
def test_per_step_patch_filter_recipe(name):
    from gan_danet_amd import clusters as C
    case = {c.name: c for c in U.CASES}[name]
    values = case.x.dtype != np.uint8
    x = torch.from_numpy(case.x).to(DEV)
    mask = torch.from_numpy(case.mask).to(DEV) if case.mask is not None else None
    for s in (1, 2, 3, U.SPACE8_TIME1):
        for min_step, min_size in ((3, 1), (5, 8)):
            want, kw = U.andreadis_oracle(case, s, min_step, min_size)
            cl = C.drought_clusters(x, case.threshold if values else 0.0, s, min_size, min_step, mask=mask)
            assert cl.n == kw and np.array_equal(cl.labels.cpu().numpy(), want), (case, U.structure_id(s), min_step, min_size)
            if kw and values:
                U.check_tracks(case, want, cl.bounds.cpu().numpy(), cl.offsets.cpu().numpy(), cl.tracks.cpu().numpy(),
                               cl.index.cpu().numpy(), None, True)


def test_clusters_of_the_event_cube():
    """drought_events' in_event fed as the uint8 cube with planar4 (no link in time): the same labels as labelling the
    cube's own copy with scipy, every step's clusters are that step's event pixels, and with the time link the runs of
    run theory (>= min_duration steps) make every cluster last at least min_duration"""
    from gan_danet_amd import clusters as C
    from gan_danet_amd import drought as D
    case = {c.name: c for c in U.CASES}["index-f64"]
    x = torch.from_numpy(case.x).to(DEV)
    ev = D.drought_events(x, case.threshold, min_duration=2, maps=("n_events",), return_steps=True)
    cube = ev.in_event
    assert cube.dtype == torch.uint8 and int(cube.sum()) > 0
    host = U.Case("in_event", cube.cpu().numpy())
    cl = C.drought_clusters(cube, structure="planar4")
    want, kw = U.labels_oracle(host, "planar4")
    assert cl.n == kw and np.array_equal(cl.labels.cpu().numpy(), want)
    assert bool((cl.duration == 1).all()) and bool(torch.isnan(cl.severity).all()) and bool(torch.isnan(cl.peak).all())
    assert np.array_equal(cl.area_series().sum(1).cpu().numpy(), (host.x != 0).sum((1, 2)).astype(np.float64))
    assert np.array_equal((cl.labels > 0).cpu().numpy(), host.x != 0)
    linked = C.drought_clusters(cube, structure=U.SPACE8_TIME1)
    assert linked.n == U.labels_oracle(host, U.SPACE8_TIME1)[1] and int(linked.duration.min()) >= 2


def test_refusals_on_the_device():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import clusters as C
    x = torch.zeros((4, 5, 6), device=DEV, dtype=torch.float64)
    for call in (lambda: C.label_components(x), lambda: C.label_components(x, float("nan")), lambda: C.label_components(x, -0.8, 4),
                 lambda: C.label_components(x, -0.8, min_size=0), lambda: C.label_components(x[0], -0.8),
                 lambda: C.label_components(x.to(torch.int32), -0.8), lambda: C.drought_clusters(x, weights=torch.ones(5, 6)),
                 lambda: C.drought_clusters(x, weights=torch.ones(5, 5, device=DEV)), lambda: C.drought_clusters(x, min_step_pixels=-1),
                 lambda: C.drought_clusters(x, mask=torch.ones(5, 5, device=DEV, dtype=torch.uint8))):
        with pytest.raises(L.GandanetError):
            call()
