"""CPU: what the argument layer of the analysis wrappers in kern.py owns, pinned through the public ``*_host`` functions, one
(or two) per family: the main array must be float32 / float64 (uint8 as well for the cluster cubes), non-empty and of the
family's ndim, and a mask / weight / times vector of the wrong length is refused, each with GandanetError; lists,
Fortran-ordered arrays and strided slices are coerced and give the bits of the contiguous float64 array; float32 input gives
float32 outputs where the device twin documents "in the dtype of x".  Where a wrapper has never made one of these checks
the case says so (``vec=None``, ``ndim=False``) instead of pinning what it does with such input."""
import numpy as np
import pytest

SERIES, CUBE = (5, 7), (3, 4, 5)


def _K():
    from gan_danet_amd import kern
    return kern


def _u8(v):
    return None if v is None else np.asarray(v, dtype=np.uint8)


def _stl(K, x, v):
    p = dict(period=2, seasonal=3, trend=3, low_pass=3, seasonal_deg=1, trend_deg=1, low_pass_deg=1, inner_iter=2, outer_iter=1)
    return K.stl_decompose_host(x, p)


def _series_stats(K, x, v):
    return K.series_stats_host(x, x, _u8(v))


def _block_mean(K, x, v):
    return K.block_mean_host(x, 2, 5, v)


def _trend(K, x, v):
    return K.trend_test_host(x, np.arange(5.0) if v is None else v, 0, None, K.L.TREND_SEN | K.L.TREND_CI, -1.96)


def _ens_verify(K, x, v):
    rec, maps = K.ens_verify_host(x, np.linspace(-1.0, 1.0, 7), _u8(v))
    return rec, maps


def _eof_gram(K, x, v):
    return K.eof_gram_host(x, np.zeros(7), np.ones(7, dtype=np.uint8), v)


def _spec_prepare(K, x, v):
    return K.spec_prepare_host(x, _u8(v), detrend="linear" if "linear" in K.L.SPEC_DETREND else "mean")


def _drought_index(K, x, v):
    clim = np.stack([np.full((2, 7), 3.0), np.zeros((2, 7)), np.full((2, 7), 2.0)])
    return K.drought_index_host(x, clim, mask=_u8(v))


def _ccl_label(K, x, v):
    return K.ccl_label_host(x, 0.0, 0x1FFF, _u8(v))


def _nbr_fraction(K, x, v):
    return K.nbr_fraction_host(x, 0.0, 3, mask=_u8(v))


def _qm_quantiles(K, x, v):
    return K.qm_quantiles_host(x, [0.25, 0.5], mask=_u8(v))


def _qm_apply(K, x, v):
    t = np.sort(np.linspace(-2.0, 2.0, 3 * 4 * 5).reshape(1, 3, 4, 5), axis=1)
    return K.qm_apply_host(x, t, t + 0.5)


# name: (the call, the shape of its main array, the length a wrong mask / weight / times vector gets (None: the wrapper has
# never known the length to compare it), does it check the ndim itself, the outputs that come in the dtype of x)
CASES = {
    "stl_decompose_host": (_stl, SERIES, None, True, lambda o: o),
    "series_stats_host": (_series_stats, SERIES, None, True, lambda o: ()),
    "block_mean_host": (_block_mean, CUBE, None, False, lambda o: o[:1]),
    "trend_test_host": (_trend, SERIES, 6, True, lambda o: ()),
    "ens_verify_host": (_ens_verify, SERIES, 8, True, lambda o: [o[1][k] for k in ("crps", "err", "spread")]),
    "eof_gram_host": (_eof_gram, SERIES, 8, True, lambda o: ()),
    "spec_prepare_host": (_spec_prepare, CUBE, 21, True, lambda o: ()),
    "drought_index_host": (_drought_index, SERIES, 8, True, lambda o: [o]),
    "ccl_label_host": (_ccl_label, CUBE, 21, True, lambda o: ()),
    "nbr_fraction_host": (_nbr_fraction, CUBE, 21, True, lambda o: ()),
    "qm_quantiles_host": (_qm_quantiles, SERIES, 8, True, lambda o: ()),
    "qm_apply_host": (_qm_apply, CUBE, None, True, lambda o: [o]),
}


def _data(shape):
    rs = np.random.RandomState(sum(shape))
    return rs.uniform(-1.0, 1.0, shape)


def _flat(o):
    if isinstance(o, dict):
        return [a for k in sorted(o) for a in _flat(o[k])]
    if isinstance(o, (tuple, list)):
        return [a for v in o for a in _flat(v)]
    return [np.asarray(o)]


def _same(a, b):
    a, b = _flat(a), _flat(b)
    return len(a) == len(b) and all(p.dtype == q.dtype and p.shape == q.shape and np.array_equal(p, q, equal_nan=p.dtype.kind == "f")
                                    for p, q in zip(a, b))


@pytest.mark.parametrize("name", sorted(CASES))
def test_bad_arrays_and_vectors_are_refused(name):
    K = _K()
    call, shape, bad_len, checks_ndim, _ = CASES[name]
    x = _data(shape)
    call(K, x, None)                                                              # the good call goes through
    bad = [("integer dtype", x.astype(np.int32)), ("empty", np.empty((0,) + shape[1:]))]
    if checks_ndim:
        bad += [("one dimension too few", x[0]), ("one dimension too many", x[None])]
    if name == "ens_verify_host":                                                 # (M, ...) members: any ndim from 2 on
        bad[2:] = [("one dimension too few", x[0])]
    for what, arr in bad:
        with pytest.raises(K.L.GandanetError):
            call(K, arr, None)
            pytest.fail(f"{name} took an array with {what}")
    if bad_len is not None:
        with pytest.raises(K.L.GandanetError):
            call(K, x, np.ones(bad_len))


@pytest.mark.parametrize("name", sorted(CASES))
def test_lists_and_strided_arrays_give_the_bits_of_the_dense_array(name):
    K = _K()
    call, shape, _, _, _ = CASES[name]
    x = _data(shape)
    want = call(K, x, None)
    wide = np.repeat(x, 2, axis=-1)
    wide[..., 1::2] = 9.0
    forms = [("list", x.tolist()), ("strided slice", wide[..., ::2])]
    fortran = np.asfortranarray(x)
    assert not fortran.flags["C_CONTIGUOUS"] and not forms[1][1].flags["C_CONTIGUOUS"]
    if name == "ens_verify_host":
        # the members are read in place, a constant stride apart, so each has to be dense: a Fortran-ordered stack is refused
        with pytest.raises(K.L.GandanetError):
            call(K, fortran, None)
        forms[1] = ("members a stride apart", np.stack([x, x + 9.0], axis=1)[:, 0])
        assert not forms[1][1].flags["C_CONTIGUOUS"]
    else:
        forms.append(("Fortran order", fortran))
    for what, arr in forms:
        assert _same(call(K, arr, None), want), (name, what)


@pytest.mark.parametrize("name", sorted(CASES))
def test_float32_input_gives_outputs_in_the_dtype_of_x(name):
    K = _K()
    call, shape, _, _, in_dtype_of_x = CASES[name]
    x = _data(shape)
    for dtype in (np.float32, np.float64):
        outs = in_dtype_of_x(call(K, x.astype(dtype), None))
        assert all(o.dtype == dtype for o in outs), (name, [o.dtype for o in outs])


def test_zone_rasterize_host_arguments():
    """the basin rasteriser takes float64 only, so it converts what it is given (integers too) instead of refusing a dtype"""
    K = _K()
    edges = np.array([[0, 0, 4, 0], [4, 0, 4, 4], [4, 4, 0, 4], [0, 4, 0, 0], [1, 1, 6, 1], [6, 1, 3, 7], [3, 7, 1, 1]], dtype=np.float64)
    off, xs, ys = [0, 4, 7], np.arange(5) + 0.5, np.arange(4) + 0.25
    want = K.zone_rasterize_host(edges, off, xs, ys)
    assert want.shape == (4, 5) and want.dtype == np.uint32 and 0 < np.count_nonzero(want) < want.size
    wide = np.repeat(edges, 2, axis=1)
    for what, e in (("list", edges.tolist()), ("Fortran order", np.asfortranarray(edges)), ("strided slice", wide[:, ::2]),
                    ("integers", edges.astype(np.int64))):
        assert np.array_equal(K.zone_rasterize_host(e, off, xs, ys), want), what
    assert np.array_equal(K.zone_rasterize_host(edges, np.array(off, dtype=np.int32), xs.tolist(), np.repeat(ys, 2)[::2]), want)
    for e, o in ((edges[0], off), (edges[None], off), (edges[:, :3], off), (edges, [7]), (edges, [[0, 4, 7]])):
        with pytest.raises(K.L.GandanetError):
            K.zone_rasterize_host(e, o, xs, ys)
