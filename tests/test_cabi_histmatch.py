"""CPU: the host twin of histogram matching (gd_hist_match_host; csrc/histmatch_core.h, the per-element code the device
kernel runs) against the numpy restatement of the notebook in tests/histmatch_util.py, BIT FOR BIT: every size pair up to
12 x 12 on quantised and continuous data at four weights, 3000 seeded random cases, the cases of the GPU file, source NaNs
of both signs, and the argument refusals of both entries (no GPU is touched: validation comes first).

Zero tolerance is a property of the arithmetic (histmatch_util's docstring), not a tuned number."""
import numpy as np
import pytest
import torch

import histmatch_util as U


def _K():
    from gan_danet_amd import kern
    return kern


def _lib():
    from gan_danet_amd import _lib as L
    return L, L.load()


def _first_difference(got, want):
    bad = np.flatnonzero(got.view(np.uint64).ravel() != want.view(np.uint64).ravel())
    return f"{bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}"


def test_every_small_size_pair_equals_numpy_bitwise():
    K = _K()
    n = 0
    for kind, src, ref in U.small_pairs():
        for w in U.WEIGHTS:
            got, want = K.hist_match_host(src, ref, w), U.restatement_batch(src, ref, w)
            assert U.same_bits(got, want), (kind, src.shape[1], ref.shape[1], w, _first_difference(got, want))
            n += 1
    assert n == 12 * 12 * 2 * 4


def test_random_cases_equal_numpy_bitwise():
    K = _K()
    n = 0
    for src, ref, w in U.random_cases(3000):
        got, want = K.hist_match_host(src, ref, w), U.restatement_batch(src, ref, w)
        assert U.same_bits(got, want), (n, src.shape[1], ref.shape[1], w, _first_difference(got, want))
        n += 1
    assert n == 3000


@pytest.mark.parametrize("name", list(U.device_cases()))
def test_device_cases_on_the_host_twin(name):
    """the shapes of test_gpu_histmatch.py (grid-stride sizes, exact quantile ties, rounding of x * nt, degenerate sizes,
    batches, extremes) on the twin, so a machine without a GPU still holds the twin to numpy there"""
    src, ref, w, exact = U.device_cases()[name]
    got, want = _K().hist_match_host(src, ref, w), U.device_want(name)
    assert got.dtype == np.float64 and got.shape == src.shape
    assert U.agree(got, want, exact), (name, _first_difference(got, want) if exact else "values differ")


def test_cpu_tensors_go_to_the_host_twin():
    from gan_danet_amd import inference as INF
    K = _K()
    src, ref = U.continuous(np.random.default_rng(1), 2, 90, 40)
    src4, ref4 = src.reshape(2, 1, 9, 10), ref.reshape(2, 1, 5, 8)
    got = K.hist_match(torch.from_numpy(src4), torch.from_numpy(ref4), 0.35)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and tuple(got.shape) == src4.shape
    assert U.same_bits(got.numpy().reshape(2, 90), U.restatement_batch(src, ref, 0.35))
    assert U.same_bits(INF.mild_histogram_matching(torch.from_numpy(src4), torch.from_numpy(ref4), 0.35).numpy(), got.numpy())
    L, _ = _lib()
    with pytest.raises(L.GandanetError):
        K.hist_match(torch.from_numpy(src4).double(), torch.from_numpy(ref4), 0.35)
    with pytest.raises(L.GandanetError):
        K.hist_match_host(src, ref[:1], 0.35)


@pytest.mark.parametrize("case", range(len(U.nan_cases())))
def test_source_nans_of_both_signs_stay_where_they_are(case):
    name, src, ref, w, mask = U.nan_cases()[case]
    want = U.restatement_batch(src, ref, w)
    assert np.array_equal(np.isnan(want), mask), f"{name}: the restatement itself does not keep NaNs to their positions"
    got = _K().hist_match_host(src, ref, w)
    assert np.array_equal(np.isnan(got), mask), name
    assert U.same_bits(got[~mask], want[~mask]), name
    # the NaNs rank above every number, so the others see them: dropping them changes the result
    if name != "nan short":
        assert not U.same_bits(got[0][~mask[0]], _K().hist_match_host(src[:1, ~mask[0]], ref[:1], w)[0])


def test_argument_refusals():
    """-1 and a gd_last_error text from both entries; the pointers are never-dereferenced addresses"""
    L, lib = _lib()
    a, b, c, d = 0x1000, 0x2000, 0x3000, 0x4000
    big = 1 << 31                                                      # 2^31 - 1 is the largest sample
    nbytes = lib.gd_hist_match_ws_bytes(100, 50)
    assert nbytes > 4 * 100 * 4 + 50 * 4
    assert lib.gd_hist_match_ws_bytes(0, 5) == 0 and lib.gd_hist_match_ws_bytes(5, big) == 0

    def host(src=a, ref=b, B=2, ns=100, nt=50, out=c):
        return lib.gd_hist_match_host(src, ref, B, ns, nt, 0.5, out)

    def dev(src=a, ref=b, B=2, ns=100, nt=50, out=c, ws=d, ws_bytes=nbytes):
        return lib.gd_hist_match(src, ref, B, ns, nt, 0.5, out, ws, ws_bytes, None)

    for fn in (host, dev):
        for kw, word in (({"src": None}, "bad arguments"), ({"ref": None}, "bad arguments"), ({"out": None}, "bad arguments"),
                         ({"B": 0}, "bad arguments"), ({"B": -1}, "bad arguments"), ({"ns": 0}, "bad arguments"),
                         ({"ns": -5}, "bad arguments"), ({"nt": 0}, "bad arguments"), ({"nt": -1}, "bad arguments"),
                         ({"ns": big}, "2^31"), ({"nt": big}, "2^31")):
            if fn is dev and ("ns" in kw or "nt" in kw):
                kw = dict(kw, ws_bytes=1 << 40)
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert word in L.last_error(), (fn.__name__, kw, L.last_error())
    assert dev(ws=None) == -1 and "bad arguments" in L.last_error()
    assert dev(ws_bytes=nbytes - 1) == -1 and "workspace" in L.last_error()
