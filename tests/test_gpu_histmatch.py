"""GPU: the histogram-matching kernels (csrc/histmatch.hip: key pass, hipCUB radix sorts, the quantile-interpolation kernel
over csrc/histmatch_core.h) against the host twin AND the numpy restatement of the notebook, bit for bit: device == twin ==
numpy.  Cases (tests/histmatch_util.py): the smallest size at which a thread of the capped grid takes a second item, source
quantiles equal to reference quantiles (ns = nt, ns = 4 nt, all distinct), size pairs where x * nt rounds across an integer,
degenerate sizes and constant inputs, batches that reuse the workspace, denormals / +-FLT_MAX / mixed zeros (values only:
numpy does not define which of the equal zeros np.unique keeps), and source NaNs of both signs.

The twin is held to numpy without a GPU in test_cabi_histmatch.py.

Measured on an MI355X: every case equal as stated; with the radix sort fed the raw source keys (no key pass) the three NaN
cases failed, 74 of the 76 finite values of the shortest wrong.  The file takes 3 s."""
import numpy as np
import pytest
import torch

import histmatch_util as U

pytestmark = pytest.mark.gpu


def _K():
    from gan_danet_amd import kern
    return kern


def _device(src, ref, w):
    got = _K().hist_match(torch.from_numpy(src).to("cuda"), torch.from_numpy(ref).to("cuda"), w)
    assert got.dtype == torch.float64 and tuple(got.shape) == src.shape
    return got.cpu().numpy()


def _report(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).ravel())
    if bad.size == 0:
        return "only zero signs or NaN payloads differ"
    return f"{bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}"


@pytest.mark.parametrize("name", list(U.device_cases()))
def test_device_equals_twin_equals_numpy(name):
    src, ref, w, exact = U.device_cases()[name]
    want = U.device_want(name)
    twin = _K().hist_match_host(src, ref, w)
    got = _device(src, ref, w)
    assert U.agree(twin, want, exact), f"{name}: twin against numpy: {_report(twin, want)}"
    assert U.agree(got, want, exact), f"{name}: device against numpy: {_report(got, want)}"
    assert U.agree(got, twin, exact), f"{name}: device against twin: {_report(got, twin)}"


@pytest.mark.parametrize("case", range(len(U.nan_cases())))
def test_source_nans_of_both_signs(case):
    """a NaN whose sign bit is set sorts to the FRONT in the radix sort's bit order, where the binary searches of every
    finite value would walk into it; the key pass makes every NaN the positive quiet NaN, which sorts last as numpy's do"""
    name, src, ref, w, mask = U.nan_cases()[case]
    want = U.restatement_batch(src, ref, w)
    assert np.array_equal(np.isnan(want), mask), f"{name}: the restatement itself does not keep NaNs to their positions"
    twin = _K().hist_match_host(src, ref, w)
    got = _device(src, ref, w)
    assert np.array_equal(np.isnan(got), mask) and np.array_equal(np.isnan(twin), mask), name
    assert U.same_bits(got[~mask], want[~mask]), f"{name}: device against numpy: {_report(got[~mask], want[~mask])}"
    assert U.same_bits(got[~mask], twin[~mask]), f"{name}: device against twin: {_report(got[~mask], twin[~mask])}"


def test_workspace_is_the_documented_size_and_is_enough():
    """a caller-owned workspace of exactly gd_hist_match_ws_bytes, placed inside a poisoned buffer: the result is right and
    nothing outside the workspace is written"""
    from gan_danet_amd import _lib as L
    lib = L.load()
    src, ref, w, _ = U.device_cases()["batch of 3"]
    B, ns, nt = src.shape[0], src.shape[1], ref.shape[1]
    nbytes = int(lib.gd_hist_match_ws_bytes(ns, nt))
    guard = 4096
    buf = torch.full((nbytes + 2 * guard,), 0xA5, device="cuda", dtype=torch.uint8)
    s, r = torch.from_numpy(src).to("cuda"), torch.from_numpy(ref).to("cuda")
    out = torch.empty(src.shape, device="cuda", dtype=torch.float64)
    rc = lib.gd_hist_match(s.data_ptr(), r.data_ptr(), B, ns, nt, w, out.data_ptr(), buf.data_ptr() + guard, nbytes,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.last_error()
    assert U.same_bits(out.cpu().numpy(), U.device_want("batch of 3"))
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + nbytes:] == 0xA5).all())
