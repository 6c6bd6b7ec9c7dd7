"""CPU: the evaluation entry points of the C ABI (include/gandanet.h, "evaluation") reject bad arguments before any
launch, gd_eval_merge_host merges records exactly and in the given order, and RegressionMetrics.compute() agrees over two
gloo ranks with uneven shards.  References are numpy in fp64 on the fp32 inputs (tests/eval_np.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from eval_np import check_metrics, metrics, offset_pair, record


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_eval_symbols_are_declared_and_bound():
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    for name in ("gd_eval_stats", "gd_eval_stats_ws_bytes", "gd_masked_plane_mean", "gd_masked_plane_mean_ws_bytes",
                 "gd_ensemble_stats", "gd_eval_merge_host"):
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name)


def test_eval_argument_errors_before_any_launch():
    """null pointer, n = 0, M = 0, M = 33, short workspace: negative code + gd_last_error, no GPU needed (the pointers
    are never dereferenced: validation comes first)"""
    L, lib = _lib()
    p = 0x1000                      # a non-null, aligned address that is never touched
    ws = int(lib.gd_eval_stats_ws_bytes(100))
    assert ws > 0 and lib.gd_eval_stats_ws_bytes(0) == 0

    def bad(rc, word):
        assert rc < 0, rc
        assert word in L.last_error(), L.last_error()

    bad(lib.gd_eval_stats(None, p, 1, 100, None, 1.0, 0.0, 0, p, p, ws, None), "null")
    bad(lib.gd_eval_stats(p, None, 1, 100, None, 1.0, 0.0, 0, p, p, ws, None), "null")
    bad(lib.gd_eval_stats(p, p, 1, 100, None, 1.0, 0.0, 0, None, p, ws, None), "null")
    bad(lib.gd_eval_stats(p, p, 1, 100, None, 1.0, 0.0, 0, p, None, ws, None), "null")
    bad(lib.gd_eval_stats(p, p, 1, 0, None, 1.0, 0.0, 0, p, p, ws, None), "n <= 0")
    bad(lib.gd_eval_stats(p, p, 0, 100, None, 1.0, 0.0, 0, p, p, ws, None), "n <= 0")
    bad(lib.gd_eval_stats(p, p, 1, 100, None, 1.0, 0.0, 0, p, p, ws - 1, None), "workspace")
    bad(lib.gd_eval_stats(p, p, 1, 100, None, 1.0, 0.0, 64, p, p, ws, None), "flag")

    pws = int(lib.gd_masked_plane_mean_ws_bytes(6, 384))
    assert pws > 0
    bad(lib.gd_masked_plane_mean(None, 6, 384, None, p, p, p, pws, None), "null")
    bad(lib.gd_masked_plane_mean(p, 6, 384, None, None, p, p, pws, None), "null")
    bad(lib.gd_masked_plane_mean(p, 6, 384, None, p, None, p, pws, None), "null")
    bad(lib.gd_masked_plane_mean(p, 6, 0, None, p, p, p, pws, None), "n <= 0")
    bad(lib.gd_masked_plane_mean(p, 0, 384, None, p, p, p, pws, None), "n <= 0")
    bad(lib.gd_masked_plane_mean(p, 6, 384, None, p, p, p, pws - 1, None), "workspace")

    bad(lib.gd_ensemble_stats(None, 5, 10, 10, 0, p, p, None), "null")
    bad(lib.gd_ensemble_stats(p, 5, 10, 10, 0, None, p, None), "null")
    bad(lib.gd_ensemble_stats(p, 5, 10, 10, 0, p, None, None), "null")
    bad(lib.gd_ensemble_stats(p, 5, 10, 0, 0, p, p, None), "n <= 0")
    bad(lib.gd_ensemble_stats(p, 0, 10, 10, 0, p, p, None), "1..32")
    bad(lib.gd_ensemble_stats(p, 33, 10, 10, 1, p, p, None), "1..32")
    bad(lib.gd_ensemble_stats(p, 5, 9, 10, 0, p, p, None), "stride")

    met = (C.c_double * 4)()
    bad(lib.gd_eval_merge_host(None, 0, None, None), "null")
    bad(lib.gd_eval_merge_host(None, 2, None, met), "no pointer")
    bad(lib.gd_eval_merge_host(None, -1, None, met), "no pointer")


def test_merge_is_exact_and_ordered():
    from gan_danet_amd import kern as K
    n = 50_000
    x, y = offset_pair(n)
    want = metrics(y, x)                                        # truth x, prediction y
    cuts = [0, 1, 8, 8 + 4096, n]                               # parts of 1, 7, 4096 and the rest
    recs = [record(y[a:b], x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    rec, got = K.eval_merge_host(recs)
    check_metrics(got, want, "four parts")
    whole = record(y, x)
    scale = math.sqrt(whole[3] * whole[4])
    for i in (0, 1, 2, 6, 7):
        assert abs(rec[i] - whole[i]) <= 1e-9 * abs(whole[i]), (i, rec[i], whole[i])
    for i in (3, 4, 5):                                         # co-moments, relative to sqrt(M2_p M2_t)
        assert abs(rec[i] - whole[i]) <= 1e-9 * scale, (i, rec[i], whole[i])

    # the case discriminates: raw sums in fp32 (sum x^2 - (sum x)^2 / n) miss the bound on this input by far
    xs, ys = x.astype(np.float32), y.astype(np.float32)
    f = np.float32
    sxx, sx = np.sum(xs * xs, dtype=f), np.sum(xs, dtype=f)
    syy, sy, sxy = np.sum(ys * ys, dtype=f), np.sum(ys, dtype=f), np.sum(xs * ys, dtype=f)
    m2x, m2y, cxy = sxx - sx * sx / f(n), syy - sy * sy / f(n), sxy - sx * sy / f(n)
    sse = syy - f(2) * sxy + sxx
    with np.errstate(all="ignore"):
        raw_r2 = float(f(1) - sse / m2x)
        raw_cc = float(cxy / np.sqrt(m2x * m2y))
    assert not abs(raw_r2 - want["r2"]) <= 1e-9
    assert not abs(raw_cc - want["cc"]) <= 1e-9

    # zero-count records anywhere change nothing, bit for bit, whatever else they hold
    junk = np.array([0.0, 5.0, -3.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    padded = [junk, recs[0], np.zeros(8), recs[1], junk, junk, recs[2], recs[3], np.zeros(8)]
    rec2, got2 = K.eval_merge_host(padded)
    assert rec2 == rec and got2 == got

    # the given order is respected: merging is a left fold, so a different order is a different rounding sequence of
    # the same quantity -- equal to the bound, and the fold itself reproduces when repeated by hand
    rec_rev, got_rev = K.eval_merge_host(recs[::-1])
    check_metrics(got_rev, want, "reversed")
    acc = K.eval_merge_host(recs[:1])[0]
    for r in recs[1:]:
        acc = K.eval_merge_host([acc, r])[0]
    assert acc == rec


def test_merge_edge_semantics():
    from gan_danet_amd import kern as K
    t = np.full(100, 2.5, dtype=np.float32)
    # constant truth, perfect prediction: r2 1.0 (SS_tot == 0 and SS_res == 0); cc NaN (both variances 0)
    m = K.eval_merge_host([record(t[:40], t[:40]), record(t[40:], t[40:])])[1]
    assert m["r2"] == 1.0 and m["mse"] == 0.0 and m["mae"] == 0.0 and math.isnan(m["cc"])
    # constant truth, imperfect prediction: r2 0.0, cc NaN
    p = t + np.linspace(-1, 1, 100).astype(np.float32)
    m = K.eval_merge_host([record(p[:40], t[:40]), record(p[40:], t[40:])])[1]
    assert m["r2"] == 0.0 and math.isnan(m["cc"]) and m["mse"] > 0
    # no records at all, and only empty ones: NaN for everything
    for recs in (np.zeros((0, 8)), np.zeros((3, 8))):
        rec, m = K.eval_merge_host(recs)
        assert m["n"] == 0.0 and all(math.isnan(m[k]) for k in ("mse", "mae", "r2", "cc"))
    # perfectly anti-correlated
    a = np.arange(10, dtype=np.float32)
    m = K.eval_merge_host([record(-a, a)])[1]
    assert abs(m["cc"] + 1.0) <= 1e-15


def test_metrics_two_ranks_gloo(tmp_path):
    from eval_ddp_worker import worker
    world = 2
    port = 35500 + (os.getpid() % 2000)
    mp.spawn(worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    res = [np.load(tmp_path / f"eval_ok{r}.npy") for r in range(world)]
    assert np.array_equal(res[0], res[1])


def test_regression_metrics_update_refuses_cpu_tensors():
    import torch
    from gan_danet_amd import RegressionMetrics
    from gan_danet_amd._lib import GandanetError
    m = RegressionMetrics("cpu")
    with pytest.raises(GandanetError):
        m.update(torch.zeros(4), torch.zeros(4))
    assert len(m) == 0
