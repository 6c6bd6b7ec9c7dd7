"""CPU: the SSA entry points of the C ABI (include/gandanet.h, "Singular spectrum analysis") are declared and bound, reject
every bad argument before any launch, and the host twin -- the per-series function of csrc/ssa.hip run with one lane over
csrc/ssa_core.h -- matches the numpy oracle of tests/ssa_util.py: integer-valued planes equal, eigenvalues within the Weyl
bound, components and groups within the gap-scaled bound wherever the oracle's margin exceeds twice the eigenvalue bound
(asserted for every planted series), the identities that need no oracle, planted recovery through ssa_fill, and the edge
series.  Each test prints its largest error over the un-scaled bound (python -m pytest -s): ssa_util.py records them.
The eigenvectors come from the optional `evec` output of gd_ssa_decompose."""
import os
import re

import numpy as np
import pytest
import torch

import ssa_util as U

NAMES = ("gd_ssa_decompose", "gd_ssa_decompose_host", "gd_ssa_fill", "gd_ssa_fill_host")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def _K():
    from gan_danet_amd import kern
    return kern


def test_ssa_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import build, kern, ssa
    L, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gandanet.h")).read()
    assert "Singular spectrum analysis" in src
    for name in NAMES:
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"int " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]), name
    for fn in ("ssa_decompose", "ssa_decompose_host", "ssa_fill", "ssa_fill_host"):
        assert hasattr(kern, fn)
    for name, val in (("MAX_M", 64), ("MAX_T", 2048), ("MAX_RANK", 16), ("MAX_ITER", 200)):
        assert f"#define GD_SSA_{name} {val}" in src and getattr(L, "SSA_" + name) == val
    assert f"#define GD_SSA_MAX_SWEEPS {L.SSA_MAX_SWEEPS}" in src and f"#define GD_SSA_CHUNK {L.SSA_CHUNK}" in src
    flat = " ".join(src.split())
    for k, name in enumerate(L.SSA_MAPS):
        assert f"GD_SSA_{name.upper()} = {k}," in flat
    assert f"GD_SSA_MAPS = {len(L.SSA_MAPS)}" in src and L.SSA_MAPS == U.MAPS
    assert "GD_SSA_BK = 0, GD_SSA_VG = 1" in src and L.SSA_METHODS == {"bk": 0, "vg": 1}
    for name, bit in L.SSA_FLAGS.items():
        assert f"GD_SSA_FLAG_{name.upper()} = {bit}" in flat
    assert (U.MASKED, U.FEW, U.CONSTANT, U.NONFINITE, U.GAPS, U.SWEEPS, U.ITER) == tuple(L.SSA_FLAGS.values())
    assert "ssa.hip" in build.SOURCES
    assert gan_danet_amd.ssa is ssa
    for name in ("SSAResult", "SSAFill", "ssa_decompose", "ssa_fill"):
        assert getattr(gan_danet_amd, name) is getattr(ssa, name)
    doc = " ".join(ssa.ssa_fill.__doc__.lower().split())
    assert "mean is held fixed" in doc and "uncertainty" in doc and "not estimated" in doc and "longer than" in doc
    assert "ssa_fill" in ssa.ssa_decompose.__doc__ and U.MEASURED_SWEEPS < L.SSA_MAX_SWEEPS


def test_ssa_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses) are not touched"""
    L, lib = _lib()
    a, b, c, d = 0x1000, 0x2000, 0x3000, 0x4000
    dec = ("x", "dtype", "T", "P", "window", "rank", "method", "mask", "eig", "maps", "rc", "evec")
    fil = ("x", "dtype", "T", "P", "window", "rank", "method", "mask", "tol", "max_iter", "min_valid", "filled", "eig", "maps")
    good = dict(x=a, dtype=1, T=181, P=7, window=24, rank=6, method=0, mask=None, eig=b, maps=c, rc=None, evec=None, tol=1e-3, max_iter=20,
                min_valid=48, filled=d)
    shared = [(dict(x=None), "null"), (dict(eig=None), "null"), (dict(maps=None), "null"), (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"),
              (dict(T=46), "T outside"), (dict(T=2049), "T outside"), (dict(T=0), "T outside"), (dict(T=2, window=2), "T outside"),
              (dict(window=1), "window"), (dict(window=65, T=200), "window"), (dict(window=0), "window"), (dict(window=-4), "window"),
              (dict(rank=0), "rank"), (dict(rank=17), "rank"), (dict(rank=5, window=4), "rank"), (dict(rank=-1), "rank"),
              (dict(method=2), "method"), (dict(method=-1), "method"), (dict(P=0), "M_pixels <= 0"), (dict(P=-3), "M_pixels <= 0"),
              (dict(P=1 << 31), "too many"), (dict(x=a + 4), "aligned"), (dict(x=a + 2, dtype=0), "aligned"), (dict(eig=b + 4), "aligned"),
              (dict(maps=c + 4), "aligned")]
    only_dec = [(dict(rc=d + 4), "aligned"), (dict(evec=d + 4), "aligned")]
    only_fil = [(dict(filled=None), "null"), (dict(filled=d + 4), "aligned"), (dict(max_iter=0), "max_iter"), (dict(max_iter=201), "max_iter"),
                (dict(max_iter=-1), "max_iter"), (dict(tol=0.0), "tol"), (dict(tol=-1e-3), "tol"), (dict(tol=float("nan")), "tol"),
                (dict(tol=float("inf")), "tol"), (dict(min_valid=1), "min_valid"), (dict(min_valid=2049), "min_valid")]
    for host in (False, True):
        for order, fn, rules in ((dec, "gd_ssa_decompose", shared + only_dec), (fil, "gd_ssa_fill", shared + only_fil)):
            f = getattr(lib, fn + ("_host" if host else ""))
            for kw, word in rules:
                v = dict(good, **kw)
                args = [v[k] for k in order]
                rc = f(*args) if host else f(*args, None)
                assert rc == -1, (fn, host, kw, rc)
                assert word in L.last_error(), (fn, host, kw, L.last_error())
    K = _K()
    x = U.series(24)
    with pytest.raises(L.GandanetError):
        K.ssa_decompose_host(x, 5, 3, "broomhead")
    with pytest.raises(L.GandanetError):
        K.ssa_decompose_host(x.astype(np.int32), 5, 3)
    with pytest.raises(L.GandanetError):
        K.ssa_fill_host(x, 5.0, 3)
    with pytest.raises(L.GandanetError):
        K.ssa_fill_host(x, 5, 3, "bk", None, 1e-3, 20.0)


@pytest.mark.parametrize("T", U.TS)
def test_host_twin_against_the_oracle(T):
    """every admissible window, both methods, fp32 and fp64 storage, the eight kinds of series of ssa_util.series"""
    K = _K()
    w_eig = w_rc = 0.0
    sweeps = 0
    for M in [m for m in U.MS if T >= 2 * m - 1]:
        r = min(M, 16)
        for method in U.METHODS:
            for dtype in (np.float64, np.float32):
                x = U.series(T, dtype)
                eig, maps, rc = K.ssa_decompose_host(x, M, r, method, None, True)
                sweeps = max(sweeps, int(maps[U.IX["sweeps"]].max()))
                for m in range(x.shape[1]):
                    o = U.decompose(x[:, m], M, method, maps[U.IX["mean"], m])
                    what = (T, M, method, np.dtype(dtype).name, m)
                    assert (maps[U.IX["n"], m], maps[U.IX["n_gaps"], m], maps[U.IX["flags"], m]) == (o["n"], o["n_gaps"], o["flags"]), what
                    assert o["flags"] == 0, what
                    assert abs(maps[U.IX["mean"], m] - o["mean"]) <= 4 * U.EPS * T * np.abs(x[:, m]).max(), what
                    assert abs(maps[U.IX["sd"], m] - o["sd"]) <= 4 * U.EPS * T * np.abs(x[:, m]).max(), what
                    ratio = np.abs(eig[:, m] - o["eig"][:r]).max() / o["eig_bound"]
                    w_eig = max(w_eig, ratio)
                    assert ratio <= U.G_EIG, (what, ratio)
                    assert abs(maps[U.IX["trace"], m] - o["trace"]) <= M * U.G_EIG * o["eig_bound"], what
                    for k in range(r):                                  # single components, where their eigenvalue is isolated
                        if o["gap"][k] > 2 * U.G_EIG * o["eig_bound"]:
                            ratio = np.abs(rc[k, :, m] - o["rc"][k]).max() / U.rc_bound(o, M, o["gap"][k])
                            w_rc = max(w_rc, ratio)
                            assert ratio <= U.G_RC, (what, k, ratio)
                    for g in ((2,), (6,)):                              # leading groups: the sinusoid's pair, the planted six
                        q = g[0]
                        planted = (q == 2 and m == 4) or (q == 6 and m == 0)
                        if q >= M or q > r or not planted:
                            continue
                        gap = o["eig"][q - 1] - o["eig"][q]
                        assert gap > 2 * U.G_EIG * o["eig_bound"], (what, q, gap)          # the margin holds for every planted series
                        ratio = np.abs(rc[:q, :, m].sum(0) - o["rc"][:q].sum(0)).max() / U.rc_bound(o, M, gap)
                        w_rc = max(w_rc, ratio)
                        assert ratio <= U.G_RC, (what, "group", q, ratio)
    assert sweeps <= U.MEASURED_SWEEPS and 2 * U.MEASURED_SWEEPS <= _lib()[0].SSA_MAX_SWEEPS      # never reached, with room
    print(f"T = {T}: eigenvalues at most {w_eig:.3f}, components and groups at most {w_rc:.3f} of the un-scaled bound; {sweeps} sweeps at most")


@pytest.mark.parametrize("method", U.METHODS)
def test_host_twin_identities(method):
    """with rank = M <= 16: the eigenvalues add up to the trace plane (M additions: M eps trace); the M components add up to the
    centred series (every sample passes through 2 M-term products with an orthogonal matrix that Jacobi leaves orthogonal to
    a few M eps: (M^2 + 8 M) eps max|y|); "bk": K times the eigenvalues are the squared singular values of the trajectory
    matrix from numpy.linalg.svd, within the eigenvalue bound times K.  With the eigenvectors (`evec`): every entry of
    E^T E - I within G_ORTH * sweeps * M * eps (a column takes M - 1 rotations a sweep, each orthogonal to a few eps), and
    ||C e - lambda e||_2, against C of the twin's own centred series, within G_RESID * (the backward error of the
    eigenvalues, eps sqrt(M) ||C||_F, plus 2 ||C||_F times the orthogonality unit: the distance of E to an exactly
    orthogonal matrix)"""
    K = _K()
    worst = w_orth = w_res = 0.0
    for T, M in ((3, 2), (9, 5), (24, 12), (47, 16), (181, 16), (65, 3)):
        for dtype in (np.float64, np.float32):
            x = U.series(T, dtype)
            eig, maps, rc, evec = K.ssa_decompose_host(x, M, M, method, None, True, True)
            assert evec.shape == (M, M, x.shape[1])
            for m in range(x.shape[1]):
                o = U.decompose(x[:, m], M, method, maps[U.IX["mean"], m])
                E = evec[:, :, m].T                                       # E[j][k]
                orth_unit = maps[U.IX["sweeps"], m] * M * U.EPS
                ratio = np.abs(E.T @ E - np.eye(M)).max() / orth_unit
                w_orth = max(w_orth, ratio)
                assert ratio <= U.G_ORTH, (T, M, m, "orthogonality", ratio)
                res = np.linalg.norm(o["C"] @ E - E * eig[:, m][None, :], axis=0).max()
                ratio = res / (o["eig_bound"] + 2.0 * np.linalg.norm(o["C"]) * orth_unit)
                w_res = max(w_res, ratio)
                assert ratio <= U.G_RESID, (T, M, m, "residual", ratio)
                assert np.all(E[np.abs(E).argmax(0), np.arange(M)] > 0)         # the sign rule
                tr = maps[U.IX["trace"], m]
                assert abs(eig[:, m].sum() - tr) <= M * U.EPS * abs(tr), (T, M, m)
                y = x[:, m].astype(np.float64) - maps[U.IX["mean"], m]
                err = np.abs(rc[:, :, m].sum(0) - y).max() / ((M * M + 8 * M) * U.EPS * np.abs(y).max())
                worst = max(worst, err)
                assert err <= 1.0, (T, M, m, err)
                if method == "bk":
                    Kk = T - M + 1
                    X = np.stack([y[i:i + Kk] for i in range(M)], 1)
                    sv = np.linalg.svd(X, compute_uv=False)
                    assert np.abs(eig[:, m] * Kk - sv ** 2).max() <= U.G_EIG * o["eig_bound"] * Kk, (T, M, m)
    print(f"{method}: the components add up to the series within {worst:.3f} of the bound; E^T E - I at most {w_orth:.3f} of sweeps M eps; "
          f"||C e - lambda e|| at most {w_res:.3f} of its un-scaled bound")


def _gappy(T, P, dtype=np.float64):
    x = U.planted_values(T, P).astype(dtype)
    truth = x.copy()
    for m in range(P):
        x[U.grace_gaps(T, m), m] = np.nan
    return x, truth


def test_planted_recovery_and_iterations():
    """noiseless trend + annual + semi-annual: rank <= 6, so eigenvalues 7 .. are rounding relative to the trace, and ssa_fill
    with rank 6 over the GRACE pattern (11 steps in a row plus scattered single steps) returns the planted values as closely
    as the oracle does (MARGIN times the oracle's own distance); iterations are equal wherever no iteration of the oracle has
    its change within ITERATE_RTOL * sd of tol * sd; the twin's iterate stays within ITERATE_RTOL * sd of the oracle's"""
    K = _K()
    T, M, P = 181, 24, 4
    full = U.planted_values(T, P)
    eig, maps, _ = K.ssa_decompose_host(full, M, 16, "bk")
    for m in range(P):
        o = U.decompose(full[:, m], M, "bk", maps[U.IX["mean"], m])
        assert np.abs(eig[6:, m]).max() <= U.G_EIG * o["eig_bound"] and eig[5, m] > 1e3 * U.G_EIG * o["eig_bound"]
    worst = 0.0
    for dtype in (np.float64, np.float32):
        x, truth = _gappy(T, P, dtype)
        for method, tol in (("bk", 1e-6), ("vg", 1e-6), ("bk", 1e-3)):
            filled, eig, maps = K.ssa_fill_host(x, M, 6, method, None, tol, 200)
            for m in range(P):
                o = U.fill(x[:, m], M, 6, method, tol, 200)
                what = (np.dtype(dtype).name, method, tol, m)
                assert (maps[U.IX["n"], m], maps[U.IX["n_gaps"], m], maps[U.IX["flags"], m]) == (o["n"], o["n_gaps"], o["flags"]), what
                own = np.abs(o["filled"] - truth[:, m].astype(np.float64)).max()
                assert np.abs(filled[:, m] - truth[:, m].astype(np.float64)).max() <= U.MARGIN * own, what
                if method == "bk" and tol == 1e-6:
                    assert own <= 1e-4 * o["sd"], what                    # the planted values do come back
                dist = np.abs(filled[:, m] - o["filled"]).max() / o["sd"]
                worst = max(worst, dist)
                assert dist <= U.ITERATE_RTOL, (what, dist)
                if all(abs(c - t) > U.ITERATE_RTOL * o["sd"] for c, t in o["changes"]):
                    assert maps[U.IX["iterations"], m] == o["iterations"], what
                valid = ~np.isnan(x[:, m])
                assert np.array_equal(filled[valid, m], x[valid, m].astype(np.float64))
                assert maps[U.IX["sweeps"], m] <= U.MEASURED_SWEEPS
    print(f"planted fill: the twin's iterate within {worst:.3e} sd of the oracle's")


def test_edge_series():
    """all NaN, one valid sample, constant, n = min_valid - 1 and n = min_valid, a gap at the first and at the last step, a gap
    longer than M, every second sample missing, an infinity, a masked pixel: the documented NaN, flag or value"""
    K = _K()
    T, M, r = 47, 5, 3
    base = U.planted_values(T, 12) + 0.1 * np.random.default_rng(3).standard_normal((T, 12))
    x = base.copy()
    x[:, 0] = np.nan
    x[1:, 1] = np.nan
    x[:, 2] = 7.25
    x[2 * M - 1:, 3] = np.nan                      # n = 2 M - 1 = min_valid - 1
    x[2 * M:, 4] = np.nan                          # n = min_valid
    x[[0, T - 1], 5] = np.nan
    x[10:10 + M + 3, 6] = np.nan
    x[1::2, 7] = np.nan
    x[20, 8] = np.inf
    x[5, 9] = np.nan                               # an ordinary gap, masked out below
    x[30, 10] = np.nan                             # one ordinary gap; column 11 is complete
    mask = np.ones(12, dtype=np.uint8)
    mask[9] = 0
    filled, eig, maps = K.ssa_fill_host(x, M, r, "bk", mask, 1e-3, 20)
    flags, n, ng = maps[U.IX["flags"]].astype(int), maps[U.IX["n"]], maps[U.IX["n_gaps"]]
    assert list(flags[[0, 1, 2, 3, 8, 9]]) == [U.FEW, U.FEW | U.CONSTANT, U.CONSTANT, U.FEW, U.NONFINITE, U.MASKED]
    assert list(n[[0, 1, 2, 3, 4, 9]]) == [0, 1, T, 2 * M - 1, 2 * M, 0] and ng[9] == 0 and ng[0] == T and ng[8] == 0
    bad = [0, 1, 2, 3, 8, 9]
    assert np.isnan(filled[:, bad]).all() and np.isnan(eig[:, bad]).all()
    assert np.isnan(maps[U.IX["trace"]:U.IX["flags"], bad]).all()
    assert np.isnan(maps[U.IX["mean"], [0, 8, 9]]).all() and maps[U.IX["mean"], 2] == 7.25 and maps[U.IX["sd"], 2] == 0.0
    ok = [4, 5, 6, 7, 10, 11]
    assert not (flags[ok] & ~U.ITER).any() and np.isfinite(filled[:, ok]).all() and np.isfinite(eig[:, ok]).all()
    assert maps[U.IX["iterations"], 11] == 0 and maps[U.IX["last_change"], 11] == 0 and np.array_equal(filled[:, 11], x[:, 11])
    for m in ok:
        o = U.fill(x[:, m], M, r, "bk", 1e-3, 20)
        valid = ~np.isnan(x[:, m])
        assert np.array_equal(filled[valid, m], x[valid, m]) and (n[m], ng[m], flags[m]) == (o["n"], o["n_gaps"], o["flags"]), m
        assert np.abs(filled[:, m] - o["filled"]).max() <= 1e-6 * o["sd"], m      # 20 iterations at tol 1e-3: far above rounding
        assert maps[U.IX["sweeps"], m] <= U.MEASURED_SWEEPS
    # the same columns through ssa_decompose: a gap is refused with its own flag
    eig, maps, rc = K.ssa_decompose_host(x, M, r, "vg", mask, True)
    flags = maps[U.IX["flags"]].astype(int)
    assert list(flags) == [U.GAPS, U.CONSTANT | U.GAPS, U.CONSTANT, U.GAPS, U.GAPS, U.GAPS, U.GAPS, U.GAPS, U.NONFINITE, U.MASKED, U.GAPS, 0]
    assert np.isnan(eig[:, :11]).all() and np.isnan(rc[:, :, :11]).all() and np.isfinite(rc[:, :, 11]).all()
    # min_valid is an argument: 2 lets the short series through, T + 1 refuses every series
    f2 = K.ssa_fill_host(x[:, 3:5], M, r, "bk", None, 1e-3, 20, 2)
    assert np.isfinite(f2[0]).all() and not (f2[2][U.IX["flags"]].astype(int) & U.FEW).any()
    f3 = K.ssa_fill_host(x[:, 10:12], M, r, "bk", None, 1e-3, 20, T + 1)
    assert np.isnan(f3[0]).all() and list(f3[2][U.IX["flags"]].astype(int)) == [U.FEW, U.FEW]


def test_cpu_and_bad_arguments_are_refused():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import ssa as S
    x = torch.zeros(24, 4, 6, dtype=torch.float64)
    for call in (lambda: S.ssa_decompose(x, 5), lambda: S.ssa_fill(x, 5), lambda: S.ssa_decompose(x.numpy(), 5),
                 lambda: S._input(x, 5, 3, "bk", "ssa_fill")):
        with pytest.raises(L.GandanetError):
            call()
    for v, lo, hi in ((1, 2, 64), (65, 2, 64), (True, 1, 4), (3.0, 1, 4)):
        with pytest.raises(L.GandanetError):
            S._int(v, lo, hi, "ssa_fill", "window")
