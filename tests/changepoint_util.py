"""Generators and the brute-force oracle of the change-point tests (test_cabi_changepoint.py, test_gpu_changepoint.py).  The
oracle restates the definitions of include/gandanet.h, "Per-pixel change points", in numpy and shares no code with
csrc/changepoint_core.h: Pettitt from the full np.sign outer difference (integers, compared for equality), the float
planes from an (n candidates) x (n samples) long-double evaluation, and -- for integer-valued series -- the fitted models
in exact fractions.Fraction arithmetic.

The bound of a float plane is a forward-error bound of the fp64 evaluation the header prescribes (every operation rounded
once, sums sequential in time order), derived term by term with u = 2^-53 and g(k) = k u / (1 - k u) (Higham, Accuracy and
Stability of Numerical Algorithms, ch. 3 and 4): a sum of c terms x_i, each known to within h_i, is within
sum h_i + g(c) sum (|x_i| + h_i) of the exact sum; a product, quotient or square root adds u times its own size to what its
operands carry.  The bounds are computed from the oracle's own long-double values, never from the result under test, and
are inflated by 1 + 2^-20 for the oracle's own rounding (long double carries 11 more bits).  Where a divisor is not larger
than its own bound (an all-equal series: rss = 0) the bound is infinite and the plane is checked by the exact tests instead.

pt_p and cs_p are compared with math.exp applied to the twin's own K, n and q, relative P_RTOL (absolute where the exact
value is subnormal or 0).
"""
import math
from fractions import Fraction

import numpy as np

MAPS = ("n", "pt_k", "pt_u", "pt_index", "pt_p", "cs_q", "cs_r", "cs_index", "cs_p", "st_index", "st_mean_before", "st_mean_after",
        "st_shift", "st_rss0", "st_rss", "st_f", "tr_index", "tr_slope_before", "tr_slope_after", "tr_intercept_before",
        "tr_intercept_after", "tr_jump", "tr_rss0", "tr_rss", "tr_f")
IX = {name: k for k, name in enumerate(MAPS)}
PETTITT, CUSUM, STEP, TREND = 1, 2, 4, 8
FAMILY = {"pt": PETTITT, "cs": CUSUM, "st": STEP, "tr": TREND}
EXACT = ("n", "pt_k", "pt_u", "pt_index")                       # integer planes: equal
INDEX = ("cs_index", "st_index", "tr_index")                    # equal where the oracle's margin allows (asserted by the tests)
PROB = ("pt_p", "cs_p")
FLOAT = tuple(nm for nm in MAPS if nm not in EXACT + INDEX + PROB)
# pt_p and cs_p against math.exp of the same K, n, q, relative.  The largest error measured on an MI355X over the cases of
# test_gpu_changepoint.py::test_device_equals_host_twin_and_oracle was 2.314e-16 (the host twin's own is 0: it calls the same
# libm as math.exp); the bound is four times that, capped at 2^-40, above which something other than rounding would be wrong.
P_MEASURED = 2.314e-16
P_RTOL = min(4 * P_MEASURED, 2.0 ** -40)
P_TINY = 2.2250738585072014e-308          # below this (subnormal or 0) the check is absolute, 1e-300
FILL = -7.0
U = 2.0 ** -53
LD = np.longdouble
KINDS = ("shift", "ramp_break", "up", "equal", "ints", "two", "outlier", "gauss")
_CACHE = {}


def g(k):
    return k * U / (1.0 - k * U)


def planes_of(flags):
    return [k for k, nm in enumerate(MAPS) if k == 0 or flags & FAMILY[nm[:2]]]


def times_of(T, uniform=True):
    if uniform:
        return np.arange(T, dtype=np.float64)
    rng = np.random.default_rng(977 + T)
    return 2002.0 + np.cumsum(rng.uniform(0.02, 0.15, T))


def series(T, M, dtype=np.float64, gaps=False, seed=0, min_seg=5, kinds=KINDS):
    """(T, M): column m is of kind kinds[m % len(kinds)]; with ``gaps`` about one sample in seven is NaN, and the columns 8 ..
    11 (where M has them) keep 0, 1, 2 min_seg - 1 and 2 min_seg valid samples"""
    rng = np.random.default_rng(20261021 + 1000 * T + seed)
    k = np.arange(T, dtype=np.float64)
    x = np.empty((T, M))
    for m in range(M):
        kind = kinds[m % len(kinds)]
        gs = rng.standard_normal(T)
        at = int(rng.integers(T // 4, max(T // 4 + 1, 3 * T // 4)))
        if kind == "shift":
            col = gs + np.where(k > at, 6.0 + m % 3, 0.0)
        elif kind == "ramp_break":
            col = 0.25 * gs + np.where(k > at, 4.0 - 0.05 * (k - at), 0.08 * k)
        elif kind == "up":
            col = np.cumsum(np.abs(gs) + 0.125)
        elif kind == "equal":
            col = np.full(T, 1.5 + m)
        elif kind == "ints":
            col = rng.integers(0, 4, T).astype(np.float64)
        elif kind == "two":
            col = np.where(gs > 0.3, 2.5, -1.0)
        elif kind == "outlier":
            col = gs + np.where(k > at, 3.0, 0.0)
            col[rng.integers(0, T)] = 1e12
        else:
            col = gs
        x[:, m] = col
    x = x.astype(dtype)
    if gaps:
        x[rng.random((T, M)) < 1.0 / 7.0] = np.nan
        for m, keep in ((8, 0), (9, 1), (10, 2 * min_seg - 1), (11, 2 * min_seg)):
            if m < M:
                keep = min(keep, T)
                x[:, m] = np.nan
                x[np.sort(rng.choice(T, size=keep, replace=False)), m] = rng.standard_normal(keep).astype(dtype)
    return np.ascontiguousarray(x)


def planted(T, M, dtype=np.float64, gaps=False, seed=0):
    """real-valued series with one planted break each (a shift, or a shift with a change of slope), the break between T / 4
    and 3 T / 4: the inputs of the tests that assert the oracle's margins for every series; ``gaps``: one sample in nine NaN"""
    x = series(T, M, dtype, gaps=False, seed=seed + 17, kinds=("shift", "ramp_break"))
    if gaps:
        x[np.random.default_rng(5 + T + seed).random(x.shape) < 1.0 / 9.0] = np.nan
    return x


def columns(M):
    want = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, M // 2, M - 2, M - 1, 62, 63, 64}
    return sorted(c for c in want if 0 <= c < M)


# ---- the pieces of the bound ------------------------------------------------------------------------------------------------
def _sum(x, h, w, c):
    """(value, bound) of the sequential fp64 sum of the terms x (known to within h) selected by the 0 / 1 weights w along the
    last axis, c terms each"""
    v = (w * x).sum(-1)
    e = (w * h).sum(-1) + g(c) * (w * (np.abs(x) + h)).sum(-1)
    return v, e


def _div(a, ea, b, eb):
    with np.errstate(all="ignore"):
        v = a / b
        room = np.abs(b) - eb
        e = np.where(room > 0, (ea + np.abs(v) * eb) / np.where(room > 0, room, 1) * (1 + U) + U * np.abs(v), np.inf)
    return v, e


def _sub(a, ea, b, eb):
    v = a - b
    return v, (ea + eb) * (1 + U) + U * np.abs(v)


def _mul(a, ea, b, eb):
    v = a * b
    return v, (np.abs(a) * eb + np.abs(b) * ea + ea * eb) * (1 + U) + U * np.abs(v)


def _sqrt(a, ea):
    with np.errstate(all="ignore"):
        v = np.sqrt(a)
        lo = np.sqrt(np.maximum(a - ea, 0))
        e = np.where(lo > 0, ea / np.where(lo > 0, lo, 1) * (1 + U) + U * v, np.inf)
    return v, e


def _pick(w, a, b):
    return np.where(w > 0, a[..., None], b[..., None])


def _step_fit(y, B, c1, c2):
    """rows = candidates: (m1, e), (m2, e), (rss1, e), (rss2, e) of the two sides selected by B (1 = before) and 1 - B"""
    z = np.zeros_like(y)
    A = 1 - B
    s1, s2 = _sum(y, z, B, c1), _sum(y, z, A, c2)
    m1, m2 = _div(*s1, c1, 0.0), _div(*s2, c2, 0.0)
    d, ed = _sub(y, z, _pick(B, m1[0], m2[0]), _pick(B, m1[1], m2[1]))
    sq = _mul(d, ed, d, ed)
    return m1, m2, _sum(*sq, B, c1 + 1), _sum(*sq, A, c2 + 1)


def _line_fit(t, y, B, c1, c2):
    """rows = candidates: per side (tbar, ybar, b, rss) as (value, bound) pairs"""
    z = np.zeros_like(y)
    A = 1 - B
    tb = [_div(*_sum(t, z, W, c), c, 0.0) for W, c in ((B, c1), (A, c2))]
    yb = [_div(*_sum(y, z, W, c), c, 0.0) for W, c in ((B, c1), (A, c2))]
    dt = _sub(t, z, _pick(B, tb[0][0], tb[1][0]), _pick(B, tb[0][1], tb[1][1]))
    dy = _sub(y, z, _pick(B, yb[0][0], yb[1][0]), _pick(B, yb[0][1], yb[1][1]))
    tt, ty = _mul(*dt, *dt), _mul(*dt, *dy)
    b = [_div(*_sum(*ty, W, c + 1), *_sum(*tt, W, c + 1)) for W, c in ((B, c1), (A, c2))]
    e = _sub(*dy, *_mul(_pick(B, b[0][0], b[1][0]), _pick(B, b[0][1], b[1][1]), *dt))
    ee = _mul(*e, *e)
    rss = [_sum(*ee, W, c + 1) for W, c in ((B, c1), (A, c2))]
    return [(tb[s], yb[s], b[s], rss[s]) for s in (0, 1)]


def _add(a, b):
    v = a[0] + b[0]
    return v, (a[1] + b[1]) * (1 + U) + U * np.abs(v)


def _best(rss, erss):
    """(position of the smallest value, first on ties; margin to the runner-up; the largest bound)"""
    k = int(np.argmin(rss))
    rest = np.delete(rss, k)
    margin = float(rest.min() - rss[k]) if rest.size else np.inf
    return k, margin, float(erss.max())


def oracle_one(yraw, traw, min_seg=5, flags=15, window=None):
    """(values (25), bounds (25), margins): the planes of one series; ``bounds`` holds 0 on the integer and index planes and
    the forward-error bound on the float ones; ``margins`` maps an index plane to (margin of its selection, bound on the
    compared quantity): the index is decided wherever margin > 2 bound"""
    T = len(yraw)
    b, e = (0, T) if window is None else window
    b = min(max(b, 0), T)
    e = min(max(e, b), T)
    yv = np.asarray(yraw, dtype=np.float64)
    idx = np.array([k for k in range(b, e) if not np.isnan(yv[k])], dtype=np.int64)
    y = yv[idx].astype(LD)
    t = np.asarray(traw, dtype=np.float64)[idx].astype(LD)
    n = int(idx.size)
    val = np.full(len(MAPS), np.nan)
    err = np.zeros(len(MAPS))
    margins = {}
    for nm in ("pt_index", "cs_index", "st_index", "tr_index"):
        val[IX[nm]] = -1.0
    val[0] = n
    infl = 1.0 + 2.0 ** -20

    def put(nm, ve):
        val[IX[nm]] = float(ve[0])
        err[IX[nm]] = float(ve[1]) * infl

    if flags & PETTITT and n >= 2:
        V = np.sign(y[:, None] - y[None, :]).astype(np.int64).sum(1)
        Uk = np.cumsum(V)[:n - 1]
        k = int(np.argmax(np.abs(Uk)))
        K = int(abs(Uk[k]))
        val[IX["pt_k"]], val[IX["pt_u"]], val[IX["pt_index"]] = K, int(Uk[k]), idx[k]
        val[IX["pt_p"]] = min(1.0, 2.0 * math.exp(-(6.0 * K * K) / (float(n) ** 3 + float(n) ** 2)))
    if flags & CUSUM and n >= 1:
        z = np.zeros_like(y)
        one = np.ones_like(y)
        ybar = _div(*_sum(y, z, one, n), n, 0.0)
        d = _sub(y, z, ybar[0], ybar[1])
        tri = np.tril(np.ones((n, n), dtype=LD))
        S = _sum(d[0][None, :], d[1][None, :], tri, np.arange(1, n + 1))
        ss = _sum(*_mul(*d, *d), one, n + 1)
        sd = _sqrt(*_div(*ss, n, 0.0))
        if sd[0] > 0 and np.isfinite(sd[1]):
            a = np.abs(S[0])
            k = int(np.argmax(a))
            rest = np.delete(a, k)
            margins["cs_index"] = (float(a[k] - rest.max()) if rest.size else np.inf, float(S[1].max()) * infl)
            es = S[1].max()
            rn = (np.sqrt(LD(n)), U * np.sqrt(LD(n)))
            put("cs_q", _div(*_div(a[k], es, *sd), *rn))
            rng = _sub(max(S[0].max(), 0), es, min(S[0].min(), 0), es)
            put("cs_r", _div(*_div(*rng, *sd), *rn))
            val[IX["cs_index"]] = idx[k]
            q = val[IX["cs_q"]]
            val[IX["cs_p"]] = cusum_p(q)
    nc = n - 2 * min_seg + 1
    if nc > 0 and flags & (STEP | TREND):
        ks = np.arange(min_seg - 1, min_seg - 1 + nc)
        B = (np.arange(n)[None, :] <= ks[:, None]).astype(LD)
        c1, c2 = (ks + 1).astype(LD), (n - ks - 1).astype(LD)
        Y, Tm = np.broadcast_to(y, B.shape), np.broadcast_to(t, B.shape)
        whole = np.ones((1, n), dtype=LD)
        if flags & STEP:
            m1, m2, r1, r2 = _step_fit(Y, B, c1, c2)
            rss = _add(r1, r2)
            k, margin, worst = _best(rss[0], rss[1])
            margins["st_index"] = (margin, worst * infl)
            r0 = _step_fit(y[None, :], whole, LD(n), LD(1))[2]
            rss0 = (r0[0][0], r0[1][0])
            val[IX["st_index"]] = idx[ks[k]]
            pk = lambda p: (p[0][k], p[1][k])
            put("st_mean_before", pk(m1))
            put("st_mean_after", pk(m2))
            put("st_shift", _sub(*pk(m2), *pk(m1)))
            put("st_rss0", rss0)
            put("st_rss", pk(rss))
            put("st_f", _div(*_sub(*rss0, *pk(rss)), *_div(*pk(rss), n - 2, 0.0)))
        if flags & TREND:
            s1, s2 = _line_fit(Tm, Y, B, c1, c2)
            rss = _add(s1[3], s2[3])
            k, margin, worst = _best(rss[0], rss[1])
            margins["tr_index"] = (margin, worst * infl)
            w0 = _line_fit(t[None, :], y[None, :], whole, LD(n), LD(1))[0]
            rss0 = (w0[3][0][0], w0[3][1][0])
            val[IX["tr_index"]] = idx[ks[k]]
            pk = lambda p: (p[0][k], p[1][k])
            line = []
            for s, side in ((s1, "before"), (s2, "after")):
                tb, yb, bb = pk(s[0]), pk(s[1]), pk(s[2])
                a = _sub(*yb, *_mul(*bb, *tb))
                put("tr_slope_" + side, bb)
                put("tr_intercept_" + side, a)
                line.append((a, bb))
            tk, tk1 = t[ks[k]], t[ks[k] + 1]
            tm = ((tk + tk1) * LD(0.5), U * abs(tk + tk1) * 0.5)
            at = [_add(a, _mul(*bb, *tm)) for a, bb in line]
            put("tr_jump", _sub(*at[1], *at[0]))
            put("tr_rss0", rss0)
            put("tr_rss", pk(rss))
            half = _sub(*rss0, *pk(rss))
            put("tr_f", _div(half[0] / 2, half[1] / 2, *_div(*pk(rss), n - 4, 0.0)))
    return val, err, margins


def cusum_p(q):
    if q != q:
        return q
    if q < 0.3:
        return 1.0
    s = 0.0
    for j in range(1, 21):
        e = math.exp(-2.0 * (j * j) * q * q)
        s = s + e if j & 1 else s - e
    return min(1.0, max(0.0, 2.0 * s))


def pettitt_p(K, n):
    return min(1.0, 2.0 * math.exp(-(6.0 * K * K) / (float(n) ** 3 + float(n) ** 2)))


def oracle(x, t, cols, min_seg=5, flags=15, mask=None, window=None):
    """values (25, len(cols)), bounds (25, len(cols)) and the list of margins of the columns ``cols`` of the (T, M) array x"""
    val = np.empty((len(MAPS), len(cols)))
    err = np.empty((len(MAPS), len(cols)))
    margins = []
    for j, m in enumerate(cols):
        w = None if window is None else (int(window[0][m]), int(window[1][m]))
        if mask is not None and not mask[m]:
            w = (0, 0)
        v, e, mg = oracle_one(x[:, m], t, min_seg, flags, w)
        val[:, j], err[:, j] = v, e
        margins.append(mg)
    return val, err, margins


def reference(key, x, t, min_seg=5, flags=15):
    """(host twin on every column, the oracle's columns, values, bounds, margins), computed once per ``key``, never changed"""
    if key not in _CACHE:
        from gan_danet_amd import kern as K
        cols = columns(x.shape[1])
        host = K.change_point_host(x, t, None, None, min_seg, flags, out=np.full((len(MAPS), x.shape[1]), FILL))
        host.setflags(write=False)
        val, err, margins = oracle(x, t, cols, min_seg, flags)
        val.setflags(write=False)
        err.setflags(write=False)
        _CACHE[key] = (host, cols, val, err, margins)
    return _CACHE[key]


def _decided(margin_of, nm):
    return nm in margin_of and margin_of[nm][0] > 2 * margin_of[nm][1]


def assert_matches(got, val, err, margins, flags, what, need_margin=False):
    """``got`` (25, C) against the oracle's values and bounds: integer planes equal; float planes within their bound (NaN
    where the oracle has NaN, +-inf where it has that); an index plane equal wherever its margin exceeds twice its bound --
    ``need_margin`` asserts that it does, for every series.  Returns the largest error as a fraction of its bound."""
    worst = 0.0
    for k in planes_of(flags):
        nm = MAPS[k]
        if nm in PROB:
            continue
        for j in range(val.shape[1]):
            gv, wv, be = got[k, j], val[k, j], err[k, j]
            if nm in EXACT:
                assert gv == wv or (gv != gv and wv != wv), (what, nm, j, gv, wv)
            elif nm in INDEX:
                if nm in margins[j]:
                    margin, bound = margins[j][nm]
                    decided = margin > 2 * bound
                    assert decided or not need_margin, (what, nm, j, "margin", margin, "bound", bound)
                    if decided:
                        assert gv == wv, (what, nm, j, gv, wv)
                else:
                    assert gv == -1.0 and wv == -1.0, (what, nm, j, gv, wv)
            elif nm[:2] in ("st", "tr") and "rss" not in nm and nm[-2:] != "_f" and not _decided(margins[j], nm[:2] + "_index"):
                continue                                                # the parameters of a break that rounding may move
            elif wv != wv:
                # the oracle has no value: no candidate, or 0 / 0 exactly; a bound of inf means the quotient is not decided
                assert gv != gv or be == np.inf or not np.isfinite(be), (what, nm, j, gv)
            elif np.isfinite(be):
                assert abs(gv - wv) <= be, (what, nm, j, gv, wv, abs(gv - wv), be)
                if be > 0:
                    worst = max(worst, abs(gv - wv) / be)
    return worst


def p_error(got):
    """the largest error of pt_p and cs_p against math.exp of the planes' own K, n and q, as a fraction of the bound (relative
    P_RTOL; absolute 1e-300 where the exact value is subnormal or 0), and the largest relative error itself"""
    worst = worst_rel = 0.0
    for j in range(got.shape[1]):
        pairs = []
        if got[IX["pt_k"], j] == FILL:
            pass
        elif got[IX["pt_k"], j] == got[IX["pt_k"], j]:
            pairs.append((got[IX["pt_p"], j], pettitt_p(got[IX["pt_k"], j], got[0, j])))
        else:
            assert got[IX["pt_p"], j] != got[IX["pt_p"], j]
        q = got[IX["cs_q"], j]
        if q == q and q != FILL:
            pairs.append((got[IX["cs_p"], j], cusum_p(q)))
        for pv, want in pairs:
            assert pv != FILL, "the family's K or q was written but its p was not"
            if want < P_TINY:
                worst = max(worst, abs(pv - want) / 1e-300)
            else:
                rel = abs(pv - want) / want
                worst_rel = max(worst_rel, rel)
                worst = max(worst, rel / P_RTOL)
    return worst, worst_rel


# ---- exact oracle for integer-valued series ----------------------------------------------------------------------------------
def exact_fits(y, t, min_seg):
    """the exact (Fraction) rss of STEP and TREND at every candidate of a series without NaN: two lists of (k, rss)"""
    y = [Fraction(float(v)) for v in y]
    t = [Fraction(float(v)) for v in t]
    n = len(y)

    def step(seg):
        m = sum(seg) / len(seg)
        return sum((v - m) ** 2 for v in seg)

    def line(ts, ys):
        tb, yb = sum(ts) / len(ts), sum(ys) / len(ys)
        stt = sum((a - tb) ** 2 for a in ts)
        b = sum((a - tb) * (v - yb) for a, v in zip(ts, ys)) / stt
        return sum(((v - yb) - b * (a - tb)) ** 2 for a, v in zip(ts, ys))

    st, tr = [], []
    for k in range(min_seg - 1, n - min_seg):
        st.append((k, step(y[:k + 1]) + step(y[k + 1:])))
        tr.append((k, line(t[:k + 1], y[:k + 1]) + line(t[k + 1:], y[k + 1:])))
    return st, tr, step(y), line(t, y)


# ---- binary segmentation in plain numpy ----------------------------------------------------------------------------------------
def segmentation(one, T, max_breaks, accept, score):
    """the breaks of one series by the level rule of ``change_points``: ``one(b, e)`` -> (index, stat) of the window [b, e);
    ``accept(stat)``; ``score(stat)`` larger = stronger"""
    open_, found = [(0, T)], []
    for _ in range(max_breaks):
        res = [one(b, e) for b, e in open_]
        cand = [(score(s), -j) for j, (i, s) in enumerate(res) if i >= 0 and accept(s)]
        cand.sort(reverse=True)
        take = sorted(-j for _, j in cand[:max_breaks - len(found)])
        if not take:
            break
        nxt = []
        for j in take:
            b, e = open_[j]
            i = res[j][0]
            found.append(i)
            nxt += [(b, i + 1), (i + 1, e)]
        open_ = nxt
    return sorted(found)
