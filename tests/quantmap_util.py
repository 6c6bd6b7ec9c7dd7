"""The oracle of the bias-correction tests (test_cabi_quantmap.py, test_gpu_quantmap.py), numpy only: np.nanquantile in a
loop over pixels and calendar slots, np.interp, and the two kinds and two extrapolations written out.  The reference
project has no quantile mapping, so there is no fixture to record from it: numpy is the reference, and the claim is
EQUALITY -- ``same`` compares bit patterns (any NaN equals any NaN; -0.0 differs from +0.0).  This file holds no bound but
one, for the one property that is not an equality:

``shift_bound`` -- qdm of x = z + c through a map fitted on (z, o), against eqm of z, plus c.  In exact arithmetic the own
table of x is the model table m shifted by c, so tau is the position of z in m and qdm(x) = eqm(z) + c.  In fp64, with
u = 2^-53, A >= every magnitude involved (|z|, |o|, |x|, |c| and their sums), h = 1 / (Q - 1), S = the largest slope
(o[j+1] - o[j]) / (m[j+1] - m[j]) of the transfer function over all brackets, and the brackets m[j+1] - m[j] >= 1e6 u A
(asserted by the test on the oracle's own tables, so that a perturbed bracket width changes a slope by less than 2):
  * a node is _lerp of two samples: d = b - a (u |d| <= 2 u A), its product with g or 1 - g and the sum: <= 8 u A; the own
    nodes w of x = fl(z + c) (u A) therefore differ from m + c by dw <= 8 u A + 8 u A + u A = 17 u A;
  * first interpolation, tau = interp(x, w, p), slope h / (w[j+1] - w[j]): the node and abscissa perturbations move it by
    <= 2 h (2 dw + u A) / (m[j+1] - m[j]) = 70 u A h / dm, and its own rounding (slope 3 u, difference u, product u, sum u
    on a value <= 1) by <= 6 u;
  * second and third, interp(tau, p, o) and interp(tau, p, m), slopes do / h and dm / h: the error of tau becomes
    70 u A (do / dm) + 6 u do / h and 70 u A + 6 u dm / h, with do, dm <= 2 A: <= 70 u A (S + 1) + 24 u A (Q - 1); their own
    rounding is <= 12 u A each (11 u A: 5 u on a term <= 2 A, u A on the sum);
  * x + (o - m): <= 5 u A; eqm's own interpolation: 12 u A; the test's fl(eqm + c): 2 u A.
A bracket that tau's error crosses changes nothing: the functions are continuous and S is the maximum over all brackets.
Sum: u A (70 (S + 1) + 24 (Q - 1) + 43).
"""
import numpy as np

U64 = 2.0 ** -53


def nodes(Q):
    """the node probabilities of a quantile map of Q nodes"""
    return np.arange(Q, dtype=np.float64) / float(Q - 1)


def same(a, b):
    """bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    iv = np.uint64 if a.dtype == np.float64 else np.uint32
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(iv)[~na], b.view(iv)[~nb]))


def quantiles(x, q, period=1, phase=0, baseline=None, mask=None, x2=None, min_samples=1):
    """(nodes (Q, period, M) float64, n (period, M) int32) of the (T, M) array x"""
    T, M = x.shape
    b0, b1 = (0, T) if baseline is None else baseline
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    out = np.full((q.size, period, M), np.nan)
    n = np.zeros((period, M), dtype=np.int32)
    t = np.arange(T)
    for s in range(period):
        steps = t[(t >= b0) & (t < b1) & ((t + phase) % period == s)]
        for m in range(M):
            if mask is not None and not mask[m]:
                continue
            v = x[steps, m].astype(np.float64)
            keep = ~np.isnan(v)
            if x2 is not None:
                keep &= ~np.isnan(x2[steps, m])
            v = v[keep]
            n[s, m] = v.size
            if v.size >= max(min_samples, 1):
                out[:, s, m] = np.nanquantile(v, q)
    return out, n


def fit(model, obs, Q, period=12, phase=0, baseline=None, mask=None, pairwise=True, min_samples=2):
    """(model_q, obs_q (period, Q, M), n_model, n_obs (period, M)) of two (T, M) arrays"""
    mq, nm = quantiles(model, nodes(Q), period, phase, baseline, mask, obs if pairwise else None, min_samples)
    oq, no = quantiles(obs, nodes(Q), period, phase, baseline, mask, model if pairwise else None, min_samples)
    return mq.transpose(1, 0, 2).copy(), oq.transpose(1, 0, 2).copy(), nm, no


def eqm_one(x, mq, oq, extrapolate):
    if np.isnan(x) or np.isnan(mq[0]) or np.isnan(oq[0]):
        return np.nan
    for e, outside in ((0, x < mq[0]), (-1, x > mq[-1])):
        if outside:
            return oq[e] if extrapolate == "clip" else x + (oq[e] - mq[e])
    return np.interp(x, mq, oq)


def qdm_one(x, mq, oq, own, p):
    if np.isnan(x) or np.isnan(mq[0]) or np.isnan(oq[0]):
        return np.nan
    tau = np.interp(x, own, p)
    return x + (np.interp(tau, p, oq) - np.interp(tau, p, mq))


def apply(x, mq, oq, kind="eqm", extrapolate="constant", phase=0, t0=0):
    """x (T, f H, f W) through the (period, Q, H, W) tables, in the dtype of x"""
    period, Q, H, W = mq.shape
    T, Hx, Wx = x.shape
    f = Hx // H
    assert (Hx, Wx) == (f * H, f * W)
    ph = (t0 + phase) % period
    xd = x.astype(np.float64)
    out = np.empty((T, Hx, Wx))
    if kind == "qdm":
        p = nodes(Q)
        own, _ = quantiles(xd.reshape(T, -1), p, period, ph)
        own = own.reshape(Q, period, Hx, Wx)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            s = (t + ph) % period
            for h in range(Hx):
                for w in range(Wx):
                    a, b = mq[s, :, h // f, w // f], oq[s, :, h // f, w // f]
                    out[t, h, w] = eqm_one(xd[t, h, w], a, b, extrapolate) if kind == "eqm" else qdm_one(xd[t, h, w], a, b, own[:, s, h, w], p)
    return out.astype(x.dtype)


def shift_bound(A, S, Q):
    """the bound of the module docstring"""
    return U64 * A * (70.0 * (S + 1.0) + 24.0 * (Q - 1) + 43.0)


# ---- the data of both test files -----------------------------------------------------------------------------------------------
def cube(T, M, seed, dtype=np.float64, nan_frac=0.0, quantised=False, specials=False):
    """a (T, M) cube of N(0, 1) values; ``quantised``: multiples of 0.25 (ties; + 0.0 turns every -0.0 into +0.0, as the order
    of the two zeros in a sample is not numpy's to define); ``nan_frac``: that share of NaNs at seeded positions;
    ``specials`` (M >= 3): series 1 all NaN, series 2 constant"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, M)) * 3.0
    if quantised:
        x = np.round(x * 4.0) / 4.0 + 0.0
    x = x.astype(dtype)
    if nan_frac:
        x[rng.random((T, M)) < nan_frac] = np.nan
    if specials:
        x[:, 1] = np.nan
        x[:, 2] = dtype(1.75)
    return x


Q_LIST = (0.0, 0.5, 1.0, 0.1, 0.37, 0.9, 1.0 / 3.0)

# name -> (T, M, period, phase, baseline, dtype, kwargs of cube, masked pixel or None, min_samples)
QUANT_CASES = {
    "months_f64": (37, 5 * 67, 12, 0, None, np.float64, dict(nan_frac=0.2, specials=True), 4, 1),
    "months_f32": (37, 5 * 67, 12, 0, None, np.float32, dict(nan_frac=0.2, specials=True), 4, 1),
    "months_min4": (37, 70, 12, 0, None, np.float64, dict(), None, 4),               # slots of 3 samples are below min_samples
    "long_150": (150, 9, 1, 0, None, np.float64, dict(nan_frac=0.2, specials=True), 0, 1),
    "long_150_f32": (150, 9, 1, 0, None, np.float32, dict(nan_frac=0.2), None, 1),
    "series_2048": (2048, 1, 1, 0, None, np.float64, dict(), None, 1),
    "slot_32": (64, 70, 2, 0, None, np.float64, dict(), None, 1),
    "slot_33": (66, 70, 2, 1, None, np.float64, dict(), None, 1),
    "slot_16": (32, 70, 2, 0, None, np.float64, dict(), None, 1),                     # the 16-register network, full
    "slot_17": (33, 70, 2, 0, None, np.float32, dict(nan_frac=0.1), None, 1),         # the 32-register network, half empty
    "ties": (37, 70, 12, 0, None, np.float64, dict(quantised=True, nan_frac=0.2, specials=True), None, 1),
    "ties_long": (150, 9, 1, 0, None, np.float64, dict(quantised=True, specials=True), None, 1),
    "baseline_phase": (37, 70, 12, 7, (5, 30), np.float64, dict(nan_frac=0.2), 3, 1),
}


def quant_case(name):
    """(x, kwargs) of a case: x (T, M) and the arguments ``quantiles`` and the kern wrappers share"""
    T, M, period, phase, baseline, dtype, kw, masked, min_samples = QUANT_CASES[name]
    x = cube(T, M, sum(map(ord, name)), dtype, **kw)
    mask = None
    if masked is not None:
        mask = np.ones(M, dtype=np.uint8)
        mask[masked] = 0
    return x, dict(period=period, phase=phase, baseline=baseline, mask=mask, min_samples=min_samples)


# name -> (T of the fit, (H, W), period, phase, Q, pairwise, dtype, f, T of x, t0)
APPLY_CASES = {
    "f3": (37, (2, 3), 12, 5, 11, True, np.float64, 3, 29, 4),
    "f3_f32": (37, (2, 3), 12, 5, 11, True, np.float32, 3, 29, 4),
    "f1_own_nans": (50, (3, 5), 4, 1, 7, False, np.float64, 1, 50, 0),
    "ties": (37, (2, 3), 12, 0, 11, True, np.float64, 2, 13, 0),
}


def apply_case(name):
    """(model, obs (T, H, W), x (T', f H, f W), fit kwargs, t0): NaNs in both cubes (a slot below min_samples included), x
    with NaNs and with values below, above and exactly on the end nodes of its tables"""
    T, (H, W), period, phase, Q, pairwise, dtype, f, Tx, t0 = APPLY_CASES[name]
    seed = sum(map(ord, name)) + 1000
    quantised = name == "ties"
    model = cube(T, H * W, seed, dtype, nan_frac=0.15, quantised=quantised).reshape(T, H, W)
    obs = (cube(T, H * W, seed + 1, dtype, nan_frac=0.15, quantised=quantised) * dtype(1.5) + dtype(0.5)).reshape(T, H, W)
    model[:, 0, 1] = np.where(np.arange(T) % period == 0, np.nan, model[:, 0, 1])     # an empty slot at one pixel
    x = cube(Tx, f * H * f * W, seed + 2, dtype, nan_frac=0.1, quantised=quantised).reshape(Tx, f * H, f * W) * dtype(1.3)
    kw = dict(Q=Q, period=period, phase=phase, pairwise=pairwise, min_samples=2)
    mq, oq, _, _ = fit(model.reshape(T, -1), obs.reshape(T, -1), **kw)
    mq = mq.reshape(period, Q, H, W)
    for t in range(min(Tx, 2 * period)):                   # end nodes exactly, and one step beyond them on both sides
        s = (t0 + t + phase) % period
        e = 0 if t < period else Q - 1
        x[t, 0::f, 0::f] = mq[s, e].astype(dtype)
        if f > 1:
            x[t, 1::f, 1::f] = (mq[s, e] + (-40.0 if e == 0 else 40.0)).astype(dtype)
    return model, obs, x, kw, t0
