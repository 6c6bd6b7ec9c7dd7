"""The numpy oracle of the regionalisation tests (include/gandanet.h, "Regionalisation"), independent of csrc/kmeans_core.h:
distances, labels (lower index on a tie), second nearest, weighted member means, counts and within-sums in np.longdouble, the
margin ``dist2 - dist`` of every label, and the forward-error bounds of the fp64 code under test.  No bit of the twin goes into
a bound.

THE BOUNDS (u = 2^-53, gamma(n) = n u / (1 - n u); Higham, "Accuracy and Stability of Numerical Algorithms", ch. 3, 4):
  sample     v^ = fl(fl(x - shift) * scale): two roundings, |v^ - v| <= e_v = gamma(2) |v|; e_v = 0 when neither vector is given
             (x - 0.0 and * 1.0 are exact).
  term       a^ = fl(v^ - c), so with a = |v - c|: |a^ - (v - c)| <= e_a = e_v + u (a + e_v); the square is one more rounding:
             |t^ - a^2| <= e_t = 2 a e_a + e_a^2 + u (a + e_a)^2.
  distance   a left-to-right sum of T non-negative terms takes T - 1 additions: |d^ - d| <= sum e_t + gamma(T - 1) sum (t + e_t).
             WITHOUT shift / scale this is a relative bound: a term carries the two roundings of the subtraction and of the
             square, (1 + u)^3 - 1 <= gamma(3) counting the subtraction's twice, and the sum T - 1 more:
             |d^ - d| <= gamma(T + 2) d, that is (T + c) u with c = 2 (to first order in u).
             WITH shift / scale the subtraction v^ - c can cancel the rounding error of v^, so the bound is absolute (the e_v
             terms above) and not a multiple of d.
  centroid   the numerator of cluster k is a sum of n_k products w v^ in the documented order: the members of a slab in
             ascending order from +0.0, then the slab sums in ascending order from +0.0: at most n_k + S additions (S slabs) and
             three roundings per addend, so |N^ - N| <= gamma(n_k + S + 3) A with A = sum |w v|; the denominator likewise
             |W^ - W| <= gamma(n_k + S) W; the division is one rounding.  With |N| <= A:
             |c^ - c| <= gamma(2 (n_k + S) + 4) A / W.
  within     sum of w d^ over the members: |e| <= sum w e_d + gamma(n_k + S + 1) sum w (d + e_d); wsum: gamma(n_k + S) W.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
SLAB, CHUNK, MAX_T, MAX_K = 1024, 64, 2048, 64

TS = (1, 2, 3, 63, 64, 65, 181)            # 63 / 65: the staging chunk of 64 steps -+ 1
MS = (1, 63, 64, 65, 257)
KS = (1, 2, 7, 8, 9, 33, 64)


def gamma(n):
    n = LD(n)
    return n * U / (LD(1) - n * U)


def blobs(T, M, K, dtype=np.float64, seed=0, spread=0.05):
    """(x (T, M) of ``dtype``, centres (K, T) fp64, planted label (M,)): Gaussian blobs plus noise, pixel m around centre m % K"""
    rng = np.random.default_rng(1000 * T + 10 * M + K + seed)
    centres = 3.0 * rng.standard_normal((K, T))
    lab = np.arange(M) % K
    x = centres[lab].T + spread * rng.standard_normal((T, M))
    return np.ascontiguousarray(x.astype(dtype)), centres + 0.01 * rng.standard_normal((K, T)), lab


def mask_for(M):
    m = np.ones(M, dtype=np.uint8)
    m[::5] = 0
    return m


def sample(x, shift=None, scale=None):
    v = x.astype(LD)
    if shift is not None:
        v = v - shift.astype(LD)[None, :]
    if scale is not None:
        v = v * scale.astype(LD)[None, :]
    return v


def assign(x, cent, shift=None, scale=None, mask=None):
    """dict: label, dist, label2, dist2, margin (longdouble distances; -1 / NaN where left out), bound (M,), bound2 (M,)"""
    T, M = x.shape
    K = cent.shape[0]
    v = sample(x, shift, scale)
    transformed = shift is not None or scale is not None
    live = np.isfinite(v.astype(np.float64)).all(axis=0) & np.isfinite(x).all(axis=0)
    if mask is not None:
        live &= mask != 0
    vz = np.where(live[None, :], v, LD(0))
    c = cent.astype(LD)
    d = np.empty((K, M), dtype=LD)
    bd = np.empty((K, M), dtype=LD)
    e_v = gamma(2) * np.abs(vz) if transformed else np.zeros_like(vz)
    for k in range(K):
        a = np.abs(vz - c[k][:, None])
        t = a * a
        e_a = e_v + U * (a + e_v)
        e_t = 2 * a * e_a + e_a * e_a + U * (a + e_a) ** 2
        d[k] = t.sum(axis=0)
        bd[k] = e_t.sum(axis=0) + gamma(max(T - 1, 0)) * (t + e_t).sum(axis=0)
    label = np.argmin(d, axis=0)                                       # the first minimum: the lower index on a tie
    cols = np.arange(M)
    dist, bound = d[label, cols], bd[label, cols]
    if K > 1:
        rest = d.copy()
        rest[label, cols] = np.inf
        label2 = np.argmin(rest, axis=0)
        dist2, bound2 = d[label2, cols], bd[label2, cols]
        if K > 2:                                                      # the third nearest: it decides the second label
            rest[label2, cols] = np.inf
            label3 = np.argmin(rest, axis=0)
            margin2 = d[label3, cols] - dist2 - (bound2 + bd[label3, cols])
        else:
            margin2 = np.full(M, np.inf, dtype=LD)
    else:
        label2, dist2, bound2 = np.full(M, -1), np.full(M, np.nan, dtype=LD), np.zeros(M, dtype=LD)
        margin2 = np.full(M, np.inf, dtype=LD)
    nan = LD(np.nan)
    out = {"label": np.where(live, label, -1).astype(np.int32), "dist": np.where(live, dist, nan),
           "label2": np.where(live, label2, -1).astype(np.int32), "dist2": np.where(live, dist2, nan),
           "bound": bound, "bound2": bound2, "live": live, "second_decided": live & (margin2 > 0)}
    out["margin"] = out["dist2"] - out["dist"]
    return out


def update(x, label, dist, dist_bound, cent, w=None, shift=None, scale=None):
    """dict: cent (K, T), wsum, count, within (longdouble) and their bounds cent_bound (K, T), wsum_bound, within_bound (K)"""
    T, M = x.shape
    K = cent.shape[0]
    nslab = -(-M // SLAB)
    v = sample(x, shift, scale)
    wl = np.ones(M, dtype=LD) if w is None else w.astype(LD)
    out_c, cb = cent.astype(LD).copy(), np.zeros((K, T), dtype=LD)
    wsum, within, count = np.zeros(K, dtype=LD), np.zeros(K, dtype=LD), np.zeros(K, dtype=np.int64)
    wsum_b, within_b = np.zeros(K, dtype=LD), np.zeros(K, dtype=LD)
    for k in range(K):
        mem = label == k
        n = int(mem.sum())
        count[k] = n
        if n == 0:
            continue
        wk = wl[mem]
        wsum[k] = wk.sum()
        wsum_b[k] = gamma(n + nslab) * wsum[k]
        dk, bk = dist[mem].astype(LD), dist_bound[mem].astype(LD)
        within[k] = (wk * dk).sum()
        within_b[k] = (wk * bk).sum() + gamma(n + nslab + 1) * (wk * (dk + bk)).sum()
        if wsum[k] > 0:
            out_c[k] = (v[:, mem] * wk[None, :]).sum(axis=1) / wsum[k]
            cb[k] = gamma(2 * (n + nslab) + 4) * np.abs(v[:, mem] * wk[None, :]).sum(axis=1) / wsum[k]
    return {"cent": out_c, "wsum": wsum, "count": count, "within": within, "cent_bound": cb, "wsum_bound": wsum_b, "within_bound": within_b}


def farthest(d, exclude=()):
    best, bi = -np.inf, -1
    for i, v in enumerate(np.asarray(d, dtype=np.float64)):
        if np.isfinite(v) and i not in exclude and v > best:
            best, bi = v, i
    return bi


def worst(err, bound):
    """the largest |err| / bound (0 / 0 counts as 0; anything over a zero bound as inf)"""
    err, bound = np.abs(np.asarray(err, dtype=LD)), np.asarray(bound, dtype=LD)
    ok = ~np.isnan(err)
    if not ok.any():
        return 0.0
    err, bound = err[ok], bound[ok]
    r = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD(1)))
    r = np.where((bound <= 0) & (err > 0), LD(np.inf), r)
    return float(r.max())


def check_assign(got, want, what, need_second=True):
    """labels equal wherever the oracle's margin exceeds the two distance bounds (asserting that no live pixel is skipped:
    the blobs leave none undecided), distances within their bounds; returns the worst multiples (dist, dist2)"""
    label, dist, label2, dist2 = got
    live = want["live"]
    K_one = not np.isfinite(want["margin"][live].astype(np.float64)).any() if live.any() else True
    if not K_one:
        decided = want["margin"] > want["bound"] + want["bound2"]
        assert decided[live].all(), (what, "the oracle leaves a pixel undecided")
    assert np.array_equal(label, want["label"]), (what, "label")
    assert np.isnan(dist[~live]).all() and not np.isnan(dist[live]).any(), (what, "NaN pattern")
    r1 = worst(dist.astype(LD) - want["dist"], want["bound"])
    assert r1 <= 1.0, (what, "dist", r1)
    r2 = 0.0
    if need_second:
        assert np.array_equal(label2[~live], np.full((~live).sum(), -1)) and np.isnan(dist2[~live]).all(), (what, "second outside")
        # the second label is decided where the third distance exceeds the second by more than their two bounds (everywhere
        # on the blobs, asserted like the first label); its distance is held to its bound everywhere
        sure = want["second_decided"]
        assert sure[live].all(), (what, "the oracle leaves a second label undecided")
        assert np.array_equal(label2[sure], want["label2"][sure]), (what, "label2")
        r2 = worst(dist2.astype(LD) - want["dist2"], want["bound2"])
        assert r2 <= 1.0, (what, "dist2", r2)
        if K_one:
            assert (label2 == -1).all() and np.isnan(dist2).all(), (what, "K = 1 second")
    return r1, r2


def check_update(got, want, what):
    cent, wsum, count, within = got
    assert np.array_equal(count, want["count"]), (what, "count")
    rc = worst(cent.astype(LD) - want["cent"], want["cent_bound"])
    rw = worst(wsum.astype(LD) - want["wsum"], want["wsum_bound"])
    ri = worst(within.astype(LD) - want["within"], want["within_bound"])
    assert rc <= 1.0 and rw <= 1.0 and ri <= 1.0, (what, rc, rw, ri)
    return rc, rw, ri


# ---- the Lloyd loop of regions.kmeans_series driven through the HOST twins (numpy), for the device / twin comparison ----------
def host_sample(x2, idx, shift=None, scale=None):
    v = x2[:, idx].astype(np.float64)
    if shift is not None:
        v = v - shift[idx]
    if scale is not None:
        v = v * scale[idx]
    return np.ascontiguousarray(v.T)


def host_maximin(Kn, x2, k, w=None, mask=None):
    T = x2.shape[0]
    zero = np.zeros((1, T))
    label, dist, _, _ = Kn.km_assign_host(x2, zero, None, None, mask)
    mean = Kn.km_update_host(x2, label, dist, zero, w)[0]
    chosen = [int(Kn.km_farthest_host(-Kn.km_assign_host(x2, mean, None, None, mask)[1])[0])]
    cent = host_sample(x2, chosen)
    near = Kn.km_assign_host(x2, cent, None, None, mask)[1]
    for _ in range(1, k):
        nxt = int(Kn.km_farthest_host(near, np.array(chosen, dtype=np.int32))[0])
        chosen.append(nxt)
        c = host_sample(x2, [nxt])
        cent = np.concatenate([cent, c])
        near = np.minimum(near, Kn.km_assign_host(x2, c, None, None, mask)[1])   # NaN (left-out pixels) stays NaN
    return cent


def host_kmeans(Kn, x2, cent, max_iter=100, w=None, mask=None):
    """(labels, centroids, inertia, n_iter, converged) of the tol = 0 loop: assign; stop if no label changed; update; re-seat
    the empty clusters in ascending order on the farthest pixels; after the loop one assign and one update"""
    prev, n_iter, converged = None, 0, False
    cent = np.array(cent, dtype=np.float64)
    for _ in range(max_iter):
        label, dist, _, _ = Kn.km_assign_host(x2, cent, None, None, mask)
        if prev is not None and np.array_equal(label, prev):
            converged = True
            break
        cent, _, count, _ = Kn.km_update_host(x2, label, dist, cent, w)
        n_iter += 1
        prev = label
        taken = []
        for kk in np.flatnonzero(count == 0):
            nxt = int(Kn.km_farthest_host(dist, np.array(taken, dtype=np.int32) if taken else None)[0])
            taken.append(nxt)
            cent[kk] = host_sample(x2, [nxt])[0]
    label, dist, _, _ = Kn.km_assign_host(x2, cent, None, None, mask)
    within = Kn.km_update_host(x2, label, dist, cent, w)[3]
    inertia = within[0]
    for v in within[1:]:
        inertia = inertia + v
    return label, cent, inertia, n_iter, converged


def ari(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    ok = (a >= 0) & (b >= 0)
    a, b = a[ok], b[ok]
    c = np.zeros((a.max() + 1, b.max() + 1))
    np.add.at(c, (a, b), 1)
    p = lambda v: (v * (v - 1) / 2).sum()
    n = c.sum()
    e = p(c.sum(1)) * p(c.sum(0)) / (n * (n - 1) / 2)
    den = 0.5 * (p(c.sum(1)) + p(c.sum(0))) - e
    return 1.0 if den == 0 else (p(c) - e) / den
