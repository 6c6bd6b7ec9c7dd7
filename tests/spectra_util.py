"""The oracle and the bounds of the spatial-spectra tests (tests/test_cabi_spectra.py, tests/test_gpu_spectra.py).

DEFINITIONS (include/gandanet.h, "Spatial spectra"), here in numpy.longdouble.  For a field x (H, W), valid where x is
finite and the mask is nonzero:
  detrend   (a, b, c) of a + b u + c v, u = i - (H - 1) / 2, v = j - (W - 1) / 2; none: 0; mean: a = valid mean
  taper     x' = (x - plane) wy[i] wx[j] for valid pixels, 0 else
  transform Z[ky, kx] = sum x'[i, j] exp(-2 pi i (ky i / H + kx j / W)), kx = 0 .. W // 2: an explicit DFT matrix whose
            twiddles come from an exact integer reduction of (i k) mod N to an octant
  normalise P = weight |Z|^2 / (H W S), S = sum over valid of wy^2 wx^2, weight 1 for kx = 0 and kx = W / 2 (W even), else 2
  PARSEVAL  sum P = sum x'^2 / S
  bin       bin = floor(k L), k = hypot(ky' / (H dy), kx / (W dx)), L = max(H dy, W dx); here with Fractions.

BOUNDS, u = 2^-53, gamma(n) = n u / (1 - n u); none is tuned.
  x'   the code evaluates the plane (2 products, 2 sums), the difference and two products: its x' differs from the
       oracle's (same coefficients) by at most gamma(3) |x'| + gamma(6) (|a| + |b u| + |c v|) wy wx.
  Z    per component |Z^ - Z| <= E = gamma(W + 2 H + 11) A, A = sum (|x'| + (|a| + |b u| + |c v|) wy wx), for any order of
       the sums (MFMA or loop).  Term by term, for Re Z = sum_i sum_j x'_ij (C_i c_j + S_i s_j) (Im alike), with the
       exact twiddles c_j, s_j (W table) and C_i, S_i (H table):
         W      stage 1 is a sum of W products per row: every term carries (1 + theta_W);
         2 H    stage 2 is a sum of 2 H products (C_i Yre_i and S_i Yim_i): every term carries (1 + theta_2H);
         6      the rounding of x' above;
         3      the table entries are off by at most u in absolute value, twice: sum |x'| u (|C_i| + |S_i|) for the W
                table and sum |x'| u (|c_j| + |s_j|) for the H table, each <= sqrt2 u sum |x'|, 2 sqrt2 < 3;
         2      the products of the above among themselves (gamma_a + gamma_b + gamma_a gamma_b <= gamma_(a + b) covers
                the relative ones; the absolute twiddle terms times a (1 + theta) add less than 2 u).
       The relative terms multiply |x'_ij| (|C_i c_j| + |S_i s_j|) <= |x'_ij| (Cauchy-Schwarz on two unit vectors), so
       both stages together cost sum |x'| once, not once per stage.
  P    |Z^|^2 - |Z|^2 <= 2 (|Re Z| + |Im Z|) E + 2 E^2; three products, a sum and a division: gamma(8) |Z|^2; S is a sum of
       n positive terms: gamma(n + 4) relative.  BP = weight ((2 (|Re| + |Im|) E + 2 E^2) (1 + gamma(8)) / (H W S)
       + gamma(n + 12) P.
  bins a bin sums its members in some order over tiles and rows: sum BP + gamma(count + 2) sum P.
  cross terms: |Za conj Zb| error <= (|Za| + Ea) Eb sqrt2 ... bounded the same way with both fields' E (cross_bound).
fp32 storage adds nothing: the samples are exact in fp64.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SHAPES = ((1, 1), (2, 2), (4, 4), (5, 7), (16, 16), (17, 33), (48, 31), (44, 90))
RAGGED = ((5, 7), (17, 33), (48, 31), (44, 90))


def gamma(n):
    return n * U / (1.0 - n * U)


def twiddles(N):
    """(cos, sin) of 2 pi r / N, r = 0 .. N - 1, longdouble, by reduction to an octant in integers"""
    c, s = np.empty(N, LD), np.empty(N, LD)
    pi = LD("3.14159265358979323846264338327950288419716939937510")
    ck, sk = (1, 0, -1, 0), (0, 1, 0, -1)
    for r in range(N):
        octant, rem = divmod(8 * r, N)
        k, back = ((octant + 1) // 2) % 4, octant % 2 == 1
        phi = pi * LD(N - rem if back else rem) / LD(4 * N)
        cp, sp = np.cos(phi), (-np.sin(phi) if back else np.sin(phi))
        c[r], s[r] = ck[k] * cp - sk[k] * sp, sk[k] * cp + ck[k] * sp
    return c, s


def dft_matrices(N, K):
    """C[k, n] = cos(2 pi k n / N), S likewise, k < K"""
    c, s = twiddles(N)
    idx = (np.arange(K)[:, None] * np.arange(N)[None, :]) % N
    return c[idx], s[idx]


def hweight(W):
    w = np.full(W // 2 + 1, 2.0)
    w[0] = 1.0
    if W % 2 == 0:
        w[W // 2] = 1.0
    return w


def valid_of(x, mask=None):
    ok = np.isfinite(x)
    return ok if mask is None else ok & (np.asarray(mask).reshape(x.shape) != 0)


def coords(H, W):
    return (np.arange(H, dtype=LD) - LD(H - 1) / 2)[:, None], (np.arange(W, dtype=LD) - LD(W - 1) / 2)[None, :]


def detrend_oracle(x, ok, detrend):
    """(a, b, c) longdouble by least squares over the valid pixels (numpy lstsq is fp64: normal equations in longdouble)"""
    H, W = x.shape
    if detrend == "none" or not ok.any():
        return np.zeros(3, LD)
    xv = np.where(ok, x, 0).astype(LD)
    n = LD(ok.sum())
    if detrend == "mean":
        return np.array([xv.sum() / n, 0, 0], LD)
    u, v = coords(H, W)
    u, v = np.broadcast_to(u, x.shape)[ok], np.broadcast_to(v, x.shape)[ok]
    z = xv[ok]
    du, dv, dz = u - u.mean(), v - v.mean(), z - z.mean()
    suu, svv, suv, sux, svx = (du * du).sum(), (dv * dv).sum(), (du * dv).sum(), (du * dz).sum(), (dv * dz).sum()
    det = suu * svv - suv * suv
    b = c = LD(0)
    if suu > 0 and svv > 0 and det > 1e-12 * suu * svv:
        b, c = (sux * svv - svx * suv) / det, (svx * suu - sux * suv) / det
    elif suu > 0 and not svv > 0:
        b = sux / suu
    elif svv > 0 and not suu > 0:
        c = svx / svv
    return np.array([z.mean() - b * u.mean() - c * v.mean(), b, c], LD)


def coef_bound(x, ok, detrend, coef):
    """|coef^ - coef| entrywise.  mean: a sum of n terms and a division, gamma(n + 2) mean|x|.  plane: every second moment
    S_pq is a sum of n products of differences from computed means, relative to A_pq = sum |dp| |dq| at most
    gamma(n + 8); first-order propagation through b = (Sux Svv - Svx Suv) / det, c likewise, doubled for the higher
    orders; a = xm - b um - c vm collects the three."""
    H, W = x.shape
    n = int(ok.sum())
    if detrend == "none" or n == 0:
        return np.zeros(3)
    ax = float(np.abs(np.where(ok, x, 0)).astype(np.float64).sum()) / n
    ea = gamma(n + 2) * ax
    if detrend == "mean":
        return np.array([ea, 0.0, 0.0])
    u, v = coords(H, W)
    u, v = np.broadcast_to(u, x.shape)[ok], np.broadcast_to(v, x.shape)[ok]
    z = np.where(ok, x, 0).astype(LD)[ok]
    du, dv, dz = np.abs(u - u.mean()), np.abs(v - v.mean()), np.abs(z - z.mean()) + 2 * U * np.abs(z).max()
    g = gamma(n + 8)
    suu, svv, suv, sux, svx = (du * du).sum(), (dv * dv).sum(), (du * dv).sum(), (du * dz).sum(), (dv * dz).sum()
    sg = np.sign
    uu, vv = (u - u.mean()), (v - v.mean())
    det = float(suu * svv - (uu * vv).sum() ** 2)
    if not det > 1e-12 * float(suu * svv):
        den = float(suu if suu > 0 else svv)
        e = 2 * g * float(sux + svx) / den if den > 0 else 0.0
        return np.array([ea + e * float(np.abs(u.mean()) + np.abs(v.mean())) + 4 * U * ax, e, e])
    ddet = 2 * g * float(suu * svv + suv * suv)
    eb = 2 * (2 * g * float(sux * svv + svx * suv) + abs(float(coef[1])) * ddet) / det
    ec = 2 * (2 * g * float(svx * suu + sux * suv) + abs(float(coef[2])) * ddet) / det
    e0 = ea + eb * float(np.abs(u.mean())) + ec * float(np.abs(v.mean())) + 4 * U * (ax + abs(float(coef[1] * u.mean())) + abs(float(coef[2] * v.mean())))
    return np.array([e0, eb, ec])


def sample(x, ok, coef, wy=None, wx=None):
    """(x' longdouble, A-terms |x'| + (|a| + |b u| + |c v|) wy wx) with the given coefficients"""
    H, W = x.shape
    u, v = coords(H, W)
    wy = np.ones(H, LD) if wy is None else np.asarray(wy).astype(LD)
    wx = np.ones(W, LD) if wx is None else np.asarray(wx).astype(LD)
    a, b, c = (LD(t) for t in coef)
    w2 = wy[:, None] * wx[None, :]
    xv = np.where(ok, x, 0).astype(LD)
    xp = np.where(ok, (xv - (a + b * u + c * v)) * w2, LD(0))
    at = np.where(ok, np.abs(xp) + (abs(a) + np.abs(b * u) + np.abs(c * v)) * np.abs(w2), LD(0))
    S = np.where(ok, w2 * w2, LD(0)).sum()
    return xp, at, S


def dft(xp):
    """(Re Z, Im Z) (H, W // 2 + 1) longdouble by explicit matrices"""
    H, W = xp.shape
    cw, sw = dft_matrices(W, W // 2 + 1)
    ch, sh = dft_matrices(H, H)
    yre, yim = xp @ cw.T, -(xp @ sw.T)
    return ch @ yre + sh @ yim, ch @ yim - sh @ yre


def power_oracle(x, coef, mask=None, wy=None, wx=None):
    """(P (H, Kx) longdouble, BP its entrywise bound (float64), S, (zre, zim, E)) of one field; NaN P without a valid pixel"""
    H, W = x.shape
    ok = valid_of(x, mask)
    xp, at, S = sample(x, ok, coef, wy, wx)
    zre, zim = dft(xp)
    n = int(ok.sum())
    if n == 0:
        return np.full(zre.shape, np.nan), np.zeros(zre.shape), S, (zre, zim, 0.0)
    E = gamma(W + 2 * H + 11) * float(at.sum())
    w = hweight(W)[None, :]
    z2 = zre * zre + zim * zim
    P = w * z2 / (LD(H) * LD(W) * S)
    dz2 = (2 * (np.abs(zre) + np.abs(zim)) * E + 2 * E * E) * (1 + gamma(8))
    BP = (w * dz2 / (LD(H) * LD(W) * S) + gamma(n + 12) * P).astype(np.float64)
    return P, BP, S, (zre, zim, E)


def cross_oracle(xa, ca, xb, cb, mask=None, wy=None, wx=None):
    """((Paa, Pbb, co, quad) (H, Kx) longdouble, their bounds); the cross terms over H W sqrt(Sa Sb): a product Za conj Zb has
    per real product error <= |za| Eb + |zb| Ea + Ea Eb, two of them per term"""
    H, W = xa.shape
    Pa, Ba, Sa, (are, aim, Ea) = power_oracle(xa, ca, mask, wy, wx)
    Pb, Bb, Sb, (bre, bim, Eb) = power_oracle(xb, cb, mask, wy, wx)
    w = hweight(W)[None, :]
    nrm = LD(H) * LD(W) * np.sqrt(Sa * Sb)
    co, qd = w * (are * bre + aim * bim) / nrm, w * (aim * bre - are * bim) / nrm
    ma, mb = np.abs(are) + np.abs(aim), np.abs(bre) + np.abs(bim)
    n = int(valid_of(xa, mask).sum()) + int(valid_of(xb, mask).sum())
    mag = w * (np.abs(are * bre) + np.abs(aim * bim) + np.abs(aim * bre) + np.abs(are * bim)) / nrm
    Bc = (w * ((ma * Eb + mb * Ea + 2 * Ea * Eb) * (1 + gamma(8))) / nrm + gamma(n + 16) * mag).astype(np.float64)
    return (Pa, Pb, co, qd), (Ba, Bb, Bc, Bc)


def binned(P, BP, bins, nbins, mag=None):
    """(sums (nbins + 1) longdouble, bounds) of an (H, Kx) image over the table; slot nbins = dropped"""
    slot = np.where(bins < 0, nbins, bins).reshape(-1)
    mag = np.abs(P) if mag is None else mag
    out, bound = np.zeros(nbins + 1, LD), np.zeros(nbins + 1)
    np.add.at(out, slot, P.reshape(-1))
    np.add.at(bound, slot, BP.reshape(-1))
    m, cnt = np.zeros(nbins + 1), np.zeros(nbins + 1)
    np.add.at(m, slot, mag.reshape(-1).astype(np.float64))
    np.add.at(cnt, slot, 1.0)
    return out, bound + gamma(cnt + 2) * m


def bins_fraction(H, W, dy, dx, nbins, kmax=0.0):
    """the bin table with Fractions: P = H dy and Q = W dx as the fp64 products, exact from there on"""
    P, Q = Fraction(float(H) * float(dy)), Fraction(float(W) * float(dx))
    Lm = max(P, Q)
    out = np.empty((H, W // 2 + 1), np.int32)
    lim = None if not kmax > 0 else (Fraction(float(kmax)) * Lm * (1 + Fraction(1, 2 ** 40))) ** 2
    for ky in range(H):
        kf = ky - H if 2 * ky > H else ky
        for kx in range(W // 2 + 1):
            q = (kf * Lm / P) ** 2 + (kx * Lm / Q) ** 2
            b = int(np.floor(np.sqrt(float(q))))
            while b * b > q:
                b -= 1
            while (b + 1) * (b + 1) <= q:
                b += 1
            out[ky, kx] = -1 if b >= nbins or (lim is not None and q > lim) else b
    return out


def field(H, W, dtype=np.float64, seed=0, T=1):
    rng = np.random.default_rng(1000 * H + W + 7919 * seed)
    return (rng.standard_normal((T, H, W)) + 0.3).astype(dtype)


def windows(name, H, W):
    from gan_danet_amd import spectra
    return spectra.window_vector(name, H), spectra.window_vector(name, W)


def messy(H, W, dtype, T=3):
    x = field(H, W, dtype, seed=3, T=T)
    mask = np.ones((H, W), np.uint8)
    if H * W >= 35:
        x[0, 1, 2], x[0, H - 1, W - 1], x[0, 2, 0] = np.nan, np.inf, -np.inf
        mask[0, 3:5] = 0
        mask[H // 2, W // 2] = 0
        x[1] = np.nan                       # a field with no valid pixel between two valid ones
    return x, mask


def check_power(got_power, got_dropped, got_p2d, x, coef, bins, nbins, mask, wy, wx, what):
    """one field against the oracle: p2d entrywise, power binned, dropped accounted, Parseval; the worst ratio"""
    P, BP, S, _ = power_oracle(x, coef, mask, wy, wx)
    if np.isnan(P).all():
        assert np.isnan(got_power).all() and np.isnan(got_dropped) and (got_p2d is None or np.isnan(got_p2d).all()), what
        return 0.0
    worst = 0.0
    if got_p2d is not None:
        err = np.abs(got_p2d.astype(LD) - P).astype(np.float64)
        assert np.all(err <= BP), (what, "p2d", float((err / np.maximum(BP, 1e-300)).max()))
        worst = float((err / np.maximum(BP, 1e-300)).max())
    want, bound = binned(P, BP, bins, nbins)
    got = np.concatenate([got_power, [got_dropped]])
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    assert np.all(err <= bound), (what, "power", float((err / np.maximum(bound, 1e-300)).max()))
    worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    # Parseval: sum power + dropped = sum x'^2 / S
    ok = valid_of(x, mask)
    xp, _, _ = sample(x, ok, coef, wy, wx)
    var = (xp * xp).sum() / S
    perr = abs(float(got.astype(LD).sum() - var))
    pb = float(bound.sum()) + gamma(nbins + 2) * float(var)
    assert perr <= pb, (what, "parseval", perr, pb)
    return max(worst, perr / max(pb, 1e-300))


def check_cross(out, dropped, xa, ca, xb, cb, bins, nbins, mask, wy, wx, what):
    (Pa, Pb, co, qd), bounds = cross_oracle(xa, ca, xb, cb, mask, wy, wx)
    worst = 0.0
    if np.isnan(Pa).all() or np.isnan(Pb).all():          # no valid pixel, or a taper that vanishes on all of them (S = 0)
        assert np.isnan(out[2:]).all() and np.isnan(dropped[2:]).all(), what
        return worst
    for q, (P, B) in enumerate(zip((Pa, Pb, co, qd), bounds)):
        want, bound = binned(P, B, bins, nbins, mag=None if q < 2 else np.sqrt(np.abs(Pa * Pb)))
        got = np.concatenate([out[q], [dropped[q]]])
        err = np.abs(got.astype(LD) - want).astype(np.float64)
        assert np.all(err <= bound), (what, q, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def sinc2_envelope(k, dx_lo, r):
    """|sum_{m<r} exp(-2 pi i k m dx_lo / r) / r|^2 = (sin(pi k dx_lo) / (r sin(pi k dx_lo / r)))^2: the spectrum of an r-fold
    nearest-neighbour repeat over that of the coarse field, along one axis at wavenumber k (1 at k = 0)"""
    k = np.asarray(k, dtype=np.float64)
    den = r * np.sin(np.pi * k * dx_lo / r)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, 1.0, (np.sin(np.pi * k * dx_lo) / den) ** 2)
