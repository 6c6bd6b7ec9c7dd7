"""GPU: the spatial-spectra module (gan_danet_amd/spectra.py, csrc/spectra.hip) against the longdouble oracle of
tests/spectra_util.py, whose docstring derives every bound.  Every kernel call runs with sentinels around each output and
the workspace, twice on the same input and once more with x one element past a 16-byte boundary, and must give the same
bits.  Each test prints its largest error over its bound (python -m pytest -s)."""
import numpy as np
import pytest
import torch

import spectra_util as U

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD = 32


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _off(a):
    buf = torch.empty(a.size + 1, device="cuda", dtype=torch.from_numpy(a[:0].reshape(-1)).dtype)
    v = buf[1:].view(a.shape)
    v.copy_(_dev(a))
    assert v.data_ptr() % 16 == a.itemsize
    return v


class _Guarded:
    """fp64 device buffers with a sentinel margin on both sides"""

    def __init__(self):
        self.bufs = []

    def new(self, shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), SENTINEL, device="cuda", dtype=torch.float64)
        self.bufs.append((buf, n))
        return buf[PAD:PAD + n].view(shape)

    def check(self):
        for buf, n in self.bufs:
            h = buf.cpu().numpy()
            assert np.all(h[:PAD] == SENTINEL) and np.all(h[PAD + n:] == SENTINEL), "written outside a buffer"


def _prepare(x, mask, wy, wx, det, off=False):
    from gan_danet_amd import kern as K
    g = _Guarded()
    T = x.shape[0]
    coef, S = g.new((T, 3)), g.new((T, 2))
    K.spec_prepare(_off(x) if off else _dev(x), _dev(mask), _dev(wy), _dev(wx), det, coef=coef, S=S)
    g.check()
    return coef.cpu().numpy().copy(), S.cpu().numpy().copy()


def _power(x, coef, S, bins, nbins, mask=None, wy=None, wx=None, two_d=True, off=False):
    from gan_danet_amd import kern as K
    T, H, W = x.shape
    g = _Guarded()
    nbytes = K.spec_power_ws_bytes(T, H, W, nbins)
    power, dropped, ws = g.new((T, nbins)), g.new((T,)), g.new((nbytes // 8,))
    p2d = g.new((T, H, W // 2 + 1)) if two_d else None
    K.spec_power(_off(x) if off else _dev(x), _dev(coef), _dev(S), _dev(K.spec_twiddle_host(H)), _dev(K.spec_twiddle_host(W)), _dev(bins),
                 nbins, _dev(mask), _dev(wy), _dev(wx), power=power, dropped=dropped, p2d=p2d, ws=ws.view(torch.uint8))
    g.check()
    out = [power.cpu().numpy().copy(), dropped.cpu().numpy().copy(), None if p2d is None else p2d.cpu().numpy().copy()]
    assert not any(np.any(o == SENTINEL) for o in out if o is not None), "an output entry was not written"
    return out


def _power3(x, coef, S, bins, nbins, mask=None, wy=None, wx=None):
    """the power of the device, run twice and once more off a 16-byte boundary: the same bits"""
    a = _power(x, coef, S, bins, nbins, mask, wy, wx)
    for off in (False, True):
        b = _power(x, coef, S, bins, nbins, mask, wy, wx, off=off)
        assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b)), ("not repeatable", x.shape, off)
    return a


def _cross(xa, xb, ca, sa, cb, sb, bins, nbins, wy=None, wx=None, off=False):
    from gan_danet_amd import kern as K
    T, H, W = xa.shape
    g = _Guarded()
    nbytes = K.spec_cross_ws_bytes(T, H, W, nbins)
    out, dropped, ws = g.new((4, T, nbins)), g.new((T, 4)), g.new((nbytes // 8,))
    K.spec_cross(_off(xa) if off else _dev(xa), _dev(xb), _dev(ca), _dev(sa), _dev(cb), _dev(sb), _dev(K.spec_twiddle_host(H)),
                 _dev(K.spec_twiddle_host(W)), _dev(bins), nbins, None, _dev(wy), _dev(wx), out=out, dropped=dropped, ws=ws.view(torch.uint8))
    g.check()
    o, d = out.cpu().numpy().copy(), dropped.cpu().numpy().copy()
    assert not np.any(o == SENTINEL) and not np.any(d == SENTINEL)
    return o, d


def _table(H, W, d=1.0):
    from gan_danet_amd import kern as K
    nbins = K.spec_default_bins(H, W, d, d)
    return K.spec_bins_host(H, W, d, d, nbins, 0.5 / d)[0], nbins


def test_power_exact_small_integers():
    """H, W in {1, 2, 4}: every twiddle is 0 or +-1, p2d must equal the integer DFT exactly"""
    rng = np.random.default_rng(2)
    for H in (1, 2, 4):
        for W in (1, 2, 4):
            for T in (1, 3):
                xi = rng.integers(-8, 9, (T, H, W))
                bins, nbins = _table(H, W)
                for dtype in (np.float64, np.float32):
                    x = xi.astype(dtype)
                    coef, S = _prepare(x, None, None, None, "none")
                    assert np.all(coef == 0) and np.all(S == H * W)
                    power, dropped, p2d = _power3(x, coef, S, bins, nbins)
                    z = np.array([[[sum(xi[t, i, j] * (1j) ** (-(4 // H) * ky * i - (4 // W) * kx * j) for i in range(H) for j in range(W))
                                    for kx in range(W // 2 + 1)] for ky in range(H)] for t in range(T)])
                    z2 = np.rint(z.real) ** 2 + np.rint(z.imag) ** 2              # integers
                    want = U.hweight(W)[None, None, :] * z2 / float((H * W) ** 2)   # powers of two below: exact
                    assert np.array_equal(p2d, want), (H, W, T, dtype)
                    assert np.array_equal(power.sum(axis=1) + dropped, want.sum(axis=(1, 2)))


@pytest.mark.parametrize("shape", U.RAGGED)
def test_power_plane_wave(shape):
    H, W = shape
    bins, nbins = _table(H, W)
    Kx = W // 2 + 1
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    worst = 0.0
    for a, b in ((1, 0), (H // 2, W // 2), (2 % H, Kx - 1), (H - 1, 8 * ((Kx - 1) // 8)), (0, 1)):
        x = np.cos(2 * np.pi * (a * i / H + b * j / W))[None]
        coef, S = _prepare(x, None, None, None, "none")
        power, dropped, p2d = _power3(x, coef, S, bins, nbins)
        worst = max(worst, U.check_power(power[0], dropped[0], p2d[0], x[0], coef[0], bins, nbins, None, None, None, (H, W, a, b)))
        # all power in the bin holding (a, b) (and its mirror image, the same bin), elsewhere below the bound
        P, BP, _, _ = U.power_oracle(x[0], coef[0])
        want, bound = U.binned(P, BP, bins, nbins)
        slot = nbins if bins[a, b] < 0 else bins[a, b]
        got = np.concatenate([power[0], dropped[:1]])
        var = float((x[0] ** 2).mean())
        assert abs(got[slot] - var) <= float(bound.sum()) + 8 * U.U * var, (H, W, a, b)
        assert np.all(np.abs(np.delete(got, slot)) <= np.delete(bound + np.abs(want).astype(np.float64), slot)), (H, W, a, b)
    print(f"plane waves {shape}: at most {worst:.3f} of the bounds")


@pytest.mark.parametrize("shape,dtype", [(s, d) for s in U.SHAPES[3:] for d in (np.float64, np.float32)] + [((88, 180), np.float64)])
def test_power_random(shape, dtype):
    """test_power_random and test_parseval: p2d entrywise, power binned, dropped accounted, sum power + dropped = variance"""
    H, W = shape
    bins, nbins = _table(H, W, 0.5)
    combos = [(d, w) for d in ("none", "mean", "plane") for w in ("none", "hann", ("tukey", 0.4))]
    if shape == (88, 180):
        combos = combos[-1:]
    worst = 0.0
    for T in (1, 3):
        x = U.field(H, W, dtype, seed=T, T=T)
        for det, win in combos:
            wy, wx = U.windows(win, H, W)
            coef, S = _prepare(x, None, wy, wx, det)
            power, dropped, p2d = _power3(x, coef, S, bins, nbins, None, wy, wx)
            for t in range(T):
                worst = max(worst, U.check_power(power[t], dropped[t], p2d[t], x[t], coef[t], bins, nbins, None, wy, wx, (H, W, det, win, t)))
    print(f"power {shape} {np.dtype(dtype).name}: at most {worst:.3f} of the bounds (p2d, bins, Parseval)")


def test_parseval():
    """sum power + dropped = the windowed valid variance, through the module: a wrong Hermitian weight or a Nyquist
    column counted twice breaks it at once.  check_power holds the same identity to its derived bound on every shape;
    here even and odd W with half the default bins, so that most of the power is in `dropped`."""
    from gan_danet_amd import spectra as SP
    worst = 0.0
    for H, W in ((16, 16), (17, 33), (48, 31)):
        x = U.field(H, W, np.float64, seed=8, T=3)
        wy, wx = U.windows("hann", H, W)
        for nb in (None, 4):
            sp = SP.power_spectrum(_dev(x), detrend="mean", window="hann", nbins=nb)
            for t in range(3):
                ok = U.valid_of(x[t])
                xp, at, S = U.sample(x[t], ok, sp.coef[t], wy, wx)
                var = float((xp * xp).sum() / S)
                P, BP, _, _ = U.power_oracle(x[t], sp.coef[t], None, wy, wx)
                bound = float(BP.sum()) + U.gamma(H * W + 8) * var
                assert abs(sp.variance[t] - var) <= bound, (H, W, nb, t)
                worst = max(worst, abs(sp.variance[t] - var) / bound)
    print(f"parseval through the module: at most {worst:.3f} of the bound")


@pytest.mark.parametrize("shape,dy,dx,nbins", [((330, 6), 1.0, 0.25, 700), ((1024, 5), 1.0, 1.0, 513)])
def test_power_large_lds(shape, dy, dx, nbins):
    """H >= 320 needs more than 64 KiB of dynamic LDS (H = 1024: the largest image, 150 KiB for the power kernel and
    154 KiB for the cross kernel), and more than 256 bins use the second and third bin register of a thread"""
    from gan_danet_amd import kern as K
    H, W = shape
    bins, _, count = K.spec_bins_host(H, W, dy, dx, nbins)
    assert bins.max() >= 512 and (count[256:] > 0).any()
    x = U.field(H, W, np.float64, seed=4)
    wy, wx = U.windows("hann", H, W)
    coef, S = _prepare(x, None, wy, wx, "plane")
    power, dropped, p2d = _power3(x, coef, S, bins, nbins, None, wy, wx)
    worst = U.check_power(power[0], dropped[0], p2d[0], x[0], coef[0], bins, nbins, None, wy, wx, shape)
    print(f"power {shape}, {nbins} bins: at most {worst:.3f} of the bounds")
    if H == 1024:                                   # the cross kernel at its largest LDS image, the same bins
        xb = U.field(H, W, np.float64, seed=6)
        cb, sb = _prepare(xb, None, wy, wx, "plane")
        out, dr = _cross(x, xb, coef, S, cb, sb, bins, nbins, wy, wx)
        o2, d2 = _cross(x, xb, coef, S, cb, sb, bins, nbins, wy, wx, off=True)
        assert np.array_equal(o2, out) and np.array_equal(d2, dr)
        worst = U.check_cross(out[:, 0], dr[0], x[0], coef[0], xb[0], cb[0], bins, nbins, None, wy, wx, shape)
        print(f"cross {shape}, {nbins} bins: at most {worst:.3f} of the bounds")

@pytest.mark.parametrize("shape", U.RAGGED)
def test_messy(shape):
    from gan_danet_amd import kern as K
    H, W = shape
    bins, nbins = _table(H, W)
    x, mask = U.messy(H, W, np.float64)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x[2] += 0.7 * i - 0.2 * j + 5.0
    wy, wx = U.windows("hann", H, W)
    worst = 0.0
    for det in ("mean", "plane"):
        coef, S = _prepare(x, mask, wy, wx, det)
        assert np.array_equal(_prepare(x, mask, wy, wx, det, off=True)[0], coef)
        for t in range(3):
            ok = U.valid_of(x[t], mask)
            want = U.detrend_oracle(x[t], ok, det)
            bound = U.coef_bound(x[t], ok, det, want)
            err = np.abs(coef[t].astype(U.LD) - want).astype(np.float64)
            assert np.all(err <= bound) and S[t, 1] == ok.sum(), (shape, det, t, err, bound)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        power, dropped, p2d = _power3(x, coef, S, bins, nbins, mask, wy, wx)
        assert np.isnan(power[1]).all() and np.isnan(dropped[1]) and S[1, 1] == 0          # the all-invalid field
        for t in (0, 2):
            worst = max(worst, U.check_power(power[t], dropped[t], p2d[t], x[t], coef[t], bins, nbins, mask, wy, wx, (shape, det, t)))
    print(f"messy {shape}: at most {worst:.3f} of the bounds; the all-invalid field is NaN, its neighbours untouched")


@pytest.mark.parametrize("shape", U.RAGGED)
def test_field_independence(shape):
    H, W = shape
    bins, nbins = _table(H, W)
    x, mask = U.messy(H, W, np.float32)
    wy, wx = U.windows("hann", H, W)
    coef, S = _prepare(x, mask, wy, wx, "plane")
    power, dropped, p2d = _power(x, coef, S, bins, nbins, mask, wy, wx)
    for t in range(3):
        c1, s1 = _prepare(x[t:t + 1], mask, wy, wx, "plane")
        assert np.array_equal(c1[0], coef[t]) and np.array_equal(s1[0], S[t])
        p1, d1, q1 = _power(x[t:t + 1], c1, s1, bins, nbins, mask, wy, wx)
        assert np.array_equal(p1[0], power[t], equal_nan=True) and np.array_equal(d1[0], dropped[t], equal_nan=True)
        assert np.array_equal(q1[0], p2d[t], equal_nan=True)


@pytest.mark.parametrize("shape", U.RAGGED)
def test_cross(shape):
    H, W = shape
    bins, nbins = _table(H, W)
    worst = 0.0
    for dtype in (np.float64, np.float32):
        xa, xb = U.field(H, W, dtype, seed=1, T=3), U.field(H, W, dtype, seed=2, T=3)
        wy, wx = U.windows("hann", H, W)
        ca, sa = _prepare(xa, None, wy, wx, "mean")
        cb, sb = _prepare(xb, None, wy, wx, "mean")
        out, dropped = _cross(xa, xb, ca, sa, cb, sb, bins, nbins, wy, wx)
        for off in (False, True):
            o2, d2 = _cross(xa, xb, ca, sa, cb, sb, bins, nbins, wy, wx, off=off)
            assert np.array_equal(o2, out) and np.array_equal(d2, dropped)
        for t in range(3):
            worst = max(worst, U.check_cross(out[:, t], dropped[t], xa[t], ca[t], xb[t], cb[t], bins, nbins, None, wy, wx, (shape, t)))
        # a against a: quad exactly 0, the powers bit for bit, coherence 1
        same, sd = _cross(xa, xa, ca, sa, ca, sa, bins, nbins, wy, wx)
        power = _power(xa, ca, sa, bins, nbins, None, wy, wx, two_d=False)[0]
        assert np.all(same[3] == 0) and np.array_equal(same[0], same[1]) and np.all(sd[:, 3] == 0)
        (Pa, _, _, _), (Ba, _, _, _) = U.cross_oracle(xa[0], ca[0], xa[0], ca[0], None, wy, wx)
        _, bound = U.binned(Pa, Ba, bins, nbins)
        assert np.all(np.abs(same[0][0] - power[0]) <= 2 * bound[:nbins])                 # tiles of 4 against tiles of 8 kx
        coh = (same[2] ** 2 + same[3] ** 2) / (same[0] * same[1])
        live = same[0] > 0
        assert np.all(np.abs(coh[live] - 1) <= 4 * (bound[None, :nbins] / np.maximum(same[0], 1e-300))[live] + 8 * U.U)
    # a circular shift by (1, 2), no window, no detrend: coherence 1 per wavenumber, the phase ramp of the shift theorem
    xa = U.field(H, W, np.float64, seed=5)
    xb = np.roll(xa, (1, 2), axis=(1, 2))
    zero, s = np.zeros((1, 3)), np.array([[float(H * W), float(H * W)]])
    ky, kx = np.meshgrid(np.arange(H), np.arange(W // 2 + 1), indexing="ij")
    ang = (2 * np.pi * (ky * 1 / H + kx * 2 / W)).reshape(-1)     # Zb = Za exp(-i ang): Za conj Zb = |Za|^2 exp(+i ang)
    (Pa, Pb, co, qd), (Ba, Bb, Bc, _) = U.cross_oracle(xa[0], zero[0], xb[0], zero[0])
    Pa, Ba, Bb, Bc = (v.astype(np.float64).reshape(-1) for v in (Pa, Ba, Bb, Bc))
    for lo in range(0, ang.size, 1024):                            # one wavenumber per bin, 1024 bins per call
        n = min(1024, ang.size - lo)
        each = np.full(ang.size, -1, np.int32)
        each[lo:lo + n] = np.arange(n)
        out, _ = _cross(xa, xb, zero, s, zero, s, each.reshape(H, -1), n)
        sl = slice(lo, lo + n)
        assert np.all(np.abs(out[2, 0] - Pa[sl] * np.cos(ang[sl])) <= Bc[sl] + 8 * U.U * Pa[sl])
        assert np.all(np.abs(out[3, 0] - Pa[sl] * np.sin(ang[sl])) <= Bc[sl] + 8 * U.U * Pa[sl])
        coh = (out[2, 0] ** 2 + out[3, 0] ** 2) / (out[0, 0] * out[1, 0])
        assert np.all(np.abs(coh - 1) <= 4 * ((Ba + Bb + 2 * Bc) / np.maximum(Pa, 1e-300))[sl] + 16 * U.U)
    print(f"cross {shape}: at most {worst:.3f} of the bounds; a against a exact; shift theorem holds")


def test_python_layer():
    from gan_danet_amd import spectra as SP
    from gan_danet_amd._lib import GandanetError
    # (T, C, H, W) flattening: every field equals its own (H, W) call
    x = U.field(17, 33, np.float32, seed=9, T=6).reshape(3, 2, 17, 33)
    sp = SP.power_spectrum(_dev(x), dx=0.5, dy=0.5, detrend="plane", window=("tukey", 0.4), two_d=True)
    assert sp.power.shape == (3, 2, sp.k.size) and sp.power_2d.shape == (3, 2, 17, 17) and sp.variance.shape == (3, 2)
    one = SP.power_spectrum(_dev(x[1, 1]), dx=0.5, dy=0.5, detrend="plane", window=("tukey", 0.4))
    assert np.array_equal(one.power, sp.power[1, 1]) and one.power.shape == (sp.k.size,)
    assert np.all(sp.valid_fraction == 1) and np.allclose(sp.wavelength * sp.k, 1) and sp.mean().shape == (sp.k.size,)
    assert np.isfinite(sp.slope()) and sp.count.sum() <= 17 * 17
    cs = SP.cross_spectrum(_dev(x), _dev(x), dx=0.5, dy=0.5)
    assert cs.co.shape == (3, 2, cs.k.size) and np.all(cs.quad == 0) and np.allclose(cs.coherence()[cs.power_a.sum((0, 1)) > 0], 1, atol=1e-12)
    assert np.all(cs.phase() == 0) and np.allclose(cs.ratio()[cs.power_b.sum((0, 1)) > 0], 1)
    # a (20, 40) field constant along y against its 5-fold nearest repeat over one domain: bin b holds kx = b alone and
    # the ratio is the sinc^2 envelope at k = b / 200; both spectra hold their ~1e-13 relative bounds, 1e-10 is far above
    # them and far below any structural error
    rng = np.random.default_rng(4)
    lo = np.repeat(rng.standard_normal((1, 40)), 20, axis=0)
    hi = np.repeat(np.repeat(lo, 5, axis=0), 5, axis=1)
    s_lo = SP.power_spectrum(_dev(lo), dx=5.0, dy=5.0, detrend="none", window="none")
    s_hi = SP.power_spectrum(_dev(hi), dx=1.0, dy=1.0, detrend="none", window="none")
    k, ratio = SP.spectral_ratio(s_hi, s_lo)
    kb = np.arange(20) / 200.0
    assert np.allclose(ratio[:20], U.sinc2_envelope(kb, 5.0, 5), rtol=1e-10, atol=0) and np.allclose(k[:20], kb + 0.5 / 200)
    with pytest.raises(GandanetError, match="domains differ"):
        SP.spectral_ratio(s_hi, SP.power_spectrum(_dev(lo), dx=4.0, dy=5.0))
    # effective resolution: a curve that crosses 0.5 half-way (in log k) between k = 0.1 and k = 0.2
    kk = np.array([0.025, 0.05, 0.1, 0.2, 0.4])
    assert abs(SP.effective_resolution([1.0, 0.9, 0.7, 0.3, 0.1], kk) - 1 / np.sqrt(0.1 * 0.2)) < 1e-12
    assert np.isnan(SP.effective_resolution([1.0, 0.9, 0.8, 0.7, 0.6], kk))
    assert abs(SP.effective_resolution([1.0, 0.4, 0.9, 0.3, 0.1], kk) - 1 / (0.1 * 2 ** (0.4 / 0.6))) < 1e-12   # a dip is not sustained
    for bad in (lambda: SP.power_spectrum(torch.zeros(4, 4)), lambda: SP.cross_spectrum(torch.zeros(4, 4), torch.zeros(4, 4))):
        with pytest.raises(GandanetError, match="GPU tensor"):
            bad()
    with pytest.raises(GandanetError, match="at most"):
        SP.power_spectrum(_dev(np.zeros((1025, 4))))
    from gan_danet_amd import kern as K
    with pytest.raises(GandanetError, match="detrend"):
        K.spec_prepare(_dev(np.zeros((1, 4, 4))), detrend="cubic")
