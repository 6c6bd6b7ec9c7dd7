"""GPU parity, kernel level, for csrc/norm.hip: BatchNorm statistics (gd_bn_stats / _local / _merge), the train and
eval folds, y = act(x * scale + shift), the backward of act(bn(x)) and gd_channel_sum -- at the shapes where their
finalize loops take a second trip, the 16384-element chunks end, the float4 / scalar switch flips and the batch
strides differ from C * HW.

Every kernel is tested alone through its ``kern`` wrapper: it gets float32 inputs, the float32 scale / shift / mean /
invstd it would get included, and is compared with the float64 reference (tests/norm_util.py, checked against
torch.nn.BatchNorm2d in tests/test_norm_reference.py) of exactly those float32 values.  The bounds are roundoff bounds
written in terms of the reference quantities, u = 2^-24; ``_hold`` prints the largest error as a fraction of its bound
before it asserts.

Every activation handed to a kernel sits at the head of a buffer whose tail is one chunk of 1e30: a read past the end
of a plane shows up in the result instead of depending on what the allocator left there."""
import numpy as np
import pytest
import torch

import norm_util as NU
from gpu_util import DEV, seeded
from norm_util import ACT_LEAKY02, ACT_NONE, ACT_RELU, CHUNK, SUM_TERMS, U

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
ACTS = [ACT_NONE, ACT_RELU, ACT_LEAKY02]
POISON = 1e30
SHAPES = [(1, 1, 1, 1), (2, 3, 1, 5), (3, 2, 7, 9), (2, 2, 16, 16), (1, 2, 129, 127), (2, 1, 128, 128),
          (2, 1, 16385, 1), (1, 2, 4097, 4), (300, 2, 2, 2), (65535, 1, 1, 1)]
SLAB_SHAPES = [(3, 7, 9), (2, 16, 16), (2, 1, 5)]       # (B, H, W) of the slab cases: scalar path, float4 path, tiny


@pytest.fixture(scope="module")
def K():
    from gan_danet_amd import _lib, kern
    _lib.load()
    return kern


def _err_type():
    from gan_danet_amd import _lib
    return _lib.GandanetError


def _sid(shape):
    return "x".join(str(s) for s in shape)


def _kshape(shape):
    """the 3-D (B, C, N) form where the plane is a single column"""
    return (shape[0], shape[1], shape[2]) if len(shape) == 4 and shape[3] == 1 else tuple(shape)


def _dev(t, offset=0):
    """``t`` on the device at ``offset`` floats into a fresh buffer, followed by one chunk of POISON"""
    n = t.numel()
    buf = torch.full((offset + n + CHUNK,), POISON, device=DEV, dtype=torch.float32)
    v = buf[offset:offset + n].view(_kshape(t.shape))
    v.copy_(t.reshape(v.shape))
    return v


def _tail(v):
    """the POISON chunk behind a whole (unsliced) tensor made by ``_dev``"""
    return torch.empty(0, device=DEV, dtype=torch.float32).set_(v.untyped_storage(), v.storage_offset() + v.numel(), (CHUNK,))


def _r32(a):
    """float64 reference values rounded to the float32 a kernel would be handed, as a CPU tensor"""
    return torch.as_tensor(np.asarray(a, dtype=np.float64).astype(np.float32))


def _np(t):
    return NU.f64(t)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _hold(name, what, got, ref, bound, keep=None):
    """|got - ref| <= bound elementwise (where ``keep``); prints the worst err / bound, then asserts"""
    got, ref = _np(got).reshape(np.shape(ref)), np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got - ref)
    if keep is not None:
        err, bound = err[keep], bound[keep]
    if err.size == 0:
        return
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max()
    print(f"[norm] {name} | {what}: err/bound {frac:.3e} (max err {err.max():.3e})")
    assert frac <= 1.0, f"{what}: {name} missed, err/bound {frac:.3e}, max err {err.max():.3e}"


def _cb(v, like):
    """(C,) -> broadcastable against the (B, C, ...) array ``like``"""
    return np.asarray(v, dtype=np.float64).reshape((1, -1) + (1,) * (like.ndim - 2))


# =====================================================================================================================
# 1. statistics
# =====================================================================================================================
MEANS = (0.0, 3.0, -1e4)
FAMILIES = ["normal0", "normal1", "normal2", "const", "outlier_first", "outlier_chunk2", "ramp"]
CHUNK2_SHAPES = [s for s in SHAPES if s[2] * s[3] > CHUNK] + [(1, 1, 1, 2 * CHUNK), (2, 2, 1, CHUNK + 4097)]


def _stats_input(shape, family):
    B, C, H, W = shape
    seed = 1000 + (B * 31 + C * 7 + H * 3 + W) % 977
    if family.startswith("normal"):         # std 1, channel means 0 / 3 / -1e4, rotated so every channel meets each
        r = int(family[-1])
        mu = torch.tensor([MEANS[(c + r) % 3] for c in range(C)]).view(1, C, 1, 1)
        return seeded(shape, seed + r) + mu
    if family == "const":
        return torch.full(shape, 1e3)
    if family == "ramp":
        i = torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W)
        return 0.25 * i + torch.arange(C).view(1, C, 1, 1) - torch.arange(B).view(B, 1, 1, 1)
    x = seeded(shape, seed + 5) + 3.0       # N(3, 1) with one element of every plane at mean + 100 sigma
    x.view(B, C, -1)[:, :, 0 if family == "outlier_first" else CHUNK] = 103.0
    return x


def _stats_cases():
    out = []
    for fam in FAMILIES:
        for s in (CHUNK2_SHAPES if fam == "outlier_chunk2" else SHAPES):
            out.append(pytest.param(s, fam, id=f"{fam}-{_sid(s)}"))
    return out


def _check_stats(what, mean, inv, rm, rv, st, rm0, rv0, m2_slack=0.0):
    """the bounds of the issue, u = 2^-24: |mean - ref| <= 4u |ref| + 1e-6 std; invstd to 2e-6 relative; running
    statistics to 4u relative of the fp64 update *plus* momentum times what the batch statistic entering it is
    allowed: the update is one rounding of (1 - m) * old + m * stat, so an error d of the statistic arrives as m * d
    whatever the update does (d = the mean bound; for the unbiased variance 2e-6 relative, the M2 bound of the
    records).  Without that term a channel whose batch mean is near zero could not meet 4u of a near-zero number.
    ``m2_slack``: an absolute allowance on M2 that the caller derives (only the merge of device-made records has one);
    it enters invstd as d invstd / invstd = dvar / (2 (var + eps))."""
    std = np.sqrt(st.var)
    mean_bound = 4 * U * np.abs(st.mean) + 1e-6 * std
    ref_inv = NU.invstd(st.var, EPS)
    _hold("stats mean", f"{what} mean", mean, st.mean, mean_bound)
    _hold("stats invstd", f"{what} invstd", inv, ref_inv, ref_inv * (2e-6 + m2_slack / st.n / (2 * (st.var + NU.f32(EPS)))))
    if rm is not None:
        ref_rm, ref_rv = NU.running_update(rm0, rv0, st, MOM)
        _hold("running mean", f"{what} running_mean", rm, ref_rm, 4 * U * np.abs(ref_rm) + NU.f32(MOM) * mean_bound)
        _hold("running var", f"{what} running_var", rv, ref_rv,
              4 * U * np.abs(ref_rv) + NU.f32(MOM) * (2e-6 * st.unb + m2_slack / np.maximum(st.n - 1, 1)))


@pytest.mark.parametrize("shape,family", _stats_cases())
def test_bn_stats_and_local_records(K, shape, family):
    C = shape[1]
    x = _stats_input(shape, family)
    xg = _dev(x)
    st = NU.channel_stats(x)
    rm0, rv0 = 0.5 * seeded((C,), 21) + 1.0, 1.0 + seeded((C,), 22) ** 2
    rm, rv = rm0.clone().to(DEV), rv0.clone().to(DEV)
    mean, inv = K.bn_stats(xg, EPS, MOM, rm, rv)
    what = f"bn_stats {family} {_sid(shape)}"
    _check_stats(what, mean, inv, rm, rv, st, rm0, rv0)
    m2, i2 = K.bn_stats(xg, EPS, MOM, None, None)            # no running statistics: the same numbers
    assert torch.equal(_bits(m2), _bits(mean)) and torch.equal(_bits(i2), _bits(inv))
    rec = K.bn_stats_local(xg)
    assert rec.shape == (C, 3)
    assert (_np(rec[:, 0]) == st.n).all(), f"{what}: count {rec[:, 0].tolist()} vs {st.n.tolist()}"
    _hold("local mean", f"{what} record mean", rec[:, 1], st.mean, 4 * U * np.abs(st.mean) + 1e-6 * np.sqrt(st.var))
    _hold("local M2", f"{what} record M2", rec[:, 2], st.m2, 2e-6 * st.m2)
    if family == "const":                                   # M2 exactly 0, so invstd is exactly 1 / sqrt(eps)
        exact = np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS))))
        assert (inv.cpu().numpy() == exact).all(), f"{what}: invstd {inv.tolist()} != {exact}"
        assert (mean.cpu().numpy() == np.float32(1e3)).all() and (rec[:, 2].cpu().numpy() == 0).all()
    if x[0, 0].numel() * shape[0] == 1:                     # one element per channel: unb = var = 0
        assert (rec[:, 2].cpu().numpy() == 0).all()
        assert np.allclose(rv.cpu().numpy(), (1 - NU.f32(MOM)) * rv0.numpy(), rtol=4 * U, atol=0)


def test_bn_stats_slab_slice(K):
    """statistics of channels 8..10 of a 32-channel slab (batch stride 32 * HW), over the B = 3, 2, 2 images of SLAB_SHAPES"""
    for B, H, W in SLAB_SHAPES:
        slab = seeded((B, 32, H, W), 31) * 1.5 + torch.arange(32).view(1, 32, 1, 1) * 0.5
        sg = _dev(slab)
        st = NU.channel_stats(slab[:, 8:11])
        rm0, rv0 = torch.zeros(3), torch.ones(3)
        rm, rv = rm0.clone().to(DEV), rv0.clone().to(DEV)
        mean, inv = K.bn_stats(sg[:, 8:11], EPS, MOM, rm, rv)
        _check_stats(f"bn_stats slab {B}x{H}x{W}", mean, inv, rm, rv, st, rm0, rv0)


@pytest.mark.parametrize("world", [1, 3, 300])
def test_bn_stats_merge(K, world):
    """(world, C, 3) records with unequal counts against the fp64 merge of the same float32 records: the kernel merges
    in double, so the issue's bounds hold as they stand, the mean -1e4 channels included"""
    C = 6
    g = torch.Generator().manual_seed(40 + world)
    cnt = torch.randint(2, 5000, (world, C), generator=g).float()
    cnt[0, 0] = 1.0                                                     # a one-element shard among them
    mu = seeded((world, C), 41 + world, 0.5) + torch.tensor([0.0, 3.0, -1e4, 0.0, 3.0, -1e4])
    m2 = cnt * (0.5 + torch.rand(world, C, generator=g))
    m2[0, 0] = 0.0
    if world == 1:
        cnt[0, 1], m2[0, 1] = 1.0, 0.0                                  # the whole batch is one element: unb = var
    recs = torch.stack([cnt, mu, m2], 2).contiguous()
    st = NU.merge(recs)
    rm0, rv0 = 0.5 * seeded((C,), 43) + 1.0, 1.0 + seeded((C,), 44) ** 2
    rm, rv = rm0.clone().to(DEV), rv0.clone().to(DEV)
    mean, inv = K.bn_stats_merge(recs.to(DEV), EPS, MOM, rm, rv)
    _check_stats(f"bn_stats_merge world={world}", mean, inv, rm, rv, st, rm0, rv0)
    m2_, i2_ = K.bn_stats_merge(recs.to(DEV), EPS, MOM, None, None)
    assert torch.equal(_bits(m2_), _bits(mean)) and torch.equal(_bits(i2_), _bits(inv))


def test_bn_stats_merge_of_kernel_records_equals_full_batch_reference(K):
    """local records of three unequal shards, merged on the device, against the fp64 statistics of the whole batch.

    Here, and only here, the reference is not computed from what the merge reads: each float32 record carries the
    error the issue allows gd_bn_stats_local, e_c = 4u |m_c| + 1e-6 std_c on its mean (a float32 cannot hold a mean
    of -1e4 closer than that) and 2e-6 relative on its M2.  The merged M2 = sum M2_c + n_c (m_c - mu)^2 then moves by
    at most sum n_c (2 |m_c - mu| e_c + e_c^2) beyond the 2e-6 (the shift of mu itself cancels to first order, since
    sum n_c (m_c - mu) = 0).  The term is formed from the fp64 statistics of the shards; it is 0 for one shard."""
    x = _stats_input((7, 3, 129, 127), "normal0")
    cuts = ((0, 1), (1, 3), (3, 7))
    recs = torch.stack([K.bn_stats_local(_dev(x[lo:hi])) for lo, hi in cuts], 0).contiguous()
    mean, inv = K.bn_stats_merge(recs, EPS, MOM, None, None)
    st = NU.channel_stats(x)
    slack = 0.0
    for lo, hi in cuts:
        sc = NU.channel_stats(x[lo:hi])
        e = 4 * U * np.abs(sc.mean) + 1e-6 * np.sqrt(sc.var)
        slack = slack + sc.n * (2 * np.abs(sc.mean - st.mean) * e + e * e)
    print(f"[norm] merge of kernel records: M2 allowance / M2 = {(slack / st.m2).tolist()}")
    _check_stats("merge of kernel records", mean, inv, None, None, st, None, None, m2_slack=slack)


# =====================================================================================================================
# 2. fold
# =====================================================================================================================
@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_bn_fold_train_and_eval(K, C):
    """scale to 2u relative, |shift - ref| <= 2u (|mean * scale| + |beta|), eval invstd_out to 2u relative"""
    gamma, beta = 1 + 0.3 * seeded((C,), 51), 0.5 * seeded((C,), 52)
    mean, inv = 3 * seeded((C,), 53), 0.2 + seeded((C,), 54) ** 2
    rv = 0.05 + seeded((C,), 55) ** 2
    scale, shift = K.bn_fold(gamma.to(DEV), beta.to(DEV), mean.to(DEV), inv.to(DEV))
    rs, rh = NU.fold(gamma, beta, mean, inv)
    _hold("fold scale", f"bn_fold C={C} scale", scale, rs, 2 * U * np.abs(rs))
    _hold("fold shift", f"bn_fold C={C} shift", shift, rh, 2 * U * (np.abs(_np(mean) * rs) + np.abs(_np(beta))))
    scale, shift, io = K.bn_fold_eval(gamma.to(DEV), beta.to(DEV), mean.to(DEV), rv.to(DEV), EPS)
    rs, rh, ri = NU.fold_eval(gamma, beta, mean, rv, EPS)
    _hold("fold_eval invstd", f"bn_fold_eval C={C} invstd_out", io, ri, 2 * U * ri)
    _hold("fold scale", f"bn_fold_eval C={C} scale", scale, rs, 2 * U * np.abs(rs))
    _hold("fold shift", f"bn_fold_eval C={C} shift", shift, rh, 2 * U * (np.abs(_np(mean) * rs) + np.abs(_np(beta))))


# =====================================================================================================================
# 3. y = act(x * scale + shift)
# =====================================================================================================================
def _affine_bound(x, scale, shift, act):
    """one fma, so |y - ref| <= u |x * sc + sh|; leaky adds the product with 0.2f (not 0.2): 2u"""
    return (2 if act == ACT_LEAKY02 else 1) * U * np.abs(NU.preact(x, scale, shift))


def _affine_params(C, seed):
    return 1 + 0.4 * seeded((C,), seed), 0.7 * seeded((C,), seed + 1)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_affine_act(K, shape, act):
    C = shape[1]
    x = seeded(shape, 61) * 2 + 0.5
    sc, sh = _affine_params(C, 62)
    xg = _dev(x)
    for s, h in ((sc, sh), (None, None), (sc, None), (None, sh)):
        y = K.affine_act(xg, None if s is None else s.to(DEV), None if h is None else h.to(DEV), act)
        assert y.shape == xg.shape
        _hold("affine_act", f"affine_act {_sid(shape)} act={act} scale={s is not None} shift={h is not None}",
              y, NU.affine_act(x, s, h, act), _affine_bound(x, s, h, act))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", [(2, 2, 16, 16), (1, 2, 4097, 4)], ids=_sid)
def test_affine_act_base_pointer_alignment(K, shape, act):
    """HW % 4 == 0: float4 path when both base pointers are 16-byte aligned, scalar path when x, y or both sit one
    float off; all four results bitwise equal, and in place (out = x) as well.

    This holds the two paths to the same numbers; it does not guard the alignment term of the switch itself: gfx950
    executes a float4 access at a 4-byte-aligned address with the same result, so a kernel that took the float4 path
    regardless of alignment passes here too (tried once, on a scratch build).  No test on this device can tell them
    apart."""
    x = seeded(shape, 63) * 2 - 0.3
    sc, sh = _affine_params(shape[1], 64)
    scg, shg = sc.to(DEV), sh.to(DEV)
    n = x.numel()
    outs = []
    for xo, yo in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xg = _dev(x, xo)
        ybuf = torch.full((yo + n + CHUNK,), POISON, device=DEV)
        yv = ybuf[yo:yo + n].view(shape)
        assert xg.data_ptr() % 16 == 4 * xo and yv.data_ptr() % 16 == 4 * yo
        assert K.affine_act(xg, scg, shg, act, out=yv) is yv
        assert (ybuf[:yo] == POISON).all() and (ybuf[yo + n:] == POISON).all(), "wrote outside the output"
        outs.append(yv)
    _hold("affine_act", f"affine_act aligned {_sid(shape)} act={act}", outs[0], NU.affine_act(x, sc, sh, act),
          _affine_bound(x, sc, sh, act))
    for o in outs[1:]:
        assert torch.equal(_bits(o), _bits(outs[0]))
    for xo in (0, 1):
        xg = _dev(x, xo)
        assert K.affine_act(xg, scg, shg, act, out=xg) is xg
        assert torch.equal(_bits(xg), _bits(outs[0])), f"in place at offset {xo}"


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("bhw", SLAB_SHAPES, ids=_sid)
def test_affine_act_slab_slices(K, bhw, act):
    """read slab[:, 8:11], write slab[:, 20:23] of a 32-channel slab: nothing else changes, bit for bit"""
    B, H, W = bhw
    slab = seeded((B, 32, H, W), 65) * 2 + 0.25
    sc, sh = _affine_params(3, 66)
    sg = _dev(slab)
    K.affine_act(sg[:, 8:11], sc.to(DEV), sh.to(DEV), act, out=sg[:, 20:23])
    after = sg.cpu()
    _hold("affine_act", f"affine_act slab {_sid(bhw)} act={act}", after[:, 20:23], NU.affine_act(slab[:, 8:11], sc, sh, act),
          _affine_bound(slab[:, 8:11], sc, sh, act))
    keep = torch.ones(32, dtype=torch.bool)
    keep[20:23] = False
    assert torch.equal(_bits(after[:, keep]), _bits(slab[:, keep])), "bytes outside the written slice changed"
    assert (_tail(sg) == POISON).all(), "wrote past the slab"


def test_affine_act_and_backward_at_exactly_zero_preactivation(K):
    """x = 0 and shift = 0: every pre-activation is exactly zero.  Forward and gradient must be what
    oracle.functional's relu (clamp_min) and leaky_relu (where(x >= 0, ...)) give under float64 autograd: y = 0 and the
    gradient passes with factor 1 for both."""
    from oracle import functional as OF
    shape = (2, 3, 4, 5)
    x, dy = torch.zeros(shape), seeded(shape, 67)
    sc, sh = 1 + 0.4 * seeded((3,), 68), torch.zeros(3)
    mean, inv = torch.zeros(3), torch.ones(3)
    for act, fn in ((ACT_RELU, OF.relu), (ACT_LEAKY02, OF.leaky_relu)):
        xr = x.double().requires_grad_(True)
        yr = fn(xr * sc.double().view(1, 3, 1, 1) + sh.double().view(1, 3, 1, 1))
        yr.backward(dy.double())
        y = K.affine_act(_dev(x), sc.to(DEV), sh.to(DEV), act)
        assert torch.equal(y.cpu().double(), yr.detach()), f"act {act}: forward at zero"
        dg, db, dx = K.bn_act_bwd(_dev(dy), _dev(x), sc.to(DEV), sh.to(DEV), mean.to(DEV), inv.to(DEV), act, False)
        _hold("zero pre-activation", f"act {act}: dx at zero", dx, _np(xr.grad), 8 * U * np.abs(_np(xr.grad)))
        assert (_np(dx) != 0).all(), f"act {act}: the oracle passes the gradient at zero"
        ref_db = NU.channel_sum(dy)
        _hold("zero pre-activation", f"act {act}: dbeta at zero", db, ref_db, SUM_TERMS * U * NU.channel_abs_sum(dy))
        rdg, rdb, rdx = NU.bn_act_bwd(dy, x, sc, sh, mean, inv, act, False)       # the reference agrees with the oracle
        assert np.array_equal(rdx, _np(xr.grad)) and np.array_equal(rdb, ref_db)


# =====================================================================================================================
# 4. backward of act(bn(x))
# =====================================================================================================================
def _bwd_inputs(shape, train, seed):
    """x ~ N(channel mean, 1.5), dy ~ N(0, 1); mean / invstd are the fp64 batch statistics rounded to float32 (train)
    or running statistics (eval); scale / shift the fp64 fold of those rounded to float32.  |beta| >= 0.15 keeps the
    pre-activation of a one-element channel (xhat = 0, so pre = beta) away from the activation kink."""
    C = shape[1]
    x = seeded(shape, seed) * 1.5 + torch.tensor([3.0, -2.0, 0.5])[:C].view(1, C, *([1] * (len(shape) - 2)))
    dy = seeded(shape, seed + 1)
    gamma = 1 + 0.3 * seeded((C,), seed + 2)
    b = seeded((C,), seed + 3)
    beta = torch.sign(b) * (0.15 + 0.3 * b.abs())
    if train:
        st = NU.channel_stats(x)
        mean, inv = _r32(st.mean), _r32(NU.invstd(st.var, EPS))
    else:
        mean = torch.tensor([3.0, -2.0, 0.5])[:C] + 0.2 * seeded((C,), seed + 4)
        inv = _r32(NU.invstd(1.5 + seeded((C,), seed + 5) ** 2, EPS))
    scale, shift = (_r32(v) for v in NU.fold(gamma, beta, mean, inv))
    return x, dy, scale, shift, mean, inv


def _kink(x, scale, shift, act):
    """elements whose fp64 pre-activation is within 4u (|x * sc| + |sh|) of the kink: the float32 fma may land on the
    other side, so they are left out of elementwise comparisons; their share must stay <= 0.1 %"""
    xa = NU.f64(x)
    if act == ACT_NONE:
        return np.zeros(xa.shape, dtype=bool)
    pre = NU.preact(x, scale, shift)
    out = np.abs(pre) < 4 * U * (np.abs(xa * _cb(scale, xa)) + np.abs(_cb(shift, xa)))
    share = out.mean()
    print(f"[norm] kink share act={act} {xa.shape}: {share:.3e} ({int(out.sum())} of {out.size})")
    assert share <= 1e-3, f"excluded share {share:.3e} > 0.1 %"
    return out


def _bwd_bounds(x, dy, scale, shift, mean, inv, act, out):
    """dbeta <= (CHUNK/256 + 16) u sum|g|; dgamma <= (CHUNK/256 + 16) u sum|g xhat| + 4u sum|g| |mean invstd| (the
    rounding of (x - mu) * is).  An element left out at the kink may take either branch: it adds |dy| (|dy xhat|) to
    the bound of its channel, which is nothing when none is left out."""
    dg, db, g = NU.bn_sums(dy, x, scale, shift, mean, inv, act)
    xh = NU.xhat(x, mean, inv)
    dya = np.abs(NU.f64(dy)) * out
    b_db = SUM_TERMS * U * NU.channel_abs_sum(g) + NU.channel_sum(dya)
    b_dg = (SUM_TERMS * U * NU.channel_abs_sum(g * xh) + 4 * U * NU.channel_abs_sum(g) * np.abs(_np(mean) * _np(inv))
            + NU.channel_sum(dya * np.abs(xh)))
    return dg, db, g, xh, b_dg, b_db


def _dx_bound(g, xh, scale, dgamma, dbeta, inv_n):
    """dx = sc (g - k_db - xhat k_dg), k = sum * inv_n: elementwise <= 8u |sc| (|g| + |k_db| + |xhat k_dg|)"""
    return 8 * U * np.abs(_cb(scale, g)) * (np.abs(g) + np.abs(_cb(dbeta, g) * inv_n) + np.abs(xh * _cb(dgamma, g) * inv_n))


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_bn_act_bwd(K, shape, act, train):
    x, dy, scale, shift, mean, inv = _bwd_inputs(shape, train, 70 + shape[0] % 13)
    out = _kink(x, scale, shift, act)
    rdg, rdb, g, xh, b_dg, b_db = _bwd_bounds(x, dy, scale, shift, mean, inv, act, out)
    _, _, rdx = NU.bn_act_bwd(dy, x, scale, shift, mean, inv, act, train)
    dev = [_dev(dy), _dev(x)] + [t.to(DEV) for t in (scale, shift, mean, inv)]
    dg, db, dx = K.bn_act_bwd(*dev, act, train)
    what = f"bn_act_bwd {_sid(shape)} act={act} train={int(train)}"
    _hold("bwd dbeta", f"{what} dbeta", db, rdb, b_db)
    _hold("bwd dgamma", f"{what} dgamma", dg, rdg, b_dg)
    n = x.numel() // shape[1]
    inv_n = 1.0 / n if train else 0.0
    sca = np.abs(_cb(scale, g))
    b_dx = _dx_bound(g, xh, scale, rdg, rdb, inv_n) + sca * inv_n * (_cb(b_db, g) + np.abs(xh) * _cb(b_dg, g))
    assert dx.shape == dev[1].shape
    _hold("bwd dx", f"{what} dx", dx, rdx, b_dx, keep=~out)
    # sums only (dx = NULL) and sums into one (2, C) buffer: the same sums, bit for bit
    dg2, db2, none = K.bn_act_bwd(*dev, act, train, want_dx=False)
    assert none is None and torch.equal(_bits(dg2), _bits(dg)) and torch.equal(_bits(db2), _bits(db))
    sums = torch.full((2, shape[1]), POISON, device=DEV)
    dg3, db3, dx3 = K.bn_act_bwd(*dev, act, train, sums_out=sums)
    assert torch.equal(_bits(sums[0]), _bits(dg)) and torch.equal(_bits(sums[1]), _bits(db))
    assert torch.equal(_bits(dx3), _bits(dx))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_bn_act_bwd_dx_from_given_sums(K, shape, act):
    """SyncBN's second half: the sums of a twice-as-large global batch are handed in (float32), inv_n = 1 / (2 n)"""
    x, dy, scale, shift, mean, inv = _bwd_inputs(shape, True, 90 + shape[0] % 13)
    out = _kink(x, scale, shift, act)
    rdg, rdb, g, xh, _, _ = _bwd_bounds(x, dy, scale, shift, mean, inv, act, out)
    sdg, sdb = _r32(rdg * 1.75 + 0.3), _r32(rdb * 2.25 - 0.2)
    inv_n = NU.f32(1.0 / (2 * (x.numel() // shape[1])))
    rdx = NU.bn_dx(dy, x, scale, shift, mean, inv, sdg, sdb, inv_n, act)
    dx = K.bn_act_bwd_dx(_dev(dy), _dev(x), *[t.to(DEV) for t in (scale, shift, mean, inv, sdg, sdb)], inv_n, act)
    _hold("dx from sums", f"bn_act_bwd_dx {_sid(shape)} act={act}", dx, rdx,
          _dx_bound(g, xh, scale, _np(sdg), _np(sdb), inv_n), keep=~out)


@pytest.mark.parametrize("fn", ["bn_act_bwd", "bn_act_bwd_eval", "bn_act_bwd_dx"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("bhw", SLAB_SHAPES, ids=_sid)
def test_bn_bwd_accumulates_into_a_slab_slice(K, bhw, act, fn):
    """dy, x and dx are channel slices of three slabs of 5, 8 and 16 channels (three different batch strides);
    accumulate_dx adds onto the seeded dx slice (one more rounding: + u |dx0 + v|) and every other byte of the dx
    slab, and the chunk behind it, stays as it was"""
    B, H, W = bhw
    full = (B, 3, H, W)
    train = fn != "bn_act_bwd_eval"
    x, dy, scale, shift, mean, inv = _bwd_inputs(full, train, 110)
    out = _kink(x, scale, shift, act)
    rdg, rdb, g, xh, b_dg, b_db = _bwd_bounds(x, dy, scale, shift, mean, inv, act, out)
    dy_slab, x_slab, dx_slab = seeded((B, 5, H, W), 111), seeded((B, 8, H, W), 112), seeded((B, 16, H, W), 113)
    dy_slab[:, 1:4], x_slab[:, 2:5] = dy, x
    dyg, xg, dxg = _dev(dy_slab), _dev(x_slab), _dev(dx_slab)
    par = [t.to(DEV) for t in (scale, shift, mean, inv)]
    n = B * H * W
    if fn != "bn_act_bwd_dx":
        sdg, sdb, inv_n = rdg, rdb, 1.0 / n if train else 0.0     # eval: no mean / variance terms in dx
        extra = np.abs(_cb(scale, g)) * inv_n * (_cb(b_db, g) + np.abs(xh) * _cb(b_dg, g))
        dg, db, ret = K.bn_act_bwd(dyg[:, 1:4], xg[:, 2:5], *par, act, train, dx=dxg[:, 8:11], accumulate_dx=True)
        _hold("bwd dbeta", f"slab {fn} {_sid(bhw)} act={act} dbeta", db, rdb, b_db)
        _hold("bwd dgamma", f"slab {fn} {_sid(bhw)} act={act} dgamma", dg, rdg, b_dg)
    else:
        sdg, sdb, inv_n, extra = _r32(rdg * 1.75 + 0.3), _r32(rdb * 2.25 - 0.2), NU.f32(1.0 / (2 * n)), 0.0
        ret = K.bn_act_bwd_dx(dyg[:, 1:4], xg[:, 2:5], *par, sdg.to(DEV), sdb.to(DEV), inv_n, act, dx=dxg[:, 8:11],
                              accumulate_dx=True)
    ref = NU.f64(dx_slab[:, 8:11]) + NU.bn_dx(dy, x, scale, shift, mean, inv, sdg, sdb, inv_n, act, train)
    after = dxg.cpu()
    _hold("dx accumulate", f"slab {fn} {_sid(bhw)} act={act} dx", after[:, 8:11], ref,
          _dx_bound(g, xh, scale, _np(sdg), _np(sdb), inv_n) + extra + U * np.abs(ref), keep=~out)
    assert ret.data_ptr() == dxg[:, 8:11].data_ptr()
    keep = torch.ones(16, dtype=torch.bool)
    keep[8:11] = False
    assert torch.equal(_bits(after[:, keep]), _bits(dx_slab[:, keep])), "bytes outside the dx slice changed"
    assert (_tail(dxg) == POISON).all(), "wrote past the dx slab"
    assert torch.equal(_bits(dyg), _bits(dy_slab)) and torch.equal(_bits(xg), _bits(x_slab)), "an input changed"


# =====================================================================================================================
# 5. channel sum
# =====================================================================================================================
def _check_channel_sum(K, what, x, xg=None, seed_out=None):
    """(CHUNK/256 + 16) u sum|x| per channel; accumulate: one more rounding of out0 + sum"""
    xg = _dev(x) if xg is None else xg
    ref, bound = NU.channel_sum(x), SUM_TERMS * U * NU.channel_abs_sum(x)
    got = K.channel_sum(xg)
    assert got.shape == (x.shape[1],)
    _hold("channel_sum", what, got, ref, bound)
    out0 = seeded((x.shape[1],), 131 if seed_out is None else seed_out) * 3
    out = out0.clone().to(DEV)
    assert K.channel_sum(xg, out=out, accumulate=True) is out
    _hold("channel_sum accumulate", f"{what} accumulate", out, ref + _np(out0), bound + U * np.abs(ref + _np(out0)))
    out = torch.full((x.shape[1],), POISON, device=DEV)
    K.channel_sum(xg, out=out, accumulate=False)                    # overwrite: what was there does not matter
    assert torch.equal(_bits(out), _bits(got))


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_channel_sum(K, shape):
    x = seeded(shape, 120 + shape[0] % 7) + 0.25
    _check_channel_sum(K, f"channel_sum {_sid(shape)}", x)
    B, C, H, W = shape
    if B * C <= 65535:
        _check_channel_sum(K, f"channel_sum view(1, B*C, HW) {_sid(shape)}", x.reshape(1, B * C, H * W))


@pytest.mark.parametrize("B", [1, 63, 257, 65535])
def test_channel_sum_linear_bias_gradient(K, B):
    """dy.view(B, N, 1): one part per row, so the finalize loop runs ceil(B / 256) trips"""
    x = seeded((B, 5), 125) + 0.1
    _check_channel_sum(K, f"channel_sum view({B}, 5, 1)", x.view(B, 5, 1))


def test_channel_sum_slab_slice(K):
    for B, H, W in SLAB_SHAPES:
        slab = seeded((B, 32, H, W), 126) + 0.5
        _check_channel_sum(K, f"channel_sum slab {B}x{H}x{W}", slab[:, 8:11], xg=_dev(slab)[:, 8:11])


# =====================================================================================================================
# 6. argument limits
# =====================================================================================================================
def _limit_calls(K, x, small):
    """name -> (call, outputs that must stay untouched); ``small``: also the launchers that need more than x"""
    C = x.shape[1]
    v = lambda val: torch.full((C,), val, device=DEV)
    outs = {n: torch.full((C,), 7.0, device=DEV) for n in ("rm", "rv", "sum")}
    calls = {
        "gd_bn_stats": lambda: K.bn_stats(x, EPS, MOM, outs["rm"], outs["rv"]),
        "gd_bn_stats_local": lambda: K.bn_stats_local(x),
        "gd_channel_sum": lambda: K.channel_sum(x, out=outs["sum"], accumulate=True),
    }
    if small:
        outs["y"], outs["dx"], outs["dx2"] = (torch.full(x.shape, 7.0, device=DEV) for _ in range(3))
        outs["sums"] = torch.full((2, C), 7.0, device=DEV)
        par = [v(1.0), v(0.0), v(0.0), v(1.0)]
        calls["gd_affine_act"] = lambda: K.affine_act(x, None, None, ACT_RELU, out=outs["y"])
        calls["gd_bn_act_bwd_dx"] = lambda: K.bn_act_bwd_dx(x, x, *par, v(1.0), v(1.0), 1e-3, ACT_RELU, dx=outs["dx"])
        calls["gd_bn_act_bwd"] = lambda: K.bn_act_bwd(x, x, *par, ACT_RELU, True, dx=outs["dx2"], sums_out=outs["sums"])
    return calls, outs


def _expect_rejected(calls, outs):
    for name, call in calls.items():
        with pytest.raises(_err_type()) as e:
            call()
        assert name in str(e.value) and "too many parts" in str(e.value), f"{name}: {e.value}"
    torch.cuda.synchronize()
    for n, t in outs.items():
        assert (t == 7.0).all(), f"output {n} was written by a rejected call"


def test_more_than_65535_parts_is_rejected_by_every_launcher(K):
    """B * chunks = 65536 with one-element planes: an argument error before any launch, outputs untouched"""
    x = torch.zeros(65536, 1, 1, device=DEV)
    _expect_rejected(*_limit_calls(K, x, small=True))


def test_more_than_65535_parts_is_rejected_with_two_chunks_per_image(K):
    """B = 32768 images of 16385 elements (two chunks each): the count is B * chunks, not B.  The 2.1 GB input is
    allocated and never touched; only the launchers that need nothing else of that size take part."""
    x = torch.empty(32768, 1, 16385, device=DEV)
    calls, outs = _limit_calls(K, x, small=False)
    calls["gd_affine_act"] = lambda: K.affine_act(x, None, None, ACT_RELU, out=x)
    _expect_rejected(calls, outs)


def test_running_statistics_must_come_together(K):
    x = seeded((2, 3, 4, 4), 140).to(DEV)
    recs = torch.ones(2, 3, 3, device=DEV)
    one = torch.full((3,), 7.0, device=DEV)
    for name, call in (("gd_bn_stats", lambda a, b: K.bn_stats(x, EPS, MOM, a, b)),
                       ("gd_bn_stats_merge", lambda a, b: K.bn_stats_merge(recs, EPS, MOM, a, b))):
        for a, b in ((one, None), (None, one)):
            with pytest.raises(_err_type()) as e:
                call(a, b)
            assert name in str(e.value) and "must come together" in str(e.value)
    torch.cuda.synchronize()
    assert (one == 7.0).all()
