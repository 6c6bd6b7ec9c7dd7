"""Exact-arithmetic data and fp64 references for the convolution kernels (host only: no GPU import).

Operands are small integers (+-1 by default), so every product of two bf16 / f32 operands is an exact integer in fp32 and
every partial sum is an integer whose magnitude is at most sum|terms|.  While sum|terms| < 2^24 an fp32 accumulation is
exact in ANY order, tiling, split or MFMA shape, so a kernel's result must equal the fp64 reference bit for bit; one
missing, doubled or mis-paired product changes an integer.  None of the value sets holds zero, so every dropped term
changes the sum.

Split ("x3") operands: the split kernels compute hi*hi + lo*hi + hi*lo and omit lo*lo BY DESIGN.  hilo() draws values
n + m 2^-10 (n, m in +-1), whose bf16 split is hi = n, lo = m 2^-10 with no rounding tie, and the reference of a split
route is that THREE-TERM sum in fp64 -- not the full product.  Its terms are multiples of 2^-10 ("unit"), so the same
argument holds with sum|terms| / unit < 2^24.  Integer data would leave every lo plane zero and could not see a dropped
lo product.

The case tables of tests/test_gpu_conv_exact.py live here as well, so that tests/test_conv_exact_reference.py can check
on the host, for every row, the conditions that make a zero-tolerance comparison legitimate."""
import torch
import torch.nn.functional as F

PM1 = (-1, 1)
BIAS_VALS = (-3, -2, -1, 1, 2, 3)        # bias and residual
SCALE_VALS = (-2, -1, 1, 2)              # in_scale: fmaf(v, sc, sh) is exact and relu(.) a small bf16-exact integer
SHIFT_VALS = (-2, -1, 0, 1, 2)           # in_shift
LO_UNIT = 2.0 ** -10                     # the lo part of hilo() values; also the unit of a three-term sum
SLOPE = 0.25                             # LeakyReLU slope of the exact tests: a power of two keeps quarter-integers exact
BF16 = torch.bfloat16


def ints(shape, seed, vals=PM1):
    """seeded draw from a value list, as fp32"""
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(vals, dtype=torch.float32)
    return v[torch.randint(len(vals), tuple(shape), generator=g)]


def hilo(shape, seed):
    """n + m 2^-10, n and m in +-1: hi = n, lo = m 2^-10, both non-zero and bf16-exact"""
    return ints(shape, seed) + ints(shape, seed + 7919) * LO_UNIT


def draw(shape, seed, x3):
    return hilo(shape, seed) if x3 else ints(shape, seed)


def split(v):
    """the kernels' split (gd_split_bf): hi = bf16(v), lo = bf16(v - hi); asserts hi + lo == v"""
    v = v.float()
    hi = v.to(BF16).float()
    lo = (v - hi).to(BF16).float()
    assert torch.equal(hi.double() + lo.double(), v.double()), "value is not a sum of two bf16 parts"
    return hi, lo


def three_term(op, a, b):
    """op(a_hi, b_hi) + op(a_lo, b_hi) + op(a_hi, b_lo) in fp64: what a split route computes (NO lo * lo term)"""
    ah, al = split(a)
    bh, bl = split(b)
    return op(ah, bh) + op(al, bh) + op(ah, bl)


def product(op, a, b, x3):
    """(value, sum|terms|) of the bilinear ``op`` in fp64; x3: the three-term sum of the split parts"""
    if not x3:
        return op(a, b), op(a.abs(), b.abs())
    ah, al = split(a)
    bh, bl = split(b)
    return three_term(op, a, b), op(ah.abs(), bh.abs()) + op(al.abs(), bh.abs()) + op(ah.abs(), bl.abs())


def conv(x, w, stride, pad):
    return F.conv2d(x.double(), w.double(), stride=stride, padding=pad)


def conv_in(dy, w, in_hw, stride, pad):
    shape = (dy.shape[0], w.shape[1], in_hw[0], in_hw[1])
    return torch.nn.grad.conv2d_input(shape, w.double(), dy.double(), stride=stride, padding=pad)


def conv_w(dy, x, k, stride, pad):
    return torch.nn.grad.conv2d_weight(x.double(), (dy.shape[1], x.shape[1], k, k), dy.double(), stride=stride, padding=pad)


def prologue(x, sc, sh, relu):
    """the fused input transform relu(sc x + sh), exact in fp32 for the value sets above"""
    if sc is None:
        return x
    v = x.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    v = v.clamp_min(0) if relu else v
    assert torch.equal(v.float().double(), v)
    return v.float()


def activate(v, act, slope=SLOPE):
    """act: None / "relu" / "leaky" (``slope``, a power of two) / "leaky02" (the slope 0.2 baked into GD_ACT_LEAKY02 and
    the generic kernels: ONE fp32 multiply by float32(0.2))"""
    if act is None:
        return v
    if act == "relu":
        return v.clamp_min(0)
    if act == "leaky":
        return torch.where(v > 0, v, v * slope)
    assert act == "leaky02"
    assert torch.equal(v.float().double(), v)
    return torch.where(v >= 0, v, (v.float() * torch.tensor(0.2, dtype=torch.float32)).double())


def _cb(t):
    return t.double()[None, :, None, None]


def fwd_ref(x, w, stride, pad, *, x3=False, sc=None, sh=None, in_relu=False, bias=None, res=None, alpha=1.0, act=None,
            slope=SLOPE, base=None):
    """act(alpha conv(relu(sc x + sh), w) + bias + res) + base in fp64 -> (value, sum|terms|, pre-activation)"""
    assert not (act == "leaky02" and (res is not None or base is not None)), "the compiler may contract 0.2 v + r into an FMA"
    val, mag = product(lambda a, b: conv(a, b, stride, pad), prologue(x, sc, sh, in_relu), w, x3)
    val, mag = val * alpha, mag * abs(alpha)
    if bias is not None:
        val, mag = val + _cb(bias), mag + _cb(bias).abs()
    if res is not None:
        val, mag = val + res.double(), mag + res.double().abs()
    pre = val
    val = activate(val, act, slope)
    if base is not None:
        val, mag = val + base.double(), mag + base.double().abs()
    return val, mag, pre


def dgrad_ref(dy, w, in_hw, stride, pad, *, x3=False, mask=None, slope=0.0, res=None, alpha=1.0, base=None):
    """alpha conv^T(dy, w) * [mask > 0 ? 1 : slope] + res + base in fp64 -> (value, sum|terms|)"""
    val, mag = product(lambda a, b: conv_in(a, b, in_hw, stride, pad), dy, w, x3)
    val, mag = val * alpha, mag * abs(alpha)
    if mask is not None:
        f = torch.where(mask.double() > 0, 1.0, float(slope)).double()
        val, mag = val * f, mag * f
    for t in (res, base):
        if t is not None:
            val, mag = val + t.double(), mag + t.double().abs()
    return val, mag


def wgrad_ref(dy, x, k, stride, pad, *, x3=False, sc=None, sh=None, in_relu=False, base=None):
    """weight gradient (of the prologue'd input) in fp64 -> (value, sum|terms|)"""
    val, mag = product(lambda a, b: conv_w(a, b, k, stride, pad), dy, prologue(x, sc, sh, in_relu), x3)
    if base is not None:
        val, mag = val + base.double(), mag + base.double().abs()
    return val, mag


def bgrad_ref(dy):
    return dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))


def to_store(ref64, kind, mag, unit=1.0):
    """the bits a kernel must store for the exact fp64 value ``ref64`` whose terms are multiples of ``unit``:
    "f32"   asserts sum|terms| / unit < 2^24 on every element and that the value is an fp32 number -> ref.float()
    "bf16"  the same, then ONE round-to-nearest-even of that exact fp32 value -> (ref.to(bf16), share of elements the
            rounding changed)
    "split" the same, then the kernels' split of the fp32 value -> (hi, lo) bf16"""
    assert float(mag.max()) / unit < 2.0 ** 24, f"sum|terms| / unit = {float(mag.max()) / unit:.4g} is not below 2^24"
    f = ref64.float()
    assert torch.equal(f.double(), ref64), "the reference is not an fp32 number"
    if kind == "f32":
        return f
    if kind == "bf16":
        b = f.to(BF16)
        return b, (b.float() != f).double().mean().item()
    assert kind == "split"
    hi = f.to(BF16)
    return hi, (f - hi.float()).to(BF16)


def unit_of(x3, leaky=False):
    """the common unit of the terms: 1 for integers, 2^-10 for three-term sums, a quarter of that behind a 0.25 slope"""
    return (LO_UNIT if x3 else 1.0) * (SLOPE if leaky else 1.0)


def sign_share(t):
    """share of strictly positive elements (a ReLU / LeakyReLU mask must hold 25 - 75 % of each sign)"""
    return (t > 0).double().mean().item()


# ======================================================================================================================
# case tables.  pick_bm(M, Ck) of conv3x3.hip: Ck <= 32 and M > 64 -> 128; M <= 64 or 0 < M % 128 <= 64 -> 64; else 128.
# The generic / 1x1 / gemm_nt kernels: M <= 32 -> 32; M <= 64 or 0 < M % 128 <= 64 -> 64; else 128.
# ======================================================================================================================
def pick_bm(M, Ck):
    if Ck <= 32 and M > 64:
        return 128
    return 64 if (M <= 64 or (M % 128 != 0 and M % 128 <= 64)) else 128


def generic_bm(M):
    return 32 if M <= 32 else 64 if (M <= 64 or (M % 128 != 0 and M % 128 <= 64)) else 128


# a. halo / patch kernel conv3x3_halo_kernel<BM, 8|4, 1|2>: name -> (B, Cin, H, W, Cout, stride, forward BM, dgrad BM)
#    tiles are 8 (stride 1) / 4 (stride 2) rows x 32 pixels, channel chunks of 32
HALO = {
    "40to24": (2, 40, 9, 33, 24, 1, 64, 64),         # ragged 64-row M tile, Cin = 32 + 8, two x tiles, two y tiles
    "72to184": (1, 72, 17, 65, 184, 1, 64, 128),     # three M tiles (last 56 rows); dgrad: M = 72 -> ragged 128 tile
    "3to64": (1, 3, 7, 31, 64, 1, 64, 64),           # Cin < 32, one ragged tile in x and y; dgrad: M = 3
    "24to136": (1, 24, 9, 33, 136, 1, 128, 64),      # the Ck <= 32 and M > 64 branch (136 % 128 = 8 would give 64)
    "s2_40to24": (1, 40, 9, 67, 24, 2, 64, None),    # stride 2: Ho x Wo = 5 x 34 straddles the 4-row and 32-pixel tile
    "s2_64to128": (2, 64, 13, 35, 128, 2, 128, None),  # stride 2, BM 128, Ho x Wo = 7 x 18
}

# b. generic implicit-GEMM kernel conv_nn_kernel<32|64|128, mode>: name -> (B, Cin, H, W, Cout, ks, stride, pad, fwd BM,
#    dgrad BM); pixel tiles of 128, k tiles of 32 channels per tap.  A strided data gradient runs as stride^2 launches,
#    one per output parity class, skipping the taps that cannot reach the class.
GENERIC = {
    "k3s1p1": (2, 33, 9, 15, 40, 3, 1, 1, 64, 64),    # Ck = 33, 135 pixels = one full + one ragged pixel tile, ragged M
    "k4s2p1": (1, 5, 13, 11, 72, 4, 2, 1, 128, 32),   # ragged BM 128, Ck < 32; dgrad: four classes of four taps, odd 13 x 11
    "k1s2p0": (1, 16, 9, 7, 24, 1, 2, 0, 32, 32),     # dgrad: classes (0,1), (1,0), (1,1) have no live tap -> exact 0
    "k3s2p1": (2, 40, 12, 11, 72, 3, 2, 1, 128, 64),  # dgrad: classes with 1 / 2 / 2 / 4 taps
    "k1s1p0": (1, 8, 5, 7, 32, 1, 1, 0, 32, 32),      # 35 pixels: never the transpose-read kernel
    "k3s1p0": (1, 8, 10, 19, 16, 3, 1, 0, 32, 32),    # pad 0: 8 x 17 = 136 output pixels
}

# c. 1x1 transpose-read kernel conv1x1_tr_plain_kernel<32|64|128, X3?>: name -> (B, Cin, H, W, Cout, fwd BM, dgrad BM,
#    served by the transpose-read kernel); eligible when H W % 4 == 0
ONE = {
    "40to24": (2, 40, 6, 10, 24, 32, 64, True),       # HW = 60 < 128, Ck = 40; dgrad Ck = 24 < 32
    "24to72": (1, 24, 12, 13, 72, 128, 32, True),     # HW = 156: one full and one ragged pixel tile; ragged BM 128
    "72to136": (1, 72, 4, 9, 136, 64, 128, True),     # three 64-row M tiles; dgrad: ragged BM 128 with Ck = 136
    "fallback": (1, 32, 5, 7, 24, 32, 32, False),     # HW = 35: the generic kernel
}

# d. pixel-major kernels conv3x3_nhwc_kernel<BM, S, EPI>: name -> (B, Cin, H, W, Cout); K % 8 == 0 with ragged 32-chunks
#    (8, 40, 72), M in (8, 24, 72, 136).  Split rows see K = 3 Cin physical channels: pick_bm(M, 3 Cin).
NHWC_S1 = {
    "40to24": (2, 40, 9, 33, 24),     # fwd BM 64; dgrad operator M = 40, K = 24: 64
    "8to72": (1, 8, 7, 31, 72),       # fwd: K <= 32 and M > 64 -> 128; dgrad M = 8, K = 72: 64
    "72to136": (1, 72, 17, 35, 136),  # fwd 136 % 128 = 8 -> 64 (three tiles); dgrad M = 72, K = 136: 128
    "40to72": (1, 40, 16, 33, 72),    # fwd 128 (ragged) with two chunks; dgrad M = 40: 64; H W % 8 == 0: pack_split serves it
    "72to8": (1, 72, 9, 33, 8),       # M = 8; dgrad M = 72, K = 8 <= 32: 128
}
NHWC_S1_SPLIT = ("40to24", "8to72", "40to72")
NHWC_F32OUT = ("40to24", "40to72")               # EPI = 0 at BM 64 and 128, into a slab slice
NHWC_S2 = {
    "40to24": (2, 40, 9, 35, 24, "leaky"),     # BM 64, Ho x Wo = 5 x 18; dgrad: odd H and W -> odd-row / odd-column tails
    "8to72": (1, 8, 13, 67, 72, "relu"),       # BM 128 (K <= 32), Wo = 34 straddles the 32-pixel tile
    "72to136": (1, 72, 7, 11, 136, None),      # BM 64 x 3; dgrad2: two 64-row tiles of K = 72, five chunks of M = 136
}
NHWC_S2_SPLIT = ("40to24",)
OPS_WIDE = (1, 128, 8, 9, 40)       # ops._wide3x3: Cin >= 128, Cout > 32, H W % 8 == 0
OPS_X3 = (2, 32, 8, 8, 8)           # ops._x3_eligible: Cin >= 32, operand mode "x3"

# e. 3x3 weight gradient conv3x3_wgrad_kernel<NW, S, CS, PIPED, ORD>: name -> (B, Cin, H, W, Cout, stride, operand form,
#    prologue).  NW (waves = 32-row M tiles) is 2 / 4 / 6, whichever pads Cout least; CS (Cout <= 32, stride 1, >= 3 chunks
#    of Cin): waves = chunks, 3 or 4 per workgroup; PIPED: both operands 16-bit and (CS or NW >= 4 at stride 1, NW == 4 at
#    stride 2).  Forms: "f32" fp32 NCHW operands, "16" channel-major bf16 dY + pixel-major bf16 x.
WGRAD3 = {
    "cs3_piped": (2, 72, 9, 33, 24, 1, "16", False),
    "cs4_piped": (1, 104, 9, 33, 24, 1, "16", False),
    "cs3_f32": (2, 72, 9, 33, 24, 1, "f32", True),
    "cs4_f32": (1, 104, 9, 33, 24, 1, "f32", False),
    "nw4_piped": (1, 40, 9, 33, 72, 1, "16", False),
    "nw6_piped": (1, 40, 9, 33, 136, 1, "16", False),
    "nw2_s1": (2, 40, 9, 33, 24, 1, "f32", False),          # two chunks: not CS
    "nw4_s1": (1, 40, 9, 33, 72, 1, "f32", False),
    "nw6_s1": (1, 40, 9, 33, 136, 1, "f32", True),
    "nw4_s2_piped": (2, 40, 9, 35, 72, 2, "16", False),
    "nw2_s2": (2, 40, 9, 35, 24, 2, "f32", False),
    "nw4_s2": (2, 40, 9, 35, 72, 2, "f32", True),
    "nw6_s2": (1, 40, 9, 35, 136, 2, "16", False),          # 16-bit operands, but only NW == 4 is pipelined at stride 2
}

# 1x1 weight gradient = gemm_nt_kernel<32|64|128, mode, VEC> over kseg = B segments of klen = H W pixels; VEC (float4
# staging) needs klen % 32 == 0.  17 / 16 k-tiles of 32 -> two k-splits.  name -> (B, Cin, H, W, Cout, BM, VEC)
WGRAD1 = {
    "bm32": (2, 40, 16, 17, 24, 32, False),
    "bm32_vec": (2, 40, 16, 16, 24, 32, True),
    "bm64": (2, 24, 16, 17, 40, 64, False),
    "bm64_vec": (1, 24, 16, 32, 40, 64, True),
    "bm128": (2, 40, 16, 17, 72, 128, False),
    "bm128_vec": (2, 40, 16, 16, 72, 128, True),
}
WGRAD_IM2COL = (2, 8, 33, 35, 24, 4, 2, 1)    # 4x4 / stride 2 / pad 1: 2 x 16 x 17 = 544 output pixels = 17 k-tiles
LINEAR = (5, 777, 130)
STEM = (2, 17, 19, 64)                        # B, H, W, Co of the Discriminator1 stem, at ci = 1 and 3


def fwd_case(B, Cin, H, W, Cout, ks, stride, pad, seed, x3=False):
    """operands of one conv geometry, drawn once: x, w, dy, bias, in_scale, in_shift, res (output-shaped), base"""
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    sc, sh = ints((Cin,), seed + 4, SCALE_VALS), ints((Cin,), seed + 5, SHIFT_VALS)
    if x3:
        # sc n + sh must not be 0: a value 0 + m 2^-10 would split as hi = m 2^-10, lo = 0 and bring 2^-20 terms.  An even
        # shift behind |sc| = 1 and an odd one behind |sc| = 2 keep the hi parts odd integers of either sign.
        sh = torch.where(sc.abs() == 1, ints((Cin,), seed + 5, (-2, 0, 2)), ints((Cin,), seed + 5, (-1, 1)))
    return {"x": draw((B, Cin, H, W), seed, x3), "w": draw((Cout, Cin, ks, ks), seed + 1, x3),
            "dy": draw((B, Cout, Ho, Wo), seed + 2, x3), "bias": ints((Cout,), seed + 3, BIAS_VALS),
            "sc": sc, "sh": sh,
            "res": ints((B, Cout, Ho, Wo), seed + 6, BIAS_VALS), "base": ints((B, Cout, Ho, Wo), seed + 7, BIAS_VALS),
            "dres": ints((B, Cin, H, W), seed + 8, BIAS_VALS), "mask": ints((B, Cin, H, W), seed + 9),
            "Ho": Ho, "Wo": Wo}


# ======================================================================================================================
# expectations: per table row, the operands and {key: (fp64 value, sum|terms|, unit, store kind)} of every comparison the
# GPU file makes, plus the tensors whose sign acts as a ReLU / LeakyReLU mask.  Built once per row (lru_cache) and shared,
# unchanged, by the host checks and the GPU tests.
# ======================================================================================================================
import functools


class Expect:
    def __init__(self, ops):
        self.ops, self.wants, self.masks = ops, {}, {}

    def want(self, key, val, mag, unit=1.0, kind="f32"):
        self.wants[key] = (val, mag, unit, kind)

    def stored(self, key):
        val, mag, unit, kind = self.wants[key]
        return to_store(val, kind, mag, unit)


@functools.lru_cache(maxsize=None)
def halo_expect(name):
    B, Cin, H, W, Cout, stride, _, dbm = HALO[name]
    o = fwd_case(B, Cin, H, W, Cout, 3, stride, 1, 1000 + 20 * sorted(HALO).index(name))
    e = Expect(o)
    v, m, pre = fwd_ref(o["x"], o["w"], stride, 1, sc=o["sc"], sh=o["sh"], in_relu=True, bias=o["bias"], act="relu")
    e.want("prologue_bias_relu", v, m)
    e.masks["prologue (sc x + sh)"] = o["x"] * o["sc"][None, :, None, None] + o["sh"][None, :, None, None]
    e.masks["relu"] = pre
    v, m, _ = fwd_ref(o["x"], o["w"], stride, 1, base=o["base"])
    e.want("accumulate", v, m)
    if dbm is not None:
        v, m = dgrad_ref(o["dy"], o["w"], (H, W), 1, 1)
        e.want("dgrad", v, m)
    return e


PRECS = ("fp32", "bf16", "x3")


@functools.lru_cache(maxsize=None)
def generic_expect(name, prec):
    B, Cin, H, W, Cout, ks, stride, pad, _, _ = GENERIC[name]
    x3 = prec == "x3"
    o = fwd_case(B, Cin, H, W, Cout, ks, stride, pad, 2000 + 20 * sorted(GENERIC).index(name), x3)
    e = Expect(o)
    v, m, pre = fwd_ref(o["x"], o["w"], stride, pad, x3=x3, sc=o["sc"], sh=o["sh"], in_relu=True, bias=o["bias"], act="relu")
    e.want("prologue_bias_relu", v, m, unit_of(x3))
    e.masks["relu"] = pre
    v, m, pre = fwd_ref(o["x"], o["w"], stride, pad, x3=x3, bias=o["bias"], act="leaky02")
    e.want("bias_leaky02", v, m, unit_of(x3))
    e.masks["leaky02"] = pre
    v, m = dgrad_ref(o["dy"], o["w"], (H, W), stride, pad, x3=x3)
    e.want("dgrad", v, m, unit_of(x3))
    v, m = dgrad_ref(o["dy"], o["w"], (H, W), stride, pad, x3=x3, alpha=2.0, base=o["dres"])
    e.want("dgrad_alpha_accumulate", v, m, unit_of(x3))
    return e


DESC = (2, 33, 9, 15, 40, 48, 56)      # B, Ck, H, W, M, Mstore, ldo of the descriptor-feature case (3x3 / stride 1 / pad 1)


@functools.lru_cache(maxsize=None)
def desc_expect(prec):
    B, Cin, H, W, M, Mstore, ldo = DESC
    x3 = prec == "x3"
    o = fwd_case(B, Cin, H, W, M, 3, 1, 1, 2500, x3)
    e = Expect(o)

    def padded(v):          # rows M .. Mstore - 1 are act(0) = 0
        return torch.cat([v, torch.zeros(B, Mstore - M, H, W, dtype=v.dtype)], 1)
    # the bf16 store keeps 8 bits: it gets the integer (hi) parts alone as operands, in every mode, so that its one rounding
    # stays the identity; the lo planes count in the two fp32 stores below
    o["x_int"], o["w_int"] = split(o["x"])[0], split(o["w"])[0]
    v, m, pre = fwd_ref(o["x_int"], o["w_int"], 1, 1, x3=x3, bias=o["bias"], act="relu")
    e.want("layout1_bf16_bias_relu", padded(v), padded(m), unit_of(x3), "bf16")
    e.masks["relu"] = pre
    v, m, _ = fwd_ref(o["x"], o["w"], 1, 1, x3=x3, res=o["res"], alpha=2.0)
    e.want("layout1_res_alpha", padded(v), padded(m), unit_of(x3))
    o["base48"] = ints((B, Mstore, H, W), 2511, BIAS_VALS)
    e.want("layout0_res_alpha_accumulate", padded(v) + o["base48"].double(), padded(m) + o["base48"].double().abs(), unit_of(x3))
    return e


@functools.lru_cache(maxsize=None)
def one_expect(name, prec):
    B, Cin, H, W, Cout, _, _, _ = ONE[name]
    x3 = prec == "x3"
    o = fwd_case(B, Cin, H, W, Cout, 1, 1, 0, 3000 + 20 * sorted(ONE).index(name), x3)
    e = Expect(o)
    v, m, pre = fwd_ref(o["x"], o["w"], 1, 0, x3=x3, sc=o["sc"], sh=o["sh"], in_relu=True, bias=o["bias"], act="relu")
    e.want("prologue_bias_relu", v, m, unit_of(x3))
    e.masks["relu"] = pre
    v, m, _ = fwd_ref(o["x"], o["w"], 1, 0, x3=x3, res=o["res"], base=o["base"])
    e.want("res_accumulate", v, m, unit_of(x3))
    v, m = dgrad_ref(o["dy"], o["w"], (H, W), 1, 0, x3=x3)
    e.want("dgrad", v, m, unit_of(x3))
    return e


@functools.lru_cache(maxsize=None)
def nhwc_s1_expect(name, split):
    B, Cin, H, W, Cout = NHWC_S1[name]
    o = fwd_case(B, Cin, H, W, Cout, 3, 1, 1, 4000 + 20 * sorted(NHWC_S1).index(name), split)
    e = Expect(o)
    kind = "split" if split else "bf16"
    v, m, pre = fwd_ref(o["x"], o["w"], 1, 1, x3=split, bias=o["bias"], act="relu")
    e.want("fwd_bias_relu", v, m, unit_of(split), kind)
    e.masks["relu"] = pre
    e.masks["dgrad mask"] = o["mask"]
    v, m = dgrad_ref(o["dy"], o["w"], (H, W), 1, 1, x3=split, mask=o["mask"], res=o["dres"])
    e.want("dgrad_mask_res", v, m, unit_of(split), kind)
    if not split and name in NHWC_F32OUT:
        v, m, _ = fwd_ref(o["x"], o["w"], 1, 1, bias=o["bias"], act="relu")
        e.want("f32out", v, m)
    return e


@functools.lru_cache(maxsize=None)
def nhwc_s2_expect(name, split):
    B, Cin, H, W, Cout, act = NHWC_S2[name]
    o = fwd_case(B, Cin, H, W, Cout, 3, 2, 1, 4500 + 20 * sorted(NHWC_S2).index(name), split)
    e = Expect(o)
    kind = "split" if split else "bf16"
    v, m, pre = fwd_ref(o["x"], o["w"], 2, 1, x3=split, bias=o["bias"], act=act)
    e.want("fwd", v, m, unit_of(split, act == "leaky"), kind)
    if act is not None:
        e.masks[act] = pre
    e.masks["dgrad leaky mask"] = o["mask"]
    v, m = dgrad_ref(o["dy"], o["w"], (H, W), 2, 1, x3=split, mask=o["mask"], slope=SLOPE)
    e.want("dgrad_leaky", v, m, unit_of(split, True), kind)
    v, m = wgrad_ref(o["dy"], o["x"], 3, 2, 1, x3=split)
    e.want("wgrad_nhwc", v, m, unit_of(split))
    v, m = bgrad_ref(o["dy"])
    e.want("bias_sums", v, m, unit_of(split))
    return e


@functools.lru_cache(maxsize=None)
def ops_expect(route):
    x3 = route == "x3"
    B, Cin, H, W, Cout = OPS_X3 if x3 else OPS_WIDE
    o = fwd_case(B, Cin, H, W, Cout, 3, 1, 1, 4900 + int(x3), x3)
    e = Expect(o)
    u = unit_of(x3)
    v, m, pre = fwd_ref(o["x"], o["w"], 1, 1, x3=x3, bias=o["bias"], act="relu")
    e.want("y", v, m, u)
    e.masks["relu"] = pre
    g = (o["dy"].double() * (pre > 0)).float()          # the ReLU backward, exact
    o["g"] = g
    v, m = dgrad_ref(g, o["w"], (H, W), 1, 1, x3=x3)
    e.want("dx", v, m, u)
    # the weight gradient reads the forward's own 16-bit pack of x against the pack of g
    v, m = wgrad_ref(g, o["x"], 3, 1, 1, x3=x3)
    e.want("dw", v, m, u)
    v, m = bgrad_ref(g)
    e.want("db", v, m, u)
    return e


@functools.lru_cache(maxsize=None)
def wgrad3_expect(name):
    B, Cin, H, W, Cout, stride, form, pro = WGRAD3[name]
    o = fwd_case(B, Cin, H, W, Cout, 3, stride, 1, 5000 + 20 * sorted(WGRAD3).index(name))
    e = Expect(o)
    o["dw0"] = ints((Cout, Cin, 3, 3), 5999, BIAS_VALS)
    kw = dict(sc=o["sc"], sh=o["sh"], in_relu=True) if pro else {}
    v, m = wgrad_ref(o["dy"], o["x"], 3, stride, 1, **kw)
    e.want("dw", v, m)
    e.want("accumulate", v + o["dw0"].double(), m + o["dw0"].double().abs())
    if pro:
        e.masks["prologue (sc x + sh)"] = o["x"] * o["sc"][None, :, None, None] + o["sh"][None, :, None, None]
    return e


WGRAD3_SPLIT = (2, 40, 8, 33, 24)      # H W % 8 == 0 (pack_split), two 4-row tiles, W = 33 straddles the 32-pixel tile


@functools.lru_cache(maxsize=None)
def wgrad3_split_expect():
    B, Cin, H, W, Cout = WGRAD3_SPLIT
    o = fwd_case(B, Cin, H, W, Cout, 3, 1, 1, 5500, True)
    e = Expect(o)
    v, m = wgrad_ref(o["dy"], o["x"], 3, 1, 1, x3=True)
    e.want("dw", v, m, LO_UNIT)
    return e


@functools.lru_cache(maxsize=None)
def wgrad1_expect(name, prec):
    B, Cin, H, W, Cout, _, _ = WGRAD1[name]
    x3 = prec == "x3"
    o = fwd_case(B, Cin, H, W, Cout, 1, 1, 0, 6000 + 20 * sorted(WGRAD1).index(name), x3)
    e = Expect(o)
    v, m = wgrad_ref(o["dy"], o["x"], 1, 1, 0, x3=x3)
    e.want("dw", v, m, unit_of(x3))
    return e


@functools.lru_cache(maxsize=None)
def im2col_expect(prec):
    B, Cin, H, W, Cout, ks, stride, pad = WGRAD_IM2COL
    x3 = prec == "x3"
    o = fwd_case(B, Cin, H, W, Cout, ks, stride, pad, 6500, x3)
    e = Expect(o)
    v, m = wgrad_ref(o["dy"], o["x"], ks, stride, pad, x3=x3, sc=o["sc"], sh=o["sh"], in_relu=True)
    e.want("dw_prologue", v, m, unit_of(x3))
    return e


@functools.lru_cache(maxsize=None)
def linear_expect():
    Bn, Kin, Nout = LINEAR
    o = {"x": ints((Bn, Kin), 7000), "w": ints((Nout, Kin), 7001), "bias": ints((Nout,), 7002, BIAS_VALS),
         "dy": ints((Bn, Nout), 7003)}
    e = Expect(o)
    x, w, dy = o["x"].double(), o["w"].double(), o["dy"].double()
    e.want("y", x @ w.t() + o["bias"].double(), x.abs() @ w.abs().t() + o["bias"].double().abs())
    e.want("dx", dy @ w, dy.abs() @ w.abs())
    e.want("dw", dy.t() @ x, dy.abs().t() @ x.abs())
    e.want("db", dy.sum(0), dy.abs().sum(0))
    return e


@functools.lru_cache(maxsize=None)
def stem_expect(ci, split):
    """the Discriminator1 stem works in fp32 FMAs from the fp32 image: its split operand is the bf16 GRADIENT, read back as
    hi + lo, so the reference is the full product (there is no lo * lo term to omit: the image and weights are not split)"""
    B, H, W, Co = STEM
    o = fwd_case(B, ci, H, W, Co, 3, 2, 1, 7500 + 10 * ci + int(split))
    if split:
        o["dy"] = hilo(tuple(o["dy"].shape), 7599 + ci)
    e = Expect(o)
    u = unit_of(split)
    v, m, pre = fwd_ref(o["x"], o["w"], 2, 1, bias=o["bias"], act="leaky")
    e.want("fwd", v, m, SLOPE, "split" if split else "bf16")
    e.masks["leaky"] = pre
    v, m = dgrad_ref(o["dy"], o["w"], (H, W), 2, 1)
    e.want("dgrad", v, m, u)
    v, m = wgrad_ref(o["dy"], o["x"], 3, 2, 1)
    e.want("dw", v, m, u)
    v, m = bgrad_ref(o["dy"])
    e.want("db", v, m, u)
    return e


def all_expectations():
    """(table name, row id, Expect) of every row the GPU file runs"""
    for n in sorted(HALO):
        yield "halo", n, halo_expect(n)
    for p in PRECS:
        for n in sorted(GENERIC):
            yield "generic", f"{n}-{p}", generic_expect(n, p)
        yield "descriptor", p, desc_expect(p)
    for p in ("bf16", "x3"):
        for n in sorted(ONE):
            yield "1x1", f"{n}-{p}", one_expect(n, p)
    for n in sorted(NHWC_S1):
        yield "nhwc_s1", n, nhwc_s1_expect(n, False)
    for n in NHWC_S1_SPLIT:
        yield "nhwc_s1", n + "-split", nhwc_s1_expect(n, True)
    for n in sorted(NHWC_S2):
        yield "nhwc_s2", n, nhwc_s2_expect(n, False)
    for n in NHWC_S2_SPLIT:
        yield "nhwc_s2", n + "-split", nhwc_s2_expect(n, True)
    for r in ("wide", "x3"):
        yield "ops", r, ops_expect(r)
    for n in sorted(WGRAD3):
        yield "wgrad3", n, wgrad3_expect(n)
    yield "wgrad3", "split", wgrad3_split_expect()
    for p in PRECS:
        for n in sorted(WGRAD1):
            yield "wgrad1", f"{n}-{p}", wgrad1_expect(n, p)
        yield "im2col", p, im2col_expect(p)
    yield "linear", "5x777x130", linear_expect()
    for ci in (1, 3):
        for sp in (False, True):
            yield "stem", f"ci{ci}-{'split' if sp else 'plain'}", stem_expect(ci, sp)


def assert_same(got, want, what):
    """torch.equal, and on failure the count of differing elements with the first few indices and got / want, so that a
    seam column, a chunk's last channel, a parity class or a padding row is readable from the output"""
    got = got.detach().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} vs {want.dtype}"
    if torch.equal(got, want):
        return
    g, w = got.double(), want.double()
    bad = ~((g == w) | (g.isnan() & w.isnan()))
    lines = [f"  {tuple(i.tolist())}: got {g[tuple(i.tolist())].item()!r}, want {w[tuple(i.tolist())].item()!r}"
             for i in bad.nonzero()[:12]]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first indices:\n" + "\n".join(lines))
