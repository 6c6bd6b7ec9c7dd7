"""float64 reference of csrc/resample.hip and of the pixel-major pooling of csrc/nhwc.hip: bicubic and bilinear resize
(forward and backward), the fused input preamble, the nine-plane tap sum with its adjoint, and the 2x2 max-pool with its
backward.  numpy only, no GPU; written from the definitions, not from ATen (tests/test_resample_reference.py holds it to
ATen in float64).

A resize is separable and linear: per axis a dense weight matrix W of shape (n_out, n_in), forward  Wy . x . Wx^T,
backward  Wy^T . dy . Wx  -- the exact transpose of the same matrices, there is no second implementation.  A matrix
is the sum over ALL integer tap positions j of kernel(src_o - j), added at column clamp(j, 0, n_in - 1): the four
(bicubic, A = -0.75) or two (bilinear) taps with a non-zero kernel value, clamped taps piling up on the border index.
The source coordinate of output o is  rs * (o + 0.5) - 0.5;  bilinear clamps it at 0 from below.  ``rs`` is an argument:
a GPU test passes the float32 value the kernel receives, widened (``f32``), so both sides use one ratio.

``Axis`` also carries E, an elementwise bound on |W_float - W|, W_float being the weights the kernel forms in float32:
  * a coordinate part.  The kernel's float32 coordinate is fl(fl(rs * (o + 0.5)) - 0.5): two roundings, off by at most
    delta_o = 2 u (|src_o| + 1), u = 2^-24.  The kernels are Lipschitz in the coordinate, also across a change of
    floor(src): |k(s + d) - k(s)| <= |d| sup|k'|, and sup|k'| over [s - d, s + d] is at most |k'(s)| + 4.5 d for the
    cubic (|k''| <= 4.5, k' continuous) and 1 for the hat, on every tap whose kernel support is within d.  For a ratio
    that is a power of two the float32 coordinate is exact and this part is ABSENT (delta = 0).
  * an evaluation part (bicubic only): the cubic polynomials in Horner form in float32.  Outer weights
    ((A x - 5A) x + 8A) x - 4A with x in [1, 2]: running error 4.5u, 16.5u, 36.5u over the three steps, plus the rounding
    of x = t + 1 or 2 - t times |k'| <= 0.75: below 38u.  Inner weights: below 11u.  ``W_EVAL = 40`` u on each tap.
    The bilinear weights are lam (exact: src - floor(src)) and 1 - lam (one rounding, counted in the chain below).
``resize_bound`` turns these into an elementwise bound on the result."""
import numpy as np

U = 2.0 ** -24            # unit roundoff of float32
A = -0.75                 # the cubic convolution parameter
W_EVAL = 40.0             # float32 evaluation of one cubic weight: at most 40 u absolute (module text)
C_FWD_CUBIC = 10.0        # 4 + 4 FMAs of the forward chain, each one rounding, plus margin: relative to the abs image
C_FWD_LINEAR = 8.0        # 1 - lx, 2 products + 1 sum, 1 - ly, 2 products + 1 sum: at most 8 roundings on any path
C_BWD = 32.0              # gather: up to 3 additions per collected weight, 14 + 14 FMAs along x and y


def f64(t):
    """torch tensor / array / scalar -> float64 ndarray (a copy)"""
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.array(t, dtype=np.float64)


def f32(v):
    """the double value of ``v`` rounded to float32: what a ``float`` argument of the C ABI holds"""
    return float(np.float32(v))


def out_size(n, scale_factor):
    """F.interpolate's output size for a scale factor: floor(n * s), in double"""
    return int(np.floor(float(n) * float(scale_factor)))


# ---- kernels -------------------------------------------------------------------------------------------------------
def cubic_kernel(s):
    s = np.abs(s)
    inner = ((A + 2.0) * s - (A + 3.0)) * s * s + 1.0
    outer = ((A * s - 5.0 * A) * s + 8.0 * A) * s - 4.0 * A
    return np.where(s <= 1.0, inner, np.where(s < 2.0, outer, 0.0))


def cubic_kernel_slope(s):
    """|k'(s)|"""
    s = np.abs(s)
    inner = 3.0 * (A + 2.0) * s * s - 2.0 * (A + 3.0) * s
    outer = 3.0 * A * s * s - 10.0 * A * s + 8.0 * A
    return np.abs(np.where(s <= 1.0, inner, np.where(s < 2.0, outer, 0.0)))


def hat_kernel(s):
    return np.maximum(1.0 - np.abs(s), 0.0)


def is_pow2(v):
    m, _ = np.frexp(float(v))
    return m == 0.5


class Axis:
    """one axis of a resize: W (n_out, n_in) float64 weights, E (n_out, n_in) bound on |W_float32 - W|"""

    def __init__(self, W, E, src):
        self.W, self.E, self.src = W, E, src
        self.n_out, self.n_in = W.shape

    @property
    def absW(self):
        return np.abs(self.W)


def source_coords(n_out, rs):
    return float(rs) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5


def coord_delta(src, rs):
    """bound on the float32 coordinate's distance from ``src``; zero for a power-of-two ratio (exact arithmetic)"""
    return np.zeros_like(src) if is_pow2(rs) else 2.0 * U * (np.abs(src) + 1.0)


def _axis(n_in, n_out, rs, cubic):
    src = source_coords(n_out, rs)
    delta = coord_delta(src, rs)
    if not cubic:
        src = np.maximum(src, 0.0)        # clamping is 1-Lipschitz: delta carries over
    reach = 2.0 if cubic else 1.0
    W, E = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    rows = np.arange(n_out)
    lo, hi = int(np.floor(src.min())) - 3, int(np.ceil(src.max())) + 3
    for j in range(lo, hi + 1):
        col = min(max(j, 0), n_in - 1)
        s = src - j
        near = np.abs(s) <= reach + delta         # taps the float32 coordinate could reach
        if cubic:
            W[rows, col] += cubic_kernel(s)
            E[rows, col] += np.where(near, delta * (cubic_kernel_slope(s) + 4.5 * delta) + W_EVAL * U, 0.0)
        else:
            W[rows, col] += hat_kernel(s)
            E[rows, col] += np.where(near, delta, 0.0)
    return Axis(W, E, src)


def cubic_axis(n_in, n_out, rs):
    return _axis(int(n_in), int(n_out), float(rs), True)


def linear_axis(n_in, n_out, rs=None):
    """bilinear, align_corners = False; the ratio defaults to what gd_bilinear_* form: float32 n_in / n_out"""
    if rs is None:
        rs = float(np.float32(n_in) / np.float32(n_out))
    return _axis(int(n_in), int(n_out), float(rs), False)


# ---- resize --------------------------------------------------------------------------------------------------------
def _apply(Ly, x, Rx):
    """Ly . x . Rx^T over the two trailing axes"""
    return np.matmul(np.matmul(Ly, f64(x)), Rx.T)


def resize_fwd(x, ay: Axis, ax: Axis):
    """(..., n_in_y, n_in_x) -> (..., n_out_y, n_out_x)"""
    return _apply(ay.W, x, ax.W)


def resize_bwd(dy, ay: Axis, ax: Axis):
    """the adjoint: (..., n_out_y, n_out_x) -> (..., n_in_y, n_in_x)"""
    return _apply(ay.W.T, dy, ax.W.T)


def abs_image(x, ay: Axis, ax: Axis, backward=False):
    """|Wy| . |x| . |Wx|^T (forward) or |Wy|^T . |dy| . |Wx| (backward)"""
    if backward:
        return _apply(ay.absW.T, np.abs(f64(x)), ax.absW.T)
    return _apply(ay.absW, np.abs(f64(x)), ax.absW)


def resize_bound(x, ay: Axis, ax: Axis, c, backward=False):
    """elementwise bound on |kernel - reference| for a kernel that forms float32 weights W + e, |e| <= E, and sums the
    products in a chain whose roundings amount to a relative c u of each product:
        sum (Wy + ey)(Wx + ex) x (1 + theta) - sum Wy Wx x,   |theta| <= c u
      <= c u  (|Wy| + Ey) |x| (|Wx| + Ex)^T  +  [ (|Wy| + Ey) |x| (|Wx| + Ex)^T - |Wy| |x| |Wx|^T ].
    The first term is the arithmetic term on the absolute-weight image, the bracket is the weight (coordinate and
    evaluation) term; with E = 0 the bracket vanishes."""
    ax_ = np.abs(f64(x))
    Ly, Rx = ay.absW + ay.E, ax.absW + ax.E
    if backward:
        full, plain = _apply(Ly.T, ax_, Rx.T), _apply(ay.absW.T, ax_, ax.absW.T)
    else:
        full, plain = _apply(Ly, ax_, Rx), _apply(ay.absW, ax_, ax.absW)
    return c * U * full + (full - plain)


# ---- the input preamble --------------------------------------------------------------------------------------------
def combine_axes(H1, W1, rs1, H2, W2, rs2, Ho, Wo):
    return (cubic_axis(H1, Ho, rs1), cubic_axis(W1, Wo, rs1)), (cubic_axis(H2, Ho, rs2), cubic_axis(W2, Wo, rs2))


def combine_inputs(lr, aux, rs1, rs2, Ho, Wo):
    """cat([bicubic(lr), bicubic(aux)], 1) at the common output size; returns the result and its bound"""
    a1, a2 = combine_axes(lr.shape[2], lr.shape[3], rs1, aux.shape[2], aux.shape[3], rs2, Ho, Wo)
    ref = np.concatenate([resize_fwd(lr, *a1), resize_fwd(aux, *a2)], 1)
    bound = np.concatenate([resize_bound(lr, *a1, C_FWD_CUBIC), resize_bound(aux, *a2, C_FWD_CUBIC)], 1)
    return ref, bound


# ---- tap sum -------------------------------------------------------------------------------------------------------
def _shift(p, dy_, dx_):
    """q[y, x] = p[y + dy_, x + dx_], zero outside"""
    H, W = p.shape[-2:]
    out = np.zeros_like(p)
    ys, xs = slice(max(0, -dy_), min(H, H - dy_)), slice(max(0, -dx_), min(W, W - dx_))
    yd, xd = slice(max(0, dy_), min(H, H + dy_)), slice(max(0, dx_), min(W, W + dx_))
    out[..., ys, xs] = p[..., yd, xd]
    return out


def shift_sum9_fwd(u, bias=None):
    """(B, 9, H, W) -> (B, 1, H, W): y[p] = bias + sum_tap u_tap[p + off_tap], off_tap = (tap // 3 - 1, tap % 3 - 1)"""
    u = f64(u)
    y = np.zeros((u.shape[0], 1) + u.shape[2:])
    for t in range(9):
        y[:, 0] += _shift(u[:, t], t // 3 - 1, t % 3 - 1)
    return y if bias is None else y + f64(bias).reshape(())


def shift_sum9_abs(u, bias=None):
    """sum of the magnitudes that enter one output: |bias| + sum_tap |u_tap[p + off_tap]|"""
    return shift_sum9_fwd(np.abs(f64(u)), None if bias is None else np.abs(f64(bias)))


def shift_sum9_bwd(dy):
    """the adjoint: du[b][tap][q] = dy[b][q - off_tap], zero outside; (B, 1, H, W) -> (B, 9, H, W)"""
    dy = f64(dy)
    du = np.zeros((dy.shape[0], 9) + dy.shape[2:])
    for t in range(9):
        du[:, t] = _shift(dy[:, 0], -(t // 3 - 1), -(t % 3 - 1))
    return du


# ---- 2x2 max-pool --------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
# windows in row-major order: all equal, all zero, zeros of both signs, a tie of the maximum in each of the six pairs,
# infinities, one NaN in each position, several NaNs, a NaN next to an infinity, a negative tie
HAND_WINDOWS = [
    [3.0, 3.0, 3.0, 3.0], [0.0, 0.0, 0.0, 0.0], [-0.0, 0.0, 0.0, -0.0],
    [5.0, 5.0, 1.0, 2.0], [5.0, 1.0, 5.0, 2.0], [5.0, 1.0, 2.0, 5.0], [1.0, 5.0, 5.0, 2.0], [1.0, 5.0, 2.0, 5.0], [1.0, 2.0, 5.0, 5.0],
    [INF, INF, 1.0, INF], [1.0, INF, INF, -INF], [-INF, -INF, -INF, -INF], [-INF, -1.0, -INF, -1.0],
    [NAN, 1.0, 2.0, 3.0], [4.0, NAN, 2.0, 3.0], [4.0, 1.0, NAN, 3.0], [4.0, 1.0, 2.0, NAN],
    [NAN, 1.0, NAN, 3.0], [INF, NAN, 1.0, 2.0], [NAN, NAN, NAN, NAN], [-1.0, -2.0, -1.0, -3.0],
]


def hand_plane():
    """the hand-built windows side by side: a (2, 2 * n) float64 plane"""
    w = np.array(HAND_WINDOWS, dtype=np.float64).reshape(-1, 2, 2)      # (n, row, col)
    return np.ascontiguousarray(w.transpose(1, 0, 2).reshape(2, -1))


def _windows(x):
    """(..., H, W) -> (..., H/2, W/2, 4), the window in row-major order"""
    x = f64(x)
    H, W = x.shape[-2:]
    v = x.reshape(x.shape[:-2] + (H // 2, 2, W // 2, 2))
    return np.moveaxis(v, -3, -2).reshape(x.shape[:-2] + (H // 2, W // 2, 4))


def maxpool2_argmax(x):
    """ATen's scan of a window in row-major order: start at the first element; a later element replaces the maximum
    when it is greater or a NaN.  So ties go to the FIRST maximum, any NaN makes the result NaN, and the index is that of
    the LAST NaN.  Returns (values, index 0..3)."""
    w = _windows(x)
    m, arg = w[..., 0].copy(), np.zeros(w.shape[:-1], dtype=np.int64)
    for q in range(1, 4):
        v = w[..., q]
        with np.errstate(invalid="ignore"):
            take = (v > m) | np.isnan(v)
        m, arg = np.where(take, v, m), np.where(take, q, arg)
    return m, arg


def maxpool2_fwd(x):
    return maxpool2_argmax(x)[0]


def maxpool2_bwd(x, dy, relu_mask=False):
    """dx = dy at the argmax of each window, zero elsewhere; relu_mask: nothing where the maximum is not > 0
    (a NaN maximum is not > 0)"""
    m, arg = maxpool2_argmax(x)
    g = f64(dy)
    if relu_mask:
        with np.errstate(invalid="ignore"):
            g = np.where(m > 0, g, 0.0)
    out = np.zeros(m.shape + (4,))
    np.put_along_axis(out, arg[..., None], g[..., None], -1)
    Ho, Wo = m.shape[-2:]
    out = np.moveaxis(out.reshape(m.shape[:-2] + (Ho, Wo, 2, 2)), -2, -3)
    return out.reshape(m.shape[:-2] + (2 * Ho, 2 * Wo))
