/* gandanet.h -- C ABI of libgandanet_hip.so: the MI355X (gfx950) kernels behind the
 * GAN-DANet G+D training hot path.
 *
 * The reference (Aster32/GAN-DANet) has no native code and no FFI: its boundary for this
 * path is the Python nn.Module surface (models/__init__.py:12-23), and the arithmetic is
 * whatever ATen kernel each nn.* / F.* line dispatches to.  Each entry point below replaces
 * one such ATen call site; the reference line(s) it stands in for are cited per function.
 * INTEGRATION.md shows the ctypes stub a maintainer would add on the reference side.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer into memory owned by the caller (outputs and
 *     workspaces included); the library allocates nothing and keeps no pointer after return;
 *   - tensors are dense row-major fp32 NCHW unless a parameter says otherwise; "bs" = batch
 *     stride in ELEMENTS (lets a call address a channel slice of a wider slab);
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work (no host sync);
 *   - return 0 on success, <0 on error (-1 bad argument, -2 launch failure); the message is
 *     retrievable with gd_last_error(); nothing throws across the boundary;
 *   - re-entrant; no global state except the last-error string (thread-local).
 */
#ifndef GANDANET_H
#define GANDANET_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GD_VERSION 100 /* 0.1.0 */
/* deterministic mode (process-global): on = every reduction in a fixed order (split-K GEMM and the 3x3 weight
 * gradient run unsplit instead of combining partial sums with fp32 atomics) -- bitwise reproducible, slower. */
void gd_set_deterministic(int on);
int gd_get_deterministic(void);
/* how deterministic mode reduces over splits (process-global, read only while gd_get_deterministic() is 1):
 *   0 = unsplit (the default): one adder per output element, as described above;
 *   1 = ordered: the split kernels keep the split count of the default mode, every split writes its partial result with
 *       plain stores into slab [split] of a caller-owned workspace, and a reduce kernel adds the slabs in ascending split
 *       order in fp32 -- no atomics, bitwise reproducible, parallel.  It applies to the entry points that take a
 *       workspace (gd_conv3x3_wgrad_ws, gd_gemm_nt_ws, gd_disc_stem_wgrad_ws, gd_nhwc_to_nchw16_ws); their split count is
 *       the default mode's, clamped so that splits * output bytes <= ws_bytes, and a call whose workspace holds fewer
 *       than two slabs (or is NULL) runs unsplit.  The workspace must be 16-byte aligned; calls on one stream may share
 *       it (every use is stream-ordered), calls on different streams must not.
 * gd_set_det_reduce returns 0, or -1 for any other mode. */
int gd_set_det_reduce(int mode);
int gd_get_det_reduce(void);
/* how a split reduction combines its parts OUTSIDE deterministic mode (process-global):
 *   0 = ordered slabs (the default): the same partial slabs and ascending sum as above, in a workspace the library owns
 *       (one hipMalloc per device and stream, grown to the largest request, at most 256 MiB per request, kept); the output
 *       is not zeroed and not read unless the call accumulates; a caller's ws is not touched;
 *   1 = atomics: the parts are added with fp32 atomics onto the zeroed output (order-dependent rounding).
 * Discriminator1's stem gradient (gd_disc_stem_wgrad) uses atomics in both.  Returns 0, or -1 for any other mode. */
int gd_set_split_reduce(int mode);
int gd_get_split_reduce(void);
/* bytes of slab workspace the library currently holds (all devices and streams) */
size_t gd_split_ws_bytes(void);
int gd_version(void);
/* copies the calling thread's last error message (NUL terminated) into buf; returns its length */
int gd_last_error(char* buf, int n);
/* sizeof() of the two descriptor structs below, so a foreign binding can verify its mirror */
int gd_sizeof_conv_desc(void);
int gd_sizeof_gemm_nt_desc(void);

enum { GD_PREC_FP32 = 0, /* exact f32 MFMA (v_mfma_f32_32x32x2_f32) */
       GD_PREC_BF16 = 1, /* bf16 operands, f32 accumulate (v_mfma_f32_32x32x16_bf16) */
       GD_PREC_X3 = 2    /* split-bf16: fp32 operands staged as hi + lo bf16, hi*hi + lo*hi + hi*lo (~2^-16 relative):
                            gd_conv2d and gd_gemm_nt only */ };
enum { GD_ACT_NONE = 0, GD_ACT_RELU = 1, GD_ACT_LEAKY02 = 2, GD_ACT_SIGMOID = 3 };   /* sigmoid: gd_act_fwd/bwd only */

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution, "NN" form:   out[b][m][p] = sum_{tap,c} A[b][m][c][tap] * X~[b][c][p (+) tap]
 * One kernel serves nn.Conv2d forward (generator.py:20,34,63,108-110,148,188,214,218,222,228;
 * discriminator.py:62-65; VGG convs losses.py:41), its data gradient (transposed gather),
 * CAM's attention*X product with per-batch "weights" (generator.py:137), and the
 * data/weight gradients of nn.Linear (discriminator.py:66-67) viewed as 1x1 convolutions.
 * ---------------------------------------------------------------------------------------- */
typedef struct gd_conv_desc {
    int B;          /* batch count (grid z) */
    int M;          /* rows of A that exist (Cout forward, Cin for the data gradient) */
    int Mstore;     /* rows written (>= M; rows in [M, Mstore) are written as zeros + epilogue) */
    int Ck;         /* reduction channels (Cin forward, Cout for the data gradient) */
    int ks;         /* square kernel size (1, 3, ...) */
    int stride, pad;
    int transposed; /* 0: iy = oy*stride - pad + kh;  1: iy = (oy + pad - kh)/stride where divisible */
    int Hi, Wi;     /* spatial size of the tensor X being gathered */
    int Ho, Wo;     /* spatial size of the output */
    /* A element (b, m, c, tap) at a[b*a_bs + m*a_sm + c*a_sc + tap*a_st] */
    const float* a; long a_bs, a_sm, a_sc, a_st;
    /* X element (b, c, y, x) at x[b*x_bs + c*Hi*Wi + y*Wi + x] */
    const float* x; long x_bs;
    /* optional fused input transform X~ = relu?(X*in_scale[c] + in_shift[c]) (BatchNorm+ReLU of
       generator.py:36 folded into the consumer); padding stays zero.  NULL = identity */
    const float* in_scale; const float* in_shift; int in_relu;
    /* output */
    void* y; long y_bs;
    int out_layout;  /* 0: y[b*y_bs + m*Ho*Wo + p];  1: y[b*y_bs + p*ldo + m] (pixel-major) */
    int out_bf16;    /* 0 fp32, 1 bf16 */
    int ldo;
    /* epilogue: v = acc * (alpha ? *alpha : 1) + bias[m] + res[b*res_bs + m*Ho*Wo + p]; act; y (+)= v */
    const float* alpha; const float* bias; const float* res; long res_bs;
    int act; int accumulate;
    int precision;
    /* output sub-lattice (0,0,0 or step 1 = every pixel): only outputs (sub_oy + a*sub_step, sub_ox + b*sub_step)
       are computed.  gd_conv2d uses it internally to split the data gradient of a STRIDED convolution into
       stride^2 launches, one per output parity class, each visiting only the taps that can reach that class
       (a stride-2 3x3 gradient then does 9/4 instead of 9 tap-GEMMs per pixel). */
    int sub_oy, sub_ox, sub_step;
} gd_conv_desc;
int gd_conv2d(const gd_conv_desc* d, void* stream);

/* 3x3 / stride 1 / pad 1 fast path (bf16 MFMA): the input patch of a TH x 32 pixel tile is staged once in LDS
 * and reused by all nine taps; weights are pre-packed into `ws` (gd_conv3x3_ws_bytes(M, Ck) bytes, caller
 * owned).  Same descriptor and epilogue contract as gd_conv2d; serves the forward conv (transposed = 0) and
 * the data gradient (transposed = 1).  gd_conv3x3_eligible() tells whether a descriptor qualifies. */
size_t gd_conv3x3_ws_bytes(int M, int Ck);
int gd_conv3x3_eligible(const gd_conv_desc* d);
int gd_conv3x3(const gd_conv_desc* d, void* ws, size_t ws_bytes, void* stream);
/* weight gradient of the same convolution (bf16 MFMA, fp32 atomics across the pixel splits):
 * dw (Cout, Cin, 3, 3) = sum_{b,p} dy[b][co][p] * relu?(x*in_scale + in_shift)[b][ci][p (+) tap]; dw is overwritten.
 * dy_bf16 (may be NULL): a dense bf16 copy (B, Cout, Ho, Wo) of dy made by the caller (gd_pack_bf16); it is then read
 * instead of dy -- worth it when Cin spans several 32-channel chunks, each of which re-reads every dY tile.
 * x_nhwc16 (may be NULL; needs in_scale == NULL): a dense PIXEL-MAJOR bf16 copy (B, H, W, x_ld) of x (the transposed
 * output of gd_pack_bf16, x_ld = Cin rounded up to 8); the patch staging is then 16-byte copies instead of strided
 * 4-byte gathers + converts -- worth it for wide convs (the 2C -> C fuse convs of DANetAttention).  x_ld may exceed Cin: the
 * rows of a wider pixel-major tensor (the split-bf16 pack's [hi | lo | hi] channels) are then read from a column offset.
 * accumulate != 0: dw is added to instead of overwritten (the three launches of a split-bf16 weight gradient). */
int gd_conv3x3_wgrad(const float* dy, long dy_bs, const void* dy_bf16, const float* x, long x_bs, const void* x_nhwc16,
                     int x_ld, const float* in_scale, const float* in_shift, int in_relu, int B, int Cout, int Cin, int H,
                     int W, int stride, int accumulate, float* dw, void* stream);   /* H, W = INPUT size; stride 1 or 2 (pad 1) */
/* the same with a workspace for the ordered deterministic mode (slabs [split][Cout][Cin][9] fp32).  ws == NULL, or any
 * other mode: exactly gd_conv3x3_wgrad. */
int gd_conv3x3_wgrad_ws(const float* dy, long dy_bs, const void* dy_bf16, const float* x, long x_bs, const void* x_nhwc16,
                        int x_ld, const float* in_scale, const float* in_shift, int in_relu, int B, int Cout, int Cin, int H,
                        int W, int stride, int accumulate, float* dw, void* stream, void* ws, size_t ws_bytes);
/* host-only: the pixel-split count gd_conv3x3_wgrad_ws will launch for these sizes under the current modes with a
 * workspace of ws_bytes, and the bytes of it that launch uses (0 when it does not touch the workspace).  No GPU call.
 * ws_bytes = SIZE_MAX asks what an unclamped ordered launch needs. */
int gd_conv3x3_wgrad_plan(int B, int Cout, int Cin, int H, int W, int stride, size_t ws_bytes, int* splits, size_t* ws_needed);

/* ------------------------------------------------------------------------------------------
 * "NT" GEMM with the long reduction split over workgroups:
 *     C[b][m][n] (+)= alpha * sum_k A[b][m][k] * B~[b][n][k]        (k contiguous in both)
 * k runs over `kseg` segments of `klen` elements (segment = one image of a batch).
 * Serves the convolution weight gradient (B~ = im2col rows, k = output pixels), CAM's Gram
 * matrix X X^T (generator.py:133), nn.Linear forward (discriminator.py:76-77) and the
 * unfused fp32 PAM products (generator.py:117,120).
 * Partial sums of different k-splits are combined with fp32 atomics.
 * ---------------------------------------------------------------------------------------- */
typedef struct gd_gemm_nt_desc {
    int B, M, N;
    int kseg; long klen;
    /* A element (b, m, s, kk) at a[b*a_bs + s*a_ss + m*lda + kk] */
    const float* a; long a_bs, a_ss, lda;
    /* B plain (im2col == 0): element (b, n, s, kk) at bm[b*b_bs + s*b_ss + n*ldb + kk] */
    const float* bm; long b_bs, b_ss, ldb;
    /* B as im2col rows (im2col == 1): n = c*ks*ks + tap, kk = oy*Wo + ox of an Ho x Wo output;
       element = X~[s][c][oy*stride - pad + kh][ox*stride - pad + kw], X at bm[s*b_ss + c*Hi*Wi + ...] */
    int im2col, ks, stride, pad, Hi, Wi, Ho, Wo;
    /* optional X~ = relu?(X * in_scale[c] + in_shift[c]); the channel is c of the im2col row, or the B row n itself
       when im2col == 0 (1x1 weight gradient with a fused BatchNorm+ReLU input) */
    const float* in_scale; const float* in_shift; int in_relu;
    /* C element (b, m, n) at c[b*c_bs + m*ldc + n]; fp32 */
    float* c; long c_bs, ldc;
    const float* alpha;  /* device scalar or NULL */
    const float* bias;   /* per-n bias (added once) or NULL */
    int accumulate;      /* 0: C is overwritten (zeroed first when splits > 1);  1: C += */
    int splits;          /* k-splits (>=1); 0 = library picks */
    int precision;
} gd_gemm_nt_desc;
int gd_gemm_nt(const gd_gemm_nt_desc* d, void* stream);
/* the same with a workspace for the ordered deterministic mode: split s writes alpha * acc into a dense [split][B][M][N]
 * fp32 slab, the reduce kernel adds the bias once and writes through c_bs / ldc, honouring accumulate.  ws == NULL, or any
 * other mode: exactly gd_gemm_nt. */
int gd_gemm_nt_ws(const gd_gemm_nt_desc* d, void* stream, void* ws, size_t ws_bytes);
/* host-only: the k-split count gd_gemm_nt_ws will launch for this descriptor (its pointers are not read) under the
 * current modes with a workspace of ws_bytes, and the bytes of it that launch uses.  No GPU call. */
int gd_gemm_nt_plan(const gd_gemm_nt_desc* d, size_t ws_bytes, int* splits, size_t* ws_needed);

/* ------------------------------------------------------------------------------------------
 * BatchNorm2d (generator.py:32,61,149,189,219,223).  x is (B, C, H, W) with batch stride x_bs.
 * ---------------------------------------------------------------------------------------- */
/* per-channel batch statistics -> mean[C], invstd[C]; if running_* != NULL they are blended
 * (momentum, unbiased variance) exactly like nn.BatchNorm2d in train mode.
 * ws: workspace of gd_bn_stats_ws_floats(...) floats. */
size_t gd_bn_stats_ws_floats(int B, int C, long HW);
int gd_bn_stats(const float* x, long x_bs, int B, int C, long HW, float eps, float momentum,
                float* mean, float* invstd, float* running_mean, float* running_var, float* ws, void* stream);
/* scale[c] = gamma[c]*invstd[c], shift[c] = beta[c] - mean[c]*scale[c]  (the folded affine) */
int gd_bn_fold(const float* gamma, const float* beta, const float* mean, const float* invstd, int C,
               float* scale, float* shift, void* stream);
/* SyncBN (optional; torch.nn.SyncBatchNorm semantics on the BatchNorm2d sites of generator.py:32,61,149,189,
 * 219,223): gd_bn_stats_local reduces this rank's shard to stats (C, 3) = (count, mean, M2) per channel; the caller
 * all-gathers the records of all ranks into stats_all (world, C, 3); gd_bn_stats_merge Chan-merges them (fp64) into the
 * GLOBAL batch's mean / invstd (+ running statistics, unbiased variance of the global count).  Backward: gd_bn_act_bwd
 * with dx = NULL gives this rank's dgamma / dbeta (they are also the parameter gradients); after their all-reduce (sum)
 * gd_bn_act_bwd_dx forms dx with inv_n = 1 / (global batch * HW). */
int gd_bn_stats_local(const float* x, long x_bs, int B, int C, long HW, float* stats, float* ws, void* stream);
int gd_bn_stats_merge(const float* stats_all, int world, int C, float eps, float momentum, float* mean, float* invstd,
                      float* running_mean, float* running_var, void* stream);
int gd_bn_act_bwd_dx(const float* dy, long dy_bs, const float* x, long x_bs, const float* scale, const float* shift,
                     const float* mean, const float* invstd, const float* dgamma_sum, const float* dbeta_sum, float inv_n,
                     int B, int C, long HW, int act, float* dx, long dx_bs, int accumulate_dx, void* stream);
/* eval mode: invstd from running_var (also written to invstd_out when non-NULL) */
int gd_bn_fold_eval(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                    float eps, int C, float* scale, float* shift, float* invstd_out, void* stream);
/* out[c] (+)= sum over (B, HW) of x[b][c][:]  (bias gradients); ws: gd_bn_stats_ws_floats(B, C, HW) floats */
int gd_channel_sum(const float* x, long x_bs, int B, int C, long HW, float* out, int accumulate, float* ws,
                   void* stream);
/* y = act(x*scale[c] + shift[c]) */
int gd_affine_act(const float* x, long x_bs, const float* scale, const float* shift, int B, int C, long HW,
                  int act, float* y, long y_bs, void* stream);
/* backward of y = act(bn(x)): given dy (grad of y), x, the folded scale/shift, mean, invstd, gamma:
 * dgamma[C], dbeta[C] (overwritten) and dx (+)= ... ; ws as gd_bn_stats_ws_floats. */
int gd_bn_act_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* scale, const float* shift,
                  const float* mean, const float* invstd, const float* gamma, int B, int C, long HW, int act,
                  int train, float* dgamma, float* dbeta, float* dx, long dx_bs, int accumulate_dx, float* ws,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Resampling (nn.Upsample bicubic generator.py:221,225; F.interpolate bilinear generator.py:244;
 * bicubic down-sampling GAN_DANet_train.ipynb:L226,L231; VGG max-pool).
 * rscale_* = the coordinate scale ATen uses (1/scale_factor, or in/out when a size was given).
 * ---------------------------------------------------------------------------------------- */
int gd_bicubic_fwd(const float* x, int BC, int Hi, int Wi, float* y, int Ho, int Wo, float rscale_h,
                   float rscale_w, void* stream);
int gd_bicubic_bwd(const float* dy, int BC, int Hi, int Wi, float* dx, int Ho, int Wo, float rscale_h,
                   float rscale_w, void* stream);
/* last step of the generator tail (generator.py:242-247) in its collapsed form: final = conv3x3(C -> 1, pad 1) of
 * up2(c) + resize4(s) equals bias + sum over the nine taps of SHIFTED "tap planes" u (B, 9, H, W), each the channel
 * contraction sum_ch w[ch][tap] (.) done at low resolution and then resized (linear maps commute): only 9 planes instead
 * of C channels live at the output resolution.  y (B, 1, H, W); the backward scatters dy into the nine shifted planes. */
int gd_shift_sum9_fwd(const float* u, const float* bias, float* y, int B, int H, int W, void* stream);
int gd_shift_sum9_bwd(const float* dy, float* du, int B, int H, int W, void* stream);
/* input preamble of the train step (GAN_DANet_train.ipynb:L218-224), one launch, no cat pass:
 *   out (B, C1+C2, Ho, Wo) = cat([F.interpolate(lr (B,C1,H1,W1), scale_factor=1/rs1, mode='bicubic'),
 *                                 F.interpolate(aux (B,C2,H2,W2), scale_factor=1/rs2, mode='bicubic')], dim=1)
 * align_corners=False, antialias off; rs = input/output coordinate ratio (2.0 and 4.0 in the notebook). */
int gd_combine_inputs(const float* lr, int C1, int H1, int W1, float rs1, const float* aux, int C2, int H2, int W2,
                      float rs2, float* out, int B, int Ho, int Wo, void* stream); /* dx (BC,Hi,Wi) overwritten */
/* y = bilinear(x) (+ y if accumulate) ; or, when res != NULL, y = res + bilinear(x) in one pass: the skip
 * addition of generator.py:245 without a separate copy */
int gd_bilinear_fwd(const float* x, int BC, int Hi, int Wi, float* y, int Ho, int Wo, int accumulate,
                    const float* res, void* stream);
int gd_bilinear_bwd(const float* dy, int BC, int Hi, int Wi, float* dx, int Ho, int Wo, void* stream);
int gd_maxpool2_fwd(const float* x, int BC, int Hi, int Wi, float* y, void* stream);
int gd_maxpool2_bwd(const float* x, const float* dy, int BC, int Hi, int Wi, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pointwise / small reductions
 * ---------------------------------------------------------------------------------------- */
/* y = act(x) ; dx = dy * act'(y) computed from the OUTPUT y (valid for relu / leaky) */
int gd_act_fwd(const float* x, float* y, long n, int act, void* stream);
int gd_act_bwd(const float* y, const float* dy, float* dx, long n, int act, void* stream);
/* y = a*x + b*y  (a, b host scalars) */
int gd_axpby(const float* x, float a, float* y, float b, long n, void* stream);
/* y = (*s_dev) * x  (scale by a device scalar: loss weights / upstream scalar gradients, no host sync) */
int gd_scale_dev(const float* x, const float* s_dev, float* y, long n, int accumulate, void* stream);
/* dst[b][r][c] = src[b][r][c], r < R, c < Cc, independent batch strides and leading dimensions */
int gd_copy_rows(const float* src, long s_bs, long s_ld, float* dst, long d_bs, long d_ld, int B, int R, int Cc,
                 void* stream);
/* strided copy of a (B, C, HW) block: dst[b*d_bs + i] (+)= src[b*s_bs + i], i < C*HW */
int gd_copy_slab(const float* src, long s_bs, float* dst, long d_bs, int B, long chw, int accumulate, void* stream);
/* row softmax, in place capable: y[r][:] = softmax(sign * x[r][:]) over `cols` (CAM uses sign=-1:
 * softmax(max - E) == softmax(-E), generator.py:134-135) */
int gd_softmax_rows(const float* x, float* y, long rows, int cols, float sign, void* stream);
/* dx[r][:] = sign * p .* (dp - sum(dp .* p)) */
int gd_softmax_rows_bwd(const float* p, const float* dp, float* dx, long rows, int cols, float sign, void* stream);
/* out[0] (+)= sum_i a[i]*b[i]  (b == NULL: sum_i a[i]) -- gamma gradients ; ws >= 1024 floats */
int gd_dot(const float* a, const float* b, long n, float* out, int accumulate, float* ws, void* stream);
/* t[b][j][i] = s[b][i][j] : (B, R, Cc) -> (B, Cc, R) */
int gd_transpose(const float* s, float* t, int B, int R, int Cc, void* stream);
/* out = a + a^T for (B, n, n) */
int gd_add_transpose(const float* a, float* out, int B, int n, void* stream);

/* losses: value -> out[0] (fp32), gradient written when the pointer is non-NULL.  ws >= 2048 floats.
 * BCEWithLogits mean vs a constant label (GAN_DANet_train.ipynb:L190,L252-253,L261) */
int gd_bce_logits(const float* z, long n, float label, float* out, float* dz, float* ws, void* stream);
/* the same against a per-element target tensor t (n); dz / dt (either may be NULL): gradients of the mean */
int gd_bce_logits_target(const float* z, const float* t, long n, float* out, float* dz, float* dt, float* ws,
                         void* stream);
/* LeakyReLU with an arbitrary negative slope (the fused conv / linear epilogues implement the reference's 0.2 only);
 * backward takes the INPUT x. */
int gd_leaky_fwd(const float* x, float* y, long n, float slope, void* stream);
int gd_leaky_bwd(const float* x, const float* dy, float* dx, long n, float slope, void* stream);
/* MSELoss / L1 mean (L191,L262; losses.py:72) */
int gd_mse(const float* a, const float* b, long n, float* out, float* da, float* ws, void* stream);
int gd_l1(const float* a, const float* b, long n, float* out, float* da, float* ws, void* stream);
/* TVLoss.forward (losses.py:81-87) */
int gd_tv(const float* x, int B, int C, int H, int W, float weight, float* out, float* dx, float* ws, void* stream);
/* SSIM mean (losses.py:109-136), forward only (the train loop never differentiates it) */
int gd_ssim(const float* a, const float* b, int BC, int H, int W, int window, float* out, float* ws, void* stream);
/* per-sample SSIM means (SSIM(size_average=False), losses.py:136): out (B) */
int gd_ssim_samples(const float* a, const float* b, int B, int C, int H, int W, int window, float* out, float* ws,
                    void* stream);
/* SSIM backward (losses.py:118-136 under autograd): gscale (B) = upstream gradient of each sample's pixels (already
 * divided by the element count of the mean); coef_ws: caller-owned scratch of 4 * B*C*H*W floats; da / db (either may
 * be NULL): gradients w.r.t. img1 / img2, overwritten. */
int gd_ssim_bwd(const float* a, const float* b, const float* gscale, int B, int C, int H, int W, int window,
                float* coef_ws, float* da, float* db, void* stream);

/* AdamW step over one tensor (torch.optim.AdamW, GAN_DANet_train.ipynb:L182-183).
 * `step` is 1-based.  The gradient is read once, multiplied by grad_scale (1/world for DP). */
int gd_adamw(float* p, const float* g, float* m, float* v, long n, int step, float lr, float beta1, float beta2,
             float eps, float weight_decay, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pixel-major (NHWC) bf16 kernels for the frozen VGG19 feature stack of PerceptualLoss (losses.py:13-73;
 * torchvision vgg19.features[:21]).  Activations (B, H, W, C) bf16, C % 8 == 0.
 *   gd_conv3x3_nhwc_pack : w (Cout, Cin, 3, 3) fp32 -> packed bf16 operator in ws; transposed = 1 packs the stride-1
 *                          data-gradient operator (channels swapped, taps flipped), transposed = 2 the stride-2 one
 *                          (channels swapped, taps as stored: gd_conv3x3_nhwc_s2_dgrad).  ws needs
 *                          gd_conv3x3_ws_bytes(M, K) bytes, (M, K) = (Cout, Cin) or (Cin, Cout).
 *   gd_conv3x3_nhwc      : y = [mask > 0] * act(conv3x3_p1(x) + bias) + res   (x: K channels, y/mask/res: M channels;
 *                          bias, mask, res may be NULL; mask = the ReLU output whose backward is being applied)
 *   gd_nhwc_stem_fwd/bwd : first conv (features[0], Ci <= 4 input channels) from / to the fp32 NCHW image
 *   gd_nhwc_maxpool2_*   : nn.MaxPool2d(2); backward takes the pooled layer's input x (first maximum wins, ATen's
 *                          tie rule) and optionally gates by x > 0
 *   gd_nhwc_l1           : out (+)= mean |a - b| (losses.py:72), ws >= 1024 floats
 *   gd_nhwc_l1_grad      : g = (*upstream) / n * sign(a - b), optionally gated by a > 0
 *   split / split_c      : operand mode "x3": the pixel-major tensors hold 3 C bf16 per pixel, [hi | lo | hi] of the C fp32
 *                          values (see gd_disc_stem_fwd below); split_c = C (0 = plain), n = the LOGICAL element count
 * ---------------------------------------------------------------------------------------- */
int gd_conv3x3_nhwc_pack(const float* w, int Cout, int Cin, int transposed, void* ws, size_t ws_bytes, void* stream);
int gd_conv3x3_nhwc(const void* x, const void* wpack, const float* bias, const void* mask, const void* res, void* y, int B,
                    int H, int W, int K, int M, int relu, int split, void* stream);
/* the same kernel with an fp32 NCHW result (B, M, H, W), batch stride y_bs elements: wide 3x3 convs of the generator on a
 * pixel-major bf16 copy of their input (gd_pack_16 transposed output, K = its leading dimension, zero padded) */
int gd_conv3x3_nhwc_f32out(const void* x, const void* wpack, const float* bias, float* y32, long y_bs, int B, int H, int W, int K,
                           int M, int relu, void* stream);
int gd_nhwc_stem_fwd(const float* img, int B, int Ci, int H, int W, const float* w, const float* bias, int Co, int relu,
                     void* y, int split, void* stream);
int gd_nhwc_stem_bwd(const void* g, int B, int Ci, int H, int W, const float* w, int Co, float* dimg, int split, void* stream);
int gd_nhwc_maxpool2_fwd(const void* x, int B, int H, int W, int C, void* y, int split, void* stream);
int gd_nhwc_maxpool2_bwd(const void* x, const void* dy, int B, int H, int W, int C, int relu_mask, void* dx, int split, void* stream);
int gd_nhwc_l1(const void* a, const void* b, long n, float* out, int accumulate, float* ws, int split_c, void* stream);
int gd_nhwc_l1_grad(const void* a, const void* b, long n, const float* upstream, int relu_mask, void* g, int split_c, void* stream);

/* ------------------------------------------------------------------------------------------
 * Discriminator1 (discriminator.py:57-77: 4 x (conv3x3 stride 2 + LeakyReLU(0.2)) -> flatten -> fc1 -> fc2) on
 * pixel-major bf16 activations.  Ho = (H-1)/2+1, Wo = (W-1)/2+1 throughout.
 *   gd_disc_stem_fwd        : conv1 (discriminator.py:60) from the fp32 NCHW image (B, Ci <= 4, H, W):
 *                             y (B, Ho, Wo, Co) bf16 = LeakyReLU(conv3x3_s2_p1(img) + bias)
 *   gd_disc_stem_wgrad      : dw (Co, Ci, 3, 3), db (Co) fp32 (overwritten; db may be NULL) from the pre-activation
 *                             gradient g (B, Ho, Wo, Co) bf16 and the image.  Co == 64.
 *   gd_disc_stem_dgrad      : dimg (B, Ci, H, W) fp32 from g (the generator step differentiates through D)
 *   gd_conv3x3_nhwc_s2      : conv2..4 (discriminator.py:61-63): x (B, H, W, K) -> y (B, Ho, Wo, M), + bias,
 *                             act 0 none / 1 ReLU / 2 LeakyReLU(slope); wpack = gd_conv3x3_nhwc_pack(transposed = 0)
 *   gd_conv3x3_nhwc_s2_dgrad: its data gradient, split by input-pixel parity (nine tap passes, no zero-stuffing):
 *                             dx (B, H, W, K) = convT(dy) * LeakyReLU'(act_out), act_out (B, H, W, K) = the activation
 *                             output this conv consumed (NULL: no mask); wpack_t = gd_conv3x3_nhwc_pack(transposed = 2)
 *   gd_nhwc_flatten_fwd/bwd : x.flatten(1) (discriminator.py:72): y (B, HW, C) bf16 -> f (B, C*HW) fp32 in (c, h, w)
 *                             order; backward g (B, HW, C) bf16 = df * LeakyReLU'(y)
 *   gd_nhwc_to_nchw16       : g (B, HW, C) bf16 -> gt (B, C, HW) bf16 (the dy_bf16 operand of gd_conv3x3_wgrad) and,
 *                             when csum != NULL, csum (C) fp32 = per-channel sums (the bias gradient; overwritten)
 * ----------------------------------------------------------------------------------------  *   split (all eight entry points; operand mode "x3" of set_precision("mixed")): 1 = every pixel-major bf16 ACTIVATION or
 *   GRADIENT tensor named above holds 3 C channels per pixel, the C fp32 values split as [hi | lo | hi] with hi = bf16(v),
 *   lo = bf16(v - hi): the operand the conv kernels take unchanged against weights split [hi ; hi ; lo] along the contraction
 *   axis (gd_split3_weights), three bf16 MFMAs per product, ~2^-16 relative.  The conv entry points then take K (forward)
 *   resp. M (data gradient) = the 3 C PHYSICAL channel count of their input and the logical count of their output;
 *   gd_nhwc_to_nchw16 writes two (B, C, HW) images, hi then lo, and the sums of hi + lo.  0 = plain bf16 (C channels).
 */
int gd_disc_stem_fwd(const float* img, int B, int Ci, int H, int W, const float* w, const float* bias, int Co, float slope,
                     void* y, int split, void* stream);
int gd_disc_stem_wgrad(const void* g, const float* img, int B, int Ci, int H, int W, int Co, float* dw, float* db, int split, void* stream);
/* with a workspace for the ordered deterministic mode: one [Ci][Co][10] fp32 slab per workgroup instead of the atomics */
int gd_disc_stem_wgrad_ws(const void* g, const float* img, int B, int Ci, int H, int W, int Co, float* dw, float* db, int split,
                          void* stream, void* ws, size_t ws_bytes);
int gd_disc_stem_dgrad(const void* g, int B, int Ci, int H, int W, const float* w, int Co, float* dimg, int split, void* stream);
int gd_conv3x3_nhwc_s2(const void* x, const void* wpack, const float* bias, void* y, int B, int H, int W, int K, int M, int act,
                       float slope, int split, void* stream);
int gd_conv3x3_nhwc_s2_dgrad(const void* dy, const void* wpack_t, const void* act_out, float slope, void* dx, int B, int H,
                             int W, int K, int M, int split, void* stream);
int gd_nhwc_flatten_fwd(const void* y, int B, int HW, int C, float* f, int split, void* stream);
int gd_nhwc_flatten_bwd(const float* df, const void* y, float slope, int B, int HW, int C, void* g, int split, void* stream);
int gd_nhwc_to_nchw16(const void* g, int B, int HW, int C, void* gt, float* csum, int split, void* stream);
/* with a workspace for the ordered deterministic mode: one [C] fp32 slab of channel sums per workgroup row */
int gd_nhwc_to_nchw16_ws(const void* g, int B, int HW, int C, void* gt, float* csum, int split, void* stream, void* ws,
                         size_t ws_bytes);

/* ------------------------------------------------------------------------------------------
 * PAM, fused (flash) form with 16-bit MFMA operands and fp32 softmax statistics (generator.py:115-122).
 * f16 = 0: bf16 operands (training default); f16 = 1: IEEE fp16 operands (BASELINE config 5) -- the packs below
 * must then have been made with gd_pack_16(..., f16 = 1).
 *   qt     : (B, Npad, 32), d zero-padded to 32, values PRE-SCALED by log2(e)  (gd_pack_bf16 scale_imm):
 *            the kernels work in the log2 domain and feed the softmax shift in as the MFMA accumulator input
 *   kt     : (B, Npad, 32), unscaled, d zero-padded to 31 and d = 31 set to 1.0 (gd_pack_bf16 ones_row = 31):
 *            the forward feeds its running row maximum through that k-slot (so r <= 31)
 *   v      : (B, Cp, Npad), Cp = C rounded up to 32   (channel-major, keys perm16-ordered: gd_pack_bf16)
 *   v_ones : != 0 when channel Cp-1 of v is a row of ones (gd_pack_bf16 ones_row; needs C < Cp): the softmax
 *            denominator then comes out of the O MFMAs instead of one VALU add per score
 *   x, out : (B, C, N) fp32 with batch strides; out = gamma * attn + x
 *   o_attn : (B, C, N) fp32 un-scaled attention output (kept for backward)
 *   lse    : (B, N) fp32 natural-log log-sum-exp of the unscaled energies.   Npad % 256 == 0.
 * ---------------------------------------------------------------------------------------- */
int gd_pam_flash_fwd(const void* qt, const void* kt, const void* v, int B, int N, int Npad, int C, int Cp,
                     int v_ones, int f16, const float* gamma, const float* x, long x_bs, float* out, long out_bs,
                     float* o_attn, float* lse, const float* k_sqnorm_max, void* stream);
/* gd_pam_flash_fwd (generator.py:115-122) with the max-free sweep for logits of ANY magnitude, bf16 operands: softmax is
 * invariant under a per-query shift, so a prepass takes m_i = max over `nsample` (128 | 256 | 512) strided keys of q_i . k_j
 * -- at most the true row maximum, hence row sums >= ~1 -- and the sweep runs exp2(s - m_i) without row maximum, test or
 * rescale.  Workgroups whose row sums leave (1e-30, 1e30) (the sample missed the true maximum by > ~100 log2 units) are
 * flagged and redone by the running-maximum sweep in a second launch in which every other workgroup exits at once.
 * ws: gd_pam_fwd_shift_ws_bytes(B, Npad) bytes of scratch.  Same outputs as gd_pam_flash_fwd. */
size_t gd_pam_fwd_shift_ws_bytes(int B, int Npad);
int gd_pam_flash_fwd_shift(const void* qt, const void* kt, const void* v, int B, int N, int Npad, int C, int Cp, int v_ones,
                           const float* gamma, const float* x, long x_bs, float* out, long out_bs, float* o_attn, float* lse,
                           int nsample, void* ws, size_t ws_bytes, void* stream);
/* k_sqnorm_max (B floats, or NULL): max_j |k_j|^2 of each image's packed keys.  Softmax is shift-invariant; when
 * |q_i| * max_j |k_j| (in log2 units, q is pre-scaled) stays inside the exponent range of the P operand type for every
 * query of a wave, that wave sweeps the keys without a running maximum (no per-tile max / test / rescale).  NULL: the
 * running maximum is always kept.  out (B floats) is overwritten. */
int gd_pam_key_sqnorm_max(const void* kt, int B, int N, int Npad, int f16, float* out, void* stream);
/* backward: 16-bit inputs qt, kt as above (B,Npad,32); kn (B,32,Npad) perm16-ordered (row 31 is don't-care);
 * vt (B,Npad,Cp); dot (B,Npad,Cp) = gamma*dOut; lse, delta (B,N) fp32 (delta = gamma*rowsum(dOut.*O)).  All packs
 * zero padded (gd_pack_bf16 does).  Outputs fp32, channel-major, overwritten: dqn, dkn (B,32,Npad), dv (B,Cp,Npad)
 * -- gradients w.r.t. the UNSCALED q, k, v.  Npad % 256 == 0.
 * form (GD_PAM_BWD_*):
 *   0 K64_ATOMIC  one key-parallel kernel, 4 waves x 64 keys per workgroup (one wave per SIMD, dK^T/dV^T in the
 *                 accumulation registers), dQ summed across key blocks with fp32 atomics (fastest; not bitwise
 *                 reproducible in dQ)
 *   1 K64_PARTS   the same kernel storing dQ as one bf16 part per 256-key block + a streaming sum (reproducible)
 *   3 TWO_KERNEL  dK/dV kernel, then a query-parallel kernel that recomputes S and dP for dQ (no scratch;
 *                 reproducible; bf16 only)
 *   (2 was the K32 parts form, an 8-wave kernel with bf16 dQ parts that form 1 superseded; the number is not reused and is
 *   rejected like any other unknown form.)
 * out_bs: 0, or (form 0 only) the batch stride in elements shared by dqn, dkn, dv when the caller passes them as row
 *   blocks of ONE (B, rows, Npad) buffer -- the three projection gradients can then run as one GEMM over that buffer.
 * scratch: caller-owned, >= gd_pam_bwd_scratch_bytes(Npad, form) (= one image's worth; more lets more images go per
 * launch); may be NULL for form 3. */
#define GD_PAM_BWD_K64_ATOMIC 0
#define GD_PAM_BWD_K64_PARTS 1
#define GD_PAM_BWD_TWO_KERNEL 3
size_t gd_pam_bwd_scratch_bytes(int Npad, int form);
int gd_pam_flash_bwd(const void* qt, const void* kt, const void* kn, const void* vt, const void* dot_,
                     const float* lse, const float* delta, int B, int N, int Npad, int Cp, int f16, int form,
                     float* dqn, float* dkn, float* dv, long out_bs, void* scratch, size_t scratch_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * PAM, fused form for WIDE attention blocks (generator.py:115-122 at 192 < C <= 511: FlexibleUpsamplingModule with a larger
 * growth_rate / num_layers_per_block, generator.py:178-186).  Operand contract as gd_pam_flash_fwd / _bwd with
 *   D      : q / k slots, 32 (r <= 31) or 64 (r <= 63); qt, kt (B, Npad, D), kt's slot D - 1 = 1.0 (gd_pack_16 ones_row = D - 1),
 *            kn (B, D, Npad) perm16
 *   Cp     : C rounded up to 32, 192 < Cp <= 512; v (B, Cp, Npad) perm16 WITHOUT a ones row; vt, dot (B, Npad, Cp)
 * The value channels are processed in chunks of at most 192 (forward: one sweep per chunk, each recomputing S; backward: a
 * dK / dQ kernel over all channels and one dV kernel per chunk).  No N x N buffer.  Outputs as the narrow kernels, with
 * dqn, dkn (B, D, Npad).  deterministic = 0: dQ summed with fp32 atomics, no scratch; 1: bf16 parts per 128-key block
 * summed in a second pass (bitwise reproducible), scratch >= gd_pam_wide_scratch_bytes(Npad, D, 1) (one image's worth). */
int gd_pam_wide_fwd(const void* qt, const void* kt, const void* v, int B, int N, int Npad, int C, int Cp, int D, int f16,
                    const float* gamma, const float* x, long x_bs, float* out, long out_bs, float* o_attn, float* lse,
                    void* stream);
/* backward of gd_pam_wide_fwd (autograd of generator.py:115-122) */
size_t gd_pam_wide_scratch_bytes(int Npad, int D, int deterministic);
int gd_pam_wide_bwd(const void* qt, const void* kt, const void* kn, const void* vt, const void* dot_, const float* lse,
                    const float* delta, int B, int N, int Npad, int Cp, int D, int f16, int deterministic, float* dqn,
                    float* dkn, float* dv, void* scratch, size_t scratch_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * PAM, fused form on EXACT fp32 operands (generator.py:115-122; the parity mode's attention without the N x N matrices).
 * Every product is a v_mfma_f32_32x32x2_f32; the softmax is online (running maximum, fp32 statistics).  8 <= C <= 511 in
 * practice (1 <= C <= 511 accepted), 1 <= r <= 63; r is padded to the MFMA k-step (2) inside the kernels only.
 *   q, k   : (B, r, Npad) fp32 planes, UNSCALED projection outputs, batch strides q_bs / k_bs (elements)
 *   v      : (B, C, Npad), batch stride v_bs
 *   Npad   : row length of those planes, a multiple of 256 >= N; columns >= N must be zero.  With N % 256 == 0 the
 *            projections' own outputs are the operands (no copy).  Planes 16-byte aligned, batch strides % 4 == 0.
 *   out    : gamma * attn + x, (B, C, N) with batch stride out_bs (may be a channel slice of the 2C DANet slab); x likewise
 *   o_attn : (B, C, N) dense, the un-scaled attention output; lse (B, N): natural-log sum-exp of the energies
 * No scratch, no N x N or N x keys buffer.  Returns 0, or -1 with gd_last_error naming the argument. */
int gd_pam_f32_fwd(const float* q, long q_bs, const float* k, long k_bs, const float* v, long v_bs, int B, int N, int Npad,
                   int C, int r, const float* gamma, const float* x, long x_bs, float* out, long out_bs, float* o_attn,
                   float* lse, void* stream);
/* backward of gd_pam_f32_fwd (autograd of generator.py:115-122): gdo (B, C, Npad) = gamma * dOut (zero columns >= N),
 * delta[b][i] = sum_c gdo[c][i] o_attn[c][i] (gd_chan_dot); dq, dk (B, r, N) and dv (B, C, N) dense, gradients w.r.t. the
 * unscaled q, k, v.  A key-parallel dV kernel per chunk of <= 192 channels, a key-parallel dK and a query-parallel dQ
 * kernel: no atomics, no scratch, bitwise reproducible. */
int gd_pam_f32_bwd(const float* q, long q_bs, const float* k, long k_bs, const float* v, long v_bs, const float* gdo,
                   long gdo_bs, const float* lse, const float* delta, int B, int N, int Npad, int C, int r, float* dq,
                   float* dk, float* dv, void* stream);

/* ------------------------------------------------------------------------------------------
 * PAM attention probe: the attention P = softmax_j(s_ij), s_ij = logit_scale * (q_i . k_j) in nats, of generator.py:115-118
 * looked at without the N x N matrix.  Operand contract of gd_pam_f32_fwd: q, k (B, r, Npad) fp32 planes with batch strides
 * q_bs / k_bs >= 0 (elements, multiples of 4), 16-byte aligned, Npad a multiple of 256 >= N, columns >= N zero, 1 <= r <= 63
 * (padded to the MFMA k-step inside the kernels only).  Every product is a v_mfma_f32_32x32x2_f32.  logit_scale = 1 for the
 * projections as they are; ln 2 for planes that hold what the 16-bit routes multiply (q log2 e and k rounded by
 * gd_round_to_16).  No atomics, no scratch, no N x N or N x tile buffer; every output element is summed by one wave in a
 * fixed order, so two runs agree bit for bit.  Nothing here is differentiable.
 * Each returns 0, or -1 with gd_last_error naming the argument (checked on the host before any GPU call).
 *
 * gd_pam_attn_stats (query-parallel sweep, online in the running maximum m: l = sum_j e^(s - m), u = sum_j e^(s - m) (s - m);
 * when m rises by d, u <- e^-d (u - d l) and l <- e^-d l); (B, N) fp32 maps, entropy / peak optional (NULL = skip):
 *   lse     = m + ln l
 *   entropy = ln l - u / l     = -sum_j P_ij ln P_ij, nats
 *   peak    = 1 / l            = max_j P_ij */
int gd_pam_attn_stats(const float* q, long q_bs, const float* k, long k_bs, int B, int N, int Npad, int r, float logit_scale,
                      float* lse, float* entropy, float* peak, void* stream);
/* key-parallel sweep with the lse of gd_pam_attn_stats: received[b][j] = sum_{i < N} exp(s_ij - lse[b][i]), (B, N) fp32: how
 * much attention key j receives from all queries; its mean over j is 1. */
int gd_pam_attn_received(const float* q, long q_bs, const float* k, long k_bs, const float* lse, int B, int N, int Npad, int r,
                         float logit_scale, float* received, void* stream);
/* attention rows of S selected queries, 1 <= S <= 256: idx holds S ints in [0, N) shared by the images of the batch (the
 * kernel clamps, so a bad index never reads out of bounds; callers check the range); rows[b][s][j] = softmax_j(s_{idx[s], j}),
 * (B, S, N) fp32 dense; lse_rows (B, S) optional (NULL = skip), bit for bit the lse of gd_pam_attn_stats at those queries.
 * Self-contained: one sweep for the row statistics, a second that writes P. */
int gd_pam_attn_rows(const float* q, long q_bs, const float* k, long k_bs, const int* idx, int S, int B, int N, int Npad, int r,
                     float logit_scale, float* rows, float* lse_rows, void* stream);
/* y[i] = float(rne16(x[i] * scale)), n elements: bf16 (f16 = 0) or IEEE fp16 (f16 = 1), the rounding gd_pack_16 applies to
 * the operands of the 16-bit PAM routes (x and y may be the same buffer) */
int gd_round_to_16(const float* x, float* y, long n, float scale, int f16, void* stream);

/* test.ipynb c1:69-85 mild_histogram_matching, per sample of a batch: out[b] = (1 - weight) * src[b] + weight *
 * interp(cdf_src(src[b]), cdf_ref, sorted unique ref[b]) with numpy's np.unique / np.interp semantics (float64 result, as
 * the notebook produces).  src (B, ns), ref (B, nt) fp32; out (B, ns) fp64; ws: caller-owned scratch of
 * gd_hist_match_ws_bytes(ns, nt) bytes (sort buffers).  One radix sort pair per sample (rocPRIM via hipCUB).
 * Keys are ordered with every NaN last, whatever its sign bit, as numpy orders them: a NaN of src gives NaN at its own
 * position and counts as larger than every number in the ranks of the others.  Non-finite values in ref are outside the
 * contract.  gd_hist_match_host: the same on host pointers (a stable CPU sort of (key, index) pairs, then the same
 * per-element function, csrc/histmatch_core.h); device and host results agree bit for bit. */
size_t gd_hist_match_ws_bytes(long ns, long nt);
int gd_hist_match(const float* src, const float* ref, int B, long ns, long nt, double weight, double* out, void* ws,
                  size_t ws_bytes, void* stream);
int gd_hist_match_host(const float* src, const float* ref, int B, long ns, long nt, double weight, double* out);
/* test.ipynb c1:87-101 smooth_blend: over the region rows [sr, er) x columns [sc, ec) of every (b, c) plane,
 * gen = gen * (1 - mask) + grace * mask, in place; mask (er-sr, ec-sc) fp32 is the feathered window the host builds. */
int gd_blend_region(float* gen, const float* grace, const float* mask, int BC, int H, int W, int sr, int er, int sc,
                    int ec, void* stream);
/* CustomDataset.apply_augmentation (datasets.py:181-208) for a batch of tiles as one gather: per-sample op word
 * ops[b] = hflip | vflip << 1 | quarter_turns << 2 | noise << 4 (flip W, flip H, torch.rot90 k, in that order; H == W
 * when a sample is turned an odd number of times -- checked by the host).  noise (same shape as dst) may be NULL;
 * it is added times noise_scale (0.05 in the reference) to the samples whose noise bit is set.  src != dst. */
int gd_augment_d4(const float* src, float* dst, int B, int C, int H, int W, const int* ops, const float* noise,
                  float noise_scale, void* stream);
/* attention gates of SqueezeExcitation / CBAMBlock (generator.py:70-101; exported by the reference, not on the
 * train path).  Dense (B, C, HW) fp32.
 *   gd_bcast_mul       : y = x * att; mode 0: att (B, C) channel gate (generator.py:84), mode 1: att (B, HW)
 *                        spatial gate (generator.py:101).  The data gradient is the same call on dy.
 *   gd_row_dot         : out[row] = sum_j a[row][j] * b[row][j]   (gate gradient of mode 0; mode 1 uses gd_chan_dot)
 *   gd_chan_maxmean_*  : y (B, 2, HW) = [max_c x, mean_c x] (generator.py:98-100), idx (B, HW) = arg max;
 *                        backward routes dy[:,0] to the arg-max channel and spreads dy[:,1] / C */
int gd_bcast_mul(const float* x, const float* att, float* y, int B, int C, long HW, int mode, void* stream);
int gd_row_dot(const float* a, const float* b, float* out, long rows, long n, void* stream);
int gd_chan_maxmean_fwd(const float* x, float* y, int* idx, int B, int C, long HW, void* stream);
int gd_chan_maxmean_bwd(const float* dy, const int* idx, float* dx, int B, int C, long HW, void* stream);
/* d_raw[b][i] = sum_c a[b][c][i]*o[b][c][i] (per-pixel channel dot), delta = (*gamma) * d_raw */
int gd_chan_dot(const float* a, long a_bs, const float* o, long o_bs, int B, int C, int N, const float* gamma,
                float* d_raw, float* delta, void* stream);
/* split-bf16 ("x3") operands of set_precision("mixed"): every conv operand v = hi + lo (hi = bf16(v), lo = bf16(v - hi)),
 * every product hi*hi + lo*hi + hi*lo on the bf16 matrix pipe with fp32 accumulation (~2^-16 relative, 5x the rate of the
 * exact f32 MFMA).  The split rides in the operand layout, so the 16-bit conv kernels above serve unchanged:
 *   gd_pack_16_split  : fp32 (B, R, Cc) planes (optionally max(0, row_scale * x + row_shift) first: the BatchNorm + ReLU
 *                       prologue of a dense layer, generator.py:36) -> up to three bf16 copies of the tile per output, copy j
 *                       at `cs` elements behind copy j - 1, holding the lo part when bit j of `pattern` is set, else the hi
 *                       part.  plain = (R, Cc) rows (channel-major, ldp == Cc), tr = the transpose (pixel-major rows of ldt
 *                       elements): [hi | lo | hi] as 3 R channels (cs = R, ldt = 3 R, pattern 0b010) is the forward /
 *                       data-gradient operand; separate hi / lo images (pattern 0b10) feed gd_conv3x3_wgrad's three
 *                       accumulating launches.  R % 8 == 0, Cc % 8 == 0.
 *   gd_split3_weights : w (A, Bn, Cn) fp32 -> (A, 3 Bn, Cn) fp32 [hi ; hi ; lo] along the middle axis (nn.Conv2d weights,
 *                       generator.py:34,148,218,222 and the VGG stack of losses.py:41: Bn = Cin for the forward, A = 1 and
 *                       Bn = Cout for the data gradient); gd_conv3x3_nhwc_pack then makes the 16-bit operator. */
int gd_pack_16_split(const float* s, long s_bs, int B, int R, int Cc, const float* row_scale, const float* row_shift, int relu,
                     void* plain, long p_bs, int ldp, long p_cs, int p_ncopy, int p_pattern, void* tr, long t_bs, int ldt,
                     long t_cs, int t_ncopy, int t_pattern, void* stream);
/* the same with the ReLU backward fused (autograd of nn.ReLU behind a conv, losses.py:41 / generator.py:219): `mask` (B, R, Cc)
 * fp32, batch stride m_bs, is the ReLU's output; elements whose mask value is not positive are packed as zero */
int gd_pack_16_split_masked(const float* s, long s_bs, int B, int R, int Cc, const float* row_scale, const float* row_shift,
                            int relu, void* plain, long p_bs, int ldp, long p_cs, int p_ncopy, int p_pattern, void* tr, long t_bs,
                            int ldt, long t_cs, int t_ncopy, int t_pattern, const float* mask, long m_bs, void* stream);
int gd_split3_weights(const float* w, long A, long Bn, long Cn, float* out, void* stream);
/* fp16 operand mode of gd_pam_flash_bwd (autograd of generator.py:115-122 under set_precision("fp16" | "mixed")): IEEE
 * fp16 loses everything below 6e-8, and gamma * dOut of a real training step sits below that.  All outputs of the backward
 * are linear in dOut, so it is packed as scales[0] * dOut with scales[0] = gamma * 2^k chosen so that the largest element has
 * magnitude in [0.5, 1); delta (B, N), computed by gd_chan_dot with gamma, is multiplied by 2^k in place; the consumers of
 * dQ / dK / dV multiply by scales[1] = 2^-k (the alpha of their GEMMs).  dout: (B, C, N) fp32, batch stride dout_bs;
 * scales: 2 floats; ws: 1024 floats. */
int gd_pam_f16_scale(const float* dout, long dout_bs, int B, int C, int N, const float* gamma, float* delta, float* scales,
                     float* ws, void* stream);
/* fp32 (B, R, Cc) planes (batch stride s_bs), times scale_imm and optionally times a device scalar -> bf16:
 *   plain      (B, Rp_plain, ld_plain)  zero padded copy          (NULL to skip)
 *   transposed (B, Ccp_t, ld_t)         zero padded transpose     (NULL to skip)
 * perm16 != 0: inside every 16 columns of `plain` the order is [0-3, 8-11, 4-7, 12-15] (the order an MFMA lane
 * half consumes an accumulator-row-ordered k-step: gd_pam_flash_fwd expects its V operand packed this way).
 * ones_row >= 0: that (padding) row of the source is taken as all ones in both outputs (-1: none). */
int gd_pack_bf16(const float* s, long s_bs, int B, int R, int Cc, const float* scale_dev, float scale_imm, void* plain,
                 int Rp_plain, int ld_plain, void* transposed, int Ccp_t, int ld_t, int perm16, int ones_row,
                 void* stream);
/* the same with the 16-bit output type selectable: f16 = 0 bf16 (== gd_pack_bf16), f16 = 1 IEEE fp16 */
int gd_pack_16(const float* s, long s_bs, int B, int R, int Cc, const float* scale_dev, float scale_imm, void* plain,
               int Rp_plain, int ld_plain, void* transposed, int Ccp_t, int ld_t, int perm16, int ones_row, int f16,
               void* stream);
/* gd_pack_16 with a per-row affine + ReLU applied first (row r -> max(0, row_scale[r] x + row_shift[r]) when relu): the
 * BatchNorm + ReLU prologue of a dense layer (generator.py:29-45), for the pixel-major bf16 copy of its input that
 * gd_conv3x3_wgrad reads (x_nhwc16).  Aligned shapes only: Cc % 4 == 0, ld % 8 == 0. */
int gd_pack_16_affine(const float* s, long s_bs, int B, int R, int Cc, const float* row_scale, const float* row_shift, int relu,
                      void* plain, int Rp_plain, int ld_plain, void* transposed, int Ccp_t, int ld_t, int f16, void* stream);

/* ------------------------------------------------------------------------------------------
 * RCCL communicator for hosts without torch.distributed (one process per GPU, one communicator per process; the
 * Python package here goes through torch.distributed's "nccl" backend, which IS RCCL, and does not call these).
 * librccl is dlopen()ed on first use (GD_RCCL_PATH overrides the search).  dtype: 0 fp32, 1 bf16, 2 fp16.  All
 * collectives are in-place-capable, sum-reducing, asynchronous on `stream`.
 *   gd_comm_unique_id : rank 0 creates the 128-byte id; the host distributes it (env, file, TCP store)
 *   gd_comm_init      : collective over `world` processes
 *   gd_allreduce      : buf (n elements) <- sum over ranks                     (gradient all-reduce, the G/D grads)
 *   gd_reduce_scatter : recv (recv_n) <- this rank's slice of the sum of send (world * recv_n)     (fc1 gradient)
 *   gd_allgather      : recv (world * send_n) <- every rank's send (send_n)                 (updated fc1 slices)
 * ---------------------------------------------------------------------------------------- */
int gd_comm_unique_id(char* id128);
int gd_comm_init(int rank, int world, const char* id128);
int gd_comm_world(void);
int gd_allreduce(void* buf, size_t n, int dtype, void* stream);
int gd_reduce_scatter(const void* send, void* recv, size_t recv_n, int dtype, void* stream);
int gd_allgather(const void* send, void* recv, size_t send_n, int dtype, void* stream);
int gd_comm_destroy(void);

/* ------------------------------------------------------------------------------------------
 * Evaluation (evalstats.hip): what the reference computes on the host after train().
 *
 * The RECORD is 8 doubles describing n pairs (p, t):
 *   [0] n   [1] mean_p   [2] mean_t   [3] M2_p = sum (p - mean_p)^2   [4] M2_t   [5] C_pt = sum (p - mean_p)(t - mean_t)
 *   [6] sum |p - t|   [7] sum (p - t)^2
 * Two records merge with Chan's pairwise formulas (n = nA + nB, d = meanB - meanA, mean = meanA + d nB / n,
 * M2 = M2A + M2B + d^2 nA nB / n, C likewise with d_p d_t; [6] and [7] add); a record with n == 0 is neutral.  Records are
 * what travels between batches and between ranks, so unequal counts are exact.
 * ---------------------------------------------------------------------------------------- */
enum { GD_EVAL_F64 = 1, GD_EVAL_SKIP_NAN = 2 };
/* ModelTrainer.evaluate (GAN_DANet_train.ipynb c0 "def evaluate"; deep_ensemble.ipynb:L249-293): the statistics behind
 * mean_squared_error / mean_absolute_error / r2_score / np.corrcoef of pred against truth, both dense planes x hw
 * elements (fp32; fp64 with GD_EVAL_F64), as ONE record written to rec (device, 8 doubles), without a host sync.
 * mask: NULL or hw bytes shared by all planes, nonzero = valid.  Both inputs are read as v * a + b (the StandardScaler
 * inverse of deep_ensemble.ipynb; a = 1, b = 0 for none).  GD_EVAL_SKIP_NAN drops pairs with a NaN on either side
 * (valid_mask of compute_uncertainty, L470-472).  fp64 co-moment accumulation, fixed order, no atomics: bitwise
 * reproducible.  ws: caller-owned, gd_eval_stats_ws_bytes(planes * hw) bytes (per-workgroup partial records). */
size_t gd_eval_stats_ws_bytes(long n);
int gd_eval_stats(const void* pred, const void* truth, long planes, long hw, const unsigned char* mask, double a, double b,
                  int flags, double* rec, void* ws, size_t ws_bytes, void* stream);
/* np.nanmean(masked, axis=(lat, lon)) of compute_uncertainty (deep_ensemble.ipynb:L451-463): mean[p] (fp64) over the valid
 * pixels of plane p of x (planes x hw, fp32, planes <= 65535), count[p] = how many; no valid pixel -> NaN, count 0.
 * mask as above (NULL: every pixel).  ws: gd_masked_plane_mean_ws_bytes(planes, hw) bytes. */
size_t gd_masked_plane_mean_ws_bytes(long planes, long hw);
int gd_masked_plane_mean(const float* x, long planes, long hw, const unsigned char* mask, double* mean, long long* count,
                         void* ws, size_t ws_bytes, void* stream);
/* np.mean / np.std (ddof 0) over the member axis (deep_ensemble.ipynb:L465-467 and the per-pixel maps of
 * predict_ensemble): x holds M rows (1 <= M <= 32) of n elements, member_stride elements apart; mean and std_out (n) in
 * the input dtype (fp32; fp64 when f64 != 0), two-pass in fp64 registers, rounded once.  16-byte loads and stores for
 * every M when the rows (member_stride, unless M == 1) and both outputs share their offset from a 16-byte boundary;
 * otherwise every element takes the scalar path. */
int gd_ensemble_stats(const void* x, int M, long member_stride, long n, int f64, void* mean, void* std_out, void* stream);
/* host only, no GPU call: merge k records (recs: k x 8 doubles, host memory) in the given order into rec_out (8 doubles,
 * may be NULL) and derive metrics[4] = mse, mae, r2, cc.  r2 as sklearn.metrics.r2_score (1 - SS_res / SS_tot; SS_tot ==
 * 0 -> 1.0 if SS_res == 0 else 0.0), cc as np.corrcoef(t, p)[0, 1] (NaN when a variance is 0); n == 0 (or k == 0): NaN
 * for all four (L288-291).  n == 1 follows the same rules: SS_tot is 0, so r2 is 1.0 or 0.0 (sklearn warns and returns
 * NaN below two samples) and cc is NaN. */
int gd_eval_merge_host(const double* recs, long k, double* rec_out, double* metrics);

/* ------------------------------------------------------------------------------------------
 * Guarded step: gradient norm, clipping, skipping of non-finite steps and an averaged copy of the weights (EMA), decided
 * and applied on the device.  One caller-owned RECORD of 6 doubles in device memory carries the decision from the norm
 * to the update kernels; the host reads it only when it wants to know:
 *   [0] sqnorm = sum (g * gscale)^2 over all gradients   [1] norm = sqrt(sqnorm)   [2] coef, the clip factor in (0, 1]
 *   [3] ok: 1 = apply this step, 0 = skip it   [4] applied_steps   [5] skipped_steps
 * A step is gd_grad_sqnorm (once, or twice with `accumulate`) -> gd_guard_finalize -> gd_adamw_guarded per tensor.
 * ---------------------------------------------------------------------------------------- */
enum { GD_GUARD_SQNORM = 0, GD_GUARD_NORM = 1, GD_GUARD_COEF = 2, GD_GUARD_OK = 3, GD_GUARD_APPLIED = 4, GD_GUARD_SKIPPED = 5,
       GD_GUARD_RECORD = 6 };
#define GD_GUARD_CHUNK 65536L /* elements of one tensor summed by one workgroup into one partial slot */
/* rec[0] = (accumulate ? rec[0] : 0) + sum over the `count` fp32 tensors (grads[t], ns[t] elements; host arrays) of
 * (g * gscale)^2.  The (pointer, n) pairs travel by value in the kernel arguments, 48 per launch: nothing is copied to
 * or pinned for the device, so gradient buffers may move from step to step.  fp64 accumulation; one partial per
 * (tensor, GD_GUARD_CHUNK elements of it) in ws, summed by a second stage in a fixed ascending order: no atomics, the
 * same bits on every run, whatever the launch geometry.  Pointers need only element alignment (16-byte loads from the
 * first 16-byte boundary of each chunk, scalar head and tail).  A non-finite gradient makes the sum non-finite.
 * ws: gd_grad_sqnorm_ws_bytes(sum_t ceil(ns[t] / GD_GUARD_CHUNK)) bytes. */
size_t gd_grad_sqnorm_ws_bytes(long total_chunks);
int gd_grad_sqnorm(const float* const* grads, const long* ns, int count, float gscale, int accumulate, double* rec, void* ws,
                   size_t ws_bytes, void* stream);
/* norm = sqrt(sqnorm); ok = isfinite(norm), or 1 whatever the norm when skip_nonfinite == 0; coef = min(1, max_norm /
 * (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), 1 when max_norm <= 0; applied_steps += ok; skipped_steps += !ok. */
int gd_guard_finalize(double* rec, double max_norm, int skip_nonfinite, void* stream);
/* gd_adamw with the gradient read as g * (grad_scale * coef), nothing written when ok == 0, and the bias corrections
 * taken from applied_steps (which gd_guard_finalize has already advanced for this step): a skipped step does not
 * advance Adam's time.  ema: NULL, or the averaged weights, updated in the same pass as ema = ema_decay * ema +
 * (1 - ema_decay) * p_new.  The scaled gradient is never written back.  16-byte accesses when all tensors share their
 * offset from a 16-byte boundary, scalar otherwise. */
int gd_adamw_guarded(float* p, const float* g, float* m, float* v, float* ema, long n, const double* rec, float lr, float beta1,
                     float beta2, float eps, float weight_decay, float grad_scale, float ema_decay, void* stream);

/* ------------------------------------------------------------------------------------------
 * Filters: the trainer's smoothing_method hook (GAN_DANet_train.ipynb: smooth_data_gaussian / _median /
 * _savitzky_golay) and the Gaussian smoothing and gap fill of datasets.py (gaussian_filter per plane,
 * fill_placeholder_with_nearest), with scipy's semantics.  A dense tensor is seen as (outer, L, inner) around the
 * filtered axis; storage fp32 (dtype 0) or fp64 (dtype 1); every sum is fp64, rounded to the storage type once per pass
 * (scipy's correlate1d).  The caller owns all memory, nothing is allocated or copied, nothing waits for the device; no
 * atomics: the same bits on every run.  Pointers need element alignment only.  Index arithmetic is 64-bit and launches
 * are cut where a grid dimension would pass its limit.  NaN inputs: the correlations propagate them like any sum; the
 * median of a window that holds a NaN is unspecified.
 * ---------------------------------------------------------------------------------------- */
enum { GD_FILTER_F32 = 0, GD_FILTER_F64 = 1 };
enum { GD_EDGE_REFLECT = 0, GD_EDGE_INTERIOR = 1 };
#define GD_FILTER_MAX_RADIUS 64 /* taps = 2 * radius + 1 <= 129: sigma <= 16 at truncate 4 */
#define GD_SAVGOL_MAX_WINDOW 33
/* host only, no GPU call: scipy's Gaussian taps.  radius = int(truncate * sigma + 0.5); w[k + radius] = exp(-0.5 / sigma^2 *
 * k^2) / sum, k = -radius .. radius, in fp64 (the sum in np.sum's order).  Returns the radius; negative when sigma <= 0 or
 * 2 * radius + 1 > cap (the capacity of w in doubles). */
int gd_gaussian_weights_host(double sigma, double truncate, double* w, int cap);
/* dst[o, l, i] = sum_{k = -radius .. radius} w_host[k + radius] * src[o, idx(l + k), i], taps added in ascending k.
 * w_host: 2 * radius + 1 doubles in HOST memory; they travel in the kernel arguments.  radius <= GD_FILTER_MAX_RADIUS.
 * src != dst.  edge_mode GD_EDGE_REFLECT = scipy's 'reflect' (half-sample symmetric): with p = 2L and j = (l + k) mod p
 * (0 <= j < p), idx = j < L ? j : p - 1 - j -- any radius against any L, L == 1 included.  GD_EDGE_INTERIOR: only
 * l in [radius, L - radius) is written, the rest of dst is left as it was (savgol_filter's interior).
 * inner > 1: lanes along inner (16 bytes per lane where inner is a whole number of 16-byte vectors and src and dst share
 * their offset from a 16-byte boundary; a scalar head and tail, or all columns scalar, otherwise); inner == 1: lanes
 * along L, a segment plus halo staged in LDS (16-byte loads for the rows that start on a 16-byte boundary). */
int gd_correlate1d_axis(const void* src, void* dst, int dtype, long outer, long L, long inner, const double* w_host, int radius,
                        int edge_mode, void* stream);
/* scipy.signal.savgol_filter's mode='interp' edges: with h = window / 2, for p < h
 *   dst[o, p, i]         = sum_j edge_dev[0][p][j] * src[o, j, i]
 *   dst[o, L - h + p, i] = sum_j edge_dev[1][p][j] * src[o, L - window + j, i]      (j < window)
 * edge_dev: (2, h, window) doubles in DEVICE memory (rows of the least-squares hat matrix).  window odd, <=
 * GD_SAVGOL_MAX_WINDOW and <= L; src != dst; nothing else of dst is written. */
int gd_savgol_edges_axis(const void* src, void* dst, int dtype, long outer, long L, long inner, const double* edge_dev,
                         int window, void* stream);
/* scipy.ndimage.median_filter(mode='reflect') over a box on a dense tensor seen as 4-D: shape4 and size4 are HOST arrays
 * (pad leading dimensions with shape 1, size 1).  Each size is 1, 3 or 5 and their product is 3, 5, 9, 25, 27 or 81.  The
 * median of an odd count is one of the inputs: the result is exact.  src != dst. */
int gd_median_nd(const void* src, void* dst, int dtype, const int64_t* shape4, const int* size4, void* stream);
/* fill_placeholder_with_nearest (datasets.py:222-250) around its two gaussian_filter calls: gd_fill_prepare writes
 * vals = x <= placeholder ? 0 : x and mask = x <= placeholder ? 0 : 1; gd_fill_ratio writes dst = num / (den == 0 ? 1 : den)
 * where x <= placeholder (the quotient in fp64, rounded once) and dst = x bit for bit elsewhere.  Every buffer is a
 * buffer of its own. */
int gd_fill_prepare(const void* x, double placeholder, void* vals, void* mask, int dtype, long n, void* stream);
int gd_fill_ratio(const void* x, const void* num, const void* den, double placeholder, void* dst, int dtype, long n,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Spline zoom (spline.hip): scipy.ndimage.zoom at orders 0, 1 and 3, which the inference notebooks apply to everything
 * behind the loader loop (test.ipynb cell 3, after the `with torch.no_grad()` loop), and the pointwise chain that turns
 * the tiles into a product in physical units.  A dense tensor is seen as (outer, L, inner) around the zoomed axis;
 * storage fp32 (dtype 0) or fp64 (dtype 1), all arithmetic fp64, one rounding to the destination type.  The caller owns
 * all memory, nothing is allocated, nothing waits for the device, no atomics.  Pointers need element alignment only.
 * The rules, per axis (grid_mode=False): output o samples the coordinate o * (Lin - 1) / (Lout - 1) (0 when Lout == 1);
 * order 0 takes sample floor(c + 0.5); order 1 taps f = floor(c) and f + 1 with weights 1 - t, t (t = c - f); order 3 taps
 * f - 1 .. f + 2 of the prefiltered coefficients with u = 1 - t, w0 = u^3 / 6, w1 = (t^2 (t - 2) 3 + 4) / 6,
 * w2 = (u^2 (u - 2) 3 + 4) / 6, w3 = 1 - w0 - w1 - w2.  A tap outside [0, n - 1] folds whole-sample symmetric: p = 2 (n - 1),
 * j = i mod p, index j < n ? j : p - j (0 when n == 1).
 * ---------------------------------------------------------------------------------------- */
enum { GD_ZOOM_MIRROR = 0, GD_ZOOM_NEAREST = 1 };
/* zoom(..., order, mode) along one axis: `trend_ups = zoom(trend25, (1, 5, 5), order=3)`, `zoom(tpbh, (5, 5), order=1)`,
 * `zoom(biash, (1, 1.25, 1.25), order=3)`, `zoom(uncr, (1, 5, 5), order=0, mode='nearest')` of test.ipynb cell 3, `tpbl =
 * zoom(tpbl, (2, 2), order=1)` of the 0.25-degree script, and the `zoom(..., order=3, mode='nearest')` calls of
 * datasets.py:294-303, one axis per call.  src (outer, Lin, inner) in src_dtype -> dst (outer, Lout, inner) in dst_dtype;
 * src != dst.  order in {0, 1, 3}.  GD_ZOOM_MIRROR is scipy's mode 'constant' (its default; the coordinates never leave the
 * array, so cval is never produced) and 'mirror'; GD_ZOOM_NEAREST is 'nearest', which at order 3 pads the line by 12 edge
 * samples either way in front of the prefilter (half-sample symmetric boundary sums) and shifts the coordinates by 12; the
 * two agree at orders 0 and 1.  ws: gd_zoom_axis_ws_bytes(outer, Lin, inner, order, mode) bytes -- the fp64 coefficients
 * of order 3 ((outer, Lin or Lin + 24, inner)); 0 bytes (ws may be NULL) at orders 0 and 1.
 * Order 3 is the prefilter into ws and the interpolation out of it.  The prefilter cuts every line into chunks that are
 * warm-started from 40 samples of look-back / look-ahead (z^40 = 1.3e-23; the exact boundary sums where the horizon
 * reaches an end of the line): inner > 1 runs lanes along inner, 64 samples per thread; inner == 1 stages row segments
 * in LDS and runs lanes along the line, 9 samples per thread. */
size_t gd_zoom_axis_ws_bytes(long outer, long Lin, long inner, int order, int mode);
int gd_zoom_axis(const void* src, void* dst, int src_dtype, int dst_dtype, long outer, long Lin, long Lout, long inner,
                 int order, int mode, void* ws, size_t ws_bytes, void* stream);
/* scipy.ndimage.spline_filter1d(order=3, mode='mirror', output=float64) along one axis, the prefilter that
 * `zoom(trend25, (1, 5, 5), order=3)` (test.ipynb cell 3) runs first: pole z = sqrt(3) - 2, the samples scaled by
 * (1 - z)(1 - 1 / z) = 6, causal c[i] += z c[i-1] from c[0] = (c[0] + z^(n-1) c[n-1] + sum_{i=1}^{n-2} z^i (c[i] +
 * z^(n-1) c[n-1-i])) / (1 - z^(2(n-1))), anticausal c[i] = z (c[i+1] - c[i]) from c[n-1] = (z c[n-2] + c[n-1]) z / (z^2 - 1);
 * a line of one sample passes through.  src (outer, L, inner) in src_dtype -> dst, fp64, same shape; src != dst. */
int gd_spline_prefilter_axis(const void* src, double* dst, int src_dtype, long outer, long L, long inner, void* stream);
/* `res = res + trend_ups`, `scaler025.inverse_transform(...)`, `* 10.0` and `res_cm[:, tpbh_hi == 0] = np.nan` of test.ipynb
 * cell 3 in one pass: dst = ((x + trend) * scale + mean) * unit in fp64, evaluated in exactly that order with every
 * operation rounded (no FMA contraction), so an fp64 dst equals numpy's bit for bit; NaN where mask[p] == 0.  x, trend,
 * dst: planes x hw elements; mask: hw bytes shared by all planes.  trend and mask may be NULL (no addition, no NaN).
 * dst may alias x only when their dtypes match. */
int gd_restore_units(const void* x, int x_dtype, const void* trend, int trend_dtype, const unsigned char* mask, long planes,
                     long hw, double scale, double mean, double unit, void* dst, int dst_dtype, void* stream);
/* `np.nanmean(res_cm, axis=(1, 2))` of test.ipynb cell 3: gd_masked_plane_mean on fp64 planes, with np.nanmean's rule that a
 * NaN pixel is left out like a masked one (a plane of NaNs gives NaN, count 0). */
size_t gd_masked_plane_mean_f64_ws_bytes(long planes, long hw);
int gd_masked_plane_mean_f64(const double* x, long planes, long hw, const unsigned char* mask, double* mean, long long* count,
                             void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dataset preparation (prepare.hip): the per-channel StandardScaler of datasets.py's load_data() (the
 * `scaler.fit_transform(hr_aux[..., i].reshape(-1, 1))` loop over the last axis and the two single-feature GRACE scalers)
 * and frequency_domain_augmentation() (datasets.py:318-347).  Storage fp32 (dtype 0) or fp64 (dtype 1), all arithmetic
 * fp64, one rounding to the output type.  The caller owns all memory, nothing is allocated, nothing waits for the device;
 * no atomics, every reduction in an order fixed by the shape: the same bits on every run.  Pointers need element
 * alignment only.  STL (detrend_and_compare) has its own section below.
 * ---------------------------------------------------------------------------------------- */
#define GD_FREQ_MAX_BINS 33                  /* K1 <= 33: seasonal_freq <= 32 */
#define GD_FREQ_LDS_BYTES 32768              /* table columns one workgroup holds; a longer axis is cut into chunks */
#define GD_FREQ_MAX_TABLE_BYTES (16L << 20)  /* the whole K1 x L table of doubles */
/* x: a channel-last array seen as (M rows, C channels).  rec (device, C x 3 doubles): count, mean, M2 = sum (x - mean)^2 of
 * every channel.  Pass one: workgroup b reduces the rows [b * R, (b + 1) * R) -- R a function of (M, C) alone -- reading
 * them as one contiguous run of R * C elements (C <= 256; 256-channel column blocks beyond), each thread a compensated
 * sum shifted by its first sample, the threads of a channel merged with Chan's formulas; pass two merges the workgroups'
 * records in ascending order.  ws: gd_channel_moments_ws_bytes(M, C) bytes. */
size_t gd_channel_moments_ws_bytes(long M, long C);
int gd_channel_moments(const void* x, int dtype, long M, long C, double* rec, void* ws, size_t ws_bytes, void* stream);
/* host only, no GPU call: sklearn's StandardScaler attributes from C records in HOST memory: mean_, var_ = M2 / count
 * (ddof 0), scale_ = sqrt(var_), and scale_ = 1 where sklearn calls the feature constant (_is_constant_feature:
 * var_ <= count * eps * var_ + (count * mean_ * eps)^2, eps = 2^-52). */
int gd_scale_from_moments_host(const double* rec, long C, double* mean, double* var, double* scale);
/* dst = (src - mean[c]) / scale[c] (inverse 0) or src * scale[c] + mean[c] (inverse 1), c the channel of the element: the
 * two operations of sklearn in their order, each rounded in fp64 (no reciprocal, no FMA), then one rounding to dst_dtype.
 * src (M, C) channel-last; mean_dev, scale_dev: C doubles in DEVICE memory.  N == 0: dst has the layout of src (16-byte
 * accesses when src and dst both start on a 16-byte boundary, scalar otherwise).  N > 0: src is (N, HW, C) with
 * N * HW == M and dst is (N, C, HW), `.permute(0, 3, 1, 2)` of CustomDataset in the same pass, as a tiled transpose
 * through LDS.  src != dst. */
int gd_channel_affine(const void* src, int src_dtype, void* dst, int dst_dtype, long M, long C, const double* mean_dev,
                      const double* scale_dev, int inverse, long N, long HW, void* stream);
/* host only, no GPU call: coef[k * L + t] = cos(2 pi ((k t) mod L) / L) / L for k < K1, t < L (K1 <= min(L, 33)). */
int gd_freq_cos_table_host(long L, int K1, double* coef);
/* frequency_domain_augmentation along one axis of a dense (outer, L, inner) tensor.  The reference adds REAL noise to the
 * FFT bins 0 .. K1 - 1, K1 = min(seasonal_freq, L - 1) + 1, and keeps the real part of the inverse FFT; by linearity
 *   dst[o, t, p] = src[o, t, p] + sum_{k < K1} noise[o, k, p] * coef[k, t]         (terms in ascending k, src added last).
 * noise: (outer, K1, inner) doubles and coef: the table of gd_freq_cos_table_host, both in DEVICE memory.  dst may be a
 * slab of a larger buffer; src != dst.  1 <= K1 <= min(L, GD_FREQ_MAX_BINS) and K1 * L * 8 <= GD_FREQ_MAX_TABLE_BYTES.
 * Lanes along inner, a thread keeps its K1 noise values in registers and walks the axis; two series per lane when inner
 * is even and src and dst start on 16-byte boundaries, one otherwise. */
int gd_freq_augment_axis(const void* src, void* dst, int dtype, long outer, long L, long inner, const double* noise, int K1,
                         const double* coef, void* stream);

/* ------------------------------------------------------------------------------------------
 * Basin analysis (basins.hip): the loop over the basins of Basin_TWSA_Comparison_GRACE_Downscaled.ipynb (cell 5), which
 * rasterises every basin polygon on the 0.25 and the 0.05 degree grid and averages both products over it.
 * The containment rule (csrc/zones.h; the device kernel, the host entry and the tests use this one rule): a zone is a set
 * of rings -- the outer rings and the holes of all its parts, in any order and orientation -- stored as edges
 * (x0, y0, x1, y1).  The point (px, py) is inside the zone iff an odd number of its edges satisfy both
 *   (y0 > py) != (y1 > py)                          half-open: a horizontal edge never counts, a ray through a vertex
 *                                                   counts once
 *   px < x0 + (py - y0) * (x1 - x0) / (y1 - y0)     in fp64, every operation rounded on its own
 * For a valid (Multi)Polygon that is shapely's `contains` at every point that is not on a boundary.  Points exactly on a
 * boundary are unspecified (shapely calls them outside).
 * The caller owns all memory, nothing is allocated, nothing waits for the device; no global atomics, every reduction in
 * an order fixed by the shape: the same bits on every run.  Pointers need element alignment only.
 * ---------------------------------------------------------------------------------------- */
#define GD_ZONE_MAX 32           /* zones per call: one bit of a word each */
#define GD_ZONE_EDGE_CHUNK 512   /* edges of a zone the rasteriser takes per pass (the capacity of a row's crossing list) */
/* `mask = np.array([polygon.contains(pt) for pt in points]).reshape(lat_grid.shape)` of cell 5, for Z polygons at once.
 * edges: (E, 4) doubles in DEVICE memory, the edges of zone z at rows edge_off[z] .. edge_off[z + 1] - 1; edge_off: Z + 1
 * longs in HOST memory, read before the launch: edge_off[0] == 0, never decreasing, edge_off[Z] == E (a zone may be
 * empty).  1 <= Z <= GD_ZONE_MAX, 1 <= E <= 2^30.  The grid is rectilinear: point (i, j) is (xs[j], ys[i]), xs (W) and
 * ys (H) doubles in DEVICE memory, not necessarily uniform, ascending or descending.  bits: (H, W) words, bit z set iff
 * the point is in zone z; every word is written (no need to clear it first).
 * A workgroup owns 4 rows x 1024 columns: per zone and per chunk of GD_ZONE_EDGE_CHUNK edges its threads test the edges
 * against the 4 rows and append the crossings of the straddling ones to per-row lists in LDS; one wave per row then
 * flips the zone's bit of every column with an odd number of crossings to its right.  O(E + W k) per row, k the
 * crossings of the row, against O(E W) point by point. */
int gd_zone_rasterize(const double* edges, long E, const long* edge_off, int Z, const double* xs, long W, const double* ys,
                      long H, unsigned int* bits, void* stream);
/* host only, no GPU call: the same arguments, all in HOST memory; plain loops over the predicate of csrc/zones.h */
int gd_zone_rasterize_host(const double* edges, long E, const long* edge_off, int Z, const double* xs, long W,
                           const double* ys, long H, unsigned int* bits);
/* `np.nanmean(data[:, mask], axis=1)` of cell 5 for all Z zones in ONE pass over the data.  x: planes x hw elements, fp32
 * (dtype 0) or fp64 (dtype 1); bits: hw words of gd_zone_rasterize shared by all planes; weights: hw doubles (for
 * instance cos(lat)) or NULL = 1 everywhere, as in the notebook.  A pixel contributes to zone z iff bit z is set and the
 * value is not NaN.  mean (planes, Z) = sum w v / sum w, count (planes, Z) = the contributing pixels; without a
 * contributing pixel, or with a weight sum of zero, the mean is NaN and the count 0.  planes <= 65535 per call.
 * ws: gd_zone_mean_ws_bytes(planes, hw, Z) bytes.  Each thread keeps the Z (8, 16 or 32 with the padding) triples
 * (sum w v, sum w, count) in registers; per-workgroup partials go to ws and a second kernel adds them in ascending order. */
size_t gd_zone_mean_ws_bytes(long planes, long hw, int Z);
int gd_zone_mean(const void* x, int dtype, long planes, long hw, const unsigned int* bits, int Z, const double* weights,
                 double* mean, long long* count, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * STL decomposition (stl.hip, csrc/stl_core.h): `detrend_and_compare` of datasets.py, which calls statsmodels'
 * `STL(y, seasonal=13, period=12).fit()` once per grid point, for all M series of a (T, M) array in one launch.
 * The algorithm is Cleveland et al. 1990 as netlib's stl.f computes it, with every jump 1.  Positions 1-based.
 *   est(y, n, len, deg, xs, nleft, nright, userw, rw): h = max(xs - nleft, nright - xs), plus (len - n) / 2 (integer) when
 *     len > n; for j = nleft .. nright, r = |j - xs|: w_j = 0 beyond 0.999 h, 1 up to 0.001 h, (1 - (r / h)^3)^3 between, times
 *     rw_j under userw; a = sum w_j, not ok when a <= 0; w_j /= a; with h > 0 and deg > 0: a = sum w_j j, b = xs - a,
 *     c = sum w_j (j - a)^2, and if sqrt(c) > 0.001 (n - 1): w_j *= (b / c) (j - a) + 1; ys = sum w_j y_j.
 *   ess(y, n, len, deg): ys = y when n < 2; the window is [1, n] when len >= n, else it starts at [1, len] and moves right by
 *     one for every position beyond (len + 1) / 2 until it touches n; ys_i = y_i where est is not ok.
 *   One inner pass, from trend (0 at first): w = y - trend; every cycle-subseries j = 1 .. period of w (length
 *     k = (n - j) / period + 1) is smoothed by ess(k, seasonal, seasonal_deg) and extended by est at positions 0 (window
 *     [1, min(seasonal, k)]) and k + 1 (window [max(1, k - seasonal + 1), k]), each falling back on the neighbouring
 *     smoothed value, giving C (n + 2 period); L = ess(n, low_pass, low_pass_deg) of the moving averages of lengths period,
 *     period and 3 of C; seasonal_i = C_(period + i) - L_i; trend = ess(n, trend, trend_deg) of y - seasonal.
 *   outer_iter + 1 outer passes of inner_iter inner passes each; after every outer pass but the last the robustness
 *     weights are renewed: r_i = |y_i - trend_i - seasonal_i|, cmad = 3 (r_(m1) + r_(m2)) over the ascending order
 *     statistics m1 = n / 2 + 1, m2 = n - m1 + 1; rw_i = 1 up to 0.001 cmad, (1 - (r_i / cmad)^2)^2 up to 0.999 cmad, 0 beyond;
 *     every est from then on runs under userw (the low-pass one never does).  resid = y - seasonal - trend.
 * Storage fp32 (dtype 0) or fp64 (dtype 1), all arithmetic fp64 with every operation rounded on its own, one rounding to
 * the output type.  The moving averages are window sums per output (stl.f keeps a running sum): the one place where the
 * order of additions differs.  The caller owns all memory, nothing is allocated on the device, nothing waits for it; no
 * global atomics, no workspace; a series' result depends on the series and the parameters alone, not on M, its column or
 * the launch.  Pointers need element alignment only.  A series that holds a non-finite value has unspecified outputs.
 * Agreement with statsmodels itself has NOT been measured (it is not available here): it rests on this text, on closed-form
 * cases and on an independent fp64 restatement in the tests.
 * ---------------------------------------------------------------------------------------- */
#define GD_STL_MAX_T 2048 /* one series' working arrays, (6 T + 6 period + 2) doubles, must fit the 160 KiB LDS of a CU */
/* x, trend_out, seasonal_out, resid_out, weights_out (NULL = not wanted; all ones when outer_iter == 0): (T, M) arrays in
 * DEVICE memory, series m at x[t * M + m] (the reference's (time, x, y) layout flattened); no output may alias x or another
 * output.  period >= 2; seasonal, trend, low_pass odd and >= 3; trend > period; low_pass > period; degrees 0 or 1;
 * inner_iter >= 1; outer_iter >= 0; 2 * period <= T <= GD_STL_MAX_T.  statsmodels' defaults are trend = the smallest odd
 * integer >= 1.5 period / (1 - 1.5 / seasonal), low_pass = the smallest odd integer > period, inner_iter 5 and outer_iter 0,
 * or 2 and 15 with robust=True; they are the caller's to fill in.
 * A workgroup of 256 threads owns S neighbouring series, S = 40960 / the bytes of one series' working arrays, within
 * 1 .. 16 (4 at T = 181, period 12), held in LDS as [t][S] images; the threads share out the (series, output point) pairs
 * of every smoothing pass, and the order statistics of cmad are found by counting ranks in LDS. */
int gd_stl_decompose(const void* x, int dtype, long T, long M, int period, int seasonal, int trend, int low_pass, int seasonal_deg,
                     int trend_deg, int low_pass_deg, int inner_iter, int outer_iter, void* trend_out, void* seasonal_out,
                     void* resid_out, void* weights_out, void* stream);
/* host only, no GPU call: the same arguments, all in HOST memory; the same fit (csrc/stl_core.h) in plain loops */
int gd_stl_decompose_host(const void* x, int dtype, long T, long M, int period, int seasonal, int trend, int low_pass,
                          int seasonal_deg, int trend_deg, int low_pass_deg, int inner_iter, int outer_iter, void* trend_out,
                          void* seasonal_out, void* resid_out, void* weights_out);

/* ------------------------------------------------------------------------------------------
 * Per-pixel time series (series.hip, csrc/series_core.h): skill of one cube against another along the time axis of every
 * pixel, a masked least-squares fit of every pixel's series against a common design matrix (trend and annual /
 * semi-annual harmonics) and the NaN-aware block mean that takes the 0.05 degree product back to the 0.25 degree grid.
 * The reference gestures at these: the map comparison of test.ipynb `_plot_spatial_distribution`, `pearsonr` of two
 * series, and taylorDiagram.py:151-159 (std with ddof 1 and corrcoef).
 * A series is a column of a dense (T, M) array, series m at x[t * M + m], as for gd_stl_decompose.  Storage fp32 (dtype 0)
 * or fp64 (dtype 1), all arithmetic fp64, one rounding to the output.  One thread owns a series and walks t in ascending
 * order, neighbouring threads own neighbouring m (every time step is one coalesced row read); T is never split, so a
 * series' result depends on the series and the parameters alone, not on M, its column or the launch.  The caller owns all
 * memory, nothing is allocated, nothing waits for the device; no global atomics, no workspace.  Pointers need element
 * alignment only.  Every device entry but gd_harmonic_finalize has a host twin (`_host`, no GPU call, every pointer in
 * HOST memory) that runs the same operations in the same order (series_core.h): records, maps, coefficients, rss and
 * block means agree bit for bit.
 * ---------------------------------------------------------------------------------------- */
/* the maps of gd_series_skill: bit k of `which` selects map k; the selected maps are written in ascending k */
enum { GD_SKILL_N = 0, GD_SKILL_MEAN_P = 1, GD_SKILL_MEAN_T = 2, GD_SKILL_BIAS = 3, GD_SKILL_RMSE = 4, GD_SKILL_MAE = 5,
       GD_SKILL_STD_P = 6, GD_SKILL_STD_T = 7, GD_SKILL_CC = 8, GD_SKILL_NSE = 9, GD_SKILL_KGE = 10, GD_SKILL_CRMSD = 11,
       GD_SKILL_MAPS = 12 };
#define GD_LSTSQ_MAX_P 8 /* columns of the design matrix: P (P + 1) / 2 + P = 44 fp64 accumulators per thread at the cap */
/* The RECORD ("Evaluation") of every series: rec is (8, M) doubles, planar, plane k of series m at rec[k * M + m].  The
 * update is sequential, one pair at a time in ascending t (the single-pair form of the merge stated under "Evaluation"):
 *   n' = n + 1, dp = p - mean_p, dt = t - mean_t, f = n / n', mean += d / n', M2_p += dp^2 f, M2_t += dt^2 f,
 *   C += dp dt f, sum|d| += |p - t|, sum d^2 += (p - t)^2.
 * mask: NULL, or M bytes; a series whose byte is 0 is skipped: its record is zeroed (n = 0), or left as it is under
 * `accumulate`.  flags: GD_EVAL_SKIP_NAN drops a pair with a NaN on either side, without it NaNs propagate.
 * accumulate != 0 continues from the record in rec (n <= 0 there counts as empty), so a cube may be fed in chunks of time
 * steps: the recurrence being sequential, chunks give the same bits as one call. */
int gd_series_stats(const void* pred, const void* truth, int dtype, long T, long M, const unsigned char* mask, int flags,
                    double* rec, int accumulate, void* stream);
int gd_series_stats_host(const void* pred, const void* truth, int dtype, long T, long M, const unsigned char* mask, int flags,
                         double* rec, int accumulate);
/* The maps selected by `which` from the records, M doubles each, the j-th selected map at out[j * M + m]:
 *   n, mean_p, mean_t, bias = mean_p - mean_t, rmse = sqrt(sum d^2 / n), mae = sum|d| / n,
 *   std_p, std_t = sqrt(M2 / (n - ddof)) (ddof 0 as np.std, 1 as taylorDiagram.py:151; NaN when n <= ddof),
 *   cc = C / sqrt(M2_p M2_t) clipped to [-1, 1] as np.corrcoef, NaN at zero variance,
 *   nse = 1 - sum d^2 / M2_t with the r2_score rules of gd_eval_merge_host at M2_t == 0,
 *   kge = 1 - sqrt((cc - 1)^2 + (sqrt(M2_p / M2_t) - 1)^2 + (mean_p / mean_t - 1)^2)  (the std ratio is free of ddof),
 *   crmsd = sqrt((M2_p + M2_t - 2 C) / n), the centred RMS difference of the Taylor diagram (clamped at 0).
 * n == 0 gives NaN everywhere except n.  A record of gd_eval_stats is an (8, 1) record set. */
int gd_series_skill(const double* rec, long M, int ddof, int which, double* out, void* stream);
int gd_series_skill_host(const double* rec, long M, int ddof, int which, double* out);
/* Masked linear least squares of every series against a common design matrix: basis is (T, P) doubles, row t at
 * basis[t * P], 1 <= P <= GD_LSTSQ_MAX_P; a sample that is NaN is left out of that series' fit.  Per series: a first pass
 * accumulates the P (P + 1) / 2 entries of A^T A and the P of A^T y in registers (the basis rows are the same for every
 * lane and come through the scalar cache), a Cholesky solve in fp64, and a second pass over the series that sums the
 * squared residuals y - A c directly (y^T y - c^T A^T y cancels).  coef: (P, M) planar.  rss, n_out: (M) doubles, either
 * may be NULL; n_out is the number of samples that entered the fit.  With fewer valid samples than P, or a pivot
 * <= P 2^-52 times its diagonal entry, coef and rss are NaN (n_out stays the valid count). */
int gd_series_lstsq(const void* x, int dtype, long T, long M, const double* basis, int P, double* coef, double* rss,
                    double* n_out, void* stream);
int gd_series_lstsq_host(const void* x, int dtype, long T, long M, const double* basis, int P, double* coef, double* rss,
                         double* n_out);
/* From the coefficient planes of a fit against the columns 1, [tau], cos w_1 t, sin w_1 t, ... cos w_K t, sin w_K t
 * (P = 1 + has_trend + 2 K, 0 <= K <= 3): amp (K, M) = hypot(c_k, s_k) and phase (K, M) = atan2(s_k, c_k), so that
 * c cos wt + s sin wt = amp cos(wt - phase); slope (M) = coef[1] * tau_scale (has_trend only); rms (M) = sqrt(rss / n).
 * Every output may be NULL; rms needs rss and n.  Device only: hypot and atan2 are the device library's. */
int gd_harmonic_finalize(const double* coef, int P, long M, int K, int has_trend, double tau_scale, const double* rss,
                         const double* n, double* amp, double* phase, double* slope, double* rms, void* stream);
/* NaN-aware mean of every fy x fx block of the last two axes of x (planes, H, W): the inverse of the notebook's
 * np.repeat(np.repeat(bias, 4, 1), 4, 2).  H % fy == 0 and W % fx == 0.  weights: NULL, or (H, W) doubles shared by all
 * planes (for instance cos(lat)).  out (planes, H / fy, W / fx), in the input dtype: sum w v / sum w over the non-NaN
 * members of the block, added in row-major order; NaN when fewer than min_count members contribute or the weight sum is
 * 0.  count (int32, may be NULL): the contributors. */
int gd_block_mean(const void* x, int dtype, long planes, long H, long W, int fy, int fx, const double* weights,
                  int min_count, void* out, int* count, void* stream);
int gd_block_mean_host(const void* x, int dtype, long planes, long H, long W, int fy, int fx, const double* weights,
                       int min_count, void* out, int* count);

/* ------------------------------------------------------------------------------------------
 * Per-pixel trend tests (trend.hip, csrc/trend_core.h): the Mann-Kendall test and the Theil-Sen slope with its confidence
 * interval for every series of a (T, M) cube, plain or in the seasonal form of Hirsch and Slack -- the significance and the
 * robust slope that a GRACE trend map carries.  scipy.stats.theilslopes (method 'separate') and scipy.stats.kendalltau
 * compute the same quantities with the same arithmetic; slope, intercept, the interval and tau equal theirs bit for bit.
 * The layout is that of the section above: series m of a dense (T, M) array at x[t * M + m], storage fp32 (dtype 0) or
 * fp64 (dtype 1), all arithmetic fp64 with every operation rounded on its own.  2 <= T <= GD_TREND_MAX_T.  times: T
 * doubles, finite and strictly increasing (the device entry does not look: its caller checks; the host twin does).  NaN
 * samples are dropped from their series; a series that holds an infinity has unspecified outputs.  mask: NULL, or M bytes,
 * 0 = leave the series out (n = 0).
 * For one series with the valid samples (t_k, y_k), k = 0 .. n - 1, in time order:
 *   s      = sum over i < j of sign(y_j - y_i);
 *   var_s  = (1.0 / 18.0) * (n (n - 1)(2 n + 5) - sum over samples of (c_i - 1)(2 c_i + 5)), c_i the samples equal to y_i;
 *   z      = (s - sgn(s)) / sqrt(var_s) under GD_TREND_CONTINUITY, else s / sqrt(var_s); NaN at var_s = 0, 0 at s = 0;
 *   p      = erfc(|z| * 0.7071067811865476), two-sided;
 *   tau    = s / sqrt(tot) / sqrt(tot - ytie) clipped to [-1, 1] (tau-b with tie-free times), tot = n (n - 1) / 2,
 *            ytie = sum over tie groups of c (c - 1) / 2; NaN when ytie = tot;
 *   slope  = the median of the nt = tot values (y_j - y_i) / (t_j - t_i), i < j (zeros as +0.0): (a + b) * 0.5 of the
 *            order statistics (nt - 1) / 2 and nt / 2;
 *   intercept = median(y) - slope * median(t);
 *   slope_lo, slope_hi = the order statistics Rl = max(rint((nt + zq sigma) / 2) - 1, 0) and
 *            Ru = min(rint((nt - zq sigma) / 2), nt - 1), sigma = sqrt(var_s), rint to even; zq is the normal quantile of
 *            alpha / 2 (negative), computed by the caller.
 * period >= 2 (0 = none): sample index k of the T belongs to season k mod period; only pairs inside a season count, ties
 * are counted inside a season, s, n (n - 1)(2 n + 5), the tie sum, tot, ytie and nt are sums over the seasons, and slope
 * and interval are order statistics of the pooled slopes; the medians of y and t are over all valid samples.
 * n < 2: n is exact, s = 0, everything else NaN.  nt = 0 (no season with two samples): slope .. slope_hi are NaN.
 * out: planar doubles, map k of series m at out[k * M + m], k as below.  flags: GD_TREND_SEN computes slope and
 * intercept, GD_TREND_CI (needs SEN) the interval; planes that were not asked for are left untouched.
 * One wave owns a series, its samples in LDS; the sums are integers; the order statistics are found by an exact radix
 * select on the monotone 64-bit key of the slope, whose every pass recomputes the slopes: no storage proportional to T^2,
 * no workspace, no global atomics, and a series' result depends on the series and the parameters alone.  The host twin
 * sorts the stored slopes of a series instead and agrees bit for bit on every map but p (each side's erfc).
 * ---------------------------------------------------------------------------------------- */
#define GD_TREND_MAX_T 2048
enum { GD_TREND_N = 0, GD_TREND_S = 1, GD_TREND_VAR_S = 2, GD_TREND_Z = 3, GD_TREND_P = 4, GD_TREND_TAU = 5, GD_TREND_SLOPE = 6,
       GD_TREND_INTERCEPT = 7, GD_TREND_SLOPE_LO = 8, GD_TREND_SLOPE_HI = 9, GD_TREND_MAPS = 10 };
enum { GD_TREND_SEN = 1, GD_TREND_CI = 2, GD_TREND_CONTINUITY = 4 };
int gd_trend_test(const void* x, int dtype, long T, long M, const double* times, int period, const unsigned char* mask,
                  int flags, double zq, double* out, void* stream);
int gd_trend_test_host(const void* x, int dtype, long T, long M, const double* times, int period, const unsigned char* mask,
                       int flags, double zq, double* out);

/* ------------------------------------------------------------------------------------------
 * Per-pixel change points (changepoint.hip, csrc/changepoint_core.h): WHEN did the behaviour of a series change -- the
 * Pettitt test (Pettitt 1979), the CUSUM statistics of Buishand (1982) and two least-squares two-segment fits (a shift of
 * the mean; two separate lines) for every series of a (T, M) cube.
 * The layout is that of "Per-pixel trend tests": series m of a dense (T, M) array at x[t * M + m], storage fp32 (dtype 0) or
 * fp64 (dtype 1), all arithmetic fp64 with every operation rounded on its own.  2 <= T <= GD_CP_MAX_T.  times: T doubles,
 * finite and strictly increasing (the device entry does not look: its caller checks; the host twin does).  NaN samples are
 * dropped from their series; a series that holds an infinity has unspecified outputs.  mask: NULL, or M bytes, 0 = leave
 * the series out (n = 0).  window: NULL, or 2 M ints, begin[m] followed by end[m]: only the samples begin <= t < end of
 * series m take part; begin is clamped to 0 .. T and end to begin .. T.  2 <= min_seg <= GD_CP_MAX_T: the smallest number of
 * valid samples on either side of a candidate break of the two fitted models (above n / 2 there is no candidate).
 * For one series with the valid samples (t_k, y_k), k = 0 .. n - 1, in time order, i_k their index among the T steps; every
 * "index" is the i_k of the LAST SAMPLE BEFORE the change, as a double:
 *   n         the number of valid samples (written whatever the flags).
 *   GD_CP_PETTITT  V_k = sum over all j of sign(y_k - y_j); U_k = sum over i <= k of V_i, k = 0 .. n - 2 (= sum over i <= k,
 *             j > k of sign(y_i - y_j)); pt_k = max |U_k|, taken at the smallest such k; pt_u the signed U there (positive:
 *             the series was higher before the change); pt_index = i_k; pt_p = min(1, 2 exp(-(6 K^2) / (n^3 + n^2))), K =
 *             pt_k, both integers exact in doubles.  All sums are integers and exact.  n < 2: NaN, index -1.
 *   GD_CP_CUSUM    ybar = (sum y) / n; S_k = sum over i <= k of (y_i - ybar); ss = sum of (y_i - ybar)^2, each sum sequential in
 *             time order; sd = sqrt(ss / n); cs_q = (max_k |S_k| / sd) / sqrt(n); cs_r = ((max(0, max S) - min(0, min S)) /
 *             sd) / sqrt(n); cs_index = i_k at the first maximum of |S_k|; cs_p = 1 where cs_q < 0.3, else
 *             2 sum over j = 1 .. 20 of (-1)^(j + 1) exp(-2 j^2 q^2), summed in that order and clipped to [0, 1]: the
 *             Brownian-bridge limit, asymptotic in n.  n < 1 or sd = 0 or NaN: NaN, index -1.
 *   GD_CP_STEP     candidates are the k with k + 1 >= min_seg and n - k - 1 >= min_seg.  m1, m2 = (sum y) / count of the
 *             samples i <= k and of the samples i > k, each summed in time order; rss_k = sum over i <= k of (y_i - m1)^2 +
 *             sum over i > k of (y_i - m2)^2, each sum in time order.  The break is the candidate of the smallest rss_k,
 *             ties to the smallest k: st_index = i_k, st_mean_before = m1, st_mean_after = m2, st_shift = m2 - m1,
 *             st_rss0 = ss as above, st_rss = rss_k, st_f = (rss0 - rss) / (rss / (n - 2)) as IEEE division gives it
 *             (0 / 0 = NaN, x / 0 = inf).  No candidate: every plane NaN, index -1.
 *   GD_CP_TREND    a segment is fitted in three passes in time order: tbar, ybar = (sum t) / count, (sum y) / count; stt =
 *             sum of (t - tbar)^2, sty = sum of (t - tbar)(y - ybar), b = sty / stt; rss_seg = sum of ((y - ybar) -
 *             b (t - tbar))^2; intercept = ybar - b tbar.  rss_k = rss_seg1 + rss_seg2; candidates and selection as for
 *             STEP.  tr_index = i_k, slopes and intercepts of both lines, tr_jump = line 2 minus line 1 at
 *             tm = (t_k + t_(k+1)) * 0.5, i.e. (a2 + b2 tm) - (a1 + b1 tm); tr_rss0 = the same three-pass fit over all n
 *             samples; tr_rss = rss_k; tr_f = ((rss0 - rss) / 2) / (rss / (n - 4)).  No candidate: every plane NaN, index -1.
 * Neither F statistic is corrected for the selection of the break among the candidates.
 * out: planar doubles, map k of series m at out[k * M + m], k as below.  flags selects the families; planes of families
 * that were not asked for are left untouched.
 * One wave owns a series, its valid (t, y, i) compacted in LDS; lanes own the candidates k in strides of 64 and the loop
 * over the samples j is uniform across the wave (sample j is an LDS broadcast, added to the "before" or "after"
 * accumulators by the predicate j <= k); U_k is an integer wave scan of V_k; the arg-max and arg-min are wave reductions
 * over (value, k) pairs.  No workspace, no global atomics, and a series' result depends on the series and the parameters
 * alone.  The host twin runs the same per-sample functions of changepoint_core.h in the same order and agrees bit for bit
 * on every map but pt_p and cs_p (each side's exp).
 * ---------------------------------------------------------------------------------------- */
#define GD_CP_MAX_T 2048
enum { GD_CP_N = 0, GD_CP_PT_K = 1, GD_CP_PT_U = 2, GD_CP_PT_INDEX = 3, GD_CP_PT_P = 4, GD_CP_CS_Q = 5, GD_CP_CS_R = 6,
       GD_CP_CS_INDEX = 7, GD_CP_CS_P = 8, GD_CP_ST_INDEX = 9, GD_CP_ST_MEAN_BEFORE = 10, GD_CP_ST_MEAN_AFTER = 11,
       GD_CP_ST_SHIFT = 12, GD_CP_ST_RSS0 = 13, GD_CP_ST_RSS = 14, GD_CP_ST_F = 15, GD_CP_TR_INDEX = 16,
       GD_CP_TR_SLOPE_BEFORE = 17, GD_CP_TR_SLOPE_AFTER = 18, GD_CP_TR_INTERCEPT_BEFORE = 19, GD_CP_TR_INTERCEPT_AFTER = 20,
       GD_CP_TR_JUMP = 21, GD_CP_TR_RSS0 = 22, GD_CP_TR_RSS = 23, GD_CP_TR_F = 24, GD_CP_MAPS = 25 };
enum { GD_CP_PETTITT = 1, GD_CP_CUSUM = 2, GD_CP_STEP = 4, GD_CP_TREND = 8 };
int gd_change_point(const void* x, int dtype, long T, long M, const double* times, const unsigned char* mask, const int* window,
                    int min_seg, int flags, double* out, void* stream);
int gd_change_point_host(const void* x, int dtype, long T, long M, const double* times, const unsigned char* mask,
                         const int* window, int min_seg, int flags, double* out);

/* ------------------------------------------------------------------------------------------
 * Lagged correlation (lagcorr.hip, csrc/lagcorr_core.h): how many months does storage run behind precipitation, an index or
 * any other driver, pixel by pixel, and how strong is the link at that lag; the autocorrelation of every series; and what a
 * correlation of two autocorrelated series is worth (effective sample size, Fisher z, p).
 * The layout is that of "Per-pixel time series": series m of a dense (T, M) array at x[t * M + m], storage fp32 (dtype 0) or
 * fp64 (dtype 1), all arithmetic fp64 with every operation rounded on its own.  1 <= T <= GD_LAG_MAX_T.
 *   Lag sign   r(l) correlates a[t] with b[t + l]: l > 0 means b follows a.  The lags are the closed range lag_lo .. lag_hi,
 *              -GD_LAG_MAX <= lag_lo <= lag_hi <= GD_LAG_MAX; lag lag_lo + k is row k of the curve.
 *   Pairs      only pairs with both members not NaN count (pairwise deletion, per lag).
 *   Centring   ma, mb: the mean of each series over its own samples that are not NaN, by the recurrence of gd_series_stats
 *              (m += (x - m) * (1 / n'), in time order).  With u = a - ma, v = b - mb the six sums n, Su, Sv, Suu, Svv, Suv
 *              run over the valid pairs of a (series, lag) in ascending t.
 *   r          va = Suu - Su Su / n, vb = Svv - Sv Sv / n, c = Suv - Su Sv / n, r = c / sqrt(va vb) clipped to [-1, 1];
 *              NaN when n < min_pairs (min_pairs >= 2), va <= 0 or vb <= 0.
 *   Broadcast  a_M == 1: a is one series of T values shared by all M series of b (an index against every pixel); else a_M == M.
 *   Best lag   over the lags whose r is not NaN: the largest |r| (GD_LAG_SELECT_ABS), the largest r (_MAX) or the smallest
 *              (_MIN); a tie goes to the smaller |l|, then to the positive lag.  best is (GD_LAG_PLANES, M) doubles, planar:
 *              best_lag (NaN when no lag is valid), best_r, best_n (the pairs at that lag, 0 when none is valid) and r0, the
 *              r of lag 0 (NaN when 0 is outside the range).  The choice is not corrected for the selection over lags.
 * r: (NL, M) doubles and n: (NL, M) int32, NL = lag_hi - lag_lo + 1, the curve and its pair counts.  r, n and best may each
 * be NULL, not all three; a curve that is not asked for is never written.  mask: NULL, or M bytes; a series whose byte is 0
 * is not read: NaN in r and best, 0 in n and best_n.
 * A workgroup owns 64 neighbouring series and walks time in chunks of GD_LAG_CHUNK steps whose centred values (with a halo
 * of the lag range for b, kept as a ring) sit in LDS; a lane holds the six sums of one series at up to 9 lags in registers
 * from the first sample to the last, the waves of the workgroup cover the lags.  The main loop reads every cube once; the
 * means come from a first pass over the same 64 columns.  No atomics, no workspace, nothing allocated: a series' result
 * depends on the series and the parameters alone, not on M, its column, the chunk length or the launch.  The host twins run
 * the same per-pair code and agree bit for bit on r, n, best and acf.
 * Errors (-1, gd_last_error): a NULL input, every output NULL, dtype, T, M, a_M not in {1, M}, a bad lag range, min_pairs < 2,
 * select or kind unknown, a pointer that is not element aligned.
 * ---------------------------------------------------------------------------------------- */
#define GD_LAG_MAX 64
#define GD_LAG_MAX_T 2048
#define GD_LAG_CHUNK 32 /* time steps per staged chunk (no result depends on it) */
enum { GD_LAG_BEST_LAG = 0, GD_LAG_BEST_R = 1, GD_LAG_BEST_N = 2, GD_LAG_R0 = 3, GD_LAG_PLANES = 4 };
enum { GD_LAG_SELECT_ABS = 0, GD_LAG_SELECT_MAX = 1, GD_LAG_SELECT_MIN = 2 };
enum { GD_ACF_PEARSON = 0, GD_ACF_STANDARD = 1 };
int gd_lag_corr(const void* a, const void* b, int dtype, long T, long M, long a_M, int lag_lo, int lag_hi, int min_pairs,
                int select, const unsigned char* mask, double* r, int* n, double* best, void* stream);
int gd_lag_corr_host(const void* a, const void* b, int dtype, long T, long M, long a_M, int lag_lo, int lag_hi, int min_pairs,
                     int select, const unsigned char* mask, double* r, int* n, double* best);
/* The autocorrelation of every series at the lags 0 .. K (0 <= K <= GD_LAG_MAX): acf (K + 1, M) doubles, n (K + 1, M) int32
 * (the valid pairs of each lag; may be NULL).  kind GD_ACF_PEARSON: r as above with a = b.  GD_ACF_STANDARD (Box-Jenkins):
 * acf_k = c_k / c_0, c_k = (1 / n0) sum (x_t - m)(x_(t+k) - m) over the valid pairs in ascending t, c_0 = (1 / n0) sum
 * (x_t - m)^2 over the n0 samples that are not NaN, m their mean; NaN at c_0 <= 0 or fewer than min_pairs pairs; acf_0 = 1. */
int gd_series_acf(const void* x, int dtype, long T, long M, int K, int kind, int min_pairs, const unsigned char* mask, double* acf,
                  int* n, void* stream);
int gd_series_acf_host(const void* x, int dtype, long T, long M, int K, int kind, int min_pairs, const unsigned char* mask,
                       double* acf, int* n);
/* What a correlation r of n pairs is worth when the two series have the lag-1 autocorrelations r1a, r1b (Bretherton et al.
 * 1999; Fisher z), M values each, r1a one value when r1a_len == 1:
 *   n_eff = n (1 - r1a r1b) / (1 + r1a r1b) clamped to [0, n];  z = atanh(r) sqrt(n_eff - 3);  p = erfc(|z| * 0.7071067811865476).
 * z and p are NaN when n_eff <= 3 or an input is NaN (an input that is NaN makes n_eff NaN too); |r| = 1 gives p = 0.  n_eff, z, p may each be
 * NULL, not all three.  Device only: atanh and erfc are the device library's. */
int gd_corr_signif(const double* r, const double* n, const double* r1a, long r1a_len, const double* r1b, long M, double* n_eff,
                   double* z, double* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ensemble verification (ensverify.hip, csrc/ensverify_core.h): is the spread of an ensemble the right size?  The
 * continuous ranked probability score, the rank (Talagrand) histogram, the spread against the error of the ensemble mean
 * and the coverage of the +-k sigma intervals, of the members in the slab of evaluate_ensemble against the truth of the
 * same batch, without a copy of any prediction to the host.
 * x: M member arrays (1 <= M <= GD_ENSV_MAX_M) of n = planes * hw elements, member_stride elements apart (>= n when M > 1);
 * y: the truth, n elements; storage fp32, or fp64 with GD_ENSV_F64.  mask: NULL or hw bytes shared by all planes, nonzero =
 * valid.  An element is VALID when the mask allows it, the truth is not NaN and no member is NaN (an input that holds an
 * infinity has unspecified outputs).  All arithmetic fp64, every operation rounded on its own.  Per valid element, with
 * d_i = (double)x_i - (double)y sorted ascending to d_(0) <= ... <= d_(M-1) and every sum taken in that order from +0.0:
 *   less = #{d_i < 0}, ties = #{d_i == 0};  rank bin = less + ties / 2 (integer division): 0 .. M;
 *   e    = (sum d_(i)) / M, the error of the ensemble mean;  s^2 = sum (d_(i) - e)^2 / (M - 1), 0 at M = 1;  s = sqrt(s^2);
 *   A    = (sum |d_(i)|) / M;  G = sum (2 i - M + 1) d_(i), which is sum over i < j of |x_i - x_j|;
 *   crps = A - G / M^2, and A - G / (M (M - 1)) under GD_ENSV_FAIR (refused at M = 1);
 *   crps_gauss = s (z erf(z / sqrt 2) + 2 phi(z) - 1 / sqrt pi), z = -e / s, phi the normal density; |e| where s = 0:
 *          the CRPS of the normal distribution N(mean, s^2) that a mean map and a std map stand for;
 *   cover_k = |e| <= z_k s for z_k = 0.674489750196082, 1, 1.644853626951472, 1.959963984540054: the nominal levels
 *          0.5, 0.6826894921370859, 0.9, 0.95.
 * The affine v a + b of a scaler's inverse acts on differences as `scale` = a > 0 alone; it is applied last: crps,
 * crps_gauss, e and s are multiplied by scale (s^2 by scale^2).
 * Maps (each may be NULL; n elements; every element is written): crps_map, err_map (e), spread_map (s) in the input
 * dtype, rounded once, NaN at an invalid element; rank_map uint8, 255 at an invalid element.
 * rec: GD_ENSV_REC doubles on the device, the sums over the valid elements:
 *   [GD_ENSV_N] n   [GD_ENSV_TIED] elements with ties > 0   [GD_ENSV_CRPS] sum crps   [GD_ENSV_CRPS_GAUSS] sum crps_gauss
 *   [GD_ENSV_ABS_E] sum |e|   [GD_ENSV_E2] sum e^2   [GD_ENSV_S2] sum s^2   [GD_ENSV_COVER + k] the four coverage counts
 *   [GD_ENSV_HIST + b] the rank histogram, b = 0 .. M (GD_ENSV_BINS slots; those behind M stay 0).
 * Counts are exact integers (below 2^53).  A zero record is neutral and records add, so they travel between batches and
 * ranks like those of gd_eval_stats.
 * Reduction: a workgroup of 256 threads, one element per lane and trip over the grid gd_ensv_grid(planes, hw) of
 * ensverify_core.h (at most 1024 workgroups; without a mask the array is one plane); float sums in registers, then a fixed
 * tree per wave, the waves ascending, one partial record per workgroup in ws (gd_ens_verify_ws_bytes), and one wave that
 * adds the partials in ascending order.  Counts by integer adds in LDS.  No global atomics, no float atomics: bitwise
 * reproducible.  gd_ens_verify_host is plain C++ over the same core without a GPU; it walks the same grid in the same
 * order, so every map and every record field equals the device's bit for bit, except [GD_ENSV_CRPS_GAUSS] (erf and exp
 * are each side's library), which agrees to the rounding of those two functions.
 * gd_ens_verify_merge_host (host only): adds k records (k x GD_ENSV_REC doubles) in the given order into rec_out (may be
 * NULL) and derives metrics[GD_ENSV_METRICS]: crps, crps_gauss, mae = sum |e| / n, rmse = sqrt(sum e^2 / n), spread =
 * sqrt(sum s^2 / n), spread_skill = sqrt((M + 1) / M) spread / rmse (1 for a statistically consistent ensemble; NaN at
 * M = 1 or rmse = 0), the four coverage fractions, reliability = sum over b <= M of |hist_b / n - 1 / (M + 1)|, tied =
 * the share of elements with a tie, and the histogram as fractions.  n = 0 (or k = 0): every metric is NaN.
 * ---------------------------------------------------------------------------------------- */
#define GD_ENSV_MAX_M 32
enum { GD_ENSV_F64 = 1, GD_ENSV_FAIR = 2 };
enum { GD_ENSV_N = 0, GD_ENSV_TIED = 1, GD_ENSV_CRPS = 2, GD_ENSV_CRPS_GAUSS = 3, GD_ENSV_ABS_E = 4, GD_ENSV_E2 = 5, GD_ENSV_S2 = 6,
       GD_ENSV_COVER = 7, GD_ENSV_HIST = 11, GD_ENSV_BINS = 33, GD_ENSV_REC = 44 };
enum { GD_ENSV_M_CRPS = 0, GD_ENSV_M_CRPS_GAUSS = 1, GD_ENSV_M_MAE = 2, GD_ENSV_M_RMSE = 3, GD_ENSV_M_SPREAD = 4,
       GD_ENSV_M_SPREAD_SKILL = 5, GD_ENSV_M_COVER = 6, GD_ENSV_M_RELIABILITY = 10, GD_ENSV_M_TIED = 11, GD_ENSV_M_HIST = 12,
       GD_ENSV_METRICS = 45 };
size_t gd_ens_verify_ws_bytes(long n);
int gd_ens_verify(const void* x, int M, long member_stride, const void* y, long planes, long hw, const unsigned char* mask,
                  double scale, int flags, double* rec, void* crps_map, void* err_map, void* spread_map, unsigned char* rank_map,
                  void* ws, size_t ws_bytes, void* stream);
int gd_ens_verify_host(const void* x, int M, long member_stride, const void* y, long planes, long hw, const unsigned char* mask,
                       double scale, int flags, double* rec, void* crps_map, void* err_map, void* spread_map,
                       unsigned char* rank_map);
int gd_ens_verify_merge_host(const double* recs, long k, int M, double* rec_out, double* metrics);

/* ------------------------------------------------------------------------------------------
 * EOF analysis (eof.hip, csrc/eof_core.h): the pieces of an empirical-orthogonal-function / principal-component analysis
 * of a (T, M) cube whose time axis is short (T <= GD_EOF_MAX_T) and whose space axis is long: validity and mean of every
 * series, the T x T Gram matrix of the weighted anomalies, the projection of every series on K coefficient columns (EOFs,
 * covariance maps) and the rank-K reconstruction.  The eigen-decomposition of the Gram matrix is the caller's (256 x 256
 * doubles at most; gan_danet_amd/eof.py uses numpy.linalg.eigh).
 * The layout is that of "Per-pixel time series": series m of a dense (T, M) array at x[t * M + m], storage fp32 (dtype 0)
 * or fp64 (dtype 1), all arithmetic fp64.  mean: M doubles; valid: M bytes; weight: NULL or M doubles >= 0 (an area
 * weight, for instance cos(lat)).  The WEIGHTED ANOMALY is
 *   a[t, m] = sqrt(weight[m]) * ((double)x[t, m] - mean[m])   for valid m,   exactly 0 for invalid m
 * (a select: the samples of an invalid series may be NaN).  The caller owns all memory, nothing is allocated, nothing waits
 * for the device, no atomics: every result is bitwise reproducible.  Every entry has a host twin (`_host`, no GPU call,
 * every pointer in HOST memory); prepare, project and reconstruct run the same operations in the same order on both sides
 * (eof_core.h, every operation rounded on its own) and agree bit for bit.
 * ---------------------------------------------------------------------------------------- */
#define GD_EOF_MAX_T 256 /* time steps of gd_eof_gram: 16 blocks of 16 rows, 136 blocks on and above the diagonal */
#define GD_EOF_MAX_K 16  /* coefficient columns of one gd_eof_project / gd_eof_reconstruct call: K register accumulators */
/* valid[m] = 1 iff the mask byte is nonzero (or mask is NULL), every sample of the series is finite, and the weight is
 * finite and > 0 (or weight is NULL): a series with a gap is left out whole, the missing set of an EOF analysis is fixed
 * in time.  mean[m] = (x[0, m] + x[1, m] + ... in ascending t, from +0.0) / T when center, else 0; 0 for an invalid
 * series.  One thread per series. */
int gd_eof_prepare(const void* x, int dtype, long T, long M, const unsigned char* mask, const double* weight, int center,
                   double* mean, unsigned char* valid, void* stream);
int gd_eof_prepare_host(const void* x, int dtype, long T, long M, const unsigned char* mask, const double* weight, int center,
                        double* mean, unsigned char* valid);
/* G (T, T) doubles: G[t, s] = sum over m of a[t, m] a[s, m]; no division.  2 <= T <= GD_EOF_MAX_T.
 * On v_mfma_f64_16x16x4_f64: T is padded to 16 nb rows; a workgroup of 8 waves stages the anomalies of 32 series for all
 * rows in LDS (fp64, rows 34 doubles apart so that the fragment reads are free of bank conflicts; padded rows, invalid
 * series and series beyond M are zeros) and accumulates the nb (nb + 1) / 2 blocks of 16 x 16 on and above the diagonal,
 * each wave a fixed contiguous run of them, a row fragment read once per 4 series and used by every block of the wave
 * that touches its row block.  The series are split over at most 256 workgroups in runs of 32-series chunks (at least 8
 * chunks per split; csrc/eof_core.h gd_eof_geom, a function of (T, M) alone); each writes one partial slab into ws
 * (gd_eof_gram_ws_bytes), and a second launch adds the slabs in ascending order and writes both triangles from the
 * upper one: G is exactly symmetric and two runs give the same bits.
 * The host twin adds over m in ascending order and is NOT bit-equal to the device; with n valid series both satisfy
 *   |G^[t, s] - G[t, s]| <= (n + 3) 2^-53 sum_m |a[t, m]| |a[s, m]|   (for any order of the sum).
 * gd_eof_gram_ws_bytes is 0 for a shape that gd_eof_gram refuses. */
size_t gd_eof_gram_ws_bytes(long T, long M);
int gd_eof_gram(const void* x, int dtype, long T, long M, const double* mean, const unsigned char* valid, const double* weight,
                double* G, void* ws, size_t ws_bytes, void* stream);
int gd_eof_gram_host(const void* x, int dtype, long T, long M, const double* mean, const unsigned char* valid,
                     const double* weight, double* G);
/* coef (T, K) doubles, row t at coef[t * K]; out (K, M) doubles, planar:
 *   out[k, m] = s_m * sum over t (ascending, from +0.0) of coef[t, k] * ((double)x[t, m] - mean[m]),
 * s_m = sqrt(weight[m]) with use_weight (weight must be given), else 1; NaN for an invalid series.
 * 1 <= K <= GD_EOF_MAX_K.  One thread per series with K register accumulators; the rows of coef are uniform across lanes.
 * With coef = U Lambda^-1/2 (eigenvectors and eigenvalues of G) and use_weight these are the EOFs, of unit norm in the
 * weighted space; with the standardised PCs divided by (T - ddof) and use_weight = 0, the covariance maps. */
int gd_eof_project(const void* x, int dtype, long T, long M, const double* mean, const unsigned char* valid, const double* weight,
                   int use_weight, const double* coef, int K, double* out, void* stream);
int gd_eof_project_host(const void* x, int dtype, long T, long M, const double* mean, const unsigned char* valid,
                        const double* weight, int use_weight, const double* coef, int K, double* out);
/* eofs (K, M) doubles planar, pcs (T, K) doubles; out (T, M) in out_dtype (fp32 0 / fp64 1):
 *   out[t, m] = mean[m] + (sum over k (ascending, from +0.0) of pcs[t, k] * eofs[k, m]) / sqrt(weight[m])
 * (no division when weight is NULL), rounded once to out_dtype; NaN for an invalid series.  1 <= K <= GD_EOF_MAX_K. */
int gd_eof_reconstruct(const double* eofs, const double* pcs, const double* mean, const unsigned char* valid, const double* weight,
                       long T, long M, int K, void* out, int out_dtype, void* stream);
int gd_eof_reconstruct_host(const double* eofs, const double* pcs, const double* mean, const unsigned char* valid,
                            const double* weight, long T, long M, int K, void* out, int out_dtype);

/* ------------------------------------------------------------------------------------------
 * Spatial spectra (spectra.hip, csrc/spectra_core.h): the radially binned spatial power spectrum of every field of a
 * (T, H, W) cube, and the co- and quadrature spectra of two such cubes, by a 2-D DFT written as matrix products on
 * v_mfma_f64_16x16x4_f64.  Storage fp32 (dtype 0) or fp64 (dtype 1), all arithmetic fp64.  No spectrum is stored (unless
 * p2d is asked for), no N x N twiddle matrix, no atomics: the same input gives the same bits, and the result of field t
 * depends on neither T nor the other fields.  The caller owns all memory, nothing waits for the device.  Every device
 * entry has a host twin (`_host`, every pointer in HOST memory): plain O(H W (H + W)) loops over spectra_core.h, a
 * separable two-stage sum over the same tables; twin and device differ in the order of their sums only.
 *
 * DEFINITIONS, for a field x (H, W); mask: NULL or H * W bytes shared by all fields; pixel (i, j) is VALID iff x is finite
 * and its mask byte is nonzero.
 *  1. detrend over the valid pixels: 0 none; 1 mean; 2 the least-squares plane.  With the centred coordinates
 *     u = i - (H - 1) / 2, v = j - (W - 1) / 2 the three coefficients (a, b, c) describe a + b u + c v (a is the plane at
 *     the field's centre; mean: b = c = 0; none: all 0).  A fit that does not determine a slope (one row, one column, a
 *     line of pixels) leaves that slope 0.
 *  2. taper: x'[i, j] = (x - (a + b u + c v)) * wy[i] * wx[j] for a valid pixel, exactly 0 for an invalid one.  wy (H) and
 *     wx (W) doubles, NULL = all ones.
 *  3. transform: Z[ky, kx] = sum_i sum_j x'[i, j] exp(-2 pi i (ky i / H + kx j / W)), ky = 0 .. H - 1, kx = 0 .. Kx - 1,
 *     Kx = W / 2 + 1.  Hermitian weight of column kx: 1 for kx = 0 and for kx = W / 2 with W even, else 2.
 *  4. normalise: P[ky, kx] = weight |Z|^2 / (H W S), S = sum over valid pixels of wy^2 wx^2.  PARSEVAL: the sum of P over
 *     all (ky, kx) is sum x'^2 / S, the windowed variance of the valid pixels.
 *  5. bin: an int32 table bin[ky * Kx + kx] in [-1, nbins), -1 = dropped.  power[b] is the sum of P over bin b; the power
 *     of the dropped wavenumbers is returned apart, so Parseval stays checkable.
 * A field with no valid pixel has S = 0, count 0, and NaN power.
 * ---------------------------------------------------------------------------------------- */
#define GD_SPEC_MAX_H 1024
#define GD_SPEC_MAX_W 2048
#define GD_SPEC_MAX_BINS 1024
/* tw: 2 N doubles, cos(2 pi r / N) for r = 0 .. N - 1, then sin.  The angle is reduced to k pi / 2 +- phi with
 * 0 <= phi <= pi / 4 in integers, cos phi and sin phi are evaluated in extended precision and rounded once: every entry
 * is within 1 ulp, and the entries at r = 0, N / 4, N / 2, 3 N / 4 are exactly 0 and +-1.  The kernels index the table by
 * (i k) mod N in integer arithmetic.  1 <= N <= GD_SPEC_MAX_W. */
int gd_spec_twiddle_host(long N, double* tw);
/* The bin table.  With P = H dy and Q = W dx (the fp64 products), L = max(P, Q) and ky' = ky folded to (-H / 2, H / 2]:
 *   k = hypot(ky' / P, kx / Q),   bin = floor(k L)   (uniform bins of width 1 / L),
 * -1 when bin >= nbins, or when kmax > 0 and k > kmax (1 + 2^-40).  The comparison of (k L)^2 with the squared edges is
 * made in integers whenever P / Q is a ratio of integers below 2^20 (equal domains, or dy = dx), else in extended
 * precision (floor(sqrt(q)) in long double; exact unless q lies within 2^-63 of a squared edge).
 * kcentre[b] = (b + 1/2) / L, count[b] = entries of the table equal to b.
 * gd_spec_default_bins: floor(min(1 / (2 dy), 1 / (2 dx)) L) + 1, at most GD_SPEC_MAX_BINS (with kmax = that Nyquist
 * wavenumber the bins run up to the smaller Nyquist wavenumber); 0 for bad arguments. */
int gd_spec_default_bins(long H, long W, double dy, double dx);
int gd_spec_bins_host(long H, long W, double dy, double dx, int nbins, double kmax, int* bin, double* kcentre, long* count);
/* coef: 3 T doubles (a, b, c per field); S: 2 T doubles (S and the count of valid pixels per field).  One workgroup per
 * field, every sum an ordered block reduction, the 3 x 3 solve (about the means) on the device; no host sync. */
int gd_spec_prepare(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy, const double* wx,
                    int detrend, double* coef, double* S, void* stream);
int gd_spec_prepare_host(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy,
                         const double* wx, int detrend, double* coef, double* S);
/* power: T x nbins doubles; dropped: T doubles; p2d: NULL or T x H x Kx doubles, the un-binned P (for tests and 2-D plots).
 * twid_h, twid_w: gd_spec_twiddle_host(H), (W) on the device; bin: the table above on the device.
 * A workgroup of 4 waves owns one field and a tile of 8 kx = 16 real columns (Re, Im).  Stage 1, Y = x' [C_W | -S_W]:
 * x' is built at the load and staged in LDS in chunks of 64 rows x 32 columns; the H x 16 result stays in LDS as fp64.
 * Stage 2: per 16 ky two MFMAs per 4 rows of Y (cos and sin of the LDS copy of the H table) leave Re Z and Im Z in the
 * accumulator; |Z|^2 is taken in registers, goes to an LDS tile of 64 ky x 8 kx, and thread t adds the entries whose bin
 * is t (mod 256) in ascending (ky, kx) to its own registers.  One slab [nbins + 1] per workgroup goes to ws; a second
 * launch adds the slabs of a field in ascending tile order and divides by H W S.  Rows and columns beyond H and W exist
 * as zeros in LDS only; every global read is clamped.
 * Refused: H or W < 1, H > GD_SPEC_MAX_H, W > GD_SPEC_MAX_W, T H W >= 2^31, nbins outside 1..GD_SPEC_MAX_BINS;
 * gd_spec_power_ws_bytes (T * ceil(Kx / 8) * (nbins + 1) doubles, a function of the shape alone) is 0 for them. */
size_t gd_spec_power_ws_bytes(long T, long H, long W, int nbins);
int gd_spec_power(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy, const double* wx,
                  const double* coef, const double* S, const double* twid_h, const double* twid_w, const int* bin, int nbins,
                  double* power, double* dropped, double* p2d, void* ws, size_t ws_bytes, void* stream);
int gd_spec_power_host(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy, const double* wx,
                       const double* coef, const double* S, const double* twid_h, const double* twid_w, const int* bin, int nbins,
                       double* power, double* dropped, double* p2d);
/* Two cubes of one shape, each with its own coefficients and S.  out: 4 x T x nbins doubles -- the bin sums of P_aa, P_bb,
 * weight Re(Z_a conj Z_b) / (H W sqrt(S_a S_b)) (co) and weight Im(Z_a conj Z_b) / (H W sqrt(S_a S_b)) (quad); dropped: T x 4
 * doubles, the same four sums over the dropped wavenumbers.  For xa == xb quad is exactly 0 and P_aa == P_bb bit for bit.
 * The kernel of gd_spec_power with tiles of 4 kx: the 16 real columns are (Re, Im) of a and of b.  NaN where either
 * field has no valid pixel.  gd_spec_cross_ws_bytes: T * ceil(Kx / 4) * 4 * (nbins + 1) doubles. */
size_t gd_spec_cross_ws_bytes(long T, long H, long W, int nbins);
int gd_spec_cross(const void* xa, const void* xb, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy,
                  const double* wx, const double* coef_a, const double* S_a, const double* coef_b, const double* S_b,
                  const double* twid_h, const double* twid_w, const int* bin, int nbins, double* out, double* dropped, void* ws,
                  size_t ws_bytes, void* stream);
int gd_spec_cross_host(const void* xa, const void* xb, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy,
                       const double* wx, const double* coef_a, const double* S_a, const double* coef_b, const double* S_b,
                       const double* twid_h, const double* twid_w, const int* bin, int nbins, double* out, double* dropped);

/* ------------------------------------------------------------------------------------------
 * Drought analysis (drought.hip, csrc/drought_core.h): where, when, how long and how severe were the droughts of a TWSA
 * cube -- the calendar climatology of every pixel, the water storage deficit (Thomas et al. 2014) and the standardised
 * GRACE-DSI (Zhao et al. 2017) against it, a non-parametric rank index, the events of run theory with their maps, and the
 * indicator cube whose zonal means (gd_zone_mean) are drought-area series.
 * The layout is that of "Per-pixel time series": series m of a dense (T, M) array at x[t * M + m], storage fp32 (dtype 0)
 * or fp64 (dtype 1), 1 <= T <= GD_DROUGHT_MAX_T, all arithmetic fp64 with every operation rounded on its own.  mask: NULL,
 * or M bytes, 0 = leave the series out (NaN in its outputs, 0 in its counts).  One thread owns a series and walks it in
 * time order; no LDS, no atomics, no workspace, nothing allocated; a series' result depends on the series and the
 * parameters alone.  Every *_host twin takes the same arguments in HOST memory, makes no GPU call, runs the same
 * per-series code (csrc/drought_core.h) and agrees bit for bit.  Every argument is checked before any launch.
 *
 * Calendar: step t belongs to slot s = (t + phase) mod period, 1 <= period <= GD_DROUGHT_MAX_PERIOD, 0 <= phase < period.
 * Baseline: the steps [b0, b1), 0 <= b0 < b1 <= T.
 *
 * gd_drought_clim: clim (3, period, M) doubles -- n, mean, M2 (the sum of squared deviations from the mean) of slot s of
 * series m at clim[(j * period + s) * M + m], j = 0, 1, 2 -- over the baseline steps of the slot that are not NaN, in time
 * order, by the recurrence of gd_series_push: d = v - mean, mean += d * (1 / (n + 1)), M2 += d * d * (n * (1 / (n + 1))),
 * d against the mean before the sample.  A slot without a sample has n = 0 and NaN mean and M2.  The slots are walked in
 * an outer loop (t = first(s); t += period): three accumulators in registers, every baseline element read once.
 *
 * gd_drought_index: out (T, M) in the dtype of x, rounded once.  GD_DROUGHT_ANOMALY: x - mean_s.  GD_DROUGHT_STANDARDIZED:
 * (x - mean_s) / sqrt(M2_s / (n_s - ddof)), ddof 0 or 1; NaN where n_s - ddof <= 0 or M2_s == 0.  A NaN sample or an empty
 * slot gives NaN.
 *
 * gd_drought_rank: for the sample v = x[t] of slot s let B be the baseline samples of the slot that are not NaN, and v
 * itself when t lies outside the baseline; n = |B|, k = 2 #{b in B: b < v} + #{b in B: b == v}, so the midrank of v in B is
 * (k + 1) / 2 and 1 <= k <= 2 n - 1.  out[t] = table[(n - 1)^2 + (k - 1)] rounded to the dtype of x; NaN for a NaN sample.
 * table: nmax^2 doubles built by the caller (a plotting position, or its normal quantile for an SPI-style index), nmax <=
 * GD_DROUGHT_MAX_N; refused where ceil((b1 - b0) / period) + 1 > nmax.  Nothing transcendental runs on the device.  The
 * O(n^2) comparisons of a slot are one thread's; the baseline samples are re-read from cache for every sample.
 *
 * gd_drought_events: a step is dry when v <= threshold (never for NaN, which ends a run).  An event is a maximal run of
 * consecutive dry steps of length >= min_duration (>= 1); its severity is the sum of (threshold - v) over its steps in time
 * order.  maps: the planes selected by the bits of `which` (bit k = map k below), in ascending k, map j of series m at
 * maps[j * M + m]:
 *   n_valid, n_dry: the steps that are not NaN / that are dry;  n_events;  event_steps: the steps inside events;
 *   max_duration;  mean_duration = event_steps / n_events, NaN without events;
 *   max_severity, total_severity (the events' severities added in time order), both 0 without events;
 *   peak: the smallest v inside events, NaN without events;
 *   longest_start, worst_start: the first step of the first longest event / of the first event of largest severity, -1
 *   without events;  last_run: the length of the run still open at step T - 1, whatever min_duration is, 0 if none.
 * A masked series has 0 in n_valid, n_dry, n_events, event_steps, max_duration and last_run and NaN elsewhere.
 * in_event: NULL, or (T, M) bytes, all written: 1 on the steps of events, else 0 (a thread writes 0 as it goes and
 * back-fills its own column when a run qualifies).
 *
 * gd_drought_exceed: out[i] = 1 where index[i] <= threshold, 0 where not, NaN where index[i] is NaN, n elements in the
 * dtype of the input: the cube whose gd_zone_mean is the (weighted) share of a zone's valid pixels in drought.
 * ---------------------------------------------------------------------------------------- */
#define GD_DROUGHT_MAX_T 2048
#define GD_DROUGHT_MAX_PERIOD 366
#define GD_DROUGHT_MAX_N 257
enum { GD_DROUGHT_ANOMALY = 0, GD_DROUGHT_STANDARDIZED = 1 };
enum { GD_DROUGHT_EV_N_VALID = 0, GD_DROUGHT_EV_N_DRY = 1, GD_DROUGHT_EV_N_EVENTS = 2, GD_DROUGHT_EV_EVENT_STEPS = 3,
       GD_DROUGHT_EV_MAX_DURATION = 4, GD_DROUGHT_EV_MEAN_DURATION = 5, GD_DROUGHT_EV_MAX_SEVERITY = 6,
       GD_DROUGHT_EV_TOTAL_SEVERITY = 7, GD_DROUGHT_EV_PEAK = 8, GD_DROUGHT_EV_LONGEST_START = 9,
       GD_DROUGHT_EV_WORST_START = 10, GD_DROUGHT_EV_LAST_RUN = 11, GD_DROUGHT_EV_MAPS = 12 };
int gd_drought_clim(const void* x, int dtype, long T, long M, int period, int phase, long b0, long b1,
                    const unsigned char* mask, double* clim, void* stream);
int gd_drought_clim_host(const void* x, int dtype, long T, long M, int period, int phase, long b0, long b1,
                         const unsigned char* mask, double* clim);
int gd_drought_index(const void* x, int dtype, long T, long M, const double* clim, int period, int phase, int kind, int ddof,
                     const unsigned char* mask, void* out, void* stream);
int gd_drought_index_host(const void* x, int dtype, long T, long M, const double* clim, int period, int phase, int kind,
                          int ddof, const unsigned char* mask, void* out);
int gd_drought_rank(const void* x, int dtype, long T, long M, int period, int phase, long b0, long b1,
                    const unsigned char* mask, const double* table, int nmax, void* out, void* stream);
int gd_drought_rank_host(const void* x, int dtype, long T, long M, int period, int phase, long b0, long b1,
                         const unsigned char* mask, const double* table, int nmax, void* out);
int gd_drought_events(const void* index, int dtype, long T, long M, double threshold, int min_duration, int which,
                      const unsigned char* mask, double* maps, unsigned char* in_event, void* stream);
int gd_drought_events_host(const void* index, int dtype, long T, long M, double threshold, int min_duration, int which,
                           const unsigned char* mask, double* maps, unsigned char* in_event);
int gd_drought_exceed(const void* index, int dtype, long n, double threshold, void* out, void* stream);
int gd_drought_exceed_host(const void* index, int dtype, long n, double threshold, void* out);

/* ------------------------------------------------------------------------------------------
 * Connected components (ccl.hip, csrc/ccl_core.h): which dry voxels of a (T, H, W) cube belong to the same drought --
 * 3-D connected-component labelling, a size filter, canonical labels, and per cluster its bounding box, its track (one
 * record per step of its life) and its totals.  The cube stays on the device; two integers cross to the host, the number
 * of clusters K (to size the tables) and the number of track records R.
 * Voxel (t, h, w) of the dense cube has raster index i = (t H + h) W + w; N = T H W < 2^31; indices and labels are int32.
 * Foreground: x fp32 (dtype 0) or fp64 (dtype 1): x[i] <= threshold (never for NaN) and, with mask (H W bytes, NULL = all),
 * mask[h W + w] != 0; x uint8 (dtype GD_CCL_U8, for instance the in_event cube of gd_drought_events): x[i] != 0 (the
 * threshold is not read).
 * Neighbourhood: any symmetric 3 x 3 x 3 structure with its centre set, as the word `structure` of its 13 backward
 * offsets: bit k, 0 <= k < 13, links (t, h, w) with (t + k / 9 - 1, h + k / 3 % 3 - 1, w + k % 3 - 1), the offsets that
 * come before the centre in raster order (the forward half follows by symmetry).  0 links nothing.
 * Every *_host twin takes the same arguments in HOST memory (no workspace, no stream), makes no GPU call and gives the
 * same bits.  Every argument is checked before any launch (-1 and gd_last_error).  No float atomics anywhere: the integer
 * outputs do not depend on the order the atomics land in, and the fp64 sums have the fixed order of csrc/ccl_core.h.
 *
 * gd_ccl_label: parent (N) int32 = the smallest raster index of the voxel's component, -1 on background.  Three kernels:
 * union-find inside tiles of GD_CCL_TILE_T x _H x _W voxels in LDS, unions across tile faces, edges and corners in global
 * memory, a flattening pass.  parent[i] <= i always holds and a parent is only lowered, by atomic min; no thread waits for
 * another (the argument is at the top of csrc/ccl_core.h).  flags GD_CCL_NO_TILES skips the LDS stage (every union in
 * global memory): the same output, kept for comparison.
 * gd_ccl_filter: components of fewer than min_size (>= 1) voxels become background, in place.  ws: gd_ccl_ws_bytes(N).
 * gd_ccl_relabel: labels (N) int32, 0 on background and 1 .. K in raster order of each component's first voxel (the
 * numbering of scipy.ndimage.label); *count = K (device memory; host memory for the twin).  The roots are flagged and
 * scanned by a plain three-pass exclusive prefix sum.  labels may be parent itself.  ws: gd_ccl_ws_bytes(N).
 * gd_ccl_bounds: bounds (K, GD_CCL_BOUNDS) int32: n, t0, t1, h0, h1, w0, w1 (inclusive) of label k + 1 at row k.
 * gd_ccl_offsets: offsets (K + 1) int32, the exclusive prefix sum of the durations t1 - t0 + 1; offsets[K] = R.
 * ws: gd_ccl_ws_bytes(K).
 * gd_ccl_tracks: tracks (R, GD_CCL_TRACK) doubles, record offsets[k] + (t - t0) for cluster k at step t: the pixel count,
 * the area sum a, the severity sum a (threshold - x), sum a h, sum a w, and the smallest x; a = weights[h W + w] (H W
 * doubles) or 1 with NULL.  index (R, 2) int32: k and t of every record.  One workgroup per record walks the bounding
 * box of the cluster in that plane.  flags GD_CCL_SEVERITY asks for severity and minimum and needs an fp32 / fp64 x (with
 * uint8 it is refused); without it x may be NULL and both are NaN.
 * gd_ccl_totals: totals (K, GD_CCL_TOTALS) doubles from the records in ascending t: the volume sum_t area, the severity,
 * the largest area and its (first) step, the smallest x, and the area-weighted centroid (t, h, w).
 * ---------------------------------------------------------------------------------------- */
#define GD_CCL_TILE_T 4
#define GD_CCL_TILE_H 8
#define GD_CCL_TILE_W 32
#define GD_CCL_U8 2
#define GD_CCL_STRUCT_BITS 13
enum { GD_CCL_NO_TILES = 1 };   /* flags of gd_ccl_label */
enum { GD_CCL_SEVERITY = 1 };   /* flags of gd_ccl_tracks */
enum { GD_CCL_B_N = 0, GD_CCL_B_T0 = 1, GD_CCL_B_T1 = 2, GD_CCL_B_H0 = 3, GD_CCL_B_H1 = 4, GD_CCL_B_W0 = 5, GD_CCL_B_W1 = 6,
       GD_CCL_BOUNDS = 7 };
enum { GD_CCL_TR_COUNT = 0, GD_CCL_TR_AREA = 1, GD_CCL_TR_SEVERITY = 2, GD_CCL_TR_SUM_H = 3, GD_CCL_TR_SUM_W = 4, GD_CCL_TR_MIN = 5,
       GD_CCL_TRACK = 6 };
enum { GD_CCL_TO_VOLUME = 0, GD_CCL_TO_SEVERITY = 1, GD_CCL_TO_PEAK_AREA = 2, GD_CCL_TO_PEAK_AREA_STEP = 3, GD_CCL_TO_PEAK = 4,
       GD_CCL_TO_CENTROID_T = 5, GD_CCL_TO_CENTROID_H = 6, GD_CCL_TO_CENTROID_W = 7, GD_CCL_TOTALS = 8 };
size_t gd_ccl_ws_bytes(long n);
int gd_ccl_label(const void* x, int dtype, long T, long H, long W, double threshold, const unsigned char* mask, int structure,
                 int flags, int* parent, void* stream);
int gd_ccl_label_host(const void* x, int dtype, long T, long H, long W, double threshold, const unsigned char* mask, int structure,
                      int flags, int* parent);
int gd_ccl_filter(int* parent, long n, int min_size, void* ws, size_t ws_bytes, void* stream);
int gd_ccl_filter_host(int* parent, long n, int min_size);
int gd_ccl_relabel(const int* parent, long n, int* labels, int* count, void* ws, size_t ws_bytes, void* stream);
int gd_ccl_relabel_host(const int* parent, long n, int* labels, int* count);
int gd_ccl_bounds(const int* labels, long T, long H, long W, int K, int* bounds, void* stream);
int gd_ccl_bounds_host(const int* labels, long T, long H, long W, int K, int* bounds);
int gd_ccl_offsets(const int* bounds, int K, int* offsets, void* ws, size_t ws_bytes, void* stream);
int gd_ccl_offsets_host(const int* bounds, int K, int* offsets);
int gd_ccl_tracks(const void* x, int dtype, long T, long H, long W, double threshold, const int* labels, const int* bounds,
                  const int* offsets, int K, long R, const double* weights, int flags, double* tracks, int* index, void* stream);
int gd_ccl_tracks_host(const void* x, int dtype, long T, long H, long W, double threshold, const int* labels, const int* bounds,
                       const int* offsets, int K, long R, const double* weights, int flags, double* tracks, int* index);
int gd_ccl_totals(const double* tracks, const int* bounds, const int* offsets, int K, double* totals, void* stream);
int gd_ccl_totals_host(const double* tracks, const int* bounds, const int* offsets, int K, double* totals);

/* ------------------------------------------------------------------------------------------
 * Neighbourhood verification (neighborhood.hip, csrc/neighborhood_core.h): at which spatial scale does a forecast field put
 * its events where the observed field puts them -- the fractions skill score (FSS) of Roberts & Lean 2008 over K thresholds
 * and S window widths, and the neighbourhood fraction field of one cube.
 * f (forecast) and o (observed): dense (T, H, W) cubes of ONE dtype, fp32 (0) or fp64 (1), on one grid; H W <= GD_NBR_MAX_HW,
 * T H W < 2^31.  mask: NULL, or H W bytes, 0 = the pixel is not used.  thr_f, thr_o: (T, K) doubles in HOST memory (also for
 * the device entry: they are checked for NaN before any launch and travel as kernel arguments), the thresholds of step t;
 * 1 <= K <= GD_NBR_MAX_K.  scales: S odd window widths n >= 1 in HOST memory, 1 <= S <= GD_NBR_MAX_S; a window wider than
 * the domain is the whole domain.  below 1: the event is x <= thr; below 0: x >= thr; compared in fp64, never for NaN.
 *
 * Pixel (t, i, j) is valid when the mask is nonzero there and neither f nor o is NaN.  I_f = valid && event(f), I_o = valid
 * && event(o).  For n = 2 h + 1, cf, co, cv at (i, j) are the sums of I_f, I_o, valid over rows i - h .. i + h and columns
 * j - h .. j + h; positions outside the domain count zero.  Per (t, k, s), over the VALID centre pixels:
 *   GD_NBR_WINDOW: sums = A, B, C = sum (cf - co)^2, sum cf^2, sum co^2 as unsigned 64-bit integers (the n^4 of the fractions
 *   c / n^2 cancels in FSS = 1 - A / (B + C)); exact, whatever the order.
 *   GD_NBR_VALID: fractions cf / cv and co / cv in fp64; sums = the fp64 sums of (pf - po)^2, pf^2, po^2 in the fixed order
 *   of csrc/neighborhood_core.h, every operation rounded on its own.
 * sums: (T, K, S, 3) 8-byte words of that kind.  base: (T, K, 3) unsigned 64-bit: sum I_f, sum I_o, the number of valid
 * pixels.  maps: NULL, or (K, S, H, W, 3) words: the same three sums per centre pixel over time; a pixel is one thread's,
 * the steps are added in ascending t.  No atomics anywhere.
 *
 * Method: per step and threshold one summed-area table of (H + 1) x (W + 1) 64-bit words with a zero leading row and column;
 * a word packs the three counts in 21-bit fields (each is at most 2^20), so a window is four 8-byte loads.  Rows are scanned
 * by a wave (cross-lane scan, a carry between 64-lane segments), columns by one thread each; then every workgroup of the
 * score kernel takes all scales of its centre pixels, one partial per workgroup and scale, added in ascending order.
 * ws: gd_nbr_ws_bytes(H, W, K, planes) bytes hold the tables and partials of `planes` steps in flight (0 for arguments
 * outside the limits); the entry walks T in chunks of as many steps as ws_bytes holds, at least one, and the result does
 * not depend on it.  gd_nbr_fraction builds tables of K = 1: gd_nbr_ws_bytes(H, W, 1, planes).
 *
 * gd_nbr_fraction: out (T, H, W) doubles, cf / n^2 (GD_NBR_WINDOW; n^2 formed in fp64, exact for n < 2^26) or cf / cv
 * (GD_NBR_VALID) of the one cube x at width `scale`; NaN at an invalid centre.  thr: T doubles in HOST memory.
 * Every *_host twin takes the same arguments with the cubes and outputs in HOST memory (no workspace, no stream), makes no
 * GPU call, runs the same per-pixel code and gives the same bits.  Every argument is checked before any launch (-1 and
 * gd_last_error).
 * ---------------------------------------------------------------------------------------- */
#define GD_NBR_MAX_HW 1048576
#define GD_NBR_MAX_K 8
#define GD_NBR_MAX_S 32
enum { GD_NBR_WINDOW = 0, GD_NBR_VALID = 1 };   /* normalize */
size_t gd_nbr_ws_bytes(long H, long W, int K, long planes);
int gd_nbr_fss(const void* f, const void* o, int dtype, long T, long H, long W, const unsigned char* mask, const double* thr_f,
               const double* thr_o, int K, int below, const int* scales, int S, int normalize, void* sums, unsigned long long* base,
               void* maps, void* ws, size_t ws_bytes, void* stream);
int gd_nbr_fss_host(const void* f, const void* o, int dtype, long T, long H, long W, const unsigned char* mask, const double* thr_f,
                    const double* thr_o, int K, int below, const int* scales, int S, int normalize, void* sums, unsigned long long* base,
                    void* maps);
int gd_nbr_fraction(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* thr, int below, int scale,
                    int normalize, double* out, void* ws, size_t ws_bytes, void* stream);
int gd_nbr_fraction_host(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* thr, int below,
                         int scale, int normalize, double* out);

/* ------------------------------------------------------------------------------------------
 * Bias correction (quantmap.hip, csrc/quantmap_core.h): empirical quantile mapping per pixel and calendar slot, and its
 * trend-preserving form, quantile delta mapping (Cannon et al. 2015, additive).
 * x: a dense (T, M) cube, series m at x[t M + m], fp32 (dtype 0) or fp64 (dtype 1), 1 <= T <= GD_QM_MAX_T.  Step t belongs
 * to slot s = (t + phase) mod period, 1 <= period <= GD_QM_MAX_PERIOD, 0 <= phase < period.  All arithmetic fp64, every
 * operation rounded on its own (nothing is contracted into an FMA), nothing transcendental: the device entries, their
 * *_host twins and numpy agree bit for bit.
 *
 * gd_qm_quantiles: the sample of (s, m) is the steps b0 <= t < b1 of slot s at which x[t, m] is not NaN (and, where x2 is
 * given -- a second cube of the shape and dtype of x --, x2[t, m] is not NaN either); at most GD_QM_MAX_N steps per slot.
 * n (period, M) ints: its size (0 for a pixel with mask[m] == 0; mask NULL or M bytes).  quant: Q <= GD_QM_MAX_Q doubles per
 * (s, m), node j = numpy.nanquantile(sample, q[j]) with method "linear": v = (n - 1) q[j], i = floor(v), g = v - i, and
 * i = i + 1 = n - 1, g = v + 1 where v >= n - 1; with a, b the i-th and (i + 1)-th smallest, d = b - a, the node is
 * a + d g, or b - d (1 - g) where g >= 0.5 (numpy's _lerp).  NaN where n < max(min_samples, 1).  layout
 * GD_QM_LAYOUT_QSM: node j of (s, m) at quant[(j period + s) M + m]; GD_QM_LAYOUT_SQM: at quant[(s Q + j) M + m].
 * q: Q doubles in [0, 1], in DEVICE memory for the device entry (HOST memory for the twin).
 * The samples are ordered by value with -0.0 below +0.0, so the result is a function of the sample alone.  route:
 * GD_QM_ROUTE_AUTO takes the register route (one thread per (s, m), a sorting network over 16 or 32 registers) where no slot
 * has more than GD_QM_SMALL_N baseline steps and the LDS route (one wave per (s, m), bitonic sort) otherwise;
 * GD_QM_ROUTE_SMALL / GD_QM_ROUTE_LONG force one (SMALL is refused above GD_QM_SMALL_N steps per slot).  Both give the
 * same bits.  No workspace, no atomics.
 *
 * gd_qm_apply: x (T, Hx, Wx) with Hx = f H, Wx = f W, 1 <= f <= GD_QM_MAX_F; model_q and obs_q (period, Q, H, W) doubles
 * (GD_QM_LAYOUT_SQM), 2 <= Q <= GD_QM_MAX_Q.  Element (t, h, w) uses slot (t + phase) mod period of the tables of pixel
 * (h / f, w / f).  out (T, Hx, Wx) in the dtype of x, rounded once.  A NaN x or a NaN first node gives NaN.
 * GD_QM_EQM: inside [model_q[0], model_q[Q - 1]], numpy.interp(x, model_q, obs_q): j the last node with model_q[j] <= x;
 * obs_q[j] where j = Q - 1 or model_q[j] == x; else s = (obs_q[j+1] - obs_q[j]) / (model_q[j+1] - model_q[j]) and
 * s (x - model_q[j]) + obs_q[j].  Outside, with e the end node of that side: x + (obs_q[e] - model_q[e])
 * (GD_QM_CONSTANT) or obs_q[e] (GD_QM_CLIP).
 * GD_QM_QDM: own_q (period, Q, Hx, Wx) is the node table of x itself on its own grid (gd_qm_quantiles of x at the same
 * period and phase, q = p); p: the Q node probabilities j / (Q - 1), DEVICE memory (HOST for the twin);
 * tau = interp(x, own_q, p) and out = x + (interp(tau, p, obs_q) - interp(tau, p, model_q)).  own_q and p are not read
 * for GD_QM_EQM.
 * Every *_host twin takes the same arguments in HOST memory (no stream), makes no GPU call and runs the same per-sample
 * code.  Every argument is checked before any launch (-1 and gd_last_error).
 * ---------------------------------------------------------------------------------------- */
#define GD_QM_MAX_T 2048
#define GD_QM_MAX_N 2048
#define GD_QM_MAX_Q 256
#define GD_QM_MAX_PERIOD 366
#define GD_QM_MAX_F 16
#define GD_QM_SMALL_N 32
enum { GD_QM_LAYOUT_QSM = 0, GD_QM_LAYOUT_SQM = 1 };
enum { GD_QM_ROUTE_AUTO = 0, GD_QM_ROUTE_SMALL = 1, GD_QM_ROUTE_LONG = 2 };
enum { GD_QM_EQM = 0, GD_QM_QDM = 1 };
enum { GD_QM_CONSTANT = 0, GD_QM_CLIP = 1 };
int gd_qm_quantiles(const void* x, const void* x2, int dtype, long T, long M, const double* q, int Q, int period, int phase, long b0,
                    long b1, const unsigned char* mask, int min_samples, int layout, int route, double* quant, int* n, void* stream);
int gd_qm_quantiles_host(const void* x, const void* x2, int dtype, long T, long M, const double* q, int Q, int period, int phase,
                         long b0, long b1, const unsigned char* mask, int min_samples, int layout, int route, double* quant, int* n);
int gd_qm_apply(const void* x, int dtype, long T, long H, long W, int f, const double* model_q, const double* obs_q,
                const double* own_q, const double* p, int Q, int period, int phase, int kind, int extrapolate, void* out, void* stream);
int gd_qm_apply_host(const void* x, int dtype, long T, long H, long W, int f, const double* model_q, const double* obs_q,
                     const double* own_q, const double* p, int Q, int period, int phase, int kind, int extrapolate, void* out);

/* ------------------------------------------------------------------------------------------
 * Triple collocation (tcol.hip, csrc/tcol_core.h): how large is the random error of each of three collocated products when
 * none of them is the truth (Stoffelen 1998; covariance form and the squared correlation with the unknown truth of McColl
 * et al. 2014), per pixel, and a moving-block bootstrap over time that puts an interval on every statistic.
 * The layout is that of "Per-pixel time series": x, y, z are dense (T, M) arrays, series m at x[t * M + m], storage fp32
 * (dtype 0) or fp64 (dtype 1), one dtype for all three; all arithmetic fp64 with every operation rounded on its own (nothing
 * is contracted into an FMA).  1 <= T <= GD_TC_MAX_T.  The method assumes mutually independent errors; a seasonal cycle
 * shared by the three products must be removed by the caller.
 *   Deletion     a step counts for a pixel only if x, y and z are all not NaN there (listwise); n is their number.
 *   Centring     mx, my, mz: the means over the counted steps by the recurrence m += (v - m) * (1 / k) in time order (k the
 *                number of counted steps so far, this one included); u = x - mx, v = y - my, w = z - mz.
 *   Sums         Su, Sv, Sw, Suu, Svv, Sww, Suv, Suw, Svw over the counted steps in ascending order, each from +0.0.
 *   Covariances  Qab = (Sab - Sa * Sb / n) / (n - 1), evaluated as written, left to right.
 *   Statistics   GD_TC_STATS = 8 planes, in this order:
 *                  err_var_x = Qxx - Qxy * Qxz / Qyz   err_var_y = Qyy - Qxy * Qyz / Qxz   err_var_z = Qzz - Qxz * Qyz / Qxy
 *                  rho2_x = Qxy * Qxz / (Qxx * Qyz)    rho2_y = Qxy * Qyz / (Qyy * Qxz)    rho2_z = Qxz * Qyz / (Qzz * Qxy)
 *                  beta_y = Qyz / Qxz                  beta_z = Qyz / Qxy      (the scale of y and z against x; beta_x = 1)
 *   Validity     all eight are NaN when the pixel is masked out (mask[m] == 0; mask NULL or M bytes; such a pixel is not
 *                read and has n = 0), when n < min_samples (min_samples >= 3), or when any of Qxy, Qxz, Qyz is not > 0 (the
 *                products do not agree in sign: collocation is undefined).  A negative error variance or a rho2 > 1 is a
 *                legitimate sampling outcome: it is returned as it is and only flagged.
 *   flags        (M,) int32, one bit per GD_TC_FLAG_*: MASKED, FEW (n < min_samples), NONPOS (a cross-covariance not > 0),
 *                NEG_X, NEG_Y, NEG_Z (that error variance < 0), RHO2 (any rho2 > 1).
 * gd_tc_estimate: stats (GD_TC_STATS, M) doubles, planar; cov (6, M) doubles Qxx Qyy Qzz Qxy Qxz Qyz, or NULL: NaN where the
 * pixel is masked or n < min_samples, else the covariances (also where the statistics are undefined); n and flags (M,)
 * int32.  One thread per series, lanes along the pixels, two passes over the cubes (means, then sums).
 *
 * gd_tc_bootstrap: idx is a (T, B) table of uint16 step numbers, idx[t * B + b] in 0 .. T - 1, in DEVICE memory, shared by all
 * pixels (every pixel is resampled at the same times); 1 <= B <= GD_TC_MAX_B.  Replicate b of a pixel takes the steps
 * idx[0, b], idx[1, b], .., idx[T - 1, b] in that order through the same deletion, the same nine sums and the same eight
 * formulas; u, v, w are centred with the means of the ORIGINAL series (the covariance form is shift invariant, the centring
 * only conditions the sums).  Per pixel and statistic, over the replicates whose value is not NaN, in ascending b:
 *   n_ok (GD_TC_STATS, M) int32: their number; with k = 1, 2, .. counting them,
 *   d = v - m;  m = m + d * (1 / k);  m2 = m2 + d * (v - m)  (m, m2 from +0.0);  mean = m,  std = sqrt(m2 / (n_ok - 1)),
 *   quantile j = numpy.nanquantile(values, q[j]) with method "linear", through the keys, sort and node rules of "Bias
 *   correction".  summary is (GD_TC_STATS, 2 + Q, M) doubles: mean, std, then the Q quantiles, 1 <= Q <= GD_TC_MAX_Q; all NaN
 *   where n_ok < 2.  q: Q doubles in [0, 1] in DEVICE memory (HOST for the twin).  replicates: NULL, or (B, GD_TC_STATS, M)
 *   doubles that receive every replicate value.
 * workspace: gd_tc_bootstrap_workspace(T, M, B) bytes hold all pixels at once; with fewer the pixels are walked in chunks
 * (whole groups of gd_tc_group(T) pixels), down to 8 + gd_tc_group(T) * GD_TC_STATS * B * 8 bytes; less is an error that names
 * the bytes needed.  The first 8 bytes receive the verdict of the index check; the call copies them back and waits for the
 * stream before the first replicate kernel (the only synchronisation), so an index >= T is an error and reads nothing.
 * A workgroup owns gd_tc_group(T) neighbouring series (8 up to T = 340, then 4, 2, 1: the three centred series of every pixel
 * of the group are staged in at most 64 KB of LDS, NaN marking a deleted step), a thread runs whole replicates with the
 * nine sums in registers, the lanes of a wave are neighbouring replicates of one pixel; the replicate values go to the
 * workspace as (GD_TC_STATS, pixels of the chunk, B); one wave per (pixel, statistic) sorts them in LDS for the quantiles and
 * one thread per (pixel, statistic) runs the mean / std recurrence.  No atomics, nothing allocated; no result depends on
 * the workspace size, on M, on a pixel's column or on the launch.  The *_host twins take every pointer in HOST memory (no
 * stream, no workspace) and run the same per-step code: all outputs agree bit for bit.
 * Errors (-1, gd_last_error): a NULL input or output, dtype, T, M, B, Q out of range, min_samples < 3, an index >= T, a
 * pointer that is not element aligned, a workspace smaller than one group.
 * ---------------------------------------------------------------------------------------- */
#define GD_TC_MAX_T 2048
#define GD_TC_MAX_B 2048
#define GD_TC_MAX_Q 8
#define GD_TC_COVS 6
enum { GD_TC_ERR_VAR_X = 0, GD_TC_ERR_VAR_Y = 1, GD_TC_ERR_VAR_Z = 2, GD_TC_RHO2_X = 3, GD_TC_RHO2_Y = 4, GD_TC_RHO2_Z = 5,
       GD_TC_BETA_Y = 6, GD_TC_BETA_Z = 7, GD_TC_STATS = 8 };
enum { GD_TC_FLAG_MASKED = 1, GD_TC_FLAG_FEW = 2, GD_TC_FLAG_NONPOS = 4, GD_TC_FLAG_NEG_X = 8, GD_TC_FLAG_NEG_Y = 16,
       GD_TC_FLAG_NEG_Z = 32, GD_TC_FLAG_RHO2 = 64 };
int gd_tc_estimate(const void* x, const void* y, const void* z, int dtype, long T, long M, int min_samples, const unsigned char* mask,
                   double* stats, double* cov, int* n, int* flags, void* stream);
int gd_tc_estimate_host(const void* x, const void* y, const void* z, int dtype, long T, long M, int min_samples,
                        const unsigned char* mask, double* stats, double* cov, int* n, int* flags);
int gd_tc_group(long T);   /* pixels per workgroup of gd_tc_bootstrap at this T (0 for a T out of range) */
size_t gd_tc_bootstrap_workspace(long T, long M, long B);
int gd_tc_bootstrap(const void* x, const void* y, const void* z, int dtype, long T, long M, const uint16_t* idx, long B,
                    int min_samples, const double* q, int Q, const unsigned char* mask, double* summary, int* n_ok, double* replicates,
                    void* workspace, size_t workspace_bytes, void* stream);
int gd_tc_bootstrap_host(const void* x, const void* y, const void* z, int dtype, long T, long M, const uint16_t* idx, long B,
                         int min_samples, const double* q, int Q, const unsigned char* mask, double* summary, int* n_ok,
                         double* replicates);

/* ------------------------------------------------------------------------------------------
 * Singular spectrum analysis (ssa.hip, csrc/ssa_core.h): the data-adaptive decomposition of every pixel series into a trend
 * and oscillatory components, and the iterative filling of gaps in time with it (Kondrashov & Ghil 2006; for the gap between
 * GRACE and GRACE-FO, Yi & Sneeuw 2021).  The layout is that of "Per-pixel time series": x is a dense (T, P) array
 * (P = M_pixels), series m at x[t * P + m], storage fp32 (dtype 0) or fp64 (dtype 1); NaN marks a gap.  All arithmetic is
 * fp64 with every operation rounded on its own (nothing is contracted into an FMA); only +, -, *, / and sqrt occur.
 *   Series       n valid (not NaN) samples, n_gaps = T - n.  mean = (sum of the valid samples in time order) / n;
 *                sd = sqrt((sum of (v - mean)^2 in time order) / n).  y = x - mean.  The mean is kept FIXED through the
 *                filling (Kondrashov & Ghil re-estimate it in every iteration; this version does not).
 *   Limits       window M: 2 <= M <= GD_SSA_MAX_M; K = T - M + 1 >= M, that is 2 M - 1 <= T <= GD_SSA_MAX_T;
 *                rank r: 1 <= r <= min(M, GD_SSA_MAX_RANK).
 *   Covariance   of a complete centred series, M x M, every sum in ascending order of its running index from +0.0:
 *                GD_SSA_BK (Broomhead & King)  C[i][j] = (sum over k = 0 .. K - 1 of y[k + i] * y[k + j]) / K: the trajectory
 *                  matrix X[k][i] = y[k + i] gives C = X^T X / K, so K times its eigenvalues are the squared singular values of X;
 *                GD_SSA_VG (Vautard & Ghil)    C[i][j] = c(|i - j|), c(l) = (sum over t = 0 .. T - l - 1 of y[t] * y[t + l]) / (T - l).
 *                Entries with i <= j are computed, C[j][i] is a copy.
 *   Eigenpairs   cyclic Jacobi.  The pairs of a sweep come in the 2 ceil(M / 2) - 1 sets of a round robin: with n1 = 2 ceil(M / 2) - 1,
 *                set s pairs s with n1 and (s + k) mod n1 with (s - k) mod n1, k = 1 .. ceil(M / 2) - 1; a pair is written p < q, and
 *                the pair that holds the index M of an odd M is a bye.  The rotation of a pair comes from the matrix as the set
 *                found it: none where |a_pq| <= thr = 2^-52 * (the largest |C[i][i]| of the matrix the solve started from), else
 *                tau = (a_qq - a_pp) / (2 a_pq), t = sign(tau) / (|tau| + sqrt(tau^2 + 1)) (sign(0) = +1), c = 1 / sqrt(t^2 + 1),
 *                s = t c.  A set is applied as all column rotations (x_p, x_q) <- (c x_p - s x_q, s x_p + c x_q), then all row
 *                rotations; an entry depends only on the 2 x 2 block of its row pair and its column pair, so the blocks are
 *                independent: those with (slot of the row pair) <= (slot of the column pair) are computed, the others are copies
 *                (the matrix stays exactly symmetric); the block of a pair with itself is a_pp - t a_pq, a_qq + t a_pq and an exact
 *                0.  The eigenvector matrix takes the column rotations.  Hence a sequential loop and a parallel one give the same
 *                bits.  Sweeps run until one rotates nothing (that sweep is counted), at most GD_SSA_MAX_SWEEPS (the suite's
 *                series need at most 14; see tests/ssa_util.py); reaching the cap with a rotating sweep sets
 *                GD_SSA_FLAG_SWEEPS and the result of the last sweep is used.  Eigenpairs are sorted by descending eigenvalue,
 *                ties to the lower original index; each eigenvector is signed so that its first entry of largest magnitude is > 0.
 *                trace = the sum of all M sorted eigenvalues in that order.
 *   Components   a_k[i] = sum over j = 0 .. M - 1 of y[i + j] * E[j][k], i = 0 .. K - 1; RC_k[t] = (sum over the j of the
 *                anti-diagonal, max(0, t - K + 1) <= j <= min(M - 1, t), ascending, of a_k[t - j] * E[j][k]) / (their number).  The
 *                sum of all M components is y.
 *   Filling      gaps of y start at 0.  For each stage q = 1 .. r, repeat: C of the current y; its eigenpairs; R[t] = RC_0[t] + ..
 *                + RC_(q-1)[t] (from +0.0, ascending k) at the gap steps; change = max over the gap steps of |R[t] - y[t]| (a NaN
 *                counts as +inf); y[t] = R[t] at the gap steps only.  A stage ends when change <= tol * sd or after max_iter
 *                iterations (then GD_SSA_FLAG_ITER is set); stage q + 1 starts from the result of stage q.  filled = x at the valid
 *                steps (converted to fp64) and mean + y at the gaps.  eig, trace and sweeps are those of the LAST solve (the series
 *                before its last update).  A series without gaps takes one solve and 0 iterations.
 *   Degenerate   a series gets NaN in eig, rc, filled and the float planes, and one flag bit for each reason: MASKED (mask[m] == 0;
 *                mask NULL or P bytes; such a pixel is not read, n = n_gaps = 0), NONFINITE (a sample is +-inf: mean and sd NaN; or the trace of a
 *                solve is not finite, the squares having overflowed), CONSTANT
 *                (sd is not > 0), FEW (gd_ssa_fill: n < min_valid, 2 <= min_valid <= GD_SSA_MAX_T), GAPS (gd_ssa_decompose: n < T;
 *                fill first).  mean and sd are still given where n >= 1 and no sample is infinite.
 * maps: (GD_SSA_MAPS, P) doubles, planar: n, n_gaps, mean, sd, trace, sweeps (of the last solve), iterations (total over the
 * stages), last_change, flags (the bits as a number).  eig: (rank, P) doubles.  rc: NULL or (rank, T, P) doubles.  evec
 * (gd_ssa_decompose): NULL or (rank, M, P) doubles, evec[(k * M + j) * P + m] = E[j][k] of series m.  filled: (T, P)
 * doubles.  One wave per series, the series, C, E and one principal component in dynamic LDS sized by T and M (above 64 KB the
 * kernel's dynamic-LDS limit is raised and its return code checked); the pixels are walked GD_SSA_CHUNK series per launch; no
 * atomics, no workspace; no result depends on P, on a pixel's column or on the chunk.  The *_host twins take every pointer in
 * HOST memory (no stream) and run the same per-series function with one lane: all outputs agree bit for bit.
 * Errors (-1, gd_last_error, before any launch): a NULL x, eig, maps or filled; dtype; window, T, rank, method, max_iter,
 * min_valid out of range; tol not finite or <= 0; M_pixels <= 0 or >= 2^31; a pointer that is not element aligned.
 * ---------------------------------------------------------------------------------------- */
#define GD_SSA_MAX_M 64
#define GD_SSA_MAX_T 2048
#define GD_SSA_MAX_RANK 16
#define GD_SSA_MAX_ITER 200
#define GD_SSA_MAX_SWEEPS 30
#define GD_SSA_CHUNK 8192
enum { GD_SSA_BK = 0, GD_SSA_VG = 1 };
enum { GD_SSA_N = 0, GD_SSA_N_GAPS = 1, GD_SSA_MEAN = 2, GD_SSA_SD = 3, GD_SSA_TRACE = 4, GD_SSA_SWEEPS = 5, GD_SSA_ITERATIONS = 6,
       GD_SSA_LAST_CHANGE = 7, GD_SSA_FLAGS = 8, GD_SSA_MAPS = 9 };
enum { GD_SSA_FLAG_MASKED = 1, GD_SSA_FLAG_FEW = 2, GD_SSA_FLAG_CONSTANT = 4, GD_SSA_FLAG_NONFINITE = 8, GD_SSA_FLAG_GAPS = 16,
       GD_SSA_FLAG_SWEEPS = 32, GD_SSA_FLAG_ITER = 64 };
int gd_ssa_decompose(const void* x, int dtype, long T, long M_pixels, int window, int rank, int method, const unsigned char* mask,
                     double* eig, double* maps, double* rc, double* evec, void* stream);
int gd_ssa_decompose_host(const void* x, int dtype, long T, long M_pixels, int window, int rank, int method, const unsigned char* mask,
                          double* eig, double* maps, double* rc, double* evec);
int gd_ssa_fill(const void* x, int dtype, long T, long M_pixels, int window, int rank, int method, const unsigned char* mask, double tol,
                int max_iter, int min_valid, double* filled, double* eig, double* maps, void* stream);
int gd_ssa_fill_host(const void* x, int dtype, long T, long M_pixels, int window, int rank, int method, const unsigned char* mask,
                     double tol, int max_iter, int min_valid, double* filled, double* eig, double* maps);

/* ------------------------------------------------------------------------------------------
 * Regionalisation (kmeans.hip, csrc/kmeans_core.h): k-means (Lloyd) on the pixel series of a cube, the step between pixel
 * maps and a table of regions.  The layout is that of "Per-pixel time series": x is a dense (T, M) array, series m at
 * x[t * M + m], storage fp32 (dtype 0) or fp64 (dtype 1).  1 <= T <= GD_KM_MAX_T, 1 <= K <= GD_KM_MAX_K, 0 < M < 2^31.  All
 * arithmetic is fp64 with every operation rounded on its own (nothing is contracted into an FMA); no floating-point atomics;
 * no result depends on the run, on the alignment of x beyond element alignment or on the size of a workspace, and a result
 * of gd_km_assign for series m depends on that series, its shift / scale and the centroids alone (not on M).
 *   Sample       v[t] = (x[t * M + m] - shift[m]) * scale[m]; a NULL shift counts as 0.0, a NULL scale as 1.0 (both exact), so
 *                centred or z-scored clustering needs no second copy of the cube.  shift, scale: NULL or M doubles.
 *   Distance     d[k] = sum over t = 0 .. T - 1, ascending from +0.0, of (v[t] - cent[k * T + t])^2, each term one subtraction
 *                and one square: never the |x|^2 - 2 x.c + |c|^2 form, which cancels.  cent: (K, T) doubles, finite.
 *   gd_km_assign label (M) int32: the k of the smallest d[k], the lower k on a tie; dist (M) doubles: that d.  label2 / dist2
 *                (each NULL or M entries): the smallest among the other k, the lower k on a tie; -1 / NaN when K = 1.  A series
 *                with mask[m] == 0 (mask NULL or M bytes; it is not read) or with a v[t] that is NaN or +-inf gets label -1,
 *                label2 -1 and NaN distances: listwise, as in the EOF analysis; fill gaps first (gd_ssa_fill).
 *   gd_km_update With a[m] = w[m] (w NULL: 1.0; M doubles, e.g. cos lat) over the members of cluster k (label[m] == k; a label
 *                outside 0 .. K - 1 belongs to none): wsum[k] = sum a, count[k] = their number (int64), within[k] = sum of
 *                a * dist[m] (the total over k is the inertia), and cent[k * T + t] = (sum of a * v[t]) / wsum[k].  A cluster
 *                whose wsum is not > 0 (no member, or zero weights) keeps the centroid it came with: cent is in / out.
 *                The order of every sum: the pixels are cut into slabs of GD_KM_SLAB neighbouring series; a slab's sum runs
 *                over its members in ascending m from +0.0; the slab sums are added in ascending slab order onto a total that
 *                starts at +0.0.  workspace: gd_km_update_ws_bytes(T, M, K) bytes hold the totals and all slabs, (1 +
 *                ceil(M / GD_KM_SLAB)) * (K * T + 3 * K) doubles; with fewer, down to gd_km_update_min_ws_bytes(T, K) (the totals
 *                and one slab), the slabs are walked in chunks and the result has the same bits; less is an error.
 *   gd_km_farthest index[0] = the i of the largest d[i] that is finite, i not in exclude[0 .. n_exclude - 1] (0 <= n_exclude <=
 *                GD_KM_MAX_K; NULL with 0), the lowest i on a tie; -1 if there is none.  d: M doubles.  It serves the maximin
 *                initialisation and the re-seating of empty clusters.
 * gd_km_assign: a workgroup of 256 neighbouring series, one per thread, reads each row segment once (coalesced); the centroids
 * are staged in LDS GD_KM_CHUNK time steps at a time and read as wave-uniform broadcasts; the K sums live in registers (the
 * kernel is a template on K rounded up to 8 / 16 / 32 / 64).  The cube is read once whatever K is.
 * The *_host twins take every pointer in HOST memory (no workspace, no stream) and run the same per-element code in the same
 * order: all outputs agree bit for bit.
 * Errors (-1, gd_last_error, before any launch): a NULL x, cent, label, dist (wsum, count, within, d, index); dtype; T, K,
 * n_exclude out of range; M <= 0 or >= 2^31; a pointer that is not element aligned; a workspace that is NULL or too small.
 * ---------------------------------------------------------------------------------------- */
#define GD_KM_MAX_T 2048
#define GD_KM_MAX_K 64
#define GD_KM_CHUNK 64
#define GD_KM_SLAB 1024
int gd_km_assign(const void* x, int dtype, long T, long M, const double* cent, int K, const double* shift, const double* scale,
                 const unsigned char* mask, int* label, double* dist, int* label2, double* dist2, void* stream);
int gd_km_assign_host(const void* x, int dtype, long T, long M, const double* cent, int K, const double* shift, const double* scale,
                      const unsigned char* mask, int* label, double* dist, int* label2, double* dist2);
size_t gd_km_update_ws_bytes(long T, long M, int K);
size_t gd_km_update_min_ws_bytes(long T, int K);
int gd_km_update(const void* x, int dtype, long T, long M, const int* label, const double* dist, const double* w, const double* shift,
                 const double* scale, int K, double* cent, double* wsum, long long* count, double* within, void* workspace,
                 size_t workspace_bytes, void* stream);
int gd_km_update_host(const void* x, int dtype, long T, long M, const int* label, const double* dist, const double* w,
                      const double* shift, const double* scale, int K, double* cent, double* wsum, long long* count, double* within);
int gd_km_farthest(const double* d, long M, const int* exclude, int n_exclude, int* index, void* stream);
int gd_km_farthest_host(const double* d, long M, const int* exclude, int n_exclude, int* index);

#ifdef __cplusplus
}
#endif
#endif /* GANDANET_H */
