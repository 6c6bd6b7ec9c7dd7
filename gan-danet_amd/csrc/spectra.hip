// Spatial spectra (include/gandanet.h, "Spatial spectra"): the radially binned power spectrum of every field of a (T, H, W)
// cube, and the co- and quadrature spectra of two cubes, as a 2-D DFT written as matrix products on
// v_mfma_f64_16x16x4_f64.  No spectrum is stored: |Z|^2 is binned in the epilogue.  The per-element arithmetic is
// spectra_core.h, shared with the host twins.
//
// prepare: one workgroup per field, two passes over it (sums, then second moments about the means), every sum through
// gd_block_sum_d; thread 0 solves the plane.
//
// dft: a workgroup of 4 waves owns one field (NF = 1) or one pair of fields (NF = 2) and a tile of KT = 8 / NF kx, 16 real
// columns: column c of the tile is field c / (2 KT), part (c / KT) & 1 (0 = Re, 1 = Im), kx0 + c % KT.
//   stage 1, Y = x' [C_W | -S_W]: chunks of 64 rows x 32 columns of x' (fill, detrend and taper applied at the load; rows
//   beyond H, columns beyond W and invalid pixels are zeros) are staged in LDS, rows SPEC_XS = 34 doubles apart, so that
//   the 32 lanes of a ds_read_b64 group (16 rows x 2 columns) fall on 32 different bank pairs, next to the 32 x 16 twiddle
//   chunk.  Wave w owns rows 16 w .. 16 w + 15 of the chunk: A = x'[16 rows][4 j], B = twiddles[4 j][16 columns].  Its
//   accumulators go to the LDS image Y[row][16] (fp64, rows 16 doubles apart: a B fragment of stage 2 is 64 consecutive
//   doubles).
//   stage 2, Z = [C_H | S_H] Y: in rounds of 64 ky, wave w the 16 ky of block 4 r + w.  Per 4 rows of Y two MFMAs into one
//   accumulator: cos(2 pi ky i / H) times Y[i][c], and sin(2 pi ky i / H) times +-Y[i][c ^ KT] (+ for a Re column, - for an
//   Im column), which leaves Re Z in the Re columns and Im Z in the Im columns.  The twiddles come from the LDS copy of the
//   table, indexed by (ky i) mod H, advanced by (4 ky) mod H per step.
//   epilogue: the Im (and second field's) values come over by lane exchange, weight |Z|^2 (or the four cross terms) go to
//   an LDS tile with their bin slots; after a barrier thread t adds, in the tile's fixed order, the values whose slot is
//   t (mod 256) to its own register accumulators.  No atomics.  One slab [NQ][nbins + 1] per workgroup; a second launch adds
//   the slabs of a field in ascending tile order and divides by H W S.
#include <algorithm>
#include <vector>

#include "elem_util.h"
#include "spectra_core.h"

namespace {

constexpr int SPEC_THREADS = 256;
constexpr int SPEC_ROWS = 64, SPEC_COLS = 32;   // the staged chunk of x'
constexpr int SPEC_XS = SPEC_COLS + 2;          // doubles per staged row: 2 * 34 = 4 (mod 64) dwords from row to row
constexpr int SPEC_SLOTS = GD_SPEC_MAX_BINS / SPEC_THREADS + 1;   // bin slots a thread owns (the last: dropped)
constexpr int SPEC_SKIP = -1;                   // slot of a tile entry beyond H or beyond W / 2

typedef double f64x4_t __attribute__((ext_vector_type(4)));

struct SpecField {
    const void* x;
    const double* coef;   // 3 per field
    const double* S;      // 2 per field: S, n
};

// doubles of LDS: the image Y, then the scratch shared by the stages
__host__ __device__ inline int spec_y_doubles(int H) { return (H + SPEC_ROWS - 1) / SPEC_ROWS * SPEC_ROWS * 16; }
__host__ __device__ inline int spec_scratch_doubles(int H, int nq) {
    const int s1 = SPEC_ROWS * SPEC_XS + SPEC_COLS * 16;
    const int s2 = 2 * H + 64 * GD_SPEC_TILE * nq / (nq > 1 ? 2 : 1) + 64 * GD_SPEC_TILE / 2;
    return s1 > s2 ? s1 : s2;
}

// ---- prepare -------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SPEC_THREADS) void spec_prepare_kernel(const T* __restrict__ x, int H, int W,
                                                                    const unsigned char* __restrict__ mask,
                                                                    const double* __restrict__ wy, const double* __restrict__ wx,
                                                                    int detrend, double* __restrict__ coef, double* __restrict__ S) {
    __shared__ double red[SPEC_THREADS / 64][5];
    __shared__ GdSpecMeans mean;
    const int tid = threadIdx.x, n = H * W;
    const T* xf = x + (long)blockIdx.x * n;
    const double uc = gd_spec_centre(H), vc = gd_spec_centre(W);
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = tid; p < n; p += SPEC_THREADS) {
        const int i = p / W, j = p - i * W;
        const double v = (double)xf[p];
        if (gd_spec_finite(v) && (!mask || mask[p] != 0)) {
            const double a = wy ? wy[i] : 1.0, b = wx ? wx[j] : 1.0;
            s[0] += 1.0;
            s[1] += (double)i - uc;
            s[2] += (double)j - vc;
            s[3] += v;
            s[4] += (a * a) * (b * b);
        }
    }
    gd_block_sum_d<5, SPEC_THREADS / 64>(s, red);
    if (tid == 0) {
        mean = gd_spec_means(s[0], s[1], s[2], s[3]);
        S[2 * blockIdx.x] = s[4];
        S[2 * blockIdx.x + 1] = s[0];
    }
    __syncthreads();
    const GdSpecMeans m = mean;
    double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (detrend == GD_SPEC_DETREND_PLANE) {
        for (int p = tid; p < n; p += SPEC_THREADS) {
            const int i = p / W, j = p - i * W;
            const double v = (double)xf[p];
            if (gd_spec_finite(v) && (!mask || mask[p] != 0)) {
                const double du = ((double)i - uc) - m.um, dv = ((double)j - vc) - m.vm, dx = v - m.xm;
                q[0] += du * du;
                q[1] += dv * dv;
                q[2] += du * dv;
                q[3] += du * dx;
                q[4] += dv * dx;
            }
        }
        __syncthreads();   // red is read by thread 0 above
        gd_block_sum_d<5, SPEC_THREADS / 64>(q, red);
    }
    if (tid == 0) gd_spec_solve(m, detrend, q[0], q[1], q[2], q[3], q[4], coef + 3 * blockIdx.x);
}

template <typename T>
static void prepare_host(const T* x, long Tn, int H, int W, const unsigned char* mask, const double* wy, const double* wx, int detrend,
                         double* coef, double* S) {
    const double uc = gd_spec_centre(H), vc = gd_spec_centre(W);
    for (long t = 0; t < Tn; ++t) {
        const T* xf = x + t * H * W;
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int pass = 0; pass < 2; ++pass) {
            const GdSpecMeans m = gd_spec_means(s[0], s[1], s[2], s[3]);
            for (int i = 0; i < H; ++i) {
                for (int j = 0; j < W; ++j) {
                    const long p = (long)i * W + j;
                    const double v = (double)xf[p];
                    if (!gd_spec_finite(v) || (mask && mask[p] == 0)) continue;
                    if (pass == 0) {
                        const double a = wy ? wy[i] : 1.0, b = wx ? wx[j] : 1.0;
                        s[0] += 1.0;
                        s[1] += (double)i - uc;
                        s[2] += (double)j - vc;
                        s[3] += v;
                        s[4] += (a * a) * (b * b);
                    } else {
                        const double du = ((double)i - uc) - m.um, dv = ((double)j - vc) - m.vm, dx = v - m.xm;
                        q[0] += du * du;
                        q[1] += dv * dv;
                        q[2] += du * dv;
                        q[3] += du * dx;
                        q[4] += dv * dx;
                    }
                }
            }
        }
        S[2 * t] = s[4];
        S[2 * t + 1] = s[0];
        gd_spec_solve(gd_spec_means(s[0], s[1], s[2], s[3]), detrend, q[0], q[1], q[2], q[3], q[4], coef + 3 * t);
    }
}

// ---- the DFT kernel ------------------------------------------------------------------------------------------------------
// NF fields; NQ = 1 (power) or 4 (power a, power b, co, quad) values per wavenumber
template <typename T, int NF>
__global__ __launch_bounds__(SPEC_THREADS) void spec_dft_kernel(SpecField fa, SpecField fb, int H, int W,
                                                                const unsigned char* __restrict__ mask, const double* __restrict__ wy,
                                                                const double* __restrict__ wx, const double* __restrict__ twh,
                                                                const double* __restrict__ tww, const int* __restrict__ bin, int nbins,
                                                                int tiles, double* __restrict__ p2d, double* __restrict__ ws) {
    constexpr int KT = GD_SPEC_TILE / NF, NQ = NF == 1 ? 1 : 4;
    extern __shared__ double spec_lds[];
    double* Y = spec_lds;
    double* scratch = spec_lds + spec_y_doubles(H);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x / tiles, tile = blockIdx.x - t * tiles, kx0 = tile * KT, Kx = W / 2 + 1;   // a field's tiles are neighbours
    const int col = lane & 15, quad = lane >> 4;
    const double uc = gd_spec_centre(H), vc = gd_spec_centre(W);

    // ---- stage 1 ----
    {
        double* xs = scratch;
        double* bc = scratch + SPEC_ROWS * SPEC_XS;
        const int sc = tid & (SPEC_COLS - 1), sr = tid >> 5;   // the thread stages column sc of rows sr + 8 r
        const int bkx = kx0 + col % KT;                        // the kx of twiddle column `col`
        const bool bim = (col / KT) & 1;
        // per field: its samples and its plane (NF is 1 or 2: scalars, not an indexed copy of the argument structs)
        const T* xf0 = (const T*)fa.x + (long)t * H * W;
        const T* xf1 = (const T*)fb.x + (long)t * H * W;
        const double a0 = fa.coef[3 * t], b0 = fa.coef[3 * t + 1], c0 = fa.coef[3 * t + 2];
        const double a1 = fb.coef[3 * t], b1 = fb.coef[3 * t + 1], c1 = fb.coef[3 * t + 2];
        for (int i0 = 0; i0 < H; i0 += SPEC_ROWS) {
            f64x4_t acc[NF];
#pragma unroll
            for (int f = 0; f < NF; ++f) acc[f] = f64x4_t{0.0, 0.0, 0.0, 0.0};
            for (int j0 = 0; j0 < W; j0 += SPEC_COLS) {
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    const T* xf = f == 0 ? xf0 : xf1;
                    const double a = f == 0 ? a0 : a1, b = f == 0 ? b0 : b1, c = f == 0 ? c0 : c1;
                    __syncthreads();   // the MFMAs before have read their fragments
                    {
                        const int j = j0 + sc, jc = j < W ? j : W - 1;
                        const double wxj = wx ? wx[jc] : 1.0, v = (double)jc - vc;
#pragma unroll
                        for (int r = 0; r < SPEC_ROWS / 8; ++r) {
                            const int i = i0 + sr + 8 * r, ic = i < H ? i : H - 1;
                            const long p = (long)ic * W + jc;
                            const double xv = (double)xf[p];
                            const bool ok = i < H && j < W && gd_spec_finite(xv) && (!mask || mask[p] != 0);
                            xs[(sr + 8 * r) * SPEC_XS + sc] = gd_spec_sample(xv, ok, a, b, c, (double)ic - uc, v, wy ? wy[ic] : 1.0, wxj);
                        }
                    }
                    if (f == 0) {
                        // twiddle chunk [32 j][16 columns]: cos for a Re column, -sin for an Im column; zero beyond W
#pragma unroll
                        for (int e = 0; e < SPEC_COLS * 16 / SPEC_THREADS; ++e) {
                            const int jl = (tid >> 4) + 16 * e, j = j0 + jl;   // tid & 15 == col
                            double v = 0.0;
                            if (j < W) {
                                const int idx = (int)(((long)bkx * j) % W);
                                v = bim ? -tww[W + idx] : tww[idx];
                            }
                            bc[jl * 16 + col] = v;
                        }
                    }
                    __syncthreads();
                    const double* af = xs + (wave * 16 + col) * SPEC_XS + quad;
                    const double* bf = bc + quad * 16 + col;
#pragma unroll
                    for (int ks = 0; ks < SPEC_COLS / 4; ++ks)
                        acc[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ks * 4], bf[ks * 64], acc[f], 0, 0, 0);
                }
            }
            // C/D: column lane & 15, row (lane >> 4) + 4 * register; column c belongs to field c / (2 KT)
            f64x4_t mine = acc[0];
            if constexpr (NF == 2) {
                if (col >= 2 * KT) mine = acc[1];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) Y[(i0 + wave * 16 + quad + 4 * q) * 16 + col] = mine[q];
        }
    }
    __syncthreads();

    // ---- stage 2 ----
    double* th = scratch;                                  // cos[H], sin[H]
    double* pt = scratch + 2 * H;                          // [64 ky][KT][NQ]
    int* bt = (int*)(pt + 64 * KT * NQ);                   // [64 ky][KT] slots
    for (int e = tid; e < 2 * H; e += SPEC_THREADS) th[e] = twh[e];
    double sum[SPEC_SLOTS][NQ];
#pragma unroll
    for (int s = 0; s < SPEC_SLOTS; ++s) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) sum[s][q] = 0.0;
    }
    const double sgn = (col & KT) ? -1.0 : 1.0;
    const int ksteps = (H + 3) / 4, nkb = (H + 15) / 16;
    const double norm_a = p2d ? (double)H * (double)W * fa.S[2 * t] : 1.0;
    for (int kb0 = 0; kb0 < nkb; kb0 += 4) {
        __syncthreads();   // the tile of the round before has been added (first round: th is complete)
        // the slots of this round's tile
        for (int e = tid; e < 64 * KT; e += SPEC_THREADS) {
            const int ky = kb0 * 16 + e / KT, kx = kx0 + e % KT;
            int slot = SPEC_SKIP;
            if (ky < H && kx < Kx) {
                const int b = bin[(long)ky * Kx + kx];
                slot = b < 0 ? nbins : b;
            }
            bt[e] = slot;
        }
        const int kb = kb0 + wave;
        if (kb < nkb) {
            f64x4_t acc = f64x4_t{0.0, 0.0, 0.0, 0.0};
            const int ky = kb * 16 + col;                  // A: row lane & 15, k lane >> 4
            int idx = (ky * quad) % H;
            const int step = (4 * ky) % H;
            const double* b1 = Y + quad * 16 + col;
            const double* b2 = Y + quad * 16 + (col ^ KT);
#pragma nounroll
            for (int ks = 0; ks < ksteps; ++ks) {
                const double c = th[idx], s = th[H + idx];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(c, b1[ks * 64], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s, sgn * b2[ks * 64], acc, 0, 0, 0);
                idx += step;
                idx -= idx >= H ? H : 0;
            }
            // Re Z of (ky = 16 kb + quad + 4 q, kx0 + col % KT) sits in the Re columns, Im Z KT lanes further
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double z = acc[q];
                const double zi = __shfl_xor(z, KT, 64);
                const int kyo = kb * 16 + quad + 4 * q, kx = kx0 + col;
                const int row = (wave * 16 + quad + 4 * q) * KT + col;
                if constexpr (NF == 1) {
                    if (col < KT) {
                        const double p = gd_spec_pow(z, zi, gd_spec_hweight(kx, W));
                        pt[row] = p;
                        if (p2d && kyo < H && kx < Kx) p2d[((long)t * H + kyo) * Kx + kx] = gd_spec_norm(p, 1.0, norm_a, fa.S[2 * t + 1] > 0.0);
                    }
                } else {
                    const double br = __shfl_xor(z, 2 * KT, 64), bi = __shfl_xor(zi, 2 * KT, 64);
                    if (col < KT) {
                        const double w = gd_spec_hweight(kx, W);
                        pt[row * 4] = gd_spec_pow(z, zi, w);
                        pt[row * 4 + 1] = gd_spec_pow(br, bi, w);
                        pt[row * 4 + 2] = gd_spec_co(z, zi, br, bi, w);
                        pt[row * 4 + 3] = gd_spec_quad(z, zi, br, bi, w);
                    }
                }
            }
        }
        __syncthreads();
        // thread t owns the slots t, t + 256, ...: the tile in ascending (ky, kx)
        for (int e = 0; e < 64 * KT; ++e) {
            const int slot = bt[e];
            if (slot >= 0 && (slot & (SPEC_THREADS - 1)) == tid) {
                const int sl = slot >> 8;
#pragma unroll
                for (int s = 0; s < SPEC_SLOTS; ++s) {
                    if (s == sl) {
#pragma unroll
                        for (int q = 0; q < NQ; ++q) sum[s][q] += pt[e * NQ + q];
                    }
                }
            }
        }
    }
    // slab [NQ][nbins + 1]
    double* slab = ws + (long)blockIdx.x * (NQ * (nbins + 1));
#pragma unroll
    for (int s = 0; s < SPEC_SLOTS; ++s) {
        const int slot = tid + s * SPEC_THREADS;
        if (slot <= nbins) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) slab[q * (nbins + 1) + slot] = sum[s][q];
        }
    }
}

// one thread per (field, value, slot): the slabs in ascending tile order, over H W S; slot nbins is `dropped`
template <int NQ>
__global__ __launch_bounds__(256) void spec_reduce_kernel(const double* __restrict__ ws, int Tn, int tiles, int nbins, double hw,
                                                          const double* __restrict__ Sa, const double* __restrict__ Sb,
                                                          double* __restrict__ out, double* __restrict__ dropped) {
    const int per = NQ * (nbins + 1);
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)Tn * per) return;
    const int t = (int)(g / per), r = (int)(g - (long)t * per), q = r / (nbins + 1), slot = r - q * (nbins + 1);
    const double* p = ws + (long)t * tiles * per + r;
    double v = p[0];
    for (int k = 1; k < tiles; ++k) v += p[(long)k * per];
    const double sa = Sa[2 * t], sb = NQ == 1 ? sa : Sb[2 * t];
    const bool any = Sa[2 * t + 1] > 0.0 && (NQ == 1 || Sb[2 * t + 1] > 0.0);
    const double s = q == 0 ? sa : (q == 1 ? sb : sqrt(sa * sb));
    const double res = gd_spec_norm(v, hw, s, any);
    if (slot < nbins) out[((long)q * Tn + t) * nbins + slot] = res;
    else dropped[(long)t * NQ + q] = res;
}

// ---- host twin: a separable two-stage sum over the same tables -----------------------------------------------------------
template <typename T>
static void field_dft_host(const T* xf, int H, int W, const unsigned char* mask, const double* wy, const double* wx, const double* coef,
                           const double* twh, const double* tww, std::vector<double>& zre, std::vector<double>& zim) {
    const int Kx = W / 2 + 1;
    const double uc = gd_spec_centre(H), vc = gd_spec_centre(W);
    std::vector<double> xr((size_t)W), yre((size_t)H * Kx), yim((size_t)H * Kx);
    for (int i = 0; i < H; ++i) {
        for (int j = 0; j < W; ++j) {
            const long p = (long)i * W + j;
            const double xv = (double)xf[p];
            const bool ok = gd_spec_finite(xv) && (!mask || mask[p] != 0);
            xr[j] = gd_spec_sample(xv, ok, coef[0], coef[1], coef[2], (double)i - uc, (double)j - vc, wy ? wy[i] : 1.0, wx ? wx[j] : 1.0);
        }
        for (int kx = 0; kx < Kx; ++kx) {
            double re = 0.0, im = 0.0;
            for (int j = 0; j < W; ++j) {
                const int idx = (int)(((long)kx * j) % W);
                re += xr[j] * tww[idx];
                im += xr[j] * -tww[W + idx];
            }
            yre[(size_t)i * Kx + kx] = re;
            yim[(size_t)i * Kx + kx] = im;
        }
    }
    zre.assign((size_t)H * Kx, 0.0);
    zim.assign((size_t)H * Kx, 0.0);
    for (int ky = 0; ky < H; ++ky) {
        for (int kx = 0; kx < Kx; ++kx) {
            double re = 0.0, im = 0.0;
            for (int i = 0; i < H; ++i) {
                const int idx = (int)(((long)ky * i) % H);
                const double c = twh[idx], s = twh[H + idx];
                re += c * yre[(size_t)i * Kx + kx];
                re += s * yim[(size_t)i * Kx + kx];
                im += c * yim[(size_t)i * Kx + kx];
                im += s * -yre[(size_t)i * Kx + kx];
            }
            zre[(size_t)ky * Kx + kx] = re;
            zim[(size_t)ky * Kx + kx] = im;
        }
    }
}

template <typename T>
static void power_host(const T* x, long Tn, int H, int W, const unsigned char* mask, const double* wy, const double* wx, const double* coef,
                       const double* S, const double* twh, const double* tww, const int* bin, int nbins, double* power, double* dropped,
                       double* p2d) {
    const int Kx = W / 2 + 1;
    const double hw = (double)H * (double)W;
    std::vector<double> zre, zim, sum((size_t)nbins + 1);
    for (long t = 0; t < Tn; ++t) {
        field_dft_host(x + t * H * W, H, W, mask, wy, wx, coef + 3 * t, twh, tww, zre, zim);
        const bool any = S[2 * t + 1] > 0.0;
        std::fill(sum.begin(), sum.end(), 0.0);
        for (int ky = 0; ky < H; ++ky) {
            for (int kx = 0; kx < Kx; ++kx) {
                const size_t e = (size_t)ky * Kx + kx;
                const double p = gd_spec_pow(zre[e], zim[e], gd_spec_hweight(kx, W));
                sum[bin[e] < 0 ? nbins : bin[e]] += p;
                if (p2d) p2d[(size_t)t * H * Kx + e] = gd_spec_norm(p, 1.0, hw * S[2 * t], any);
            }
        }
        for (int b = 0; b < nbins; ++b) power[t * nbins + b] = gd_spec_norm(sum[b], hw, S[2 * t], any);
        dropped[t] = gd_spec_norm(sum[nbins], hw, S[2 * t], any);
    }
}

template <typename T>
static void cross_host(const T* xa, const T* xb, long Tn, int H, int W, const unsigned char* mask, const double* wy, const double* wx,
                       const double* coefa, const double* Sa, const double* coefb, const double* Sb, const double* twh, const double* tww,
                       const int* bin, int nbins, double* out, double* dropped) {
    const int Kx = W / 2 + 1;
    const double hw = (double)H * (double)W;
    std::vector<double> are, aim, bre, bim, sum(4 * ((size_t)nbins + 1));
    for (long t = 0; t < Tn; ++t) {
        field_dft_host(xa + t * H * W, H, W, mask, wy, wx, coefa + 3 * t, twh, tww, are, aim);
        field_dft_host(xb + t * H * W, H, W, mask, wy, wx, coefb + 3 * t, twh, tww, bre, bim);
        const bool any = Sa[2 * t + 1] > 0.0 && Sb[2 * t + 1] > 0.0;
        std::fill(sum.begin(), sum.end(), 0.0);
        for (int ky = 0; ky < H; ++ky) {
            for (int kx = 0; kx < Kx; ++kx) {
                const size_t e = (size_t)ky * Kx + kx;
                const double w = gd_spec_hweight(kx, W);
                double* s = sum.data() + 4 * (size_t)(bin[e] < 0 ? nbins : bin[e]);
                s[0] += gd_spec_pow(are[e], aim[e], w);
                s[1] += gd_spec_pow(bre[e], bim[e], w);
                s[2] += gd_spec_co(are[e], aim[e], bre[e], bim[e], w);
                s[3] += gd_spec_quad(are[e], aim[e], bre[e], bim[e], w);
            }
        }
        const double nrm[4] = {Sa[2 * t], Sb[2 * t], sqrt(Sa[2 * t] * Sb[2 * t]), sqrt(Sa[2 * t] * Sb[2 * t])};
        for (int q = 0; q < 4; ++q) {
            for (int b = 0; b < nbins; ++b) out[((size_t)q * Tn + t) * nbins + b] = gd_spec_norm(sum[4 * (size_t)b + q], hw, nrm[q], any);
            dropped[t * 4 + q] = gd_spec_norm(sum[4 * (size_t)nbins + q], hw, nrm[q], any);
        }
    }
}

static bool spec_shape_ok(long T, long H, long W) {
    return T >= 1 && H >= 1 && W >= 1 && H <= GD_SPEC_MAX_H && W <= GD_SPEC_MAX_W && T < (1L << 31) && T * H * W < (1L << 31);
}

template <typename T, int NF>
static int dft_launch(SpecField fa, SpecField fb, int Tn, int H, int W, const unsigned char* mask, const double* wy, const double* wx,
                      const double* twh, const double* tww, const int* bin, int nbins, double* p2d, double* ws, hipStream_t st) {
    constexpr int NQ = NF == 1 ? 1 : 4;
    const size_t bytes = (size_t)(spec_y_doubles(H) + spec_scratch_doubles(H, NQ)) * sizeof(double);
    if (bytes > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&spec_dft_kernel<T, NF>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            gd_set_error(hipGetErrorString(e));
            return -2;
        }
    }
    const int tiles = (int)gd_spec_tiles(W, NF);   // Tn * tiles <= Tn * W < 2^31
    hipLaunchKernelGGL((spec_dft_kernel<T, NF>), dim3((unsigned)(Tn * tiles)), dim3(SPEC_THREADS), bytes, st, fa, fb, H, W, mask, wy, wx, twh,
                       tww, bin, nbins, tiles, p2d, ws);
    return 0;
}

}  // namespace

// ---- tables (host only) --------------------------------------------------------------------------------------------------
// cos and sin of 2 pi r / N: the angle is k pi / 2 +- phi with phi = pi m / (4 N) in [0, pi / 4], m an integer; cos phi and
// sin phi in extended precision, rounded once; the multiples of pi / 2 are exact
extern "C" int gd_spec_twiddle_host(long N, double* tw) {
    GD_CHECK_ARG(tw, "gd_spec_twiddle_host: null pointer");
    GD_CHECK_ARG(N >= 1 && N <= GD_SPEC_MAX_W, "gd_spec_twiddle_host: N outside 1..GD_SPEC_MAX_W");
    static const int ck[4] = {1, 0, -1, 0}, sk[4] = {0, 1, 0, -1};
    const long double quarter_pi = 0.785398163397448309615660845819875721L;
    for (long r = 0; r < N; ++r) {
        const long p = 8 * r, oct = p / N, rem = p - oct * N;
        const int k = (int)(((oct + 1) / 2) & 3);
        const bool back = oct & 1;
        const long m = back ? N - rem : rem;
        const long double phi = quarter_pi * (long double)m / (long double)N;
        const long double c = cosl(phi), s = back ? -sinl(phi) : sinl(phi);
        tw[r] = (double)((long double)ck[k] * c - (long double)sk[k] * s);
        tw[N + r] = (double)((long double)sk[k] * c + (long double)ck[k] * s);
    }
    return 0;
}

// nbins that reach the smaller Nyquist wavenumber: floor(min(1 / (2 dy), 1 / (2 dx)) * max(H dy, W dx)) + 1
extern "C" int gd_spec_default_bins(long H, long W, double dy, double dx) {
    if (H < 1 || W < 1 || !(dy > 0.0) || !(dx > 0.0) || !gd_spec_finite(dy) || !gd_spec_finite(dx)) return 0;
    const double P = (double)H * dy, Q = (double)W * dx, L = P > Q ? P : Q;
    const double ny = 0.5 / (dy > dx ? dy : dx);
    const double nb = floor(ny * L * (1.0 + 0x1p-40)) + 1.0;
    return nb > GD_SPEC_MAX_BINS ? GD_SPEC_MAX_BINS : (int)nb;
}

extern "C" int gd_spec_bins_host(long H, long W, double dy, double dx, int nbins, double kmax, int* bin, double* kcentre, long* count) {
    GD_CHECK_ARG(bin && kcentre && count, "gd_spec_bins_host: null pointer");
    GD_CHECK_ARG(H >= 1 && W >= 1 && H <= GD_SPEC_MAX_H && W <= GD_SPEC_MAX_W, "gd_spec_bins_host: H or W outside the supported range");
    GD_CHECK_ARG(dy > 0.0 && dx > 0.0 && gd_spec_finite(dy) && gd_spec_finite(dx), "gd_spec_bins_host: dy or dx not positive and finite");
    GD_CHECK_ARG(nbins >= 1 && nbins <= GD_SPEC_MAX_BINS, "gd_spec_bins_host: nbins outside 1..GD_SPEC_MAX_BINS");
    GD_CHECK_ARG(!(kmax != kmax), "gd_spec_bins_host: kmax is NaN");
    // the domain lengths are the fp64 products; q = (k L)^2 = (ky' L / P)^2 + (kx L / Q)^2, bin = floor(sqrt(q))
    const double P = (double)H * dy, Q = (double)W * dx, L = P > Q ? P : Q;
    // P / Q as a ratio of small integers where it is one: then q * den^2 is an integer and the edges are exact
    long mp = 0, mq = 0;
    {
        int ep, eq;
        double fp = frexp(P, &ep), fq = frexp(Q, &eq);
        long ip = (long)ldexp(fp, 53), iq = (long)ldexp(fq, 53);
        ep -= 53;
        eq -= 53;
        while (!(ip & 1)) ip >>= 1, ++ep;
        while (!(iq & 1)) iq >>= 1, ++eq;
        const int e = ep < eq ? ep : eq;
        if (ep - e < 20 && eq - e < 20 && ip < (1L << 20) && iq < (1L << 20)) {
            ip <<= ep - e;
            iq <<= eq - e;
            long a = ip, b = iq;
            while (b) {
                const long r = a % b;
                a = b;
                b = r;
            }
            ip /= a;
            iq /= a;
            if (ip < (1L << 20) && iq < (1L << 20)) mp = ip, mq = iq;
        }
    }
    const long Kx = W / 2 + 1;
    const long double lim = kmax > 0.0 ? (long double)kmax * L * (1.0L + 0x1p-40L) : -1.0L;
    for (int b = 0; b < nbins; ++b) {
        kcentre[b] = ((double)b + 0.5) / L;
        count[b] = 0;
    }
    for (long ky = 0; ky < H; ++ky) {
        const long kf = 2 * ky > H ? ky - H : ky, ka = kf < 0 ? -kf : kf;
        for (long kx = 0; kx < Kx; ++kx) {
            const long double ay = ((long double)ka * L) / P, ax = ((long double)kx * L) / Q;
            const long double q = ay * ay + ax * ax;
            long b = (long)floorl(sqrtl(q));
            if (mp) {
                // P >= Q: ay = ka, ax = kx mp / mq; else ay = ka mq / mp, ax = kx: q = num / den in integers, b^2 den <= num < (b + 1)^2 den
                const unsigned long ny = mp > mq ? 1 : mq, dyn = mp > mq ? 1 : mp;   // ay = ka ny / dyn
                const unsigned long nx = mp > mq ? mp : 1, dxn = mp > mq ? mq : 1;   // ax = kx nx / dxn
                const unsigned __int128 den = (unsigned __int128)(dyn * dyn) * (dxn * dxn);
                const unsigned __int128 num = (unsigned __int128)((unsigned long)ka * ka) * (ny * ny) * (dxn * dxn) +
                                              (unsigned __int128)((unsigned long)kx * kx) * (nx * nx) * (dyn * dyn);
                while (b > 0 && (unsigned __int128)(b * b) * den > num) --b;
                while ((unsigned __int128)((b + 1) * (b + 1)) * den <= num) ++b;
            }
            const bool drop = b >= nbins || (lim >= 0.0L && sqrtl(q) > lim);
            bin[ky * Kx + kx] = drop ? -1 : (int)b;
            if (!drop) ++count[b];
        }
    }
    return 0;
}

// ---- entries ---------------------------------------------------------------------------------------------------------------
#define SPEC_SHAPE_CHECKS(fn)                                                                        \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                   \
    GD_CHECK_ARG(T >= 1 && H >= 1 && W >= 1, fn ": T, H or W < 1");                                  \
    GD_CHECK_ARG(H <= GD_SPEC_MAX_H && W <= GD_SPEC_MAX_W, fn ": H > GD_SPEC_MAX_H or W > GD_SPEC_MAX_W"); \
    GD_CHECK_ARG(T < (1L << 31) && T * H * W < (1L << 31), fn ": too many elements")

#define SPEC_PREPARE_CHECKS(fn)                                                                                 \
    GD_CHECK_ARG(x && coef && S, fn ": null pointer");                                                         \
    SPEC_SHAPE_CHECKS(fn);                                                                                      \
    GD_CHECK_ARG(detrend >= 0 && detrend <= 2, fn ": detrend outside {0, 1, 2}");                               \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(wy, 8) && gd_aligned(wx, 8) && gd_aligned(coef, 8) && gd_aligned(S, 8), \
                 fn ": pointer not element aligned")

extern "C" int gd_spec_prepare(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy,
                               const double* wx, int detrend, double* coef, double* S, void* stream) {
    SPEC_PREPARE_CHECKS("gd_spec_prepare");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        hipLaunchKernelGGL(spec_prepare_kernel<E>, dim3((unsigned)T), dim3(SPEC_THREADS), 0, GD_S, (const E*)x, (int)H, (int)W, mask, wy, wx,
                           detrend, coef, S);
    });
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_spec_prepare_host(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy,
                                    const double* wx, int detrend, double* coef, double* S) {
    SPEC_PREPARE_CHECKS("gd_spec_prepare_host");
    gd_with_dtype(dtype, [&](auto zero) { prepare_host((const decltype(zero)*)x, T, (int)H, (int)W, mask, wy, wx, detrend, coef, S); });
    return 0;
}

extern "C" size_t gd_spec_power_ws_bytes(long T, long H, long W, int nbins) {
    if (!spec_shape_ok(T, H, W) || nbins < 1 || nbins > GD_SPEC_MAX_BINS) return 0;
    return (size_t)T * gd_spec_tiles(W, 1) * (nbins + 1) * sizeof(double);
}

extern "C" size_t gd_spec_cross_ws_bytes(long T, long H, long W, int nbins) {
    if (!spec_shape_ok(T, H, W) || nbins < 1 || nbins > GD_SPEC_MAX_BINS) return 0;
    return (size_t)T * gd_spec_tiles(W, 2) * 4 * (nbins + 1) * sizeof(double);
}

#define SPEC_POWER_CHECKS(fn)                                                                                             \
    GD_CHECK_ARG(x && coef && S && twid_h && twid_w && bin && power && dropped, fn ": null pointer");                    \
    SPEC_SHAPE_CHECKS(fn);                                                                                                \
    GD_CHECK_ARG(nbins >= 1 && nbins <= GD_SPEC_MAX_BINS, fn ": nbins outside 1..GD_SPEC_MAX_BINS");                      \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(wy, 8) && gd_aligned(wx, 8) && gd_aligned(coef, 8) && gd_aligned(S, 8) && \
                     gd_aligned(twid_h, 8) && gd_aligned(twid_w, 8) && gd_aligned(bin, 4) && gd_aligned(power, 8) &&      \
                     gd_aligned(dropped, 8) && gd_aligned(p2d, 8),                                                        \
                 fn ": pointer not element aligned")

extern "C" int gd_spec_power(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy, const double* wx,
                             const double* coef, const double* S, const double* twid_h, const double* twid_w, const int* bin, int nbins,
                             double* power, double* dropped, double* p2d, void* ws, size_t ws_bytes, void* stream) {
    SPEC_POWER_CHECKS("gd_spec_power");
    GD_CHECK_ARG(ws && gd_aligned(ws, 8) && ws_bytes >= gd_spec_power_ws_bytes(T, H, W, nbins),
                 "gd_spec_power: workspace missing, misaligned or too small");
    const SpecField f{x, coef, S};
    const int rc = gd_with_dtype(dtype, [&](auto zero) {
        return dft_launch<decltype(zero), 1>(f, f, (int)T, (int)H, (int)W, mask, wy, wx, twid_h, twid_w, bin, nbins, p2d, (double*)ws, GD_S);
    });
    if (rc) return rc;
    GD_LAUNCH_CHECK();
    hipLaunchKernelGGL(spec_reduce_kernel<1>, dim3(gd_cdiv(T * (nbins + 1), 256)), dim3(256), 0, GD_S, (const double*)ws, (int)T,
                       (int)gd_spec_tiles(W, 1), nbins, (double)H * (double)W, S, S, power, dropped);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_spec_power_host(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy,
                                  const double* wx, const double* coef, const double* S, const double* twid_h, const double* twid_w,
                                  const int* bin, int nbins, double* power, double* dropped, double* p2d) {
    SPEC_POWER_CHECKS("gd_spec_power_host");
    gd_with_dtype(dtype, [&](auto zero) {
        power_host((const decltype(zero)*)x, T, (int)H, (int)W, mask, wy, wx, coef, S, twid_h, twid_w, bin, nbins, power, dropped, p2d);
    });
    return 0;
}

#define SPEC_CROSS_CHECKS(fn)                                                                                                   \
    GD_CHECK_ARG(xa && xb && coef_a && S_a && coef_b && S_b && twid_h && twid_w && bin && out && dropped, fn ": null pointer"); \
    SPEC_SHAPE_CHECKS(fn);                                                                                                      \
    GD_CHECK_ARG(nbins >= 1 && nbins <= GD_SPEC_MAX_BINS, fn ": nbins outside 1..GD_SPEC_MAX_BINS");                            \
    GD_CHECK_ARG(gd_elem_aligned(xa, dtype) && gd_elem_aligned(xb, dtype) && gd_aligned(wy, 8) && gd_aligned(wx, 8) &&          \
                     gd_aligned(coef_a, 8) && gd_aligned(S_a, 8) && gd_aligned(coef_b, 8) && gd_aligned(S_b, 8) &&              \
                     gd_aligned(twid_h, 8) && gd_aligned(twid_w, 8) && gd_aligned(bin, 4) && gd_aligned(out, 8) &&              \
                     gd_aligned(dropped, 8),                                                                                    \
                 fn ": pointer not element aligned")

extern "C" int gd_spec_cross(const void* xa, const void* xb, int dtype, long T, long H, long W, const unsigned char* mask, const double* wy,
                             const double* wx, const double* coef_a, const double* S_a, const double* coef_b, const double* S_b,
                             const double* twid_h, const double* twid_w, const int* bin, int nbins, double* out, double* dropped, void* ws,
                             size_t ws_bytes, void* stream) {
    SPEC_CROSS_CHECKS("gd_spec_cross");
    GD_CHECK_ARG(ws && gd_aligned(ws, 8) && ws_bytes >= gd_spec_cross_ws_bytes(T, H, W, nbins),
                 "gd_spec_cross: workspace missing, misaligned or too small");
    const SpecField fa{xa, coef_a, S_a}, fb{xb, coef_b, S_b};
    const int rc = gd_with_dtype(dtype, [&](auto zero) {
        return dft_launch<decltype(zero), 2>(fa, fb, (int)T, (int)H, (int)W, mask, wy, wx, twid_h, twid_w, bin, nbins, nullptr, (double*)ws, GD_S);
    });
    if (rc) return rc;
    GD_LAUNCH_CHECK();
    hipLaunchKernelGGL(spec_reduce_kernel<4>, dim3(gd_cdiv(T * 4 * (nbins + 1), 256)), dim3(256), 0, GD_S, (const double*)ws, (int)T,
                       (int)gd_spec_tiles(W, 2), nbins, (double)H * (double)W, S_a, S_b, out, dropped);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_spec_cross_host(const void* xa, const void* xb, int dtype, long T, long H, long W, const unsigned char* mask,
                                  const double* wy, const double* wx, const double* coef_a, const double* S_a, const double* coef_b,
                                  const double* S_b, const double* twid_h, const double* twid_w, const int* bin, int nbins, double* out,
                                  double* dropped) {
    SPEC_CROSS_CHECKS("gd_spec_cross_host");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        cross_host((const E*)xa, (const E*)xb, T, (int)H, (int)W, mask, wy, wx, coef_a, S_a, coef_b, S_b, twid_h, twid_w, bin, nbins, out, dropped);
    });
    return 0;
}
