// Singular spectrum analysis (include/gandanet.h, "Singular spectrum analysis"): the arithmetic of one term of a lag
// covariance, the Jacobi rotation of one pair, the update of one 2 x 2 block and of one row of the eigenvector matrix, the
// round-robin pairing, the sort and sign rule, the diagonal-average weight and the convergence test.  Shared by the device
// kernel (ssa.hip) and its host twin so both perform the same operations in the same order.  All arithmetic fp64, every
// operation rounded on its own (no contraction into FMA); nothing transcendental: division and sqrt are correctly rounded
// on both sides, so every output agrees bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// 2^-52: a rotation is skipped when |a_pq| <= GD_SSA_JTOL * (the largest |diagonal entry| of the matrix it started from)
#define GD_SSA_JTOL 2.220446049250313e-16

// ---- sums -------------------------------------------------------------------------------------------------------------------
// one product joins a running sum (the covariance term, the principal component, the anti-diagonal of a component)
__host__ __device__ inline double gd_ssa_mac(double s, double a, double b) {
#pragma clang fp contract(off)
    return s + a * b;
}
__host__ __device__ inline double gd_ssa_sq_dev(double s, double v, double mean) {
#pragma clang fp contract(off)
    const double d = v - mean;
    return s + d * d;
}
__host__ __device__ inline double gd_ssa_sd(double ss, int n) { return sqrt(ss / (double)n); }
// a sample that is neither finite nor NaN
__host__ __device__ inline bool gd_ssa_is_inf(double v) { return v == v && !(v - v == 0.0); }

// ---- round robin ------------------------------------------------------------------------------------------------------------
// Set s (0 .. np2 - 2, np2 = M rounded up to even) pairs the np2 indices off: slot 0 is (np2 - 1, s), slot k >= 1 is
// ((s + k) mod (np2 - 1), (s - k) mod (np2 - 1)).  Returned with p < q; q = -1 marks the bye of an odd M (its partner would
// be the index M, which does not exist).
__host__ __device__ inline void gd_ssa_pair(int M, int set, int slot, int* p, int* q) {
    const int np2 = (M + 1) & ~1, n1 = np2 - 1;
    int a, b;
    if (slot == 0) {
        a = set;
        b = n1;
    } else {
        a = (set + slot) % n1;
        b = (set - slot + n1) % n1;
    }
    if (a > b) {
        const int t = a;
        a = b;
        b = t;
    }
    *p = a;
    *q = b >= M ? -1 : b;
}

// ---- one rotation -----------------------------------------------------------------------------------------------------------
// J = [[c, s], [-s, c]] that annihilates a_pq of [[a_pp, a_pq], [a_pq, a_qq]] (Golub & Van Loan, symmetric Schur); t = s / c.
// |a_pq| <= thr: the identity, and `rotated` is false.
struct GdSsaRot {
    double c, s, t;
    bool rotated;
};
__host__ __device__ inline GdSsaRot gd_ssa_rotation(double app, double aqq, double apq, double thr) {
#pragma clang fp contract(off)
    GdSsaRot r;
    if (!(fabs(apq) > thr)) {
        r.c = 1.0;
        r.s = 0.0;
        r.t = 0.0;
        r.rotated = false;
        return r;
    }
    const double tau = (aqq - app) / (2.0 * apq);
    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(tau * tau + 1.0));
    r.c = 1.0 / sqrt(t * t + 1.0);
    r.s = t * r.c;
    r.t = t;
    r.rotated = true;
    return r;
}
// (x, y) <- (c x - s y, s x + c y): a column update of rows (.., p), (.., q), or a row update with the rotation of the row pair
__host__ __device__ inline void gd_ssa_rot2(double c, double s, double& x, double& y) {
#pragma clang fp contract(off)
    const double nx = c * x - s * y, ny = s * x + c * y;
    x = nx;
    y = ny;
}

// The 2 x 2 block of the row pair `a` (rows pa < qa) and the column pair `b` (columns pb < qb), slot a <= slot b, of the
// symmetric matrix A (ld = M): the column rotation of b, then the row rotation of a, in place; the mirror block receives
// copies, so A stays exactly symmetric.  A bye (q = -1) has no second row / column.  The diagonal block (a == b) takes
// a_pp - t a_pq, a_qq + t a_pq and an exact zero.
__host__ __device__ inline void gd_ssa_block(double* A, int M, bool diag, int pa, int qa, const GdSsaRot& ra, int pb, int qb, const GdSsaRot& rb) {
#pragma clang fp contract(off)
    if (diag) {
        if (qa < 0 || !ra.rotated) return;
        const double apq = A[pa * M + qa];
        A[pa * M + pa] = A[pa * M + pa] - ra.t * apq;
        A[qa * M + qa] = A[qa * M + qa] + ra.t * apq;
        A[pa * M + qa] = 0.0;
        A[qa * M + pa] = 0.0;
        return;
    }
    double x00 = A[pa * M + pb], x01 = qb >= 0 ? A[pa * M + qb] : 0.0;
    double x10 = qa >= 0 ? A[qa * M + pb] : 0.0, x11 = (qa >= 0 && qb >= 0) ? A[qa * M + qb] : 0.0;
    gd_ssa_rot2(rb.c, rb.s, x00, x01);   // columns
    gd_ssa_rot2(rb.c, rb.s, x10, x11);
    gd_ssa_rot2(ra.c, ra.s, x00, x10);   // rows
    gd_ssa_rot2(ra.c, ra.s, x01, x11);
    A[pa * M + pb] = x00;
    A[pb * M + pa] = x00;
    if (qb >= 0) {
        A[pa * M + qb] = x01;
        A[qb * M + pa] = x01;
    }
    if (qa >= 0) {
        A[qa * M + pb] = x10;
        A[pb * M + qa] = x10;
    }
    if (qa >= 0 && qb >= 0) {
        A[qa * M + qb] = x11;
        A[qb * M + qa] = x11;
    }
}
// row i of the eigenvector matrix V takes the column rotation of the pair (p, q)
__host__ __device__ inline void gd_ssa_vrow(double* V, int M, int i, int p, int q, const GdSsaRot& r) {
    if (q < 0 || !r.rotated) return;
    gd_ssa_rot2(r.c, r.s, V[i * M + p], V[i * M + q]);
}

// ---- sort and sign ------------------------------------------------------------------------------------------------------------
// the place of eigenvalue i in descending order, ties to the lower original index
__host__ __device__ inline int gd_ssa_rank(const double* A, int M, int i) {
    const double di = A[i * M + i];
    int r = 0;
    for (int j = 0; j < M; ++j) {
        const double dj = A[j * M + j];
        r += (dj > di || (dj == di && j < i)) ? 1 : 0;
    }
    return r;
}
// +1 or -1: the first entry of largest magnitude of column `col` of V becomes positive
__host__ __device__ inline double gd_ssa_sign(const double* V, int M, int col) {
    double best = -1.0, at = 0.0;
    for (int j = 0; j < M; ++j) {
        const double v = V[j * M + col], a = fabs(v);
        if (a > best) {
            best = a;
            at = v;
        }
    }
    return at < 0.0 ? -1.0 : 1.0;
}

// ---- reconstruction -----------------------------------------------------------------------------------------------------------
// the lags j of the anti-diagonal of step t: j0 <= j <= j1, j1 - j0 + 1 of them (the diagonal-average weight is 1 / that)
__host__ __device__ inline void gd_ssa_diag_range(int t, int M, int K, int* j0, int* j1) {
    *j0 = t - (K - 1) > 0 ? t - (K - 1) : 0;
    *j1 = t < M - 1 ? t : M - 1;
}
__host__ __device__ inline double gd_ssa_diag_mean(double sum, int count) { return sum / (double)count; }

// ---- the iteration --------------------------------------------------------------------------------------------------------------
// |new - old| of one gap sample joins the largest change; a NaN counts as +inf, so the result does not depend on the order
__host__ __device__ inline double gd_ssa_change(double worst, double now, double before) {
#pragma clang fp contract(off)
    double d = fabs(now - before);
    if (!(d == d)) d = (double)INFINITY;
    return d > worst ? d : worst;
}
__host__ __device__ inline bool gd_ssa_converged(double change, double tol, double sd) {
#pragma clang fp contract(off)
    return change <= tol * sd;
}
