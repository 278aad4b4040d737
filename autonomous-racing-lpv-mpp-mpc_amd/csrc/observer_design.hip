// observer_design.hip -- batched design of the estimator's vertex gains on the device (include/lpvmpc.h, "Per-vehicle state
// estimator").  One problem per (vehicle b, polytope p in {LS, HS}, vertex i in 0..15): A = A_obs at the vertex from the vehicle's
// row {lf, lr, m, Iz, Cf, Cr, mu} (Continuous_AB_Comp as obs_step writes it), the filter Riccati equation
// A P + P A^T - P C^T Ro^-1 C P + Qo = 0, and L = -P C^T Ro^-1 (observer_vertex_gains' sign: A + L C is Hurwitz).
//
// Algorithm: matrix-sign Newton iteration on the Hamiltonian Z = [[A^T, -C^T Ro^-1 C], [-Qo, -A]] (12 x 12),
// Z <- (c Z + Z^-1 / c) / 2 with the norm scaling c = sqrt(|Z^-1|_F / |Z|_F), until |dZ|_F <= 1e-13 |Z|_F (cap 40); then
// [W12; W22 + I] P = -[W11 + I; W21] of W = sign(Z) by its normal equations and a 6 x 6 Cholesky, and P symmetrised.
//
// Mapping: the matrices are far too small for the matrix cores and two of them per lane (288 doubles) would spill, so one problem
// is spread over a 16-lane group, four problems per wavefront.  Lane r < 12 of a group holds row r of Z and of the running inverse
// in registers (lanes 12..15 hold zero rows and only take part in the reductions).  The inverse is a Gauss-Jordan elimination with
// partial pivoting and no row exchange: step p takes the unused row with the largest |Z[., p]| (the lowest row on a tie), found by
// a width-16 butterfly, and that lane's row is broadcast with width-16 shuffles; the rows are put in order once at the end.  The
// Frobenius norms and the 57 sums of the normal equations are width-16 butterflies as well: a fixed order inside the group, so a
// vehicle's tables are the same words whatever the batch around it and wherever its problems land.  Every register array is
// indexed with compile-time indices (the loops are unrolled); the one lane-dependent read, A by row, goes through an LDS tile.
// No atomics.  A group whose problem index is past the end does nothing.
#include "lpvmpc_device.hpp"
#include "observer_design.hpp"

namespace lpvmpc {

namespace {

constexpr int kW = 16;                                     // lanes per problem
constexpr int kD = 12;                                     // order of the Hamiltonian

__device__ inline double grp_sum(double v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, kW);
    return v;
}

// this lane's row of Z^-1 in w from its row of Z in a (destroyed); r = the lane's row (12..15: a zero row that is never a pivot)
__device__ inline void grp_inverse(int r, double a[kD], double w[kD]) {
    bool used = r >= kD;
    int src = r;                                           // the lane that ends up with row r of the inverse
#pragma unroll
    for (int c = 0; c < kD; ++c) w[c] = r == c ? 1.0 : 0.0;
#pragma unroll
    for (int p = 0; p < kD; ++p) {
        double best = used ? -1.0 : fabs(a[p]);
        int piv = r;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best, m, kW);
            const int oi = __shfl_xor(piv, m, kW);
            const bool take = ob > best || (ob == best && oi < piv);
            best = take ? ob : best; piv = take ? oi : piv;
        }
        const bool mine = r == piv;
        const double pv = __shfl(a[p], piv, kW);
        const double f = a[p] / pv;
        // columns < p of an unused row are zero already, column p is set below
#pragma unroll
        for (int c = p + 1; c < kD; ++c) {
            const double t = __shfl(a[c], piv, kW);
            a[c] = mine ? t / pv : a[c] - f * t;
        }
#pragma unroll
        for (int c = 0; c < kD; ++c) {
            const double t = __shfl(w[c], piv, kW);
            w[c] = mine ? t / pv : w[c] - f * t;
        }
        a[p] = mine ? 1.0 : 0.0;
        used = used || mine;
        src = r == p ? piv : src;
    }
#pragma unroll
    for (int c = 0; c < kD; ++c) w[c] = __shfl(w[c], src, kW);
}

}  // namespace

// rows [B][7] (host layout); cst: ObsDesignConst; L_ls / L_hs [B][6][5][16] with (stride_b, stride_e, stride_i) words between
// vehicles, gain elements and vertices (the public layout: 480, 16, 1; the binding's [480][B] planes: 1, 16 B, B); iters [B][2][16]
// or null
__global__ void __launch_bounds__(64) observer_design_kernel(int B, const double *__restrict__ rows, const double *__restrict__ cst,
                                                             double *__restrict__ L_ls, double *__restrict__ L_hs, long long stride_b,
                                                             long long stride_e, long long stride_i, int32_t *__restrict__ iters) {
    __shared__ double As[64 / kW][36];
    const int grp = threadIdx.x / kW, r = threadIdx.x % kW;
    const long long q = (long long)blockIdx.x * (64 / kW) + grp;           // problem: ((b * 2) + poly) * 16 + vertex
    const bool live = q < (long long)B * 32;
    const int vtx = (int)(q & 15), poly = (int)((q >> 4) & 1);
    const long long b = q >> 5;
    if (live && r == 0) {
        const double *row = rows + b * kPlantWords;
        const double lf = row[0], lr = row[1], m = row[2], I = row[3], Cf = row[4], Cr = row[5], mu = row[6];
        const double *lim = cst + ObsDesignConst::kLim + poly * 12;
        const double vx = lim[0 + ((vtx >> 3) & 1)], vy = lim[2 + ((vtx >> 2) & 1)], steer = lim[6 + ((vtx >> 1) & 1)], th = lim[10 + (vtx & 1)];
        double ss, cs, sth, cth;
        sincos(steer, &ss, &cs);
        sincos(th, &sth, &cth);
        double *A = As[grp];
#pragma unroll
        for (int i = 0; i < 36; ++i) A[i] = 0.0;
        A[0] = -mu;
        A[1] = (ss * Cf) / (m * vx);
        A[2] = (ss * Cf * lf) / (m * vx) + vy;
        A[7] = -(Cr + Cf * cs) / (m * vx);
        A[8] = -(lf * Cf * cs - lr * Cr) / (m * vx) - vx;
        A[13] = -(lf * Cf * cs - lr * Cr) / (I * vx);
        A[14] = -(lf * lf * Cf * cs + lr * lr * Cr) / (I * vx);
        A[18] = cth; A[19] = -sth;
        A[24] = sth; A[25] = cth;
        A[32] = 1.0;
    }
    __syncthreads();
    if (!live) return;
    // this lane's row of Z = [[A^T, -G], [-Qo, -A]]
    double z[kD], a[kD], w[kD];
    {
        const double *A = As[grp], *Qo = cst + ObsDesignConst::kQo, *G = cst + ObsDesignConst::kG;
        const int lo = r < 6 ? r : (r < kD ? r - 6 : 0);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double top0 = A[c * 6 + lo], top1 = -G[lo * 6 + c], bot0 = -Qo[lo * 6 + c], bot1 = -A[lo * 6 + c];
            z[c] = r < 6 ? top0 : (r < kD ? bot0 : 0.0);
            z[6 + c] = r < 6 ? top1 : (r < kD ? bot1 : 0.0);
        }
    }
    int it = -1;
    for (int k = 1; k <= 40; ++k) {
        double sz = 0.0, sw = 0.0;
#pragma unroll
        for (int c = 0; c < kD; ++c) { a[c] = z[c]; sz += z[c] * z[c]; }
        grp_inverse(r, a, w);
#pragma unroll
        for (int c = 0; c < kD; ++c) sw += w[c] * w[c];
        sz = grp_sum(sz); sw = grp_sum(sw);
        const double cc = sqrt(sqrt(sw) / sqrt(sz));
        double sd = 0.0, sn = 0.0;
#pragma unroll
        for (int c = 0; c < kD; ++c) {
            const double n = 0.5 * (cc * z[c] + w[c] / cc), d = n - z[c];
            sd += d * d; sn += n * n;
            z[c] = n;
        }
        sd = grp_sum(sd); sn = grp_sum(sn);
        if (sqrt(sd) <= 1e-13 * sqrt(sn)) { it = k; break; }               // (uniform in the group; false for a NaN)
    }
    // [W12; W22 + I] P = -[W11 + I; W21]: this lane's rows of M and N, then S = M^T M (lower triangle) and T = M^T N in every lane
    double Mr[6], Nr[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        Mr[c] = z[6 + c] + (r == 6 + c ? 1.0 : 0.0);
        Nr[c] = -(z[c] + (r == c ? 1.0 : 0.0));
    }
    double S[6][6], T[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) S[i][j] = grp_sum(Mr[i] * Mr[j]);
#pragma unroll
        for (int j = 0; j < 6; ++j) T[i][j] = grp_sum(Mr[i] * Nr[j]);
    }
    // Cholesky S = C C^T in place (lower), then C C^T X = T column by column, in every lane alike
    bool ok = it > 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = S[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= S[j][k] * S[j][k];
        ok = ok && d > 0.0;
        d = sqrt(d);
        S[j][j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = S[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= S[i][k] * S[j][k];
            S[i][j] = s / d;
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double s = T[i][c];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= S[i][k] * T[k][c];
            T[i][c] = s / S[i][i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double s = T[i][c];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) s -= S[k][i] * T[k][c];
            T[i][c] = s / S[i][i];
        }
    }
    // L = -sym(P) C^T Ro^-1, element e = row * 5 + column written by lane e mod 16
    const double *K = cst + ObsDesignConst::kCtRi;                         // C^T Ro^-1 [6][5]
    double *out = (poly ? L_hs : L_ls) + b * stride_b + vtx * stride_i;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) s += (0.5 * (T[i][k] + T[k][i])) * K[k * 5 + c];
            const int e = i * 5 + c;
            if (r == (e & 15)) out[e * stride_e] = ok ? -s : nan;
        }
    if (iters && r == 0) iters[q] = ok ? it : -1;
}

hipError_t launch_observer_design(int B, const double *rows, const double *cst, double *L_ls, double *L_hs, long long stride_b,
                                  long long stride_e, long long stride_i, int32_t *iters, hipStream_t s) {
    const long long groups = (long long)B * 32, blocks = (groups + 3) / 4;
    hipLaunchKernelGGL(observer_design_kernel, dim3((unsigned)blocks), dim3(64), 0, s, B, rows, cst, L_ls, L_hs, stride_b, stride_e, stride_i, iters);
    return hipGetLastError();
}

}  // namespace lpvmpc
