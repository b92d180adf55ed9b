// sgp_train.hip - one training step of the BO loop's sparse GP (bayesian_optimization/sparse_gp_theano_internal.py:
// getContributionToEnergy and its gradient; `SparseGP.energy` + backward of dagnn_amd/sgp.py): the energy of a minibatch and
// the six parameter gradients in float64, by the analytic adjoints of the whitened form.  No autograd graph,
// no float atomic: every sum has one fixed order, two calls on the same inputs are bitwise equal.
//
// Kernels:
//   st_prep       exp() of the log parameters, zeroed scalars.
//   st_kern_fwd   k(rows, z) from the differences, [rows, M] (+ jitter on the diagonal for rows = z).
//   st_potrf_diag one 64 x 64 diagonal block per matrix in LDS: its Cholesky factor, the factor's inverse, sum log diag.  A pivot
//                 that is not positive (or NaN) becomes NaN and bumps the failure counter; no trip count depends on data.
//   st_gemm       C = alpha op(A) op(B) + beta C on v_mfma_f64_16x16x4_f64, 32 x 32 tiles (a 16 x 16 tile per wave), operands addressed by two strides
//                 each (NN / NT / TN are choices of strides), batched over blockIdx.z = (matrix, diagonal block pair).  The
//                 blocked factorisation (panel, trailing update), the factor's inverse (block pairs merged level by level: 64,
//                 128, 256) and every M x M x M / M x M x b product of the step run on it.
//   st_gemv       the matrix-vector products (t, alpha, beta, rho, d mParamPost).
//   st_rows       per minibatch row: v, mean, the log-likelihood term and their adjoints back to U.
//   st_elem       the element-wise steps between products (S_c and S_1, A's adjoint, tril, Phi).
//   st_kern_bwd   K and its adjoint contracted into d z and per-inducing-row partials of d lls, d lsf; no [rows, M, d] array.
//   st_final      the partials added in ascending order: E, d lls, d lsf, d lvar_noise.
#include "common.h"

#include <math.h>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int ST_MAX_M = DAGNN_SGP_MAX_M;
constexpr int ST_MAX_D = DAGNN_SGP_MAX_D;
constexpr int64_t ST_MAX_B = int64_t(1) << 24;
constexpr int NB = 64;                      // the factorisation's block
constexpr int GT = 32, GK = 32, GP = GT + 4; // the product's tile, k step and LDS pitch
constexpr int RW_COLS = 64;                 // minibatch rows of one st_rows workgroup
constexpr double ST_JITTER = 1e-3;

// scalar slots of the workspace (doubles)
enum { SC_SF = 0, SC_NOISE, SC_LOGD_K, SC_LOGD_C, SC_LOGD_1, SC_COUNT = 8 };

struct StLayout {   // offsets in doubles
    int64_t sc, il, L, W, L2, W2, zero_end;   // [L .. zero_end) is cleared per call
    int64_t Kzz, S, C, A, S2, Si2, Tmp, Ab, X1, Lb, Y, Z, Kb;
    int64_t t, ab, rho, tb;                   // vectors; ab = [alpha; beta], pitch Mv
    int64_t Kx, U, R, Ub, Rs, KxbT, dmean, part, Plls, Plsf;
    int64_t total, Mv;
};

inline int64_t al8(int64_t x) { return (x + 7) & ~int64_t(7); }

StLayout st_layout(int M, int d, int64_t b) {
    StLayout o;
    const int64_t MM = al8((int64_t)M * M), MB = al8((int64_t)M * b), Mv = al8(M);
    int64_t p = 0;
    auto take = [&](int64_t n) { int64_t r = p; p += al8(n); return r; };
    o.Mv = Mv;
    o.sc = take(SC_COUNT); o.il = take(d);
    o.L = take(MM); o.W = take(MM); o.L2 = take(2 * MM); o.W2 = take(2 * MM); o.zero_end = p;
    o.Kzz = take(MM); o.S = take(MM); o.C = take(MM); o.A = take(MM); o.S2 = take(2 * MM); o.Si2 = take(2 * MM);
    o.Tmp = take(2 * MM); o.Ab = take(MM); o.X1 = take(MM); o.Lb = take(MM); o.Y = take(MM); o.Z = take(MM); o.Kb = take(MM);
    o.t = take(Mv); o.ab = take(2 * Mv); o.rho = take(Mv); o.tb = take(Mv);
    o.Kx = take(MB); o.U = take(MB); o.R = take(MB); o.Ub = take(MB); o.Rs = take(MB); o.KxbT = take(MB);
    o.dmean = take(b); o.part = take(4 * ((b + RW_COLS - 1) / RW_COLS));
    o.Plls = take((int64_t)M * d); o.Plsf = take(Mv);
    o.total = p;
    return o;
}

// ---------------------------------------------------------------------------------------------- small kernels
__global__ void st_prep_kernel(const double* __restrict__ lls, const double* __restrict__ lsf, const double* __restrict__ lvn, int d,
                               double* __restrict__ il, double* __restrict__ sc) {
    const int t = threadIdx.x;
    if (t < d) il[t] = exp(-lls[t]);
    if (t == 0) { sc[SC_SF] = exp(lsf[0]); sc[SC_NOISE] = exp(lvn[0]); }
    if (t >= SC_LOGD_K && t < SC_COUNT) sc[t] = 0.0;
}

// out[r, m] = sf exp(-1/2 sum_c (x_rc - z_mc)^2 il_c) (+ jitter sf at r == m); out2 (may be NULL) receives a copy
__global__ void __launch_bounds__(256) st_kern_fwd_kernel(const double* __restrict__ x, int64_t ld_x, int64_t rows,
                                                          const double* __restrict__ z, int M, int d, const double* __restrict__ il,
                                                          const double* __restrict__ sc, int jitter, double* __restrict__ out,
                                                          double* __restrict__ out2) {
    const int m = blockIdx.y * 64 + (threadIdx.x & 63);
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M || r >= rows) return;
    const double* __restrict__ xr = x + r * ld_x;
    const double* __restrict__ zm = z + (int64_t)m * d;
    double acc = 0.0;
    for (int c = 0; c < d; ++c) {
        const double df = xr[c] - zm[c];
        acc = fma(df * il[c], df, acc);
    }
    const double sf = sc[SC_SF];
    double k = sf * exp(-0.5 * acc);
    if (jitter && r == m) k += ST_JITTER * sf;
    out[r * M + m] = k;
    if (out2) out2[r * M + m] = k;
}

// the element-wise steps, one thread per entry (i, j) of an M x M matrix
enum { EL_S = 0, EL_ABAR, EL_TRIL, EL_PHI };
struct ElemArgs {
    int mode, M;
    int64_t b, Mv;
    double c;
    const double* A;      // EL_S: A;  EL_ABAR: Sci (S1i at + MMs)
    int64_t MMs;
    double* out;          // EL_S: S2 (S_c, then S_1 at + MMs);  EL_ABAR: T3 in, Abar out;  EL_TRIL: Lb;  EL_PHI: Y
    const double* ab;     // [alpha; beta]
    const double* rho;
    double* tb;           // EL_ABAR: t_bar out;  EL_TRIL: t_bar in
    const double* mP;
};

__global__ void __launch_bounds__(256) st_elem_kernel(ElemArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int M = a.M;
    if (e >= (int64_t)M * M) return;
    const int i = (int)(e / M), j = (int)(e - (int64_t)i * M);
    const double c = a.c, bb = (double)a.b;
    if (a.mode == EL_S) {
        const double v = a.A[e], one = i == j ? 1.0 : 0.0;
        a.out[e] = one + c * v;
        a.out[a.MMs + e] = one + v;
    } else if (a.mode == EL_ABAR) {
        const double* __restrict__ al = a.ab;
        const double* __restrict__ be = a.ab + a.Mv;
        const double sc_ = -0.5 * bb * a.A[e] - 0.5 * bb * c * c * (al[i] * al[j]) - a.out[e] -
                           0.5 * c * (a.rho[i] * al[j] + al[i] * a.rho[j]);
        a.out[e] = c * sc_ + 0.5 * c * bb * (a.A[a.MMs + e] + be[i] * be[j]);
        if (j == 0) a.tb[i] = bb * c * c * al[i] + c * a.rho[i] - c * bb * be[i];
    } else if (a.mode == EL_TRIL) {
        a.out[e] = j <= i ? a.out[e] + a.mP[i] * a.tb[j] : 0.0;
    } else {
        const double v = a.out[e];
        a.out[e] = j < i ? v : (j == i ? 0.5 * v : 0.0);
    }
}

// ---------------------------------------------------------------------------------------------- the diagonal block
// Block j0 .. j0 + nb of the matrix blockIdx.x (S + z MMs): L_jj into L, L_jj^-1 into W (both with a zero upper triangle),
// sum log diag L_jj added to logd[z] (launches of one call follow each other on the stream: a plain read-modify-write).
__global__ void __launch_bounds__(256) st_potrf_diag_kernel(const double* __restrict__ S, double* __restrict__ L, double* __restrict__ W,
                                                            int64_t MMs, int M, int j0, double* __restrict__ logd,
                                                            unsigned* __restrict__ fail) {
    __shared__ double a[NB][NB + 1];   // below the diagonal: the factor; above it, transposed, its inverse: w(i, j) = a[j][i + 1]
    __shared__ double dg[NB];          // the factor's diagonal
    __shared__ double colraw[2][NB];   // the step's column as its owners hold it
    __shared__ unsigned nbad;
    const int tid = threadIdx.x;
    const int64_t zo = (int64_t)blockIdx.x * MMs;
    S += zo; L += zo; W += zo;
    const int nb = min(NB, M - j0);
    if (tid == 0) nbad = 0u;
    for (int e = tid; e < NB * NB; e += 256) {   // the lower triangle, mirrored; past the end: the identity
        const int i = e >> 6, j = e & 63;
        const int hi = max(i, j), lo = min(i, j);
        a[i][j] = hi < nb ? S[(int64_t)(j0 + hi) * M + j0 + lo] : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    {   // right-looking, a column per step.  Thread (i, q) keeps the entries j = q, q + 4, ... of row i in registers; per step
        // the owners of column k publish it (two buffers in turn: one barrier per step), everyone takes the pivot and its
        // own entries of the column from there: a_ij -= (a_ik / a_kk) a_jk, and the owner keeps l_ik = a_ik / sqrt(a_kk)
        const int i = tid >> 2, q = tid & 3;
        double r[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) r[t] = a[i][q + 4 * t];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            double* __restrict__ col = colraw[k & 1];
            if (q == (k & 3)) col[i] = r[k >> 2];
            __syncthreads();
            const double dkk = col[k], ri = col[i];
            const bool bad = !(dkk > 0.0);
            const double lkk = bad ? __builtin_nan("") : sqrt(dkk);
            const double f = ri * (bad ? __builtin_nan("") : 1.0 / dkk);
            if (q == (k & 3)) {
                if (i > k) r[k >> 2] = ri / lkk;
                else if (i == k) { r[k >> 2] = lkk; dg[k] = lkk; if (bad) atomicAdd(&nbad, 1u); }
            }
#pragma unroll
            for (int t = (k + 1) >> 2; t < 16; ++t) {
                const int j = q + 4 * t;
                const double cj = col[j];
                if (j > k && j <= i) r[t] = fma(-f, cj, r[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < 16; ++t)
            if (q + 4 * t <= i) a[i][q + 4 * t] = r[t];
    }
    __syncthreads();
    {   // column j of the inverse by forward substitution (rows above j are zero); the four lanes of a column split the
        // dot product (k = j + q, j + q + 4, ...) and add their parts as (0 + 1) + (2 + 3)
        const int j = tid >> 2, q = tid & 3;
        for (int i = j; i < NB; ++i) {
            double x[16], y[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {   // (all loads first: one LDS round trip per row, not one per term)
                const int k = min(j + q + 4 * t, NB - 1);
                x[t] = a[i][k];
                y[t] = a[j][k + 1];
            }
            double p = 0.0;
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (j + q + 4 * t < i) p = fma(x[t], y[t], p);
            p += __shfl_xor(p, 1, 64);
            p += __shfl_xor(p, 2, 64);
            if (q == 0) a[j][i + 1] = ((i == j ? 1.0 : 0.0) - p) / dg[i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the column's lanes share a wave: its LDS traffic is ordered
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    __syncthreads();
    for (int e = tid; e < NB * NB; e += 256) {
        const int i = e >> 6, j = e & 63;
        if (i < nb && j < nb) {
            const int64_t o = (int64_t)(j0 + i) * M + j0 + j;
            L[o] = j < i ? a[i][j] : (j == i ? dg[i] : 0.0);
            W[o] = j <= i ? a[j][i + 1] : 0.0;
        }
    }
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < nb; ++i) s += log(dg[i]);
        logd[blockIdx.x] += s;
        if (nbad) atomicAdd(fail, nbad);
    }
}

// ---------------------------------------------------------------------------------------------- the product
struct GemmArgs {
    const double* A; int64_t a_rs, a_ks;   // A(i, k) = A[i a_rs + k a_ks]
    const double* B; int64_t b_ks, b_cs;   // B(k, j) = B[k b_ks + j b_cs]
    double* C; int64_t ldc;                // C(i, j) = C[i ldc + j]
    int m, n, k;
    double alpha, beta;
    int np;                                // blockIdx.z = matrix * np + pair
    int64_t a_zs, b_zs, c_zs;              // per matrix
    int64_t a_ps, b_ps, c_ps;              // per pair
    int clip, clip_total, clip_step;       // rem = clip_total - pair * clip_step;  bit 0: m = min(m, rem), bit 1: k = min(k, rem)
};

__global__ void __launch_bounds__(256) st_gemm_kernel(GemmArgs g) {
    __shared__ double As[GK][GP];
    __shared__ double Bs[GK][GP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int zm = blockIdx.z / g.np, zp = blockIdx.z - zm * g.np;
    int m = g.m, k = g.k;
    const int n = g.n;
    if (g.clip) {
        const int rem = g.clip_total - zp * g.clip_step;
        if (g.clip & 1) m = min(m, rem);
        if (g.clip & 2) k = min(k, rem);
    }
    const int i0 = blockIdx.y * GT, j0 = blockIdx.x * GT;
    if (i0 >= m || j0 >= n) return;   // (uniform per workgroup)
    const double* __restrict__ A = g.A + zm * g.a_zs + zp * g.a_ps;
    const double* __restrict__ B = g.B + zm * g.b_zs + zp * g.b_ps;
    double* __restrict__ C = g.C + zm * g.c_zs + zp * g.c_ps;
    const bool a_kfast = g.a_ks == 1, b_cfast = g.b_cs == 1;
    const int wr = (wave >> 1) * 16, wc = (wave & 1) * 16;   // a wave owns one 16 x 16 tile: M = 500 gives 1024 waves, one per SIMD
    const int fr = lane & 15, fk = lane >> 4;
    f64x4 acc;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = 0.0;

    // a thread's 4 + 4 values of the next k step travel in registers while the matrix cores work on this one
    double ra[4], rb[4];
    int ar[4], ak[4], bc[4], bk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q;
        ar[q] = a_kfast ? e >> 5 : e & 31; ak[q] = a_kfast ? e & 31 : e >> 5;
        bc[q] = b_cfast ? e & 31 : e >> 5; bk[q] = b_cfast ? e >> 5 : e & 31;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        ra[q] = (i0 + ar[q] < m && ak[q] < k) ? A[(int64_t)(i0 + ar[q]) * g.a_rs + (int64_t)ak[q] * g.a_ks] : 0.0;
        rb[q] = (j0 + bc[q] < n && bk[q] < k) ? B[(int64_t)bk[q] * g.b_ks + (int64_t)(j0 + bc[q]) * g.b_cs] : 0.0;
    }
    for (int k0 = 0; k0 < k; k0 += GK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { As[ak[q]][ar[q]] = ra[q]; Bs[bk[q]][bc[q]] = rb[q]; }
        __syncthreads();
        const int k1 = k0 + GK;
        if (k1 < k) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ra[q] = (i0 + ar[q] < m && k1 + ak[q] < k) ? A[(int64_t)(i0 + ar[q]) * g.a_rs + (int64_t)(k1 + ak[q]) * g.a_ks] : 0.0;
                rb[q] = (j0 + bc[q] < n && k1 + bk[q] < k) ? B[(int64_t)(k1 + bk[q]) * g.b_ks + (int64_t)(j0 + bc[q]) * g.b_cs] : 0.0;
            }
        }
#pragma unroll
        for (int kk = 0; kk < GK; kk += 4)   // A / B fragment: lane & 15 -> row / column, lane >> 4 -> k
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[kk + fk][wr + fr], Bs[kk + fk][wc + fr], acc, 0, 0, 0);
        __syncthreads();
    }
    // C / D of the f64 16 x 16 MFMA: col = lane & 15, row = (lane >> 4) + 4 e
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = i0 + wr + fk + 4 * e, j = j0 + wc + fr;
        if (i < m && j < n) {
            double* __restrict__ cp = C + (int64_t)i * g.ldc + j;
            double v = g.alpha * acc[e];
            if (g.beta != 0.0) v = fma(g.beta, *cp, v);
            *cp = v;
        }
    }
}

// y = alpha op(A) x for the matrix blockIdx.y (A + z a_zs, y + z y_zs), A(i, k) = A[i rs + k ks].  ks == 1 (rows contiguous): a wave
// per row, lane l adds k = l, l + 64, ..., then the butterfly; otherwise (rs == 1) a lane per row, the four waves split k
// (k = w, w + 4, ...) and are added as ((0 + 1) + 2) + 3.
__global__ void __launch_bounds__(256) st_gemv_kernel(const double* __restrict__ A, int64_t rs, int64_t ks, int64_t a_zs,
                                                      const double* __restrict__ x, double* __restrict__ y, int64_t y_zs, int m, int k,
                                                      double alpha) {
    __shared__ double red[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    A += blockIdx.y * a_zs;
    y += blockIdx.y * y_zs;
    if (ks == 1) {
        const int i = blockIdx.x * 4 + wave;
        if (i >= m) return;   // (uniform per wave; no barrier on this path)
        const double* __restrict__ row = A + (int64_t)i * rs;
        double s = 0.0;
        for (int q = lane; q < k; q += 64) s = fma(row[q], x[q], s);
        s = wave_sum(s);
        if (lane == 0) y[i] = alpha * s;
    } else {
        const int i = blockIdx.x * 64 + lane;
        double s = 0.0;
        if (i < m)
            for (int q = wave; q < k; q += 4) s = fma(A[(int64_t)i * rs + (int64_t)q * ks], x[q], s);
        red[wave][lane] = s;
        __syncthreads();
        if (wave == 0 && i < m) y[i] = alpha * (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
    }
}

// ---------------------------------------------------------------------------------------------- the minibatch rows
// Column i of U, R [M, b]: v = sf - |U_i|^2 + U_i . R_i, mean = c alpha . U_i, out = |v| + noise, the log-likelihood term and
//   d_out = -1/2 / out + 1/2 r^2 / out^2,  d_v = d_out sign(v),  d_mean = r / out,
//   Ub_i = 2 (R_i - U_i) d_v + c alpha d_mean,   Rs_i = R_i d_v.
// A workgroup owns 64 columns; the M terms of a column are added by four threads (m = s, s + 4, ...), combined as
// ((0 + 1) + 2) + 3; part[blockIdx.x] = {sum ll, sum d_out, sum d_v} over its columns in ascending order.
__global__ void __launch_bounds__(256) st_rows_kernel(const double* __restrict__ U, const double* __restrict__ R, int M, int64_t b,
                                                      const double* __restrict__ alpha, const double* __restrict__ y, double c,
                                                      const double* __restrict__ sc, double* __restrict__ Ub, double* __restrict__ Rs,
                                                      double* __restrict__ dmean, double* __restrict__ part) {
    __shared__ double red[3][4][RW_COLS];
    __shared__ double col[3][RW_COLS];   // d_v, d_mean, then {ll, d_out, d_v} for the sums
    __shared__ double sums[3][RW_COLS];
    const int tid = threadIdx.x, ci = tid & 63, s = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * RW_COLS + ci;
    const bool live = i < b;
    double uu = 0.0, ur = 0.0, ua = 0.0;
    if (live)
        for (int m = s; m < M; m += 4) {
            const double u = U[(int64_t)m * b + i], r = R[(int64_t)m * b + i];
            uu = fma(u, u, uu);
            ur = fma(u, r, ur);
            ua = fma(alpha[m], u, ua);
        }
    red[0][s][ci] = uu; red[1][s][ci] = ur; red[2][s][ci] = ua;
    __syncthreads();
    if (s == 0) {
        double ll = 0.0, d_out = 0.0, d_v = 0.0, d_mean = 0.0;
        if (live) {
            uu = ((red[0][0][ci] + red[0][1][ci]) + red[0][2][ci]) + red[0][3][ci];
            ur = ((red[1][0][ci] + red[1][1][ci]) + red[1][2][ci]) + red[1][3][ci];
            ua = ((red[2][0][ci] + red[2][1][ci]) + red[2][2][ci]) + red[2][3][ci];
            const double v = sc[SC_SF] - uu + ur, mean = c * ua, out = fabs(v) + sc[SC_NOISE], r = y[i] - mean;
            ll = -0.5 * log(6.283185307179586477 * out) - 0.5 * r * r / out;
            d_out = -0.5 / out + 0.5 * r * r / (out * out);
            d_v = v > 0.0 ? d_out : (v < 0.0 ? -d_out : 0.0 * d_out);
            d_mean = r / out;
            dmean[i] = d_mean;
        }
        col[0][ci] = d_v; col[1][ci] = d_mean;
        sums[0][ci] = ll; sums[1][ci] = d_out; sums[2][ci] = d_v;
    }
    __syncthreads();
    if (tid < 3) {
        double t = 0.0;
        for (int q = 0; q < RW_COLS; ++q) t += sums[tid][q];
        part[(int64_t)blockIdx.x * 4 + tid] = t;
    }
    if (live) {
        const double d_v = col[0][ci], cdm = c * col[1][ci];
        for (int m = s; m < M; m += 4) {
            const int64_t o = (int64_t)m * b + i;
            const double u = U[o], r = R[o];
            Ub[o] = fma(2.0 * (r - u), d_v, alpha[m] * cdm);
            Rs[o] = r * d_v;
        }
    }
}

// ---------------------------------------------------------------------------------------------- the kernel's adjoint
// Workgroup m: with gx_r = KxbT[m, r] Kx[r, m] over the b minibatch rows and gz_r = (Kb[r, m] + Kb[m, r]) Kzz[r, m] over the M
// inducing rows,
//   g_z[m, c] = il_c (sum_r gx_r (x_rc - z_mc) + sum_r gz_r (z_rc - z_mc)),
//   Plls[m, c] = sum_r gx_r (x_rc - z_mc)^2 + 1/2 sum_r gz_r (z_rc - z_mc)^2,      Plsf[m] = sum_r gx_r + 1/2 sum_r gz_r.
// Thread (c, s): the rows r = s, s + S, ... (S = 256 / d), first the minibatch, then z; the S partials are added in ascending s.
__global__ void __launch_bounds__(256) st_kern_bwd_kernel(const double* __restrict__ X, int64_t ld_x, int64_t b,
                                                          const double* __restrict__ z, int M, int d, const double* __restrict__ il,
                                                          const double* __restrict__ Kx, const double* __restrict__ KxbT,
                                                          const double* __restrict__ Kzz, const double* __restrict__ Kb,
                                                          double* __restrict__ g_z, double* __restrict__ Plls,
                                                          double* __restrict__ Plsf) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x, m = blockIdx.x;
    const int S = 256 / d;
    const int c = tid % d, s = tid / d;
    double az = 0.0, al = 0.0, as = 0.0;
    if (s < S) {
        const double zc = z[(int64_t)m * d + c];
        for (int64_t r = s; r < b; r += S) {
            const double g = KxbT[(int64_t)m * b + r] * Kx[r * M + m];
            const double df = X[r * ld_x + c] - zc;
            az = fma(g, df, az);
            al = fma(g * df, df, al);
            as += g;
        }
        for (int r = s; r < M; r += S) {
            const double g = (Kb[(int64_t)r * M + m] + Kb[(int64_t)m * M + r]) * Kzz[(int64_t)r * M + m];
            const double df = z[(int64_t)r * d + c] - zc;
            az = fma(g, df, az);
            al = fma(0.5 * g * df, df, al);
            as = fma(0.5, g, as);
        }
    }
    red[0][tid] = az; red[1][tid] = al; red[2][tid] = as;
    __syncthreads();
    if (tid < d) {
        double tz = 0.0, tl = 0.0;
        for (int q = 0; q < S; ++q) { tz += red[0][q * d + tid]; tl += red[1][q * d + tid]; }
        g_z[(int64_t)m * d + tid] = il[tid] * tz;
        Plls[(int64_t)m * d + tid] = tl;
    }
    if (tid == 255) {   // (the threads with c = 0 hold the same sum as every other c)
        double ts = 0.0;
        for (int q = 0; q < S; ++q) ts += red[2][q * d];
        Plsf[m] = ts;
    }
}

// One workgroup: every remaining sum, each in one fixed order.
//   E = b G + sum ll,   G = -logd_c + 1/2 c^2 t . alpha - c (-logd_1 + 1/2 t . beta)
//   g_lls[c] = 1/2 il_c sum_m Plls[m, c],   g_lsf = sum_m Plsf[m] + sf sum d_v,   g_noise = noise sum d_out
__global__ void __launch_bounds__(256) st_final_kernel(int M, int d, int64_t b, int64_t nparts, double c, const double* __restrict__ sc,
                                                       const double* __restrict__ il, const double* __restrict__ t,
                                                       const double* __restrict__ ab, int64_t Mv, const double* __restrict__ part,
                                                       const double* __restrict__ Plls, const double* __restrict__ Plsf,
                                                       double* __restrict__ E, double* __restrict__ g_lls, double* __restrict__ g_lsf,
                                                       double* __restrict__ g_noise) {
    __shared__ double sh[6];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {   // thread (c, s): m = s, s + S, ...; the S parts in ascending s
        const int S = 256 / d, c = tid % d, s_ = tid / d;
        double s = 0.0;
        if (s_ < S)
            for (int m = s_; m < M; m += S) s += Plls[(int64_t)m * d + c];
        red[tid] = s;
        __syncthreads();
        if (tid < d) {
            double tl = 0.0;
            for (int q = 0; q < S; ++q) tl += red[q * d + tid];
            g_lls[tid] = 0.5 * il[tid] * tl;
        }
    }
    // a wave per sum: lane l adds the terms l, l + 64, ..., then the butterfly
    if (wave < 2) {          // t . alpha, t . beta
        const double* __restrict__ v = ab + wave * Mv;
        double s = 0.0;
        for (int m = lane; m < M; m += 64) s = fma(t[m], v[m], s);
        s = wave_sum(s);
        if (lane == 0) sh[wave] = s;
    } else if (wave == 2) {  // sum ll, sum d_out, sum d_v
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int64_t q = lane; q < nparts; q += 64) { s0 += part[q * 4]; s1 += part[q * 4 + 1]; s2 += part[q * 4 + 2]; }
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) { sh[2] = s0; sh[3] = s1; sh[4] = s2; }
    } else {
        double s = 0.0;
        for (int m = lane; m < M; m += 64) s += Plsf[m];
        s = wave_sum(s);
        if (lane == 0) sh[5] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const double G = -sc[SC_LOGD_C] + 0.5 * c * c * sh[0] - c * (-sc[SC_LOGD_1] + 0.5 * sh[1]);
        E[0] = (double)b * G + sh[2];
        g_noise[0] = sc[SC_NOISE] * sh[3];
        g_lsf[0] = sh[5] + sc[SC_SF] * sh[4];
    }
}

// ---------------------------------------------------------------------------------------------- host side
int gemm(hipStream_t st, const GemmArgs& g, int nz) {
    if (g.m <= 0 || g.n <= 0 || nz <= 0) return DAGNN_OK;
    hipLaunchKernelGGL(st_gemm_kernel, dim3((unsigned)((g.n + GT - 1) / GT), (unsigned)((g.m + GT - 1) / GT), (unsigned)nz), dim3(256), 0, st, g);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

GemmArgs mk(const double* A, int64_t a_rs, int64_t a_ks, const double* B, int64_t b_ks, int64_t b_cs, double* C, int64_t ldc, int m, int n,
            int k, double alpha = 1.0, double beta = 0.0) {
    GemmArgs g;
    g.A = A; g.a_rs = a_rs; g.a_ks = a_ks; g.B = B; g.b_ks = b_ks; g.b_cs = b_cs; g.C = C; g.ldc = ldc;
    g.m = m; g.n = n; g.k = k; g.alpha = alpha; g.beta = beta;
    g.np = 1; g.a_zs = g.b_zs = g.c_zs = 0; g.a_ps = g.b_ps = g.c_ps = 0; g.clip = 0; g.clip_total = 0; g.clip_step = 0;
    return g;
}

// nmat matrices S (+ z MMs; destroyed) -> L = chol(S), W = L^-1 (both pre-zeroed), logd[z] += sum log diag L.  Right-looking
// over 64-column panels: diagonal block, panel L_ij = S_ij W_jj^T, trailing S -= P P^T; then the inverse's off-diagonal blocks
// by merging diagonal block pairs, [[A, 0], [B, C]]^-1 = [[A^-1, 0], [-C^-1 B A^-1, C^-1]], at block sizes 64, 128, 256.
int factor(hipStream_t st, double* S, double* L, double* W, double* Tmp, int64_t MMs, int nmat, int M, double* logd, unsigned* fail) {
    const int64_t ld = M;
    for (int j0 = 0; j0 < M; j0 += NB) {
        const int nb = M - j0 < NB ? M - j0 : NB, rem = M - j0 - nb;
        hipLaunchKernelGGL(st_potrf_diag_kernel, dim3((unsigned)nmat), dim3(256), 0, st, S, L, W, MMs, M, j0, logd, fail);
        DAGNN_CHECK_LAUNCH();
        if (rem <= 0) break;
        double* P = L + (int64_t)(j0 + nb) * ld + j0;
        GemmArgs g = mk(S + (int64_t)(j0 + nb) * ld + j0, ld, 1, W + (int64_t)j0 * (ld + 1), 1, ld, P, ld, rem, nb, nb);
        g.a_zs = g.b_zs = g.c_zs = MMs;
        int rc = gemm(st, g, nmat);
        if (rc != DAGNN_OK) return rc;
        g = mk(P, ld, 1, P, 1, ld, S + (int64_t)(j0 + nb) * (ld + 1), ld, rem, rem, nb, -1.0, 1.0);
        g.a_zs = g.b_zs = g.c_zs = MMs;
        rc = gemm(st, g, nmat);
        if (rc != DAGNN_OK) return rc;
    }
    for (int bs = NB; bs < M; bs *= 2) {
        const int np = (M - bs + 2 * bs - 1) / (2 * bs);
        const int64_t ps = (int64_t)2 * bs * (ld + 1);
        GemmArgs g = mk(L + (int64_t)bs * ld, ld, 1, W, ld, 1, Tmp + (int64_t)bs * ld, ld, bs, bs, bs);   // T = B A^-1
        g.np = np; g.a_zs = g.b_zs = g.c_zs = MMs; g.a_ps = g.b_ps = g.c_ps = ps;
        g.clip = 1; g.clip_total = M - bs; g.clip_step = 2 * bs;
        int rc = gemm(st, g, nmat * np);
        if (rc != DAGNN_OK) return rc;
        g = mk(W + (int64_t)bs * (ld + 1), ld, 1, Tmp + (int64_t)bs * ld, ld, 1, W + (int64_t)bs * ld, ld, bs, bs, bs, -1.0, 0.0);   // -C^-1 T
        g.np = np; g.a_zs = g.b_zs = g.c_zs = MMs; g.a_ps = g.b_ps = g.c_ps = ps;
        g.clip = 3; g.clip_total = M - bs; g.clip_step = 2 * bs;
        rc = gemm(st, g, nmat * np);
        if (rc != DAGNN_OK) return rc;
    }
    return DAGNN_OK;
}

int gemv(hipStream_t st, const double* A, int64_t rs, int64_t ks, int64_t a_zs, const double* x, double* y, int64_t y_zs, int m, int k, int nz,
         double alpha = 1.0) {
    const int rows = ks == 1 ? 4 : 64;
    hipLaunchKernelGGL(st_gemv_kernel, dim3((unsigned)((m + rows - 1) / rows), (unsigned)nz), dim3(256), 0, st, A, rs, ks, a_zs, x, y, y_zs, m, k, alpha);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

int elem(hipStream_t st, const ElemArgs& a) {
    const int64_t n = (int64_t)a.M * a.M;
    hipLaunchKernelGGL(st_elem_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

}  // namespace

#define ST_TRY(x)                      \
    do {                               \
        const int rc_ = (x);           \
        if (rc_ != DAGNN_OK) return rc_; \
    } while (0)

extern "C" size_t dagnn_sgp_energy_grad_bytes(int M, int d, int64_t b) {
    if (M < 1 || M > ST_MAX_M || d < 1 || d > ST_MAX_D || b < 1 || b > ST_MAX_B) return 0;
    return (size_t)st_layout(M, d, b).total * sizeof(double);
}

extern "C" int dagnn_sgp_energy_grad(const double* X, int64_t ld_x, const double* y, int64_t b, int M, int d, double n_points,
                                     const double* lls, const double* lsf, const double* z, const double* mP, const double* Lp,
                                     const double* lvar_noise, double* E, double* g_lls, double* g_lsf, double* g_z, double* g_m,
                                     double* g_Lp, double* g_noise, void* work, size_t work_bytes, unsigned* fail, void* stream) {
    if (M < 1 || M > ST_MAX_M || d < 1 || d > ST_MAX_D || b < 1 || b > ST_MAX_B || ld_x < d || !(n_points >= 1.0))
        return DAGNN_EINVAL;
    if (!X || !y || !lls || !lsf || !z || !mP || !Lp || !lvar_noise || !E || !g_lls || !g_lsf || !g_z || !g_m || !g_Lp || !g_noise ||
        !work || ((uintptr_t)work & 7) || !fail)
        return DAGNN_EINVAL;
    const StLayout o = st_layout(M, d, b);
    if (work_bytes < (size_t)o.total * sizeof(double)) return DAGNN_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    double* w = reinterpret_cast<double*>(work);
    const int64_t MMs = al8((int64_t)M * M), ld = M, Mv = o.Mv;
    const int bi = (int)b;
    const double c = (n_points - 1.0) / n_points;
    double *sc = w + o.sc, *il = w + o.il, *L = w + o.L, *W = w + o.W, *L2 = w + o.L2, *W2 = w + o.W2, *Kzz = w + o.Kzz, *S = w + o.S;
    double *C = w + o.C, *A = w + o.A, *S2 = w + o.S2, *Si2 = w + o.Si2, *Tmp = w + o.Tmp, *Ab = w + o.Ab, *X1 = w + o.X1, *Lb = w + o.Lb;
    double *Y = w + o.Y, *Z = w + o.Z, *Kb = w + o.Kb, *t = w + o.t, *ab = w + o.ab, *rho = w + o.rho, *tb = w + o.tb, *Kx = w + o.Kx;
    double *U = w + o.U, *R = w + o.R, *Ub = w + o.Ub, *Rs = w + o.Rs, *KxbT = w + o.KxbT, *dmean = w + o.dmean, *part = w + o.part;
    double *Plls = w + o.Plls, *Plsf = w + o.Plsf;

    hipError_t he = hipMemsetAsync(L, 0, (size_t)(o.zero_end - o.L) * sizeof(double), st);
    if (he != hipSuccess) return DAGNN_EHIP(he);
    hipLaunchKernelGGL(st_prep_kernel, dim3(1), dim3(128), 0, st, lls, lsf, lvar_noise, d, il, sc);
    DAGNN_CHECK_LAUNCH();
    // Kzz = L L^T, W = L^-1
    hipLaunchKernelGGL(st_kern_fwd_kernel, dim3((unsigned)((M + 3) / 4), (unsigned)((M + 63) / 64)), dim3(256), 0, st, z, (int64_t)d,
                       (int64_t)M, z, M, d, il, sc, 1, Kzz, S);
    DAGNN_CHECK_LAUNCH();
    ST_TRY(factor(st, S, L, W, Tmp, MMs, 1, M, sc + SC_LOGD_K, fail));
    // C = Lp^T L, A = C^T C, S_c = I + c A, S_1 = I + A and their factors
    ST_TRY(gemm(st, mk(Lp, 1, ld, L, ld, 1, C, ld, M, M, M), 1));
    ST_TRY(gemm(st, mk(C, 1, ld, C, ld, 1, A, ld, M, M, M), 1));
    ElemArgs ea;
    ea.mode = EL_S; ea.M = M; ea.b = b; ea.Mv = Mv; ea.c = c; ea.A = A; ea.MMs = MMs; ea.out = S2; ea.ab = ab; ea.rho = rho; ea.tb = tb; ea.mP = mP;
    ST_TRY(elem(st, ea));
    ST_TRY(factor(st, S2, L2, W2, Tmp, MMs, 2, M, sc + SC_LOGD_C, fail));
    {   // S_c^-1 = Wc^T Wc, S_1^-1 = W1^T W1
        GemmArgs g = mk(W2, 1, ld, W2, ld, 1, Si2, ld, M, M, M);
        g.a_zs = g.b_zs = g.c_zs = MMs;
        ST_TRY(gemm(st, g, 2));
    }
    // t = L^T m, alpha = S_c^-1 t, beta = S_1^-1 t
    ST_TRY(gemv(st, L, 1, ld, 0, mP, t, 0, M, M, 1));
    ST_TRY(gemv(st, Si2, ld, 1, MMs, t, ab, Mv, M, M, 2));
    // the data side: Kx = k(X, z), U = W Kx^T, R = S_c^-1 U, the rows
    hipLaunchKernelGGL(st_kern_fwd_kernel, dim3((unsigned)((b + 3) / 4), (unsigned)((M + 63) / 64)), dim3(256), 0, st, X, ld_x, b, z, M, d,
                       il, sc, 0, Kx, (double*)nullptr);
    DAGNN_CHECK_LAUNCH();
    ST_TRY(gemm(st, mk(W, ld, 1, Kx, 1, ld, U, b, M, bi, M), 1));
    ST_TRY(gemm(st, mk(Si2, ld, 1, U, b, 1, R, b, M, bi, M), 1));
    const int64_t nparts = (b + RW_COLS - 1) / RW_COLS;
    hipLaunchKernelGGL(st_rows_kernel, dim3((unsigned)nparts), dim3(256), 0, st, U, R, M, b, ab, y, c, sc, Ub, Rs, dmean, part);
    DAGNN_CHECK_LAUNCH();
    // rho = R d_mean, T3 = Rs R^T, then A's adjoint and t's
    ST_TRY(gemv(st, R, b, 1, 0, dmean, rho, 0, M, bi, 1));
    ST_TRY(gemm(st, mk(Rs, b, 1, R, 1, b, Ab, ld, M, M, bi), 1));
    ea.mode = EL_ABAR; ea.A = Si2; ea.out = Ab;
    ST_TRY(elem(st, ea));
    // X1 = C Abar, g_Lp = 2 L X1^T, g_m = L t_bar
    ST_TRY(gemm(st, mk(C, ld, 1, Ab, ld, 1, X1, ld, M, M, M), 1));
    ST_TRY(gemm(st, mk(L, ld, 1, X1, 1, ld, g_Lp, ld, M, M, M, 2.0), 1));
    ST_TRY(gemv(st, L, ld, 1, 0, tb, g_m, 0, M, M, 1));
    // KxbT = W^T Ub, L_bar = tril(2 Lp X1 - KxbT U^T + m t_bar^T)
    ST_TRY(gemm(st, mk(W, 1, ld, Ub, b, 1, KxbT, b, M, bi, M), 1));
    ST_TRY(gemm(st, mk(Lp, ld, 1, X1, ld, 1, Lb, ld, M, M, M, 2.0), 1));
    ST_TRY(gemm(st, mk(KxbT, b, 1, U, 1, b, Lb, ld, M, M, bi, -1.0, 1.0), 1));
    ea.mode = EL_TRIL; ea.out = Lb;
    ST_TRY(elem(st, ea));
    // the Cholesky adjoint: Kb = W^T Phi(L^T L_bar) W
    ST_TRY(gemm(st, mk(L, 1, ld, Lb, ld, 1, Y, ld, M, M, M), 1));
    ea.mode = EL_PHI; ea.out = Y;
    ST_TRY(elem(st, ea));
    ST_TRY(gemm(st, mk(Y, ld, 1, W, ld, 1, Z, ld, M, M, M), 1));
    ST_TRY(gemm(st, mk(W, 1, ld, Z, ld, 1, Kb, ld, M, M, M), 1));
    hipLaunchKernelGGL(st_kern_bwd_kernel, dim3((unsigned)M), dim3(256), 0, st, X, ld_x, b, z, M, d, il, Kx, KxbT, Kzz, Kb, g_z, Plls, Plsf);
    DAGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(st_final_kernel, dim3(1), dim3(256), 0, st, M, d, b, nparts, c, sc, il, t, ab, Mv, part, Plls, Plsf, E, g_lls, g_lsf,
                       g_noise);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
