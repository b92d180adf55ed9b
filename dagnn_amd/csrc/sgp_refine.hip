// sgp_refine.hip - the refinement of the sparse GP's greedy EI proposals on the device (bayesian_optimization/sparse_gp.py:24-43,
// `global_optimization`: after the grid, L-BFGS-B from the best grid row; sparse_gp_theano_internal.py: compute_log_ei,
// compute_log_averaged_ei and their gradients).
//
// Reference path replaced: one scipy L-BFGS-B run per greedy step, a chain of 20 to 40 dependent evaluations of a Theano
// graph, each two (M + j)^2 matrix-vector products on the host.  Here S <= 32 starts advance in lock-step, so that an
// evaluation of all of them is a float64 tile product, and the optimiser itself (a projected L-BFGS with 8 curvature pairs and
// a halving Armijo search: the state machine of `refine_host` in dagnn_amd/sgp.py, which is its definition) runs on the device
// too: the host enqueues max_evals ticks without looking at the device.
//
// A tick, with K [Me, 32] the kernel columns of the S trial points (column pitch 32, columns from S on are never read back):
//   rf_gemm_kernel   U = T K           (T = G for the posterior, T = W_e lower triangular for the averaged EI: tri skips the
//   rf_gemm_kernel   C = T^T U          tiles above the diagonal; the incumbent's mean needs neither)
//   rf_tick_kernel   a workgroup per start: mean, |U|^2, d mean / dx, d v / dx by fixed-order sums over m, f and its gradient,
//                    one transition of the state machine (wave 0), then the column of K of the next trial point.
// Kernel boundaries are the only synchronisation: no ticket, no spinning, no floating-point atomic.
//
// Layouts.  gemm: 256 threads own one 16 x 16 output tile; the k range is split in four contiguous quarters, a wave each, on
// v_mfma_f64_16x16x4_f64 (A / B: lane & 15 -> row / column, lane >> 4 -> k; C / D: col = lane & 15, row = (lane >> 4) + 4 e),
// added as ((0 + 1) + 2) + 3.  The tick's workgroup has 1024 threads: the sums over m are short chains of loads, and 16 waves
// cut the chain where more workgroups would need another launch.  Sums over m: thread t adds m = t, t + 1024, ... in order,
// the 64 lanes of a wave as a butterfly, the 16 waves in ascending order; the gradient vectors: lane l owns the coordinates
// l and l + 64, wave w adds m = w, w + 16, ..., the waves as before.  Sums over d in the kernel column run in ascending order in one thread; those of the
// state machine are lane l's two coordinates, then the butterfly - one fixed order, so two runs are bitwise equal.
#include "common.h"

#include <math.h>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int RF_THREADS = 1024;                               // per start: 16 waves split the sums over m (latency, not work, is the cost)
constexpr int RF_WAVES = RF_THREADS / 64;
constexpr int RF_GEMM_THREADS = 256;
constexpr int RF_SP = 32;                                      // column pitch of K, U, C
constexpr int RF_H = DAGNN_SGP_REFINE_HISTORY;
constexpr int RF_MAX_S = DAGNN_SGP_REFINE_MAX_STARTS;
constexpr int RF_MAX_D = DAGNN_SGP_MAX_D;
constexpr int RF_MAX_ME = DAGNN_SGP_MAX_M + DAGNN_SGP_MAX_Q;
constexpr int RF_MAX_HALVINGS = 20;
constexpr int RF_HDR = 16;                                     // per start: f, t, y.y of the newest pair, -, s.y per slot [8]
constexpr int RF_INTS = 8;                                     // per start: status, evaluations, halvings, pairs, oldest slot
enum { RI_STATUS = 0, RI_EVALS = 1, RI_HALV = 2, RI_NHIST = 3, RI_HEAD = 4 };
enum { RH_F = 0, RH_T = 1, RH_YY = 2, RH_SY = 4 };

static_assert(RF_SP >= RF_MAX_S && RF_MAX_D <= 128 && RF_H == 8, "the lane maps below assume these");

struct RfLayout { int64_t K, U, C, st, ist, stride, total; };   // in doubles
__host__ __device__ inline RfLayout rf_layout(int Me, int d, int S) {
    RfLayout L;
    L.K = 0;
    L.U = (int64_t)Me * RF_SP;
    L.C = 2 * (int64_t)Me * RF_SP;
    L.st = 3 * (int64_t)Me * RF_SP;
    L.stride = RF_HDR + (int64_t)(4 + 2 * RF_H) * d;            // x, g, p, xt, s [8], y [8]
    L.ist = L.st + (int64_t)S * L.stride;
    L.total = L.ist + (int64_t)S * RF_INTS / 2;
    return L;
}

struct RfOps {
    int mode, S, d, M, Me;
    const double *ze, *zet, *inv_ls, *a, *lo, *up;   // zet [d, ld_zt]: ze transposed (zet[c * ld_zt + m] = ze[m][c])
    int64_t ld_zt;
    double sf, inc;
    double *K, *U, *C, *st;
    int* ist;
    int64_t stride;
};

struct RfShared {
    double x[RF_MAX_D], il[RF_MAX_D], dm[RF_MAX_D], dv[RF_MAX_D], g[RF_MAX_D];
    double part[RF_WAVES][2][RF_MAX_D];
    double red[RF_WAVES][2];
    double sc[4];   // mean, v, f
};

__device__ __forceinline__ double rf_wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double rf_wmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double rf_clip(double v, double lo, double up) { return v < lo ? lo : (v > up ? up : v); }   // (NaN stays NaN)

// column s of K at the point sh.x: thread t owns m = t, t + 1024, ... (zet: a wave reads 64 consecutive m); the sum over d in
// ascending order
__device__ __forceinline__ void rf_kcol(const RfOps& o, int s, const RfShared& sh, int tid) {
    for (int m = tid; m < o.Me; m += RF_THREADS) {
        const double* __restrict__ zc = o.zet + m;
        double acc = 0.0;
#pragma unroll 8
        for (int c = 0; c < o.d; ++c) {
            const double df = sh.x[c] - zc[(int64_t)c * o.ld_zt];
            acc = fma(df * sh.il[c], df, acc);
        }
        o.K[(int64_t)m * RF_SP + s] = o.sf * exp(-0.5 * acc);
    }
}

// (-log EI, d / d mean, d / d v) of the branch expression of dagnn_sgp_ei_step; mode MEAN: (mean, 1, 0)
__device__ __forceinline__ void rf_objective(int mode, double mean, double v, double inc, double& f, double& fm, double& fv) {
    if (mode == DAGNN_SGP_REFINE_MEAN) { f = mean; fm = 1.0; fv = 0.0; return; }
    fm = 0.0; fv = 0.0;
    if (!(v > 0.0)) { f = __builtin_nan(""); return; }
    const double sd = sqrt(v), u = inc - mean, s = u / sd;
    double rho, drho;
    if (s < -10.0) {
        const double s2 = s * s, s3 = s2 * s, s4 = s2 * s2, s5 = s3 * s2, s6 = s3 * s3, s7 = s5 * s2, s8 = s4 * s4;
        rho = -(1.0 / s - 1.0 / s3 + 3.0 / s5 - 15.0 / s7);
        drho = 1.0 / s2 - 3.0 / s4 + 15.0 / s6 - 105.0 / s8;
    } else {
        const double phi = exp(-0.5 * s * s) * 0.39894228040143267794;
        if (phi == 0.0) { f = -__builtin_inf(); return; }   // (s beyond 38: the formula's own overflow)
        rho = 0.5 * erfc(-s * 0.70710678118654752440) / phi;
        drho = 1.0 + s * rho;
    }
    const double h = u * rho + sd;
    if (!(h > 0.0)) { f = __builtin_nan(""); return; }
    const double gs = (rho + s * drho) / (s * rho + 1.0) - s;
    f = -(log(h) - 0.91893853320467274178 - 0.5 * s * s);
    fm = gs / sd;
    fv = -(1.0 - gs * s) / (2.0 * v);
}

// the sums over m of column s at the point sh.x: sh.sc = {mean, v, f}, sh.dm, sh.dv (d mean / dx, d v / dx), sh.g (d f / dx)
__device__ __forceinline__ void rf_reduce(const RfOps& o, int s, RfShared& sh, int tid) {
    const int lane = tid & 63, wave = tid >> 6, d = o.d;
    const bool ei = o.mode == DAGNN_SGP_REFINE_EI;
    double pm = 0.0, pn = 0.0;
    for (int m = tid; m < o.Me; m += RF_THREADS) {
        if (m < o.M) pm = fma(o.a[m], o.K[(int64_t)m * RF_SP + s], pm);
        if (ei) {
            const double u = o.U[(int64_t)m * RF_SP + s];
            pn = fma(u, u, pn);
        }
    }
    pm = rf_wsum(pm);
    pn = rf_wsum(pn);
    if (lane == 0) { sh.red[wave][0] = pm; sh.red[wave][1] = pn; }
    const int c0 = lane, c1 = lane + 64;
    const bool in0 = c0 < d, in1 = c1 < d;
    const double x0 = in0 ? sh.x[c0] : 0.0, x1 = in1 ? sh.x[c1] : 0.0;
    const double l0 = in0 ? sh.il[c0] : 0.0, l1 = in1 ? sh.il[c1] : 0.0;
    double am0 = 0.0, am1 = 0.0, av0 = 0.0, av1 = 0.0;
    for (int mb = wave; mb < o.Me; mb += 4 * RF_WAVES) {   // four m in flight: the loads of a turn are issued before its sums
        double kv[4], z0[4], z1[4], am[4], cm[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int m = mb + u * RF_WAVES;
            const bool ok = m < o.Me;
            const int64_t mc = ok ? m : o.Me - 1;
            kv[u] = ok ? o.K[mc * RF_SP + s] : 0.0;
            z0[u] = in0 ? o.ze[mc * d + c0] : 0.0;
            z1[u] = in1 ? o.ze[mc * d + c1] : 0.0;
            am[u] = m < o.M ? o.a[mc] : 0.0;
            cm[u] = (ei && ok) ? o.C[mc * RF_SP + s] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // (a term past the end is an exact zero: kv = am = cm = 0)
            const double dk0 = -kv[u] * (x0 - z0[u]) * l0, dk1 = -kv[u] * (x1 - z1[u]) * l1;
            am0 = fma(am[u], dk0, am0); am1 = fma(am[u], dk1, am1);
            av0 = fma(cm[u], dk0, av0); av1 = fma(cm[u], dk1, av1);
        }
    }
    sh.part[wave][0][c0] = am0; sh.part[wave][0][c1] = am1;
    sh.part[wave][1][c0] = av0; sh.part[wave][1][c1] = av1;
    __syncthreads();
    if (tid == 0) {
        double mean = sh.red[0][0], nu = sh.red[0][1];
        for (int w = 1; w < RF_WAVES; ++w) { mean += sh.red[w][0]; nu += sh.red[w][1]; }
        double f, fm, fv;
        const double v = o.sf - nu;
        rf_objective(o.mode, mean, v, o.inc, f, fm, fv);
        sh.sc[0] = mean; sh.sc[1] = v; sh.sc[2] = f;
        sh.red[0][0] = fm; sh.red[0][1] = fv;
    }
    __syncthreads();
    if (tid < d) {
        double dm = sh.part[0][0][tid], dv = sh.part[0][1][tid];
        for (int w = 1; w < RF_WAVES; ++w) { dm += sh.part[w][0][tid]; dv += sh.part[w][1][tid]; }
        dv *= -2.0;
        sh.dm[tid] = dm; sh.dv[tid] = dv;
        sh.g[tid] = sh.red[0][0] * dm + sh.red[0][1] * dv;
    }
    __syncthreads();
}

// one transition of start s (wave 0; every lane holds the same scalars: the butterflies are symmetric).  ft = sh.sc[2] and
// sh.g are the objective at the trial point sh.x; on return sh.x (and the state's xt) is the point of the next evaluation.
__device__ void rf_advance(const RfOps& o, int s, RfShared& sh, int lane) {
    const int d = o.d;
    double* __restrict__ st = o.st + (int64_t)s * o.stride;
    int* __restrict__ is = o.ist + (int64_t)s * RF_INTS;
    double* X = st + RF_HDR; double* G = X + d; double* P = G + d; double* XT = P + d; double* SH = XT + d; double* YH = SH + (int64_t)RF_H * d;
    const int c0 = lane, c1 = lane + 64;
    const bool in0 = c0 < d, in1 = c1 < d;
#define RF_LD(p, v0, v1) const double v0 = in0 ? (p)[c0] : 0.0, v1 = in1 ? (p)[c1] : 0.0
#define RF_ST(p, v0, v1) do { if (in0) (p)[c0] = (v0); if (in1) (p)[c1] = (v1); } while (0)
#define RF_DOT(a0, a1, b0, b1) rf_wsum(fma((a1), (b1), (a0) * (b0)))
    int status = is[RI_STATUS];
    double x0 = in0 ? X[c0] : 0.0, x1 = in1 ? X[c1] : 0.0;
    if (status != DAGNN_SGP_REFINE_RUNNING) {   // a stopped start evaluates its accepted point again; the result is discarded
        if (status != DAGNN_SGP_REFINE_DEAD) { RF_ST(sh.x, x0, x1); }
        return;
    }
    RF_LD(o.lo, lo0, lo1);
    RF_LD(o.up, up0, up1);
    RF_LD(sh.x, xt0, xt1);
    RF_LD(sh.g, gt0, gt1);
    double g0 = in0 ? G[c0] : 0.0, g1 = in1 ? G[c1] : 0.0;
    const double ft = sh.sc[2];
    double f = st[RH_F], t = st[RH_T], yy = st[RH_YY];
    double sy[RF_H];
#pragma unroll
    for (int i = 0; i < RF_H; ++i) sy[i] = st[RH_SY + i];
    int nh = is[RI_NHIST], head = is[RI_HEAD], halv = is[RI_HALV];
    const int evals = is[RI_EVALS] + 1;
    const bool finite = __builtin_isfinite(ft);
    bool took = false;
    double nx0 = 0.0, nx1 = 0.0;   // the next trial point
    bool moved = false;
    if (evals == 1) {
        if (!finite) status = DAGNN_SGP_REFINE_DEAD;
        else { x0 = xt0; x1 = xt1; g0 = gt0; g1 = gt1; f = ft; took = true; }
    } else {
        const double s0 = xt0 - x0, s1 = xt1 - x1;
        const double gd = RF_DOT(g0, g1, s0, s1);
        if (finite && ft <= f + 1e-4 * gd) {
            const double y0 = gt0 - g0, y1 = gt1 - g1;
            const double sdy = RF_DOT(s0, s1, y0, y1), ss = RF_DOT(s0, s1, s0, s1), yn = RF_DOT(y0, y1, y0, y1);
            if (sdy > 1e-10 * sqrt(ss) * sqrt(yn)) {
                int slot;
                if (nh < RF_H) { slot = (head + nh) & (RF_H - 1); ++nh; }
                else { slot = head; head = (head + 1) & (RF_H - 1); }
                RF_ST(SH + (int64_t)slot * d, s0, s1);
                RF_ST(YH + (int64_t)slot * d, y0, y1);
#pragma unroll
                for (int i = 0; i < RF_H; ++i) if (i == slot) sy[i] = sdy;
                yy = yn;
            }
            if (f - ft <= 2.2e-9 * fmax(fmax(fabs(f), fabs(ft)), 1.0)) status = DAGNN_SGP_REFINE_CONVERGED;
            x0 = xt0; x1 = xt1; g0 = gt0; g1 = gt1; f = ft; took = true;
        } else if (halv >= RF_MAX_HALVINGS) {
            status = DAGNN_SGP_REFINE_STALLED;
        } else {
            ++halv;
            t *= 0.5;
            RF_LD(P, p0, p1);
            nx0 = rf_clip(x0 + t * p0, lo0, up0); nx1 = rf_clip(x1 + t * p1, lo1, up1);
            moved = true;
        }
    }
    if (took) {
        RF_ST(X, x0, x1);
        RF_ST(G, g0, g1);
    }
    if (took && status == DAGNN_SGP_REFINE_RUNNING) {
        const double pg = rf_wmax(fmax(fabs(x0 - rf_clip(x0 - g0, lo0, up0)), fabs(x1 - rf_clip(x1 - g1, lo1, up1))));
        if (pg <= 1e-5) {
            status = DAGNN_SGP_REFINE_CONVERGED;
        } else {
            const bool fr0 = !((x0 <= lo0 && g0 > 0.0) || (x0 >= up0 && g0 < 0.0));
            const bool fr1 = !((x1 <= lo1 && g1 > 0.0) || (x1 >= up1 && g1 < 0.0));
            double q0 = fr0 ? g0 : 0.0, q1 = fr1 ? g1 : 0.0;
            // the pairs, oldest first, all loads in flight at once (a lane reads what it wrote: its own two coordinates)
            double hs0[RF_H], hs1[RF_H], hy0[RF_H], hy1[RF_H], hsy[RF_H], alpha[RF_H];
#pragma unroll
            for (int i = 0; i < RF_H; ++i) {
                const int slot = (head + i) & (RF_H - 1);
                const bool on = i < nh;
                hs0[i] = (on && in0) ? SH[(int64_t)slot * d + c0] : 0.0; hs1[i] = (on && in1) ? SH[(int64_t)slot * d + c1] : 0.0;
                hy0[i] = (on && in0) ? YH[(int64_t)slot * d + c0] : 0.0; hy1[i] = (on && in1) ? YH[(int64_t)slot * d + c1] : 0.0;
                double sys = 1.0;
#pragma unroll
                for (int k = 0; k < RF_H; ++k) if (on && k == slot) sys = sy[k];
                hsy[i] = sys;
            }
#pragma unroll
            for (int i = RF_H - 1; i >= 0; --i) {   // newest to oldest
                alpha[i] = 0.0;
                if (i < nh) {
                    alpha[i] = RF_DOT(hs0[i], hs1[i], q0, q1) / hsy[i];
                    q0 -= alpha[i] * hy0[i]; q1 -= alpha[i] * hy1[i];
                }
            }
            double gamma = 1.0;
#pragma unroll
            for (int i = 0; i < RF_H; ++i) if (i == nh - 1) gamma = hsy[i] / yy;
            double r0 = gamma * q0, r1 = gamma * q1;
#pragma unroll
            for (int i = 0; i < RF_H; ++i) {        // oldest to newest
                if (i < nh) {
                    const double beta = RF_DOT(hy0[i], hy1[i], r0, r1) / hsy[i];
                    r0 += hs0[i] * (alpha[i] - beta); r1 += hs1[i] * (alpha[i] - beta);
                }
            }
            double p0 = fr0 ? -r0 : 0.0, p1 = fr1 ? -r1 : 0.0;
            const double gp = RF_DOT(g0, g1, p0, p1);
            if (!(gp < 0.0)) {
                nh = 0; head = 0;
                p0 = fr0 ? -g0 : 0.0; p1 = fr1 ? -g1 : 0.0;
            }
            t = nh > 0 ? 1.0 : fmin(1.0, 1.0 / sqrt(RF_DOT(p0, p1, p0, p1)));
            halv = 0;
            RF_ST(P, p0, p1);
            nx0 = rf_clip(x0 + t * p0, lo0, up0); nx1 = rf_clip(x1 + t * p1, lo1, up1);
            moved = true;
        }
    }
    if (status != DAGNN_SGP_REFINE_RUNNING && status != DAGNN_SGP_REFINE_DEAD) { nx0 = x0; nx1 = x1; moved = true; }
    if (moved) {
        RF_ST(XT, nx0, nx1);
        RF_ST(sh.x, nx0, nx1);
    }
    if (lane == 0) {
        st[RH_F] = f; st[RH_T] = t; st[RH_YY] = yy;
#pragma unroll
        for (int i = 0; i < RF_H; ++i) st[RH_SY + i] = sy[i];
        is[RI_STATUS] = status; is[RI_EVALS] = evals; is[RI_HALV] = halv; is[RI_NHIST] = nh; is[RI_HEAD] = head;
    }
#undef RF_LD
#undef RF_ST
#undef RF_DOT
}

__device__ __forceinline__ void rf_load_il(const RfOps& o, RfShared& sh, int tid) {
    if (tid < o.d) sh.il[tid] = o.inv_ls[tid];
}

// ---------------------------------------------------------------------------------------------- one evaluation
__global__ void __launch_bounds__(RF_THREADS) rf_kern_kernel(RfOps o, const double* __restrict__ X) {
    __shared__ RfShared sh;
    const int tid = threadIdx.x, s = blockIdx.x;
    rf_load_il(o, sh, tid);
    if (tid < o.d) sh.x[tid] = X[(int64_t)s * o.d + tid];
    __syncthreads();
    rf_kcol(o, s, sh, tid);
}

__global__ void __launch_bounds__(RF_THREADS) rf_reduce_kernel(RfOps o, const double* __restrict__ X, double* __restrict__ out) {
    __shared__ RfShared sh;
    const int tid = threadIdx.x, s = blockIdx.x, d = o.d;
    rf_load_il(o, sh, tid);
    if (tid < d) sh.x[tid] = X[(int64_t)s * d + tid];
    __syncthreads();
    rf_reduce(o, s, sh, tid);
    double* __restrict__ row = out + (int64_t)s * (4 + 2 * d);
    if (tid == 0) { row[0] = sh.sc[2]; row[1] = sh.sc[0]; row[2] = sh.sc[1]; row[3] = 0.0; }
    if (tid < d) { row[4 + tid] = sh.dm[tid]; row[4 + d + tid] = sh.dv[tid]; }
}

// ---------------------------------------------------------------------------------------------- the run
__global__ void __launch_bounds__(RF_THREADS) rf_init_kernel(RfOps o, const double* __restrict__ X0, const int* __restrict__ nstart) {
    __shared__ RfShared sh;
    const int tid = threadIdx.x, s = blockIdx.x, d = o.d;
    double* __restrict__ st = o.st + (int64_t)s * o.stride;
    rf_load_il(o, sh, tid);
    for (int i = tid; i < o.stride; i += RF_THREADS) {
        double v = 0.0;
        const int c = i - (RF_HDR + 3 * d);   // xt = clip(x0)
        if (c >= 0 && c < d) { v = rf_clip(X0[(int64_t)s * d + c], o.lo[c], o.up[c]); sh.x[c] = v; }
        st[i] = v;
    }
    if (tid < RF_INTS) {
        const int live = nstart ? nstart[0] : o.S;
        o.ist[(int64_t)s * RF_INTS + tid] = (tid == RI_STATUS && s >= live) ? DAGNN_SGP_REFINE_DEAD : 0;
    }
    __syncthreads();
    rf_kcol(o, s, sh, tid);
}

__global__ void __launch_bounds__(RF_THREADS) rf_tick_kernel(RfOps o) {
    __shared__ RfShared sh;
    const int tid = threadIdx.x, s = blockIdx.x, d = o.d;
    rf_load_il(o, sh, tid);
    if (tid < d) sh.x[tid] = o.st[(int64_t)s * o.stride + RF_HDR + 3 * d + tid];
    __syncthreads();
    rf_reduce(o, s, sh, tid);
    if (tid < 64) rf_advance(o, s, sh, tid);
    __syncthreads();
    rf_kcol(o, s, sh, tid);
}

// out: best start, its f, its x [d], status [S], evaluations [S], f [S]; xs (may be NULL) [S, d]: every start's accepted point
// (NaN for a dead start); a start still running is out of ticks
__global__ void __launch_bounds__(128) rf_finish_kernel(RfOps o, double* __restrict__ out, double* __restrict__ xs) {
    __shared__ int best_s;
    const int tid = threadIdx.x, d = o.d, S = o.S;
    if (tid == 0) {
        int best = -1;
        double fb = 0.0;
        for (int s = 0; s < S; ++s) {
            const int status = o.ist[(int64_t)s * RF_INTS + RI_STATUS];
            const double f = o.st[(int64_t)s * o.stride + RH_F];
            if (status != DAGNN_SGP_REFINE_DEAD && __builtin_isfinite(f) && (best < 0 || f < fb)) { best = s; fb = f; }
        }
        best_s = best;
        out[0] = (double)best;
        out[1] = best >= 0 ? fb : __builtin_nan("");
    }
    __syncthreads();
    const int best = best_s;
    if (tid < d) out[2 + tid] = best >= 0 ? o.st[(int64_t)best * o.stride + RF_HDR + tid] : 0.0;
    if (tid < S) {
        int status = o.ist[(int64_t)tid * RF_INTS + RI_STATUS];
        if (status == DAGNN_SGP_REFINE_RUNNING) status = DAGNN_SGP_REFINE_BUDGET;
        out[2 + d + tid] = (double)status;
        out[2 + d + S + tid] = (double)o.ist[(int64_t)tid * RF_INTS + RI_EVALS];
        out[2 + d + 2 * S + tid] = status == DAGNN_SGP_REFINE_DEAD ? __builtin_nan("") : o.st[(int64_t)tid * o.stride + RH_F];
    }
    if (xs) {
        for (int i = tid; i < S * d; i += 128) {
            const int s = i / d, c = i - s * d;
            xs[i] = o.ist[(int64_t)s * RF_INTS + RI_STATUS] == DAGNN_SGP_REFINE_DEAD ? __builtin_nan("")
                                                                                    : o.st[(int64_t)s * o.stride + RF_HDR + c];
        }
    }
}

// ---------------------------------------------------------------------------------------------- the products
// Out [Me, 32] = op(T) In [Me, 32], op = T (trans == 0) or T^T; tri: T is lower triangular, so k < i0 + 16 (k >= i0 for T^T)
__global__ void __launch_bounds__(RF_GEMM_THREADS) rf_gemm_kernel(const double* __restrict__ T, int64_t ldt, int trans, int tri, int Me,
                                                             const double* __restrict__ In, double* __restrict__ Out) {
    __shared__ double red[3][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fk = lane >> 4;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    int kb = 0, ke = Me;
    if (tri) {
        if (trans) kb = i0;
        else ke = min(Me, i0 + 16);
    }
    const int nsteps = (ke - kb + 3) >> 2, per = (nsteps + 3) >> 2;
    const int s_beg = wave * per, s_end = min(nsteps, s_beg + per);
    const int ai = i0 + fr;
    const bool aok = ai < Me;
    const int64_t aic = aok ? ai : Me - 1;
    f64x4 acc;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = 0.0;
#pragma unroll 4
    for (int q = s_beg; q < s_end; ++q) {
        const int k = kb + 4 * q + fk;
        const bool kok = k < ke;
        const int64_t kc = kok ? k : Me - 1;
        const double av = (aok && kok) ? (trans ? T[kc * ldt + aic] : T[aic * ldt + kc]) : 0.0;
        const double bv = In[kc * RF_SP + j0 + fr];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave - 1][e][lane] = acc[e];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i0 + fk + 4 * e;
            if (i < Me) Out[(int64_t)i * RF_SP + j0 + fr] = ((acc[e] + red[0][e][lane]) + red[1][e][lane]) + red[2][e][lane];
        }
    }
}

bool rf_shape_ok(int S, int d, int M, int Me) {
    return S >= 1 && S <= RF_MAX_S && d >= 1 && d <= RF_MAX_D && M >= 1 && M <= DAGNN_SGP_MAX_M && Me >= M && Me <= RF_MAX_ME;
}

int rf_make_ops(RfOps& o, int mode, int S, int d, int M, int Me, const double* ze, const double* zet, int64_t ld_zt, const double* inv_ls,
                double sf, const double* a, const double* T, int64_t ld_t, double incumbent, void* work, size_t work_bytes) {
    if (mode != DAGNN_SGP_REFINE_MEAN && mode != DAGNN_SGP_REFINE_EI) return DAGNN_EINVAL;
    if (!rf_shape_ok(S, d, M, Me) || !ze || !zet || ld_zt < Me || !inv_ls || !a || !work || ((uintptr_t)work & 7)) return DAGNN_EINVAL;
    if (mode == DAGNN_SGP_REFINE_EI && (!T || ld_t < Me)) return DAGNN_EINVAL;
    if (work_bytes < dagnn_sgp_refine_bytes(Me, d, S)) return DAGNN_ENOSPC;
    const RfLayout L = rf_layout(Me, d, S);
    double* w = reinterpret_cast<double*>(work);
    o.mode = mode; o.S = S; o.d = d; o.M = M; o.Me = Me;
    o.ze = ze; o.zet = zet; o.ld_zt = ld_zt; o.inv_ls = inv_ls; o.a = a; o.lo = nullptr; o.up = nullptr;
    o.sf = sf; o.inc = incumbent;
    o.K = w + L.K; o.U = w + L.U; o.C = w + L.C; o.st = w + L.st;
    o.ist = reinterpret_cast<int*>(w + L.ist);
    o.stride = L.stride;
    return DAGNN_OK;
}

void rf_products(const RfOps& o, const double* T, int64_t ld_t, int tri, hipStream_t stream) {
    const dim3 grid((unsigned)((o.S + 15) / 16), (unsigned)((o.Me + 15) / 16));
    hipLaunchKernelGGL(rf_gemm_kernel, grid, dim3(RF_GEMM_THREADS), 0, stream, T, ld_t, 0, tri, o.Me, (const double*)o.K, o.U);
    hipLaunchKernelGGL(rf_gemm_kernel, grid, dim3(RF_GEMM_THREADS), 0, stream, T, ld_t, 1, tri, o.Me, (const double*)o.U, o.C);
}

}  // namespace

extern "C" size_t dagnn_sgp_refine_bytes(int Me, int d, int S) {
    if (!rf_shape_ok(S, d, 1, Me)) return 0;
    return (size_t)rf_layout(Me, d, S).total * sizeof(double);
}

extern "C" int dagnn_sgp_refine_eval(int mode, int S, int d, int M, int Me, const double* X, const double* ze, const double* zet,
                                     int64_t ld_zt, const double* inv_ls, double sf, const double* a, const double* T, int64_t ld_t, int tri, double incumbent, double* out,
                                     void* work, size_t work_bytes, void* stream) {
    RfOps o;
    const int rc = rf_make_ops(o, mode, S, d, M, Me, ze, zet, ld_zt, inv_ls, sf, a, T, ld_t, incumbent, work, work_bytes);
    if (rc != DAGNN_OK) return rc;
    if (!X || !out) return DAGNN_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rf_kern_kernel, dim3((unsigned)S), dim3(RF_THREADS), 0, st, o, X);
    if (mode == DAGNN_SGP_REFINE_EI) rf_products(o, T, ld_t, tri, st);
    hipLaunchKernelGGL(rf_reduce_kernel, dim3((unsigned)S), dim3(RF_THREADS), 0, st, o, X, out);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_sgp_refine_run(int mode, int S, int d, int M, int Me, const double* X0, const int* nstart, const double* lower,
                                    const double* upper, const double* ze, const double* zet, int64_t ld_zt, const double* inv_ls,
                                    double sf, const double* a,
                                    const double* T, int64_t ld_t, int tri, double incumbent, int max_evals, double* out, double* xs,
                                    void* work, size_t work_bytes, void* stream) {
    RfOps o;
    const int rc = rf_make_ops(o, mode, S, d, M, Me, ze, zet, ld_zt, inv_ls, sf, a, T, ld_t, incumbent, work, work_bytes);
    if (rc != DAGNN_OK) return rc;
    if (!X0 || !lower || !upper || !out || max_evals < 4 || max_evals > 1024) return DAGNN_EINVAL;
    o.lo = lower; o.up = upper;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rf_init_kernel, dim3((unsigned)S), dim3(RF_THREADS), 0, st, o, X0, nstart);
    DAGNN_CHECK_LAUNCH();
    for (int tick = 0; tick < max_evals; ++tick) {
        if (mode == DAGNN_SGP_REFINE_EI) rf_products(o, T, ld_t, tri, st);
        hipLaunchKernelGGL(rf_tick_kernel, dim3((unsigned)S), dim3(RF_THREADS), 0, st, o);
    }
    hipLaunchKernelGGL(rf_finish_kernel, dim3(1), dim3(128), 0, st, o, out, xs);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
