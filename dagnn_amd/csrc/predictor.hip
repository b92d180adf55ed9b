// predictor.hip - the performance predictor of the D-VAE loop (dvae/train.py:184-191, 243-250; bayesian_optimization/bo.py:250-286).
//
// The reference hangs  Linear(nz, hs) -> Tanh -> Linear(hs, 1)  on mu and adds MSELoss(reduction='sum') against the graphs'
// scores to the loss.  Reference path replaced:
//   dagnn_predictor_mse      `y_pred = model.predictor(mu); pred = model.mseloss(y_pred, y)` and everything autograd runs
//                            behind it for an upstream gradient of 1 - d mu, d W1, d b1, d W2, d b2 - in ONE launch.
//   dagnn_predictor_forward  `model.predictor(Z)` over the rows of a latent matrix (bo.py:251, 277).
//   dagnn_fit_sums           the sums behind `Test RMSE` / `Pearson r` of bo.py:253-286, in float64.
//
// Layout.  A workgroup owns tiles of PR_ROWS rows and walks all hs units: thread t holds the units t, t + 256,
// ...; the tile of mu sits in LDS as [k][row], so a unit's row of W1 is read once per tile and meets 8 rows.  With a tile's
// rows in one workgroup y_pred, d y, d pre and d mu are complete locally; only d W1 / d b1 / d W2 / d b2 and the loss cross
// workgroups.  Each workgroup keeps its own partial of those in a slab nobody else touches (tile after tile, rows ascending)
// and draws an integer ticket; the workgroup that draws the last one adds the slabs in workgroup order.  The grid is a
// function of B alone, every sum has one fixed order, there is no float atomic: the results are bitwise repeatable.
// `pr_tile_forward` is the one definition of a row's arithmetic, used by both kernels: the same row gives the same bits in
// either, at any position of any tile.
#include "common.h"

namespace {

constexpr int PR_ROWS = DAGNN_PREDICTOR_ROWS;
constexpr int PR_THREADS = 256;
constexpr int PR_MAX_NZ = DAGNN_PREDICTOR_MAX_NZ;
constexpr int PR_MAX_HS = DAGNN_PREDICTOR_MAX_HS;
constexpr int PR_MAX_BLOCKS = 32;       // training call: slabs the last workgroup adds
constexpr int PR_FWD_MAX_BLOCKS = 2048;
constexpr int FIT_MAX_BLOCKS = 256;
static_assert(PR_ROWS == 8, "the tile is read from LDS as two float4");

struct __align__(16) PrShared {
    float mu[PR_MAX_NZ][PR_ROWS];        // the tile of mu, [k][row]; rows past the end hold 0
    float h[PR_ROWS][PR_MAX_HS];         // tanh(pre), later d pre
    float dm[PR_THREADS][PR_ROWS];       // d mu: one partial per (unit group, column)
    float red[4][PR_ROWS];
    float yp[PR_ROWS], dy[PR_ROWS], sq[PR_ROWS];
    unsigned last;
};

__device__ __forceinline__ void pr_load8(const float* p, float (&v)[PR_ROWS]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// y_pred of the rows [row0, row0 + PR_ROWS) into S.yp, tanh(pre) into S.h.  Per row and unit: two fused multiply-add chains
// over the even and the odd columns (the even one starts at b1), added once; per row: a thread's units ascending, the
// butterfly of the wave, the four waves as (0 + 1) + (2 + 3), then + b2.
__device__ __forceinline__ void pr_tile_forward(PrShared& S, const float* __restrict__ x, int64_t ld, int64_t row0, int64_t rows,
                                                int nz, int hs, const float* __restrict__ W1, const float* __restrict__ b1,
                                                const float* __restrict__ W2, const float* __restrict__ b2) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < nz * PR_ROWS; i += PR_THREADS) {
        const int r = i / nz, k = i - r * nz;
        S.mu[k][r] = row0 + r < rows ? x[(row0 + r) * ld + k] : 0.f;
    }
    __syncthreads();
    float yp[PR_ROWS];
#pragma unroll
    for (int r = 0; r < PR_ROWS; ++r) yp[r] = 0.f;
    for (int j = tid; j < hs; j += PR_THREADS) {
        const float* __restrict__ w = W1 + (int64_t)j * nz;
        float a0[PR_ROWS], a1[PR_ROWS], m[PR_ROWS];
        const float bj = b1[j];
#pragma unroll
        for (int r = 0; r < PR_ROWS; ++r) { a0[r] = bj; a1[r] = 0.f; }
        int k = 0;
        for (; k + 1 < nz; k += 2) {
            const float w0 = w[k], w1 = w[k + 1];
            pr_load8(S.mu[k], m);
#pragma unroll
            for (int r = 0; r < PR_ROWS; ++r) a0[r] = fmaf(w0, m[r], a0[r]);
            pr_load8(S.mu[k + 1], m);
#pragma unroll
            for (int r = 0; r < PR_ROWS; ++r) a1[r] = fmaf(w1, m[r], a1[r]);
        }
        if (k < nz) {
            const float w0 = w[k];
            pr_load8(S.mu[k], m);
#pragma unroll
            for (int r = 0; r < PR_ROWS; ++r) a0[r] = fmaf(w0, m[r], a0[r]);
        }
        const float w2 = W2[j];
#pragma unroll
        for (int r = 0; r < PR_ROWS; ++r) {
            const float hv = tanhf(a0[r] + a1[r]);
            S.h[r][j] = hv;
            yp[r] = fmaf(w2, hv, yp[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < PR_ROWS; ++r) {
        const float v = wave_sum(yp[r]);
        if (lane == 0) S.red[wave][r] = v;
    }
    __syncthreads();
    if (tid < PR_ROWS) S.yp[tid] = ((S.red[0][tid] + S.red[1][tid]) + (S.red[2][tid] + S.red[3][tid])) + b2[0];
    __syncthreads();
}

// slab / out layout with gradients: d W1 [hs nz], d b1 [hs], d W2 [hs], d b2, loss = P floats; without: the loss alone
__global__ void __launch_bounds__(PR_THREADS) predictor_mse_kernel(const float* __restrict__ mu, int64_t ld, const float* __restrict__ y,
                                                                   int B, int nz, int hs, const float* __restrict__ W1,
                                                                   const float* __restrict__ b1, const float* __restrict__ W2,
                                                                   const float* __restrict__ b2, float* __restrict__ y_pred,
                                                                   float* __restrict__ out, float* __restrict__ dmu,
                                                                   float* __restrict__ work, unsigned* __restrict__ counter, int grads) {
    __shared__ PrShared S;
    const int tid = threadIdx.x;
    const int64_t P = grads ? (int64_t)hs * nz + 2 * (int64_t)hs + 2 : 1;
    float* __restrict__ slab = work + (int64_t)blockIdx.x * P;
    const int tiles = (B + PR_ROWS - 1) / PR_ROWS;
    float loss_acc = 0.f, db2_acc = 0.f;   // (thread 0: tile after tile, rows ascending)
    bool first = true;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x, first = false) {
        const int row0 = t * PR_ROWS;
        pr_tile_forward(S, mu, ld, row0, B, nz, hs, W1, b1, W2, b2);
        if (tid < PR_ROWS) {
            const int row = row0 + tid;
            float d = 0.f;
            if (row < B) {
                y_pred[row] = S.yp[tid];
                d = S.yp[tid] - y[row];
            }
            S.dy[tid] = 2.0f * d;   // a row past the end: 0 - it adds nothing to any sum below
            S.sq[tid] = d * d;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int r = 0; r < PR_ROWS; ++r) { loss_acc += S.sq[r]; db2_acc += S.dy[r]; }
        }
        if (grads) {
            float dy[PR_ROWS];
#pragma unroll
            for (int r = 0; r < PR_ROWS; ++r) dy[r] = S.dy[r];
            for (int j = tid; j < hs; j += PR_THREADS) {
                const float w2 = W2[j];
                float dp[PR_ROWS], m[PR_ROWS];
                float dw2 = 0.f, db1 = 0.f;
#pragma unroll
                for (int r = 0; r < PR_ROWS; ++r) {
                    const float hv = S.h[r][j];
                    dw2 = fmaf(dy[r], hv, dw2);
                    dp[r] = (dy[r] * w2) * fmaf(-hv, hv, 1.0f);
                    db1 += dp[r];
                    S.h[r][j] = dp[r];
                }
                float* __restrict__ dw1 = slab + (int64_t)j * nz;
                float* __restrict__ sb1 = slab + (int64_t)hs * nz + j;
                float* __restrict__ sw2 = sb1 + hs;
                sb1[0] = first ? db1 : sb1[0] + db1;
                sw2[0] = first ? dw2 : sw2[0] + dw2;
                for (int k = 0; k < nz; ++k) {
                    pr_load8(S.mu[k], m);
                    float v = 0.f;
#pragma unroll
                    for (int r = 0; r < PR_ROWS; ++r) v = fmaf(dp[r], m[r], v);
                    dw1[k] = first ? v : dw1[k] + v;
                }
            }
            __syncthreads();
            if (dmu) {
                // column k = tid % kw, unit group g = tid / kw: the units g, g + G, ... in two interleaved chains; then the G
                // groups in order
                const int kw = nz <= 64 ? 64 : 128, G = PR_THREADS / kw;
                const int k = tid & (kw - 1), g = tid / kw;
                float a0[PR_ROWS], a1[PR_ROWS];
#pragma unroll
                for (int r = 0; r < PR_ROWS; ++r) { a0[r] = 0.f; a1[r] = 0.f; }
                if (k < nz) {
                    int j = g;
                    for (; j + G < hs; j += 2 * G) {
                        const float w0 = W1[(int64_t)j * nz + k], w1 = W1[(int64_t)(j + G) * nz + k];
#pragma unroll
                        for (int r = 0; r < PR_ROWS; ++r) {
                            a0[r] = fmaf(S.h[r][j], w0, a0[r]);
                            a1[r] = fmaf(S.h[r][j + G], w1, a1[r]);
                        }
                    }
                    if (j < hs) {
                        const float w0 = W1[(int64_t)j * nz + k];
#pragma unroll
                        for (int r = 0; r < PR_ROWS; ++r) a0[r] = fmaf(S.h[r][j], w0, a0[r]);
                    }
                }
#pragma unroll
                for (int r = 0; r < PR_ROWS; ++r) S.dm[tid][r] = a0[r] + a1[r];
                __syncthreads();
                for (int i = tid; i < nz * PR_ROWS; i += PR_THREADS) {
                    const int r = i / nz, kk = i - r * nz;
                    float v = S.dm[kk][r];
                    for (int q = 1; q < G; ++q) v += S.dm[q * kw + kk][r];
                    if (row0 + r < B) dmu[(int64_t)(row0 + r) * nz + kk] = v;
                }
            }
        }
        __syncthreads();   // the next tile overwrites S
    }
    if (tid == 0) {
        if (grads) slab[P - 2] = db2_acc;
        slab[P - 1] = loss_acc;
    }
    // publish the slab: every wave's stores have left, then one agent-scope release in front of the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        S.last = ticket == gridDim.x - 1 ? 1u : 0u;
        if (S.last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (S.last) {   // (uniform per workgroup) every slab is visible: add them in workgroup order
        const int nb = gridDim.x;
        for (int64_t i = tid; i < P; i += PR_THREADS) {
            float v = __hip_atomic_load(work + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int q = 1; q < nb; ++q) v += __hip_atomic_load(work + (int64_t)q * P + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            out[i] = v;
        }
        if (tid == 0) counter[0] = 0u;   // ready for the next call
    }
}

__global__ void __launch_bounds__(PR_THREADS) predictor_forward_kernel(const float* __restrict__ Z, int64_t ld, int64_t M, int nz, int hs,
                                                                       const float* __restrict__ W1, const float* __restrict__ b1,
                                                                       const float* __restrict__ W2, const float* __restrict__ b2,
                                                                       float* __restrict__ pred) {
    __shared__ PrShared S;
    const int64_t tiles = (M + PR_ROWS - 1) / PR_ROWS;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t row0 = t * PR_ROWS;
        pr_tile_forward(S, Z, ld, row0, M, nz, hs, W1, b1, W2, b2);
        if (threadIdx.x < PR_ROWS && row0 + threadIdx.x < M) pred[row0 + threadIdx.x] = S.yp[threadIdx.x];
        // (S.yp is next written behind two barriers of the next tile; S.mu and S.h were last read in front of the last one)
    }
}

// ---------------------------------------------------------------------------------------------- fit sums
// out [6] = sum p, sum y, sum p^2, sum y^2, sum p y, sum (p - y)^2 with p = (-pred - mean) / std, all in float64: a thread
// adds the elements tid + 256 (block + blocks c) in order, the wave butterfly, the four waves in order, the workgroups' partials
// in order by the last one in.
__global__ void __launch_bounds__(256) fit_sums_kernel(const float* __restrict__ pred, const void* __restrict__ y, int y_f64, int64_t M,
                                                       double mean, double sd, double* __restrict__ part,
                                                       unsigned* __restrict__ counter, double* __restrict__ out) {
    __shared__ double red[4][6];
    __shared__ unsigned last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < M; i += (int64_t)gridDim.x * 256) {
        const double p = (-(double)pred[i] - mean) / sd;
        const double t = y_f64 ? reinterpret_cast<const double*>(y)[i] : (double)reinterpret_cast<const float*>(y)[i];
        const double d = p - t;
        s[0] += p; s[1] += t; s[2] += p * p; s[3] += t * t; s[4] += p * t; s[5] += d * d;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double v = wave_sum(s[q]);
        if (lane == 0) red[wave][q] = v;
    }
    __syncthreads();
    if (tid < 6) part[(int64_t)blockIdx.x * 6 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (last && tid < 6) {
        double v = 0.0;
        for (unsigned q = 0; q < gridDim.x; ++q)
            v += __hip_atomic_load(part + (int64_t)q * 6 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[tid] = v;
        if (tid == 0) counter[0] = 0u;   // ready for the next call
    }
}

bool pr_dims_ok(int nz, int hs) { return nz >= 1 && nz <= PR_MAX_NZ && hs >= 1 && hs <= PR_MAX_HS; }

int pr_blocks(int B) {
    const int tiles = (B + PR_ROWS - 1) / PR_ROWS;
    return tiles < PR_MAX_BLOCKS ? tiles : PR_MAX_BLOCKS;
}

int64_t fit_blocks(int64_t M) {
    const int64_t b = (M + 1023) / 1024;   // four elements a thread before another workgroup pays
    return b < 1 ? 1 : (b < FIT_MAX_BLOCKS ? b : FIT_MAX_BLOCKS);
}

}  // namespace

extern "C" size_t dagnn_predictor_mse_bytes(int B, int nz, int hs, int want_grads) {
    if (B <= 0 || !pr_dims_ok(nz, hs)) return 0;
    const size_t P = want_grads ? (size_t)hs * nz + 2 * (size_t)hs + 2 : 1;
    return (size_t)pr_blocks(B) * P * sizeof(float);
}

extern "C" int dagnn_predictor_mse(const float* mu, int64_t ld_mu, const float* y, int B, int nz, int hs, const float* W1,
                                   const float* b1, const float* W2, const float* b2, float* y_pred, float* out, float* dmu,
                                   void* work, size_t work_bytes, unsigned* counter, int want_grads, void* stream) {
    if (B <= 0 || !pr_dims_ok(nz, hs) || ld_mu < nz) return DAGNN_EINVAL;
    if (!mu || !y || !W1 || !b1 || !W2 || !b2 || !y_pred || !out || !work || ((uintptr_t)work & 3) || !counter ||
        (dmu && !want_grads))
        return DAGNN_EINVAL;
    if (work_bytes < dagnn_predictor_mse_bytes(B, nz, hs, want_grads)) return DAGNN_ENOSPC;
    hipLaunchKernelGGL(predictor_mse_kernel, dim3((unsigned)pr_blocks(B)), dim3(PR_THREADS), 0, (hipStream_t)stream, mu, ld_mu, y, B,
                       nz, hs, W1, b1, W2, b2, y_pred, out, dmu, reinterpret_cast<float*>(work), counter, want_grads ? 1 : 0);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_predictor_forward(const float* Z, int64_t ld_z, int64_t M, int nz, int hs, const float* W1, const float* b1,
                                       const float* W2, const float* b2, float* pred, void* stream) {
    if (M < 0 || M >= (int64_t(1) << 31) || !pr_dims_ok(nz, hs) || ld_z < nz) return DAGNN_EINVAL;
    if (M == 0) return DAGNN_OK;
    if (!Z || !W1 || !b1 || !W2 || !b2 || !pred) return DAGNN_EINVAL;
    const int64_t tiles = (M + PR_ROWS - 1) / PR_ROWS;
    const unsigned blocks = (unsigned)(tiles < PR_FWD_MAX_BLOCKS ? tiles : PR_FWD_MAX_BLOCKS);
    hipLaunchKernelGGL(predictor_forward_kernel, dim3(blocks), dim3(PR_THREADS), 0, (hipStream_t)stream, Z, ld_z, M, nz, hs, W1, b1,
                       W2, b2, pred);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" size_t dagnn_fit_sums_bytes(int64_t M) {
    if (M <= 0) return 0;
    return (size_t)fit_blocks(M) * 6 * sizeof(double);
}

extern "C" int dagnn_fit_sums(const float* pred, const void* y, int y_is_f64, int64_t M, double mean, double std_, double* out,
                              void* work, size_t work_bytes, unsigned* counter, void* stream) {
    if (M <= 0 || !pred || !y || !out || !work || ((uintptr_t)work & 7) || !counter) return DAGNN_EINVAL;
    if (work_bytes < dagnn_fit_sums_bytes(M)) return DAGNN_ENOSPC;
    hipLaunchKernelGGL(fit_sums_kernel, dim3((unsigned)fit_blocks(M)), dim3(256), 0, (hipStream_t)stream, pred, y, y_is_f64 ? 1 : 0, M,
                       mean, std_, reinterpret_cast<double*>(work), counter, out);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
