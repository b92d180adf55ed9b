// sgp.hip - the sparse GP of the D-VAE BO loop on its grids (bayesian_optimization/sparse_gp.py: `predict`, `get_incumbent`,
// `optimize_ei`, `batched_greedy_ei`; sparse_gp_theano_internal.py: compute_output, compute_log_ei, compute_log_averaged_ei).
//
// Reference path replaced, per grid and per greedy step: compute_kernel(x, z) [N, M] in memory, two [N, M] x [M, M] products
// against freshly inverted matrices, and for the averaged EI the inverse of the (M + j)^2 matrix Kzz_expanded - all inside a
// Theano graph.  Here the matrices are derived once per parameter version on the host side and
//   dagnn_sgp_project  builds a 32-row tile of k(X, z) in LDS, multiplies it by T^T on v_mfma_f32_32x32x2_f32 and reduces
//                      the squared row norms in one fixed order: mean, posterior variance, residual variance and the rows
//                      U = W k of the incremental factor in ONE launch; k never reaches memory.
//   dagnn_sgp_ei_step  appends one chosen point to the factor (a column of U, r -= w^2), evaluates log EI per row in float64
//                      and reduces to numpy.argmin's answer; partials are merged by the last workgroup to draw a ticket.
//
// Layout.  project: 256 threads, 4 waves.  Thread t builds the columns m = t, t + 256 of the tile (32 accumulators, x from LDS
// as a broadcast, z transposed so that a wave reads 64 consecutive m), stored k-major with pitch 33: the MFMA A fragment
// (lane & 31 -> row, lane >> 5 -> k) and the mean's walk over m are both conflict-free.  Wave w owns the 32-column tiles
// 2w, 2w + 1, 2w + 8, ... of the output, two accumulators that share the A fragment; B comes straight from Tt (k-major: a half
// wave reads 128 consecutive bytes).  Squared norms: a lane adds its tiles in ascending order, the 32 lanes of a row as a
// butterfly, the four waves as (0 + 1) + (2 + 3).
#include "common.h"

#include <math.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SP_ROWS = 32;
constexpr int SP_THREADS = 256;
constexpr int SP_PITCH = SP_ROWS + 1;
constexpr int SP_MAX_M = DAGNN_SGP_MAX_M;
constexpr int SP_MAX_D = DAGNN_SGP_MAX_D;

__host__ __device__ inline int sp_mp(int M) { return (M + 7) & ~7; }   // four MFMA steps (k = 2 each) per turn
inline size_t sp_lds_bytes(int M, int d) {
    return ((size_t)sp_mp(M) * SP_PITCH + (size_t)SP_ROWS * d + 4 * SP_ROWS * 2) * sizeof(float);
}

__global__ void __launch_bounds__(SP_THREADS) sgp_project_kernel(const float* __restrict__ X, int64_t ld_x, int64_t N, int d, int M,
                                                                 const float* __restrict__ zt, int64_t ld_z,
                                                                 const float* __restrict__ inv_ls, float sf,
                                                                 const float* __restrict__ Tt, int64_t ld_t, int Mt, int split,
                                                                 const float* __restrict__ a, float* __restrict__ U, int64_t ld_u,
                                                                 int u_col0, float* __restrict__ var0, float* __restrict__ var1,
                                                                 float* __restrict__ mean) {
    extern __shared__ __align__(16) float sp_lds[];
    const int Mp = sp_mp(M);
    float* __restrict__ Ks = sp_lds;                              // [Mp][SP_PITCH]: k(x_r, z_m) at m * SP_PITCH + r
    float* __restrict__ Xs = Ks + (size_t)Mp * SP_PITCH;          // [SP_ROWS][d]
    float* __restrict__ red = Xs + (size_t)SP_ROWS * d;           // [4 waves][SP_ROWS][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fk = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * SP_ROWS;

    for (int i = tid; i < SP_ROWS * d; i += SP_THREADS) {
        const int r = i / d, c = i - r * d;
        Xs[i] = row0 + r < N ? X[(row0 + r) * ld_x + c] : 0.f;
    }
    __syncthreads();
    for (int m = tid; m < Mp; m += SP_THREADS) {
        float acc[SP_ROWS];
#pragma unroll
        for (int r = 0; r < SP_ROWS; ++r) acc[r] = 0.f;
        if (m < M) {
            for (int c = 0; c < d; ++c) {
                const float zc = zt[(int64_t)c * ld_z + m], il = inv_ls[c];
#pragma unroll
                for (int r = 0; r < SP_ROWS; ++r) {
                    const float df = Xs[r * d + c] - zc;
                    acc[r] = fmaf(df * il, df, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < SP_ROWS; ++r)
            Ks[m * SP_PITCH + r] = (m < M && row0 + r < N) ? sf * expf(-0.5f * acc[r]) : 0.f;   // rows / columns past the end: 0
    }
    __syncthreads();

    if (mean) {   // wave w: the rows 8 w .. 8 w + 7; a lane adds m = lane, lane + 64, ... in order, then the butterfly
        for (int rr = 0; rr < SP_ROWS / 4; ++rr) {
            const int r = wave * (SP_ROWS / 4) + rr;
            float s = 0.f;
            for (int m = lane; m < M; m += 64) s = fmaf(Ks[m * SP_PITCH + r], a[m], s);
            s = wave_sum(s);
            if (lane == 0 && row0 + r < N) mean[row0 + r] = s;
        }
    }

    if (Mt > 0) {
        float s0[16], s1[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) { s0[e] = 0.f; s1[e] = 0.f; }
        const int nct = (Mt + 31) / 32;
        for (int ct = 2 * wave; ct < nct; ct += 8) {
            const bool two = ct + 1 < nct;   // (uniform per wave)
            const int j0 = ct * 32 + fr, j1 = j0 + 32;
            const float* __restrict__ t0 = Tt + (j0 < Mt ? j0 : Mt - 1);
            const float* __restrict__ t1 = Tt + (j1 < Mt ? j1 : Mt - 1);
            f32x16 acc0, acc1;
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
            if (two) {
                for (int k8 = 0; k8 < Mp; k8 += 8) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int kk = k8 + 2 * q + fk;
                        const int64_t kl = (int64_t)(kk < M ? kk : M - 1) * ld_t;   // (the tile holds 0 at kk >= M: the product is 0)
                        const float av = Ks[kk * SP_PITCH + fr];
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, t0[kl], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, t1[kl], acc1, 0, 0, 0);
                    }
                }
            } else {
                for (int k8 = 0; k8 < Mp; k8 += 8) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int kk = k8 + 2 * q + fk;
                        const int64_t kl = (int64_t)(kk < M ? kk : M - 1) * ld_t;
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[kk * SP_PITCH + fr], t0[kl], acc0, 0, 0, 0);
                    }
                }
            }
            // C / D layout of the 32 x 32 MFMA: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = (e & 3) + 8 * (e >> 2) + 4 * fk;
                const bool live = row0 + r < N;
                if (j0 < Mt) {
                    const float v = acc0[e];
                    if (U && live && j0 >= u_col0) U[(row0 + r) * ld_u + (j0 - u_col0)] = v;
                    if (j0 < split) s0[e] = fmaf(v, v, s0[e]); else s1[e] = fmaf(v, v, s1[e]);
                }
                if (two && j1 < Mt) {
                    const float v = acc1[e];
                    if (U && live && j1 >= u_col0) U[(row0 + r) * ld_u + (j1 - u_col0)] = v;
                    if (j1 < split) s0[e] = fmaf(v, v, s0[e]); else s1[e] = fmaf(v, v, s1[e]);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            float u0 = s0[e], u1 = s1[e];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {   // the 32 lanes that share lane >> 5
                u0 += __shfl_xor(u0, o, 64);
                u1 += __shfl_xor(u1, o, 64);
            }
            if (fr == 0) {
                const int r = (e & 3) + 8 * (e >> 2) + 4 * fk;
                red[(wave * SP_ROWS + r) * 2 + 0] = u0;
                red[(wave * SP_ROWS + r) * 2 + 1] = u1;
            }
        }
        __syncthreads();
        if (tid < SP_ROWS && row0 + tid < N) {
            const int r = tid;
            const float n0 = (red[(0 * SP_ROWS + r) * 2] + red[(1 * SP_ROWS + r) * 2]) +
                             (red[(2 * SP_ROWS + r) * 2] + red[(3 * SP_ROWS + r) * 2]);
            const float n1 = (red[(0 * SP_ROWS + r) * 2 + 1] + red[(1 * SP_ROWS + r) * 2 + 1]) +
                             (red[(2 * SP_ROWS + r) * 2 + 1] + red[(3 * SP_ROWS + r) * 2 + 1]);
            if (var0) var0[row0 + r] = sf - n0;
            if (var1) var1[row0 + r] = sf - n1;
        }
    }
}

// ---------------------------------------------------------------------------------------------- the greedy step
constexpr int EI_THREADS = 256;
constexpr int EI_RPW = 16;                    // rows a wave owns: lane i < 16 runs the float64 epilogue of row i
constexpr int EI_ROWS = 4 * EI_RPW;           // rows a workgroup owns

struct __align__(16) EiPart {
    double key;
    long long idx;    // -1: no row
    long long bad;
    long long pad;
};

// does (ka, ia) come before (kb, ib) in numpy.argmin's order?  idx < 0 never does; a NaN beats every number; equal keys (and
// two NaN) go to the lower index
__device__ __forceinline__ bool ei_before(double ka, long long ia, double kb, long long ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    const bool na = ka != ka, nb = kb != kb;
    if (na || nb) return na && nb ? ia < ib : na;
    if (ka != kb) return ka < kb;
    return ia < ib;
}

__device__ __forceinline__ double ei_neg_log_ei(double m, double v, double inc) {
    if (!(v > 0.0)) return __builtin_nan("");
    const double sd = sqrt(v), u = inc - m, s = u / sd;
    double ratio;
    if (s < -10.0) {
        const double x2 = s * s, x3 = x2 * s, x5 = x3 * x2, x7 = x5 * x2;
        ratio = -(1.0 / s - 1.0 / x3 + 3.0 / x5 - 15.0 / x7);
    } else {
        ratio = (0.5 * erfc(-s * 0.70710678118654752440)) / (exp(-0.5 * s * s) * 0.39894228040143267794);
    }
    return -(log(u * ratio + sd) - 0.91893853320467274178 - 0.5 * s * s);
}

__global__ void __launch_bounds__(EI_THREADS) sgp_ei_step_kernel(int mode, int64_t N, const float* __restrict__ mean, float* __restrict__ r,
                                                                 double incumbent, const float* __restrict__ X, int64_t ld_x, int d,
                                                                 const float* __restrict__ inv_ls, float sf, const float* __restrict__ p,
                                                                 float* __restrict__ U, int64_t ld_u, int Me, const float* __restrict__ c,
                                                                 float inv_delta, double* __restrict__ keys, long long* __restrict__ result,
                                                                 EiPart* __restrict__ part, unsigned* __restrict__ counter) {
    __shared__ EiPart wpart[4];
    __shared__ unsigned last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = ((int64_t)blockIdx.x * 4 + wave) * EI_RPW;
    const int64_t row = base + lane;
    const bool own = lane < EI_RPW && row < N;
    float rv = own ? r[row] : 0.f;
    if (U) {
        float dot = 0.f, r2 = 0.f;
        for (int i = 0; i < EI_RPW; ++i) {
            const int64_t x = base + i;
            if (x >= N) break;   // (uniform per wave)
            const float* __restrict__ u = U + x * ld_u;
            float s = 0.f, t = 0.f;
            for (int j = lane; j < Me; j += 64) s = fmaf(u[j], c[j], s);
            for (int q = lane; q < d; q += 64) {
                const float df = X[x * ld_x + q] - p[q];
                t = fmaf(df * inv_ls[q], df, t);
            }
            s = wave_sum(s);
            t = wave_sum(t);
            if (lane == i) { dot = s; r2 = t; }
        }
        if (own) {
            const float w = (sf * expf(-0.5f * r2) - dot) * inv_delta;
            U[row * ld_u + Me] = w;
            rv = fmaf(-w, w, rv);
            r[row] = rv;
        }
    }
    double key = 0.0;
    long long idx = -1, bad = 0;
    if (own) {
        const double m = (double)mean[row];
        if (mode == DAGNN_SGP_ARGMIN_MEAN) {
            key = m;
        } else {
            key = ei_neg_log_ei(m, (double)rv, incumbent);
            bad = (double)rv > 0.0 ? 0 : 1;
        }
        idx = row;
        if (keys) keys[row] = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double k2 = __shfl_xor(key, o, 64);
        const long long i2 = __shfl_xor(idx, o, 64);
        bad += __shfl_xor(bad, o, 64);
        if (ei_before(k2, i2, key, idx)) { key = k2; idx = i2; }
    }
    if (lane == 0) { wpart[wave].key = key; wpart[wave].idx = idx; wpart[wave].bad = bad; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            bad += wpart[w].bad;
            if (ei_before(wpart[w].key, wpart[w].idx, key, idx)) { key = wpart[w].key; idx = wpart[w].idx; }
        }
        EiPart* __restrict__ mine = part + blockIdx.x;
        mine->key = key; mine->idx = idx; mine->bad = bad; mine->pad = 0;
        // publish: the stores have left, one agent-scope release in front of the ticket
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (last && wave == 0) {   // every partial is visible: a lane merges the workgroups lane, lane + 64, ..., then the butterfly
        key = 0.0; idx = -1; bad = 0;
        for (unsigned q = lane; q < gridDim.x; q += 64) {
            const double k2 = __hip_atomic_load(&part[q].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const long long i2 = __hip_atomic_load(&part[q].idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bad += __hip_atomic_load(&part[q].bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ei_before(k2, i2, key, idx)) { key = k2; idx = i2; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double k2 = __shfl_xor(key, o, 64);
            const long long i2 = __shfl_xor(idx, o, 64);
            bad += __shfl_xor(bad, o, 64);
            if (ei_before(k2, i2, key, idx)) { key = k2; idx = i2; }
        }
        if (lane == 0) {
            result[0] = idx;
            result[1] = bad;
            result[2] = __double_as_longlong(key);
            result[3] = 0;
            counter[0] = 0u;   // ready for the next call
        }
    }
}

int64_t ei_blocks(int64_t N) { return (N + EI_ROWS - 1) / EI_ROWS; }

std::atomic<unsigned long long> sp_attr_done{0};

}  // namespace

extern "C" int dagnn_sgp_project(const float* X, int64_t ld_x, int64_t N, int d, int M, const float* zt, int64_t ld_z,
                                 const float* inv_ls, float sf, const float* Tt, int64_t ld_t, int Mt, int split, const float* a,
                                 float* U, int64_t ld_u, int u_col0, float* var0, float* var1, float* mean, void* stream) {
    if (N < 0 || N >= (int64_t(1) << 31) * SP_ROWS || d < 1 || d > SP_MAX_D || M < 1 || M > SP_MAX_M || ld_x < d || ld_z < M)
        return DAGNN_EINVAL;
    if (Mt < 0 || Mt > 2 * SP_MAX_M || split < 0 || split > Mt || u_col0 < 0 || u_col0 > Mt) return DAGNN_EINVAL;
    if (Mt > 0 && (!Tt || ld_t < Mt)) return DAGNN_EINVAL;
    if (Mt == 0 && (U || var0 || var1)) return DAGNN_EINVAL;
    if (U && ld_u < Mt - u_col0) return DAGNN_EINVAL;
    if (mean && !a) return DAGNN_EINVAL;
    if (N == 0) return DAGNN_OK;
    if (!X || !zt || !inv_ls) return DAGNN_EINVAL;
    const size_t lds = sp_lds_bytes(M, d);
    const hipError_t e = dagnn_lds_attr_once(sp_attr_done, reinterpret_cast<const void*>(sgp_project_kernel), (int)sp_lds_bytes(SP_MAX_M, SP_MAX_D));
    if (e != hipSuccess) return DAGNN_EHIP(e);
    const int64_t tiles = (N + SP_ROWS - 1) / SP_ROWS;
    hipLaunchKernelGGL(sgp_project_kernel, dim3((unsigned)tiles), dim3(SP_THREADS), lds, (hipStream_t)stream, X, ld_x, N, d, M, zt, ld_z,
                       inv_ls, sf, Tt, ld_t, Mt, split, a, U, ld_u, u_col0, var0, var1, mean);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" size_t dagnn_sgp_ei_step_bytes(int64_t N) {
    if (N <= 0) return 0;
    return (size_t)ei_blocks(N) * sizeof(EiPart);
}

extern "C" int dagnn_sgp_ei_step(int mode, int64_t N, const float* mean, float* r, double incumbent, const float* X, int64_t ld_x,
                                 int d, const float* inv_ls, float sf, const float* p, float* U, int64_t ld_u, int Me,
                                 const float* c, float inv_delta, double* keys, int64_t* result, void* work, size_t work_bytes,
                                 unsigned* counter, void* stream) {
    if (mode != DAGNN_SGP_ARGMIN_MEAN && mode != DAGNN_SGP_ARGMIN_EI) return DAGNN_EINVAL;
    if (N <= 0 || ei_blocks(N) >= (int64_t(1) << 31) || !mean || !r || !result || !work || ((uintptr_t)work & 7) || !counter)
        return DAGNN_EINVAL;
    if (U) {
        if (!X || !inv_ls || !p || !c || d < 1 || d > SP_MAX_D || ld_x < d || Me < 1 || Me >= SP_MAX_M + DAGNN_SGP_MAX_Q ||
            ld_u <= Me)
            return DAGNN_EINVAL;
    }
    if (work_bytes < dagnn_sgp_ei_step_bytes(N)) return DAGNN_ENOSPC;
    hipLaunchKernelGGL(sgp_ei_step_kernel, dim3((unsigned)ei_blocks(N)), dim3(EI_THREADS), 0, (hipStream_t)stream, mode, N, mean, r,
                       incumbent, X, ld_x, d, inv_ls, sf, p, U, ld_u, Me, c, inv_delta, keys, reinterpret_cast<long long*>(result),
                       reinterpret_cast<EiPart*>(work), counter);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
