// lp.hip - the tail of the longest-path (LP) task's loop (ogbg-code/main_pyg_lp.py): targets, class loss, accuracy.
//
// Reference path replaced, per batch:
//   dagnn_graph_depth  `len_longest_path` of the reference's patched reader (ogb/io/read_graph_pyg.py:51-54) - the maximum of
//                      `_bi_layer_idx0` per graph - for a batch that does not carry the attribute: `batch` is sorted, so a
//                      graph's nodes are one contiguous range; a wave per graph finds the range by bisection and folds it
//                      with shuffles.  No atomics; a graph id without nodes gives 0.
//   dagnn_class_ce     `CrossEntropyLoss()(pred, targ.to(torch.long))` on ONE [B, C] head (main_pyg_lp.py:56-58), loss and
//                      d loss / d logits = (softmax - onehot) / B in one launch.  loss.hip's seq_ce_kernel with S = 1, stage
//                      for stage (same sums in the same order, same error analysis: DESIGN.md 4i), except that the target
//                      is read as what the reference hands over - int64, or the float tensor it concatenates - and
//                      truncated toward zero in the kernel instead of by a launch in front of it.
//   dagnn_class_hits   the `argmax` + copy to the host + `Evaluator._eval_acc` (main_pyg_lp.py:66-74,93-107;
//                      ogb/graphproppred/evaluate.py:221-229) of one batch as ONE (hits, labelled) int64 pair in device
//                      memory.  The argmax is predict.hip's order (lowest column among equals, a NaN beats every number).
#include <limits.h>

#include "common.h"

namespace {

__device__ __forceinline__ float lp_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float lp_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long lp_wave_max_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ long long lp_wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------- targets
// first index in [0, N) whose batch id is >= g (batch sorted ascending)
__device__ __forceinline__ int64_t lp_lower_bound(const long long* __restrict__ batch, int64_t N, long long g) {
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (batch[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) graph_depth_kernel(const long long* __restrict__ layer, const long long* __restrict__ batch,
                                                          int64_t N, int64_t B, long long* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t g = wave; g < B; g += nwaves) {   // (uniform per wave)
        const int64_t v0 = lp_lower_bound(batch, N, g), v1 = lp_lower_bound(batch, N, g + 1);
        long long m = 0;   // (layer ids start at 0: the maximum over nothing is 0)
        for (int64_t v = v0 + lane; v < v1; v += 64) {
            const long long l = layer[v];
            m = l > m ? l : m;
        }
        m = lp_wave_max_ll(m);
        if (lane == 0) out[g] = m;
    }
}

// ---------------------------------------------------------------------------------------------- targets as the reference holds them
enum { LP_I64 = DAGNN_LP_INT64, LP_F32 = DAGNN_LP_FLOAT32, LP_F64 = DAGNN_LP_FLOAT64 };

// `targ.to(torch.long)`: truncation toward zero; what has no int64 value (NaN, out of range) becomes -1: outside [0, C)
__device__ __forceinline__ long long lp_class_of(const void* __restrict__ targ, int kind, int64_t b) {
    if (kind == LP_I64) return reinterpret_cast<const long long*>(targ)[b];
    const double v = kind == LP_F32 ? (double)reinterpret_cast<const float*>(targ)[b] : reinterpret_cast<const double*>(targ)[b];
    if (!(v > -9.0e18 && v < 9.0e18)) return -1;
    return (long long)v;
}

// ---------------------------------------------------------------------------------------------- loss
__global__ void __launch_bounds__(256) class_ce_kernel(const float* __restrict__ logits, long long ld, const void* __restrict__ targ,
                                                       int kind, int B, int C, float* __restrict__ dlogits, long long ld_d,
                                                       float* __restrict__ row_loss, float* __restrict__ loss,
                                                       unsigned* __restrict__ counter) {
    __shared__ float red[4];
    __shared__ unsigned last;
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ x = logits + (long long)b * ld;
    const long long t = lp_class_of(targ, kind, b);
    float m = -INFINITY;
    for (int j = tid; j < C; j += 256) m = fmaxf(m, x[j]);
    m = lp_wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float z = 0.f;
    for (int j = tid; j < C; j += 256) z += __expf(x[j] - m);
    z = lp_wave_sum(z);
    if (lane == 0) red[wave] = z;
    __syncthreads();
    z = (red[0] + red[1]) + (red[2] + red[3]);
    const float lse = m + __logf(z);
    const bool ok = t >= 0 && t < C;
    if (dlogits) {
        const float scale = 1.0f / (float)B, inv = 1.0f / z;
        float* __restrict__ d = dlogits + (long long)b * ld_d;
        for (int j = tid; j < C; j += 256) d[j] = (__expf(x[j] - m) * inv - (j == t ? 1.0f : 0.0f)) * scale;
    }
    if (tid == 0) {
        row_loss[b] = ok ? lse - x[t] : NAN;
        __threadfence();
        last = atomicAdd(counter, 1u) == (unsigned)(B - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (last) {   // (uniform per workgroup) the last row in: every row loss is visible - sum them in index order
        __threadfence();
        float acc = 0.f;
        for (int j = tid; j < B; j += 256) acc += __hip_atomic_load(row_loss + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        acc = lp_wave_sum(acc);
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        if (tid == 0) {
            loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)B;
            counter[0] = 0u;   // ready for the next call
        }
    }
}

// ---------------------------------------------------------------------------------------------- accuracy
// predict.hip's order of logits as one integer: (monotone key of the value, ~column)
__device__ __forceinline__ long long lp_pack(float v, int col) {
    int key;
    if (v != v) key = INT_MAX;
    else {
        const int bits = __float_as_int(v);
        key = bits >= 0 ? bits : (int)(0x80000000u - (unsigned)bits);
    }
    return (long long)(((unsigned long long)(unsigned)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)col));
}

// _eval_acc on one row: labelled = the target is not NaN; hit = target and prediction are equal AS VALUES (numpy compares a
// float target with the int64 prediction in float64: 3.0 matches class 3, 3.5 matches nothing)
__device__ __forceinline__ void lp_compare(const void* __restrict__ targ, int kind, int64_t b, long long pred, long long& hits,
                                           long long& labelled) {
    if (kind == LP_I64) {
        labelled += 1;
        hits += reinterpret_cast<const long long*>(targ)[b] == pred;
        return;
    }
    const double v = kind == LP_F32 ? (double)reinterpret_cast<const float*>(targ)[b] : reinterpret_cast<const double*>(targ)[b];
    if (v != v) return;
    labelled += 1;
    hits += v == (double)pred;
}

constexpr int HITS_ROWS = 64;   // rows of one workgroup in the logits form (16 per wave, one after the other)

// logits != NULL: a wave per row, 4 rows at a time per workgroup, HITS_ROWS rows per workgroup; else a thread per token,
// 256 per workgroup.  Every workgroup leaves one (hits, labelled) partial; the last one in adds them (integers: exact in
// any order) and writes the pair.
__global__ void __launch_bounds__(256) class_hits_kernel(const float* __restrict__ logits, int64_t ld, const long long* __restrict__ tok,
                                                         int64_t B, int C, const void* __restrict__ targ, int kind,
                                                         long long* __restrict__ part, unsigned* __restrict__ counter,
                                                         long long* __restrict__ out) {
    __shared__ long long red[4][2];
    __shared__ unsigned last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long hits = 0, labelled = 0;
    if (logits) {
        const int64_t row0 = (int64_t)blockIdx.x * HITS_ROWS;
        const int64_t row1 = row0 + HITS_ROWS < B ? row0 + HITS_ROWS : B;
        for (int64_t b = row0 + wave; b < row1; b += 4) {   // (uniform per wave)
            const float* __restrict__ x = logits + b * ld;
            long long best = LLONG_MIN;
            for (int c = lane; c < C; c += 64) {
                const long long p = lp_pack(x[c], c);
                best = p > best ? p : best;
            }
            best = lp_wave_max_ll(best);
            if (lane == 0) lp_compare(targ, kind, b, (long long)(0xffffffffu - (unsigned)(unsigned long long)best), hits, labelled);
        }
    } else {
        const int64_t b = (int64_t)blockIdx.x * 256 + tid;
        if (b < B) lp_compare(targ, kind, b, tok[b], hits, labelled);
    }
    hits = lp_wave_sum_ll(hits);
    labelled = lp_wave_sum_ll(labelled);
    if (lane == 0) { red[wave][0] = hits; red[wave][1] = labelled; }
    __syncthreads();
    if (tid == 0) {
        part[2 * (int64_t)blockIdx.x] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        part[2 * (int64_t)blockIdx.x + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
        __threadfence();
        last = atomicAdd(counter, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (last) {   // (uniform per workgroup)
        __threadfence();
        long long h = 0, l = 0;
        for (unsigned j = tid; j < gridDim.x; j += 256) {
            h += __hip_atomic_load(part + 2 * (int64_t)j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            l += __hip_atomic_load(part + 2 * (int64_t)j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        h = lp_wave_sum_ll(h);
        l = lp_wave_sum_ll(l);
        if (lane == 0) { red[wave][0] = h; red[wave][1] = l; }
        __syncthreads();
        if (tid == 0) {
            out[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
            out[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
            counter[0] = 0u;   // ready for the next call
        }
    }
}

bool lp_kind_ok(int kind) { return kind == LP_I64 || kind == LP_F32 || kind == LP_F64; }

int64_t hits_blocks(int64_t B, bool logits) { return logits ? (B + HITS_ROWS - 1) / HITS_ROWS : (B + 255) / 256; }

}  // namespace

extern "C" int dagnn_graph_depth(const int64_t* layer, const int64_t* batch, int64_t N, int64_t B, int64_t* depth, void* stream) {
    if (N < 0 || B < 0) return DAGNN_EINVAL;
    if (B == 0) return DAGNN_OK;
    if (!depth || (N > 0 && (!layer || !batch))) return DAGNN_EINVAL;
    int64_t blocks = (B + 3) / 4;   // 4 waves per block, one graph per wave
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(graph_depth_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(layer), reinterpret_cast<const long long*>(batch), N, B,
                       reinterpret_cast<long long*>(depth));
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_class_ce(const float* logits, int64_t ld, const void* targ, int targ_kind, int B, int C, float* dlogits,
                              int64_t ld_d, float* row_loss, float* loss, unsigned* counter, void* stream) {
    if (!logits || !targ || !row_loss || !loss || !counter || !lp_kind_ok(targ_kind) || B <= 0 || C <= 0 || ld < C ||
        (dlogits && ld_d < C))
        return DAGNN_EINVAL;
    hipLaunchKernelGGL(class_ce_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, logits, (long long)ld, targ,
                       targ_kind, B, C, dlogits, (long long)ld_d, row_loss, loss, counter);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" size_t dagnn_class_hits_bytes(int64_t B, int from_logits) {
    if (B < 0 || B >= (int64_t(1) << 31)) return 0;
    return (size_t)(B > 0 ? hits_blocks(B, from_logits != 0) : 1) * 2 * sizeof(int64_t);
}

extern "C" int dagnn_class_hits(const float* logits, int64_t ld, const int64_t* tok, int64_t B, int C, const void* targ,
                                int targ_kind, void* work, size_t work_bytes, unsigned* counter, int64_t* out, void* stream) {
    if (B <= 0 || B >= (int64_t(1) << 31) || !lp_kind_ok(targ_kind) || (logits != nullptr) == (tok != nullptr)) return DAGNN_EINVAL;
    if (logits && (C <= 0 || ld < C)) return DAGNN_EINVAL;
    if (!targ || !work || ((uintptr_t)work & 7) || !counter || !out) return DAGNN_EINVAL;
    if (work_bytes < dagnn_class_hits_bytes(B, logits != nullptr)) return DAGNN_ENOSPC;
    hipLaunchKernelGGL(class_hits_kernel, dim3((unsigned)hits_blocks(B, logits != nullptr)), dim3(256), 0, (hipStream_t)stream,
                       logits, ld, reinterpret_cast<const long long*>(tok), B, C, targ, targ_kind,
                       reinterpret_cast<long long*>(work), counter, reinterpret_cast<long long*>(out));
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
