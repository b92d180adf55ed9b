// lp.hip - the tail of the longest-path (LP) task's loop (ogbg-code/main_pyg_lp.py): targets and accuracy
// (the class loss, dagnn_class_ce, is the S = 1 instance of loss.hip's kernel).
//
// Reference path replaced, per batch:
//   dagnn_graph_depth  `len_longest_path` of the reference's patched reader (ogb/io/read_graph_pyg.py:51-54) - the maximum of
//                      `_bi_layer_idx0` per graph - for a batch that does not carry the attribute: `batch` is sorted, so a
//                      graph's nodes are one contiguous range; a wave per graph finds the range by bisection and folds it
//                      with shuffles.  No atomics; a graph id without nodes gives 0.
//   dagnn_class_hits   the `argmax` + copy to the host + `Evaluator._eval_acc` (main_pyg_lp.py:66-74,93-107;
//                      ogb/graphproppred/evaluate.py:221-229) of one batch as ONE (hits, labelled) int64 pair in device
//                      memory.  The argmax is the order of rows_dev.h (lowest column among equals, a NaN beats every number).
#include "rows_dev.h"

namespace {

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
        m = wave_max(m);
        if (lane == 0) out[g] = m;
    }
}

// ---------------------------------------------------------------------------------------------- accuracy
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
                const long long p = logit_pack(logit_key(x[c]), c);
                best = p > best ? p : best;
            }
            best = wave_max(best);
            if (lane == 0) hits_compare(targ, kind, b, logit_col(best), hits, labelled);
        }
    } else {
        const int64_t b = (int64_t)blockIdx.x * 256 + tid;
        if (b < B) hits_compare(targ, kind, b, tok[b], hits, labelled);
    }
    hits = wave_sum(hits);
    labelled = wave_sum(labelled);
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
        h = wave_sum(h);
        l = wave_sum(l);
        if (lane == 0) { red[wave][0] = h; red[wave][1] = l; }
        __syncthreads();
        if (tid == 0) {
            out[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
            out[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
            counter[0] = 0u;   // ready for the next call
        }
    }
}

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
