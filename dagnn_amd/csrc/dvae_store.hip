// dvae_store.hip - the device-resident store of a D-VAE data set (dagnn_amd/dvae_store.py): its layerings at pack time
// and a batch in one launch.
//
// Reference path replaced, per batch: `_collate_fn`'s deep copies and `Batch.from_data_list` (dvae/batch.py:26-146) over
// the graphs `decode_ENAS_to_pygraph` / `decode_BN_to_pygraph` (dvae/util.py:290-385) made, the copies of the batch to the
// device, and the walk over every vertex that `loss()` makes for the decoder's schedule (models_pyg.py:405-420).  The
// graphs are dense by construction - n vertices each, n <= 32, edges from a lower to a higher vertex - so a graph is 2n
// mask words (layout: include/dagnn_hip.h) and a batch is a gather.
//
// As in store.hip the work is divided by OUTPUT element: thread t writes element t of x (a [N, nvt] one-hot, taken as
// N * nvt consecutive floats), node row t (N = B * n, so graph slot and vertex are a division), edge column t and graph
// slot t.  An edge finds its slot by bisection in the B + 1 edge offsets, its source by a running popcount over the
// graph's `succs` words and its target as the k-th set bit of that word.  Mask words are unsigned everywhere: with 32
// vertices bit 31 is an edge.  Consecutive lanes write consecutive addresses, every word has one writer, no atomics.
#include "common.h"

namespace {

// largest b in [0, B) with off[b] <= e (e < off[B])
__device__ __forceinline__ int64_t dag_slot(const int64_t* __restrict__ off, int64_t B, int64_t e) {
    int64_t lo = 0, hi = B;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) dag_store_gather_kernel(const dagnn_dag_store_gather_args A, int64_t items) {
    const int64_t B = A.B, n = A.n, nvt = A.nvt, E = A.E, N = B * n, X = N * nvt;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += step) {
        if (t < X) {   // ---- one element of the one-hot rows
            const int64_t row = t / nvt, b = row / n;
            const int32_t type = A.types[A.idx[b] * n + (row - b * n)];
            A.out_x[t] = (int64_t)type == t - row * nvt ? 1.f : 0.f;
        }
        if (t < N) {   // ---- one node row
            const int64_t b = t / n, src = A.idx[b] * n + (t - b * n);
            A.out_batch[t] = b;
            A.out_bi_layer_index[t] = A.layer_f[src];
            A.out_bi_layer_index[N + t] = t;
            A.out_bi_layer_index[2 * N + t] = A.layer_b[src];
            A.out_bi_layer_index[3 * N + t] = t;
            if (A.out_types) A.out_types[t] = A.types[src];
            if (A.out_preds) A.out_preds[t] = A.preds[src];
        }
        if (t < E) {   // ---- one edge column: the slot's edges source-major, targets ascending
            const int64_t b = dag_slot(A.offsets, B, t);
            const uint32_t* __restrict__ succ = reinterpret_cast<const uint32_t*>(A.succs) + A.idx[b] * n;
            uint32_t k = (uint32_t)(t - A.offsets[b]), u = 0, w = 0;
            for (; u < (uint32_t)n; ++u) {
                w = succ[u];
                const uint32_t c = (uint32_t)__popc(w);
                if (k < c) break;
                k -= c;
            }
            if (u == (uint32_t)n) u = 0, w = 0, k = 0;              // (offsets that claim more edges than the masks hold)
            for (; k > 0; --k) w &= w - 1u;                         // drop the k lowest set bits (k < popcount(w))
            const uint32_t v = w ? (uint32_t)__ffs((int)w) - 1u : 0u;
            A.out_edge_index[t] = b * n + (int64_t)u;
            A.out_edge_index[E + t] = b * n + (int64_t)v;
        }
        if (t <= B) {   // ---- one graph slot (ptr has B + 1 entries)
            A.out_ptr[t] = t * n;
            if (t < B && A.out_y) A.out_y[t] = A.y[A.idx[t]];
        }
    }
}

// one thread per graph: vertices are topologically numbered, so one ascending walk layers the forward direction and one
// descending walk the reverse one; a vertex reads the layers this thread wrote before
__global__ void __launch_bounds__(256) dag_store_layers_kernel(const uint32_t* __restrict__ preds, const uint32_t* __restrict__ succs,
                                                               int64_t M, int n, int32_t* __restrict__ layer_f,
                                                               int32_t* __restrict__ layer_b) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < M; g += step) {
        const int64_t base = g * n;
        for (int v = 0; v < n; ++v) {
            uint32_t m = preds[base + v] & (v ? (0xFFFFFFFFu >> (32 - v)) : 0u);          // bits below v
            int32_t l = 0;
            for (; m; m &= m - 1u) {
                const int32_t lu = layer_f[base + (__ffs((int)m) - 1)] + 1;
                l = lu > l ? lu : l;
            }
            layer_f[base + v] = l;
        }
        const uint32_t all = n == 32 ? 0xFFFFFFFFu : ((1u << n) - 1u);
        for (int u = n - 1; u >= 0; --u) {
            uint32_t m = succs[base + u] & all & (u == 31 ? 0u : (0xFFFFFFFFu << (u + 1)));   // bits above u, below n
            int32_t l = 0;
            for (; m; m &= m - 1u) {
                const int32_t lv = layer_b[base + (__ffs((int)m) - 1)] + 1;
                l = lv > l ? lv : l;
            }
            layer_b[base + u] = l;
        }
    }
}

}  // namespace

extern "C" int dagnn_dag_store_gather(const dagnn_dag_store_gather_args* a, void* stream) {
    if (!a) return DAGNN_EINVAL;
    if (a->B < 0 || a->E < 0 || a->n < 1 || a->n > 32 || a->nvt < 1 || a->nvt > (int64_t(1) << 20)) return DAGNN_EINVAL;
    if (a->B == 0) return a->E > 0 ? DAGNN_EINVAL : DAGNN_OK;
    if (a->B >= (int64_t(1) << 31) || a->E > a->B * (a->n * (a->n - 1) / 2)) return DAGNN_EINVAL;
    if (!a->types || !a->layer_f || !a->layer_b || !a->idx || !a->offsets) return DAGNN_EINVAL;
    if (!a->out_x || !a->out_bi_layer_index || !a->out_batch || !a->out_ptr) return DAGNN_EINVAL;
    // (an extent of zero elements has no address: the edge pointers may be NULL without an edge)
    if (a->E > 0 && (!a->succs || !a->out_edge_index)) return DAGNN_EINVAL;
    if ((a->out_preds && !a->preds) || (a->out_y && !a->y)) return DAGNN_EINVAL;
    int64_t items = a->B * a->n * a->nvt;   // (>= N >= B; B + 1 > it only for n = nvt = 1)
    if (a->E > items) items = a->E;
    if (a->B + 1 > items) items = a->B + 1;
    int64_t blocks = (items + 255) / 256;
    if (blocks > (int64_t(1) << 20)) blocks = int64_t(1) << 20;   // (grid-stride beyond: 2^28 elements per sweep)
    hipLaunchKernelGGL(dag_store_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a, items);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_dag_store_layers(const int32_t* preds, const int32_t* succs, int64_t M, int n, int32_t* layer_f,
                                      int32_t* layer_b, void* stream) {
    if (M < 0 || n < 1 || n > 32) return DAGNN_EINVAL;
    if (M == 0) return DAGNN_OK;
    if (!preds || !succs || !layer_f || !layer_b) return DAGNN_EINVAL;
    int64_t blocks = (M + 255) / 256;
    if (blocks > (int64_t(1) << 20)) blocks = int64_t(1) << 20;
    hipLaunchKernelGGL(dag_store_layers_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(preds), reinterpret_cast<const uint32_t*>(succs), M, n, layer_f, layer_b);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
