// store.hip - a batch of the device-resident graph store (dagnn_amd/store.py) in one launch.
//
// Reference path replaced, per batch: the loader workers' `augment_edge2` (ogbg-code/utils2.py:31-79) and
// `add_order_info_01` (src/utils_dag.py:39-52) per graph, the collation of ogbg-code/tg/dataloader.py:13-35 and the copy of
// eleven tensors to the device.  Everything per graph is fixed for the life of the dataset and sits packed in device memory
// (layout: include/dagnn_hip.h); a batch is a gather.
//
// Work is divided by OUTPUT element, not by graph: thread t writes node row t, edge column t, graph slot t, label word t
// and reference id t (whichever exist), and finds the graph slot an element belongs to by bisection in the batch's B + 1
// offsets (at most 17 probes of an array that stays in L2).  A batch of one 1 100-node graph therefore spreads over as many
// threads as a batch of forty 30-node graphs, consecutive lanes write consecutive addresses in every output, every word has
// one writer, and there are no atomics and nothing to hand over between workgroups.
#include "common.h"

namespace {

typedef long long store_ll2 __attribute__((ext_vector_type(2)));

// largest b in [0, B) with off[b] <= v (v < off[B]; slots without elements are stepped over)
__device__ __forceinline__ int64_t store_slot(const int64_t* __restrict__ off, int64_t B, int64_t v) {
    int64_t lo = 0, hi = B;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}
// the same over the sum of two offset rows (AST edges + next-token edges = the slot's first edge column)
__device__ __forceinline__ int64_t store_slot2(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t B, int64_t v) {
    int64_t lo = 0, hi = B;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] + b[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) store_gather_kernel(const dagnn_store_gather_args A, int64_t items) {
    const int64_t B = A.B, N = A.N, E = A.E, S = A.S, R = A.R;
    const int64_t* __restrict__ off_n = A.offsets;
    const int64_t* __restrict__ off_a = A.offsets + A.ld_offsets;
    const int64_t* __restrict__ off_t = A.offsets + 2 * A.ld_offsets;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += step) {
        if (t < N) {   // ---- one node row
            const int64_t b = store_slot(off_n, B, t);
            const int64_t v = A.node_ptr[A.idx[b]] + (t - off_n[b]);
            const int2 xv = reinterpret_cast<const int2*>(A.x)[v];
            store_ll2 row;
            row.x = xv.x;
            row.y = xv.y;
            reinterpret_cast<store_ll2*>(A.out_x)[t] = row;
            A.out_depth[t] = A.depth[v];
            A.out_batch[t] = b;
            A.out_index0[t] = t;
            A.out_index1[t] = t;
            if (A.out_layer_f) A.out_layer_f[t] = A.layer_f[v];
            if (A.out_layer_b) A.out_layer_b[t] = A.layer_b[v];
        }
        if (t < E) {   // ---- one edge column: the slot's AST edges in stored order, then its next-token edges
            const int64_t b = store_slot2(off_a, off_t, B, t);
            const int64_t g = A.idx[b];
            const int64_t k = t - (off_a[b] + off_t[b]), n_ast = off_a[b + 1] - off_a[b], shift = off_n[b];
            int64_t u, w;
            float2 attr;
            if (k < n_ast) {
                const int64_t e = A.edge_ptr[g] + k;
                u = A.src[e];
                w = A.dst[e];
                attr = make_float2(0.f, 0.f);
            } else {
                const int64_t p = A.tok_ptr[g] + (k - n_ast);
                u = A.tok[p];
                w = A.tok[p + 1];
                attr = make_float2(1.f, 0.f);
            }
            A.out_edge_index[t] = u + shift;
            A.out_edge_index[E + t] = w + shift;
            reinterpret_cast<float2*>(A.out_edge_attr)[t] = attr;
        }
        if (t <= B) {   // ---- one graph slot (ptr has B + 1 entries)
            A.out_ptr[t] = off_n[t];
            if (t < B) {
                const int64_t g = A.idx[t];
                if (A.out_llp) A.out_llp[t] = (float)A.depth_max[g];
                if (A.out_ref_extra) A.out_ref_extra[t] = A.ref_extra[g];
            }
        }
        if (A.out_y_arr && t < B * S) A.out_y_arr[t] = A.y_arr[A.idx[t / S] * S + t % S];
        if (A.out_ref_ids && t < B * R) A.out_ref_ids[t] = A.ref_ids[A.idx[t / R] * R + t % R];
    }
}

}  // namespace

extern "C" int dagnn_store_gather(const dagnn_store_gather_args* a, void* stream) {
    if (!a) return DAGNN_EINVAL;
    if (a->B < 0 || a->N < 0 || a->E < 0 || a->S < 0 || a->R < 0) return DAGNN_EINVAL;
    if (a->B == 0) return a->N > 0 || a->E > 0 ? DAGNN_EINVAL : DAGNN_OK;
    if (a->B >= (int64_t(1) << 31) || a->ld_offsets < a->B + 1) return DAGNN_EINVAL;
    if (!a->idx || !a->offsets || !a->node_ptr || !a->out_ptr) return DAGNN_EINVAL;
    // (an extent of zero elements has no address: its pointers may be NULL)
    if (a->N > 0 && (!a->x || !a->depth || !a->out_x || !a->out_depth || !a->out_batch || !a->out_index0 || !a->out_index1))
        return DAGNN_EINVAL;
    if (a->E > 0 && (!a->edge_ptr || !a->tok_ptr || !a->src || !a->dst || !a->tok || !a->out_edge_index || !a->out_edge_attr))
        return DAGNN_EINVAL;
    if ((a->out_layer_f && !a->layer_f) || (a->out_layer_b && !a->layer_b) || (a->out_llp && !a->depth_max)) return DAGNN_EINVAL;
    if (a->out_y_arr && (!a->y_arr || a->S == 0)) return DAGNN_EINVAL;
    if ((a->out_ref_ids != nullptr) != (a->out_ref_extra != nullptr)) return DAGNN_EINVAL;
    if (a->out_ref_ids && (!a->ref_ids || !a->ref_extra || a->R == 0)) return DAGNN_EINVAL;
    if (((uintptr_t)a->out_x & 15) || ((uintptr_t)a->x & 7) || ((uintptr_t)a->out_edge_attr & 7)) return DAGNN_EINVAL;
    int64_t items = a->N > a->E ? a->N : a->E;
    if (a->B + 1 > items) items = a->B + 1;
    if (a->out_y_arr && a->B * a->S > items) items = a->B * a->S;
    if (a->out_ref_ids && a->B * a->R > items) items = a->B * a->R;
    int64_t blocks = (items + 255) / 256;
    if (blocks > (int64_t(1) << 20)) blocks = int64_t(1) << 20;   // (grid-stride beyond: 2^28 elements per sweep)
    hipLaunchKernelGGL(store_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a, items);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
