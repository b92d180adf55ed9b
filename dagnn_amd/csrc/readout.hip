// readout.hip - the read-out (dagnn.py:119-126,184-202: max / add / mean over the output nodes of a direction or over
// all nodes of a graph) for several matrices in ONE launch, and its backward: all the read-out code there is, for every
// (bidirectional, out_pool_all, out_pool, out_wx), training and evaluation.  Grid (graph, job); a thread owns a
// (graph, column) pair and every node belongs to one graph, so nothing here is atomic and two runs agree bit for bit.
#include "common.h"

namespace {

struct PoolJobs { dagnn_pool_job j[DAGNN_MAX_READOUT_JOBS]; };
struct PoolBwdJobs { dagnn_pool_bwd_job j[DAGNN_MAX_READOUT_JOBS]; };

// [p0, p1) of graph g in `scope`: positions into order[1 - scope] (scope 0 / 1: the layer-0 frontier of the opposite
// direction, a contiguous range the plan holds) or node ids themselves (scope 2, `order` = nullptr).
__device__ inline void scope_range(const int32_t* __restrict__ plan, const PlanLayout& L, int scope, int g, int& p0, int& p1,
                                   const int32_t*& order) {
    const int n0 = plan[L.node_ptr + g];
    order = nullptr;
    if (scope == 2) {
        p0 = n0; p1 = plan[L.node_ptr + g + 1];
    } else {
        const int od = 1 - scope;
        const int depth = plan[L.depth[od] + g];
        const int32_t* ls = plan + L.lstart[od] + n0 + g;
        order = plan + L.order[od];
        p0 = depth > 0 ? ls[0] : 0; p1 = depth > 0 ? ls[1] : 0;
    }
}

// out[g, col_off + j] = the pool of h[v, j] over the nodes v in scope, visited in range order; `inv` is exactly 1 for max
// and add, and multiplying by it changes no float.
__global__ void __launch_bounds__(256) readout_pool_batch_kernel(const int32_t* __restrict__ plan, PlanLayout L, PoolJobs J,
                                                                  float* __restrict__ out, int ld_out) {
    const dagnn_pool_job& K = J.j[blockIdx.y];
    const int g = blockIdx.x;
    int p0, p1;
    const int32_t* order;
    scope_range(plan, L, K.scope, g, p0, p1, order);
    const int mode = K.mode;
    const float* __restrict__ h = K.h;
    const int ld_h = K.ld_h;
    const float inv = mode == DAGNN_POOL_MEAN ? 1.f / (float)max(p1 - p0, 1) : 1.f;
    for (int j = threadIdx.x; j < K.width; j += blockDim.x) {
        float m = 0.f;  // graphs nothing lands on stay at zero
        for (int p = p0; p < p1; ++p) {
            const float v = h[(int64_t)(order ? order[p] : p) * ld_h + j];
            m = mode == DAGNN_POOL_MAX ? ((p == p0) ? v : fmaxf(m, v)) : m + v;
        }
        out[(int64_t)g * ld_out + K.col_off + j] = m * inv;
    }
}

// grad_h[v, j] += the share of grad_out[g, col_off + j] node v has in the pool (ADD: all of it; MEAN: it times the
// forward's own factor, rounded once; MAX: all of it at the first node in visiting order that attains the maximum: a
// later node wins only if strictly greater, scatter-max's single winner).  A graph with nothing in scope writes nothing.
__global__ void __launch_bounds__(256) readout_pool_bwd_batch_kernel(const int32_t* __restrict__ plan, PlanLayout L, PoolBwdJobs J,
                                                                      const float* __restrict__ gout, int ld_out) {
    const dagnn_pool_bwd_job& K = J.j[blockIdx.y];
    const int g = blockIdx.x;
    int p0, p1;
    const int32_t* order;
    scope_range(plan, L, K.scope, g, p0, p1, order);
    if (p1 <= p0) return;
    const int mode = K.mode;
    const float inv = mode == DAGNN_POOL_MEAN ? 1.f / (float)max(p1 - p0, 1) : 1.f;
    for (int j = threadIdx.x; j < K.width; j += blockDim.x) {
        const float go = gout[(int64_t)g * ld_out + K.col_off + j];
        if (mode == DAGNN_POOL_MAX) {
            int best = order ? order[p0] : p0;
            float m = K.h[(int64_t)best * K.ld_h + j];
            for (int p = p0 + 1; p < p1; ++p) {
                const int v = order ? order[p] : p;
                const float x = K.h[(int64_t)v * K.ld_h + j];
                if (x > m) { m = x; best = v; }
            }
            K.grad_h[(int64_t)best * K.ld_g + j] += go;
        } else {
            // (one multiply of its own: the addend is a rounded fp32 number, never the inside of a fused multiply-add)
            const float a = mode == DAGNN_POOL_MEAN ? __fmul_rn(go, inv) : go;
            for (int p = p0; p < p1; ++p)
                K.grad_h[(int64_t)(order ? order[p] : p) * K.ld_g + j] += a;
        }
    }
}

inline bool scope_mode_ok(int scope, int mode) {
    return scope >= 0 && scope <= 2 && mode >= DAGNN_POOL_MAX && mode <= DAGNN_POOL_MEAN;
}

}  // namespace

extern "C" int dagnn_readout_pool_batch(const dagnn_plan* pl, const dagnn_pool_job* jobs, int n, float* out, int ld_out,
                                        void* stream) {
    if (!pl || n < 0 || n > DAGNN_MAX_READOUT_JOBS) return DAGNN_EINVAL;
    if (n == 0) return DAGNN_OK;
    if (!pl->data || !jobs || !out) return DAGNN_EINVAL;
    PoolJobs J;
    for (int k = 0; k < n; ++k) {
        const dagnn_pool_job& q = jobs[k];
        if (!q.h || q.width <= 0 || !scope_mode_ok(q.scope, q.mode) || q.ld_h < q.width || q.col_off < 0 ||
            ld_out < q.col_off + q.width)
            return DAGNN_EINVAL;
        J.j[k] = q;
    }
    if (pl->B == 0) return DAGNN_OK;
    PlanLayout L = dagnn_plan_layout_words(pl->N, pl->E, pl->B, pl->num_edge_feats);
    hipLaunchKernelGGL(readout_pool_batch_kernel, dim3((unsigned)pl->B, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                       (const int32_t*)pl->data, L, J, out, ld_out);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_readout_pool_backward_batch(const dagnn_plan* pl, const dagnn_pool_bwd_job* jobs, int n,
                                                 const float* grad_out, int ld_out, void* stream) {
    if (!pl || n < 0 || n > DAGNN_MAX_READOUT_JOBS) return DAGNN_EINVAL;
    if (n == 0) return DAGNN_OK;
    if (!pl->data || !jobs || !grad_out) return DAGNN_EINVAL;
    PoolBwdJobs J;
    for (int q = 0; q < n; ++q) {
        const dagnn_pool_bwd_job& k = jobs[q];
        if (!k.grad_h || k.width <= 0 || !scope_mode_ok(k.scope, k.mode) || (k.mode == DAGNN_POOL_MAX && (!k.h || k.ld_h < k.width)) ||
            k.ld_g < k.width || k.col_off < 0 || ld_out < k.col_off + k.width)
            return DAGNN_EINVAL;
        for (int p = 0; p < q; ++p)   // two jobs adding into the same rows would race
            if (jobs[p].grad_h == k.grad_h) return DAGNN_EINVAL;
        J.j[q] = k;
    }
    if (pl->B == 0) return DAGNN_OK;
    PlanLayout L = dagnn_plan_layout_words(pl->N, pl->E, pl->B, pl->num_edge_feats);
    hipLaunchKernelGGL(readout_pool_bwd_batch_kernel, dim3((unsigned)pl->B, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                       (const int32_t*)pl->data, L, J, grad_out, ld_out);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
