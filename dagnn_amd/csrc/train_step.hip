// train_step.hip - the loss launch of a training step that also leaves the step's share of the epoch's bookkeeping.
//
// Reference path replaced, per step of `train()` (ogbg-code/main_pyg.py:39-88 for the TOK task, main_pyg_lp.py:43-74 for LP):
// the loss loop, `loss_accum += loss.item()` (a host synchronisation), the S `torch.argmax` + `cat` over the training
// logits, `decode_arr_to_seq` per row and the evaluator's set arithmetic (TOK) / the two copies to the host and `_eval_acc`
// (LP).  The loss kernels (loss.hip: seq_ce_kernel, lp.hip: class_ce_kernel) already read every logit of the step and
// already compute every row's maximum; the workgroup that draws the last ticket already sees every row.  So:
//   dagnn_seq_ce_step    seq_ce_kernel stage for stage (loss and d logits are its bits), plus tok [B, S] - each row's
//                        argmax in predict.hip's order, a by-product of the first pass over the row - and, in the last
//                        workgroup, the epoch's loss sum in float64, its step counter and the F1 counts of the B graphs
//                        (seq_f1_counts_kernel's arithmetic, a thread per graph) at their place in the epoch's table;
//   dagnn_class_ce_step  class_ce_kernel likewise, plus tok [B] and the (hits, labelled) pair of class_hits_kernel added
//                        into the epoch's pair.
// One launch per step, one read per epoch.  The softmax's maximum stays the fmaxf chain; the argmax is a reduction of its
// own over (monotone key of the value, ~column) packed into one int64 - across a thread's strided columns, the wave, the
// four waves - so the float arithmetic is untouched.  Tokens travel to the last workgroup as the row losses do: written
// before `__threadfence` and the ticket, read with agent-scope loads after it.  Integer ticket only, no float atomics.
#include <limits.h>

#include "common.h"

namespace {

__device__ __forceinline__ float ts_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float ts_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long ts_wave_max_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ long long ts_wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// predict.hip's order of logits as one integer: (monotone key of the value, ~column).  -0 and +0 share a key, every NaN
// sits on INT_MAX; the integer maximum is "greatest value, lowest column"
__device__ __forceinline__ long long ts_pack(float v, int col) {
    int key;
    if (v != v) key = INT_MAX;
    else {
        const int bits = __float_as_int(v);
        key = bits >= 0 ? bits : (int)(0x80000000u - (unsigned)bits);
    }
    return (long long)(((unsigned long long)(unsigned)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)col));
}
__device__ __forceinline__ long long ts_col(long long p) { return (long long)(0xffffffffu - (unsigned)(unsigned long long)p); }

__device__ __forceinline__ long long ts_tok(const long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------- TOK
struct SeqStepArgs {
    const float* logits; long long ld;
    const long long* y;
    int B, S, V;
    float* dlogits; long long ld_d;
    float* row_loss; float* loss;
    long long* tok; long long eos;
    const int* ref_ids; int R; const int* ref_extra;
    int* counts;            // already moved to the step's first graph
    double* epoch_sum; long long* epoch_steps;
    unsigned* counter;
};

__global__ void __launch_bounds__(256) seq_ce_step_kernel(SeqStepArgs a) {
    __shared__ float red[4];
    __shared__ long long redp[4];
    __shared__ unsigned last;
    const int B = a.B, S = a.S, V = a.V;
    const int row = blockIdx.x, b = row / S, s = row - b * S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ x = a.logits + (long long)b * a.ld + (long long)s * V;
    const long long t = a.y[(long long)b * S + s];
    float m = -INFINITY;
    long long best = LLONG_MIN;
    for (int j = tid; j < V; j += 256) {
        const float v = x[j];
        m = fmaxf(m, v);
        const long long p = ts_pack(v, j);
        best = p > best ? p : best;
    }
    m = ts_wave_max(m);
    best = ts_wave_max_ll(best);
    if (lane == 0) { red[wave] = m; redp[wave] = best; }
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) best = redp[w] > best ? redp[w] : best;
        a.tok[row] = ts_col(best);
    }
    __syncthreads();
    float z = 0.f;
    for (int j = tid; j < V; j += 256) z += __expf(x[j] - m);
    z = ts_wave_sum(z);
    if (lane == 0) red[wave] = z;
    __syncthreads();
    z = (red[0] + red[1]) + (red[2] + red[3]);
    const float lse = m + __logf(z);
    const bool ok = t >= 0 && t < V;
    if (a.dlogits) {
        const float scale = 1.0f / ((float)B * (float)S), inv = 1.0f / z;
        float* __restrict__ d = a.dlogits + (long long)b * a.ld_d + (long long)s * V;
        for (int j = tid; j < V; j += 256) d[j] = (__expf(x[j] - m) * inv - (j == t ? 1.0f : 0.0f)) * scale;
    }
    if (tid == 0) {
        a.row_loss[row] = ok ? lse - x[t] : NAN;
        __threadfence();   // (row loss and token, both this thread's stores, before the ticket)
        last = atomicAdd(a.counter, 1u) == (unsigned)(B * S - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;   // (uniform per workgroup)
    // the last row in: every row's loss and token is visible
    __threadfence();
    const int n = B * S;
    float acc = 0.f;
    for (int j = tid; j < n; j += 256) acc += __hip_atomic_load(a.row_loss + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    acc = ts_wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        const float l = ((red[0] + red[1]) + (red[2] + red[3])) / (float)n;
        a.loss[0] = l;
        a.epoch_sum[0] += (double)l;   // launches of one stream are ordered: `loss_accum += loss.item()` in step order
        a.epoch_steps[0] += 1;
    }
    if (a.ref_ids) {   // seq_f1_counts_kernel's arithmetic, a thread per graph
        const int R = a.R;
        for (int g = tid; g < B; g += 256) {
            const long long* tk = a.tok + (long long)g * S;
            const int* __restrict__ ref = a.ref_ids + (long long)g * R;
            int len = S;
            for (int i = S - 1; i >= 0; --i)
                if (ts_tok(tk + i) == a.eos) len = i;
            int n_ref = 0;
            for (int i = 0; i < R; ++i) {
                const int v = ref[i];
                bool fresh = v >= 0;
                for (int j = 0; j < i && fresh; ++j) fresh = ref[j] != v;
                n_ref += fresh;
            }
            int n_pred = 0, tp = 0;
            for (int i = 0; i < len; ++i) {
                const long long v = ts_tok(tk + i);
                bool fresh = true;
                for (int j = 0; j < i && fresh; ++j) fresh = ts_tok(tk + j) != v;
                if (!fresh) continue;
                ++n_pred;
                bool hit = false;
                for (int j = 0; j < R && !hit; ++j) hit = ref[j] >= 0 && (long long)ref[j] == v;
                tp += hit;
            }
            const int extra = a.ref_extra ? a.ref_extra[g] : 0;
            reinterpret_cast<int4*>(a.counts)[g] = make_int4(tp, n_pred, n_ref + extra, len);
        }
    }
    if (tid == 0) a.counter[0] = 0u;   // ready for the next call
}

// ---------------------------------------------------------------------------------------------- LP
enum { TS_I64 = DAGNN_LP_INT64, TS_F32 = DAGNN_LP_FLOAT32, TS_F64 = DAGNN_LP_FLOAT64 };

// lp.hip's lp_class_of: `targ.to(torch.long)`, truncation toward zero; what has no int64 value becomes -1
__device__ __forceinline__ long long ts_class_of(const void* __restrict__ targ, int kind, int64_t b) {
    if (kind == TS_I64) return reinterpret_cast<const long long*>(targ)[b];
    const double v = kind == TS_F32 ? (double)reinterpret_cast<const float*>(targ)[b] : reinterpret_cast<const double*>(targ)[b];
    if (!(v > -9.0e18 && v < 9.0e18)) return -1;
    return (long long)v;
}

// lp.hip's lp_compare: _eval_acc on one row - a NaN target is unlabelled, target and prediction are compared as values
__device__ __forceinline__ void ts_compare(const void* __restrict__ targ, int kind, int64_t b, long long pred, long long& hits,
                                           long long& labelled) {
    if (kind == TS_I64) {
        labelled += 1;
        hits += reinterpret_cast<const long long*>(targ)[b] == pred;
        return;
    }
    const double v = kind == TS_F32 ? (double)reinterpret_cast<const float*>(targ)[b] : reinterpret_cast<const double*>(targ)[b];
    if (v != v) return;
    labelled += 1;
    hits += v == (double)pred;
}

struct ClassStepArgs {
    const float* logits; long long ld;
    const void* targ; int kind;
    int B, C;
    float* dlogits; long long ld_d;
    float* row_loss; float* loss;
    long long* tok;
    long long* epoch_hits;
    double* epoch_sum; long long* epoch_steps;
    unsigned* counter;
};

__global__ void __launch_bounds__(256) class_ce_step_kernel(ClassStepArgs a) {
    __shared__ float red[4];
    __shared__ long long redp[4];
    __shared__ long long redh[4][2];
    __shared__ unsigned last;
    const int B = a.B, C = a.C;
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ x = a.logits + (long long)b * a.ld;
    const long long t = ts_class_of(a.targ, a.kind, b);
    float m = -INFINITY;
    long long best = LLONG_MIN;
    for (int j = tid; j < C; j += 256) {
        const float v = x[j];
        m = fmaxf(m, v);
        const long long p = ts_pack(v, j);
        best = p > best ? p : best;
    }
    m = ts_wave_max(m);
    best = ts_wave_max_ll(best);
    if (lane == 0) { red[wave] = m; redp[wave] = best; }
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) best = redp[w] > best ? redp[w] : best;
        a.tok[b] = ts_col(best);
    }
    __syncthreads();
    float z = 0.f;
    for (int j = tid; j < C; j += 256) z += __expf(x[j] - m);
    z = ts_wave_sum(z);
    if (lane == 0) red[wave] = z;
    __syncthreads();
    z = (red[0] + red[1]) + (red[2] + red[3]);
    const float lse = m + __logf(z);
    const bool ok = t >= 0 && t < C;
    if (a.dlogits) {
        const float scale = 1.0f / (float)B, inv = 1.0f / z;
        float* __restrict__ d = a.dlogits + (long long)b * a.ld_d;
        for (int j = tid; j < C; j += 256) d[j] = (__expf(x[j] - m) * inv - (j == t ? 1.0f : 0.0f)) * scale;
    }
    if (tid == 0) {
        a.row_loss[b] = ok ? lse - x[t] : NAN;
        __threadfence();   // (row loss and token, both this thread's stores, before the ticket)
        last = atomicAdd(a.counter, 1u) == (unsigned)(B - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;   // (uniform per workgroup)
    __threadfence();
    float acc = 0.f;
    long long hits = 0, labelled = 0;
    for (int j = tid; j < B; j += 256) {
        acc += __hip_atomic_load(a.row_loss + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ts_compare(a.targ, a.kind, j, ts_tok(a.tok + j), hits, labelled);
    }
    acc = ts_wave_sum(acc);
    hits = ts_wave_sum_ll(hits);
    labelled = ts_wave_sum_ll(labelled);
    if (lane == 0) { red[wave] = acc; redh[wave][0] = hits; redh[wave][1] = labelled; }
    __syncthreads();
    if (tid == 0) {
        const float l = ((red[0] + red[1]) + (red[2] + red[3])) / (float)B;
        a.loss[0] = l;
        a.epoch_sum[0] += (double)l;
        a.epoch_steps[0] += 1;
        a.epoch_hits[0] += (redh[0][0] + redh[1][0]) + (redh[2][0] + redh[3][0]);   // (integers: exact in any order)
        a.epoch_hits[1] += (redh[0][1] + redh[1][1]) + (redh[2][1] + redh[3][1]);
        a.counter[0] = 0u;   // ready for the next call
    }
}

}  // namespace

extern "C" int dagnn_seq_ce_step(const float* logits, int64_t ld, const int64_t* y, int B, int S, int V, float* dlogits,
                                 int64_t ld_d, float* row_loss, float* loss, int64_t* tok, int64_t eos_id, const int32_t* ref_ids,
                                 int R, const int32_t* ref_extra, int32_t* counts, int64_t counts_rows, int64_t graph_offset,
                                 double* epoch_sum, int64_t* epoch_steps, unsigned* counter, void* stream) {
    if (!logits || !y || !row_loss || !loss || !counter || B <= 0 || S <= 0 || V <= 0 || ld < (int64_t)S * V ||
        (dlogits && ld_d < (int64_t)S * V))
        return DAGNN_EINVAL;
    if ((int64_t)B * S >= (1ll << 31)) return DAGNN_EINVAL;
    if (!tok || !epoch_sum || !epoch_steps || ((uintptr_t)epoch_sum & 7) || ((uintptr_t)epoch_steps & 7) || R < 1 || graph_offset < 0)
        return DAGNN_EINVAL;
    if (ref_ids) {
        if (!counts || ((uintptr_t)counts & 15) || counts_rows < 0) return DAGNN_EINVAL;
        if (graph_offset > counts_rows || (int64_t)B > counts_rows - graph_offset) return DAGNN_ENOSPC;
    }
    SeqStepArgs a;
    a.logits = logits; a.ld = (long long)ld; a.y = reinterpret_cast<const long long*>(y);
    a.B = B; a.S = S; a.V = V;
    a.dlogits = dlogits; a.ld_d = (long long)ld_d; a.row_loss = row_loss; a.loss = loss;
    a.tok = reinterpret_cast<long long*>(tok); a.eos = (long long)eos_id;
    a.ref_ids = ref_ids; a.R = R; a.ref_extra = ref_extra;
    a.counts = ref_ids ? counts + 4 * graph_offset : nullptr;
    a.epoch_sum = epoch_sum; a.epoch_steps = reinterpret_cast<long long*>(epoch_steps); a.counter = counter;
    hipLaunchKernelGGL(seq_ce_step_kernel, dim3((unsigned)(B * S)), dim3(256), 0, (hipStream_t)stream, a);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_class_ce_step(const float* logits, int64_t ld, const void* targ, int targ_kind, int B, int C, float* dlogits,
                                   int64_t ld_d, float* row_loss, float* loss, int64_t* tok, int64_t* epoch_hits, double* epoch_sum,
                                   int64_t* epoch_steps, unsigned* counter, void* stream) {
    const bool kind_ok = targ_kind == TS_I64 || targ_kind == TS_F32 || targ_kind == TS_F64;
    if (!logits || !targ || !row_loss || !loss || !counter || !kind_ok || B <= 0 || C <= 0 || ld < C || (dlogits && ld_d < C))
        return DAGNN_EINVAL;
    if (!tok || !epoch_hits || !epoch_sum || !epoch_steps || ((uintptr_t)epoch_hits & 7) || ((uintptr_t)epoch_sum & 7) ||
        ((uintptr_t)epoch_steps & 7))
        return DAGNN_EINVAL;
    ClassStepArgs a;
    a.logits = logits; a.ld = (long long)ld; a.targ = targ; a.kind = targ_kind; a.B = B; a.C = C;
    a.dlogits = dlogits; a.ld_d = (long long)ld_d; a.row_loss = row_loss; a.loss = loss;
    a.tok = reinterpret_cast<long long*>(tok); a.epoch_hits = reinterpret_cast<long long*>(epoch_hits);
    a.epoch_sum = epoch_sum; a.epoch_steps = reinterpret_cast<long long*>(epoch_steps); a.counter = counter;
    hipLaunchKernelGGL(class_ce_step_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
