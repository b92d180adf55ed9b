// rows_dev.h - what the kernels that walk rows of logits share (device only): the arg-max order, the LP task's targets and
// comparison, the F1 evaluator's set arithmetic of one graph, the cross-entropy row stage and its last-workgroup-in loss
// sum.  Every definition exists once; loss.hip, lp.hip and predict.hip are built on them, so the bits they produce agree
// by construction.
#pragma once
#include <limits.h>

#include "common.h"

// ---------------------------------------------------------------------------------------------- the order of logits
// Every value maps to a 32-bit integer key that is monotone in the value, with -0 and +0 on the same key and every NaN on
// INT_MAX (torch.argmax: NaN beats everything, the first one wins); (key, ~column) packed into one int64 makes "greatest
// value, lowest column" a single integer maximum, so merges are exact, associative and independent of the order they run in.
constexpr int KEY_NAN = INT_MAX;

static __device__ __forceinline__ int logit_key(float v) {
    if (v != v) return KEY_NAN;
    const int b = __float_as_int(v);
    return b >= 0 ? b : (int)(0x80000000u - (unsigned)b);
}
static __device__ __forceinline__ long long logit_pack(int key, int col) {
    return (long long)(((unsigned long long)(unsigned)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)col));
}
static __device__ __forceinline__ int logit_col(long long p) { return (int)(0xffffffffu - (unsigned)(unsigned long long)p); }

// ---------------------------------------------------------------------------------------------- LP targets as the reference holds them
// `targ.to(torch.long)` (kind: DAGNN_LP_*): truncation toward zero; what has no int64 value (NaN, out of range) becomes -1:
// outside [0, C)
static __device__ __forceinline__ long long class_of(const void* __restrict__ targ, int kind, int64_t b) {
    if (kind == DAGNN_LP_INT64) return reinterpret_cast<const long long*>(targ)[b];
    const double v = kind == DAGNN_LP_FLOAT32 ? (double)reinterpret_cast<const float*>(targ)[b] : reinterpret_cast<const double*>(targ)[b];
    if (!(v > -9.0e18 && v < 9.0e18)) return -1;
    return (long long)v;
}

// _eval_acc on one row: labelled = the target is not NaN; hit = target and prediction are equal AS VALUES (numpy compares a
// float target with the int64 prediction in float64: 3.0 matches class 3, 3.5 matches nothing)
static __device__ __forceinline__ void hits_compare(const void* __restrict__ targ, int kind, int64_t b, long long pred, long long& hits,
                                                    long long& labelled) {
    if (kind == DAGNN_LP_INT64) {
        labelled += 1;
        hits += reinterpret_cast<const long long*>(targ)[b] == pred;
        return;
    }
    const double v = kind == DAGNN_LP_FLOAT32 ? (double)reinterpret_cast<const float*>(targ)[b] : reinterpret_cast<const double*>(targ)[b];
    if (v != v) return;
    labelled += 1;
    hits += v == (double)pred;
}

static inline bool lp_kind_ok(int kind) { return kind == DAGNN_LP_INT64 || kind == DAGNN_LP_FLOAT32 || kind == DAGNN_LP_FLOAT64; }

// ---------------------------------------------------------------------------------------------- the evaluator's counts
// (true_positive, n_pred, n_ref + extra, len) of one graph: `tok_load(i)` is its i-th predicted token, cut at the first
// `eos`; `ref` its R label ids (negative: none).  S and R are a handful (max_seq_len = 5, label lengths of method names),
// so the set arithmetic is plain quadratic loops over the graph's own rows.
template <class TokLoad>
static __device__ __forceinline__ int4 f1_counts_of_graph(TokLoad tok_load, int S, long long eos, const int* __restrict__ ref, int R,
                                                          int extra) {
    int len = S;
    for (int i = S - 1; i >= 0; --i)
        if (tok_load(i) == eos) len = i;
    int n_ref = 0;
    for (int i = 0; i < R; ++i) {
        const int v = ref[i];
        bool fresh = v >= 0;
        for (int j = 0; j < i && fresh; ++j) fresh = ref[j] != v;
        n_ref += fresh;
    }
    int n_pred = 0, tp = 0;
    for (int i = 0; i < len; ++i) {
        const long long v = tok_load(i);
        bool fresh = true;
        for (int j = 0; j < i && fresh; ++j) fresh = tok_load(j) != v;
        if (!fresh) continue;
        ++n_pred;
        bool hit = false;
        for (int j = 0; j < R && !hit; ++j) hit = ref[j] >= 0 && (long long)ref[j] == v;
        tp += hit;
    }
    return make_int4(tp, n_pred, n_ref + extra, len);
}

// ---------------------------------------------------------------------------------------------- the cross-entropy row stage
// One workgroup of 256 threads on one row x[0, V) with target t: writes d[j] = (softmax(x)[j] - (j == t)) * scale to the row
// d = dlogits + d_off when dlogits is not null (the sum is formed behind that test, next to its use: no workgroup waits
// for it in front of the first pass) and returns - in thread 0 - the row's loss, log-sum-exp minus x[t], NaN for a target
// outside [0, V).  Under ARGMAX thread 0 also stores the row's arg-max in the order above to *tok, as soon as it is known
// (the store is long done when the caller fences).  The sums and their order are fixed (every caller's bits depend on them):
// the maximum is the fmaxf chain per thread, per wave, then over the four waves' `red`; exp(x - m) is added per thread in
// column order, per wave, then (red0 + red1) + (red2 + red3).  The arg-max is a reduction of its own over packed integers -
// across a thread's strided columns, the wave, the four waves' `redp` (unused without ARGMAX) - so the float arithmetic is
// the same with and without it.  Ends with `red` read by every thread and no barrier behind it.
template <bool ARGMAX>
static __device__ __forceinline__ float ce_row(const float* __restrict__ x, int V, long long t, float scale,
                                               float* __restrict__ dlogits, long long d_off, float* red, long long* redp,
                                               long long* tok) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m = -INFINITY;
    long long best = LLONG_MIN;
    for (int j = tid; j < V; j += 256) {
        const float v = x[j];
        m = fmaxf(m, v);
        if constexpr (ARGMAX) {
            const long long p = logit_pack(logit_key(v), j);
            best = p > best ? p : best;
        }
    }
    m = wave_max(m);
    if constexpr (ARGMAX) best = wave_max(best);
    if (lane == 0) {
        red[wave] = m;
        if constexpr (ARGMAX) redp[wave] = best;
    }
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if constexpr (ARGMAX) {
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) best = redp[w] > best ? redp[w] : best;
            *tok = logit_col(best);
        }
    }
    __syncthreads();
    float z = 0.f;
    for (int j = tid; j < V; j += 256) z += __expf(x[j] - m);
    z = wave_sum(z);
    if (lane == 0) red[wave] = z;
    __syncthreads();
    z = (red[0] + red[1]) + (red[2] + red[3]);
    const float lse = m + __logf(z);
    if (dlogits) {
        const float inv = 1.0f / z;
        float* __restrict__ d = dlogits + d_off;
        for (int j = tid; j < V; j += 256) d[j] = (__expf(x[j] - m) * inv - (j == t ? 1.0f : 0.0f)) * scale;
    }
    return tid == 0 ? (t >= 0 && t < V ? lse - x[t] : NAN) : 0.f;
}

// The hand-off to the last workgroup: thread 0 has stored its row's results; it fences them and draws an integer ticket
// (no float atomics anywhere: the loss is bitwise reproducible).  True, in every thread, in the workgroup that drew the
// last of the n tickets: every row's results are visible to agent-scope loads.  `last`: one LDS word.
static __device__ __forceinline__ bool ce_finish(unsigned* counter, int n, unsigned* last) {
    if (threadIdx.x == 0) {
        __threadfence();
        *last = atomicAdd(counter, 1u) == (unsigned)(n - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!*last) return false;   // (uniform per workgroup)
    __threadfence();
    return true;
}

// In the last workgroup: the mean of the n row losses, added in index order per thread, per wave, then
// (red0 + red1) + (red2 + red3); the value is thread 0's.  `per_row(j)` runs beside the load of row j's loss (what else the
// caller reads of that row: its loads overlap this one's).  One barrier, between the waves' stores to `red` and its reads.
template <class PerRow>
static __device__ __forceinline__ float ce_loss_sum(const float* row_loss, int n, float* red, PerRow per_row) {
    const int tid = threadIdx.x;
    float acc = 0.f;
    for (int j = tid; j < n; j += 256) {
        acc += __hip_atomic_load(row_loss + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        per_row(j);
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    return ((red[0] + red[1]) + (red[2] + red[3])) / (float)n;
}
