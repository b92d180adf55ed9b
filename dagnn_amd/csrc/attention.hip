// Attention weights of a finished evaluation pass, scattered to original edge ids (dagnn_attention_weights, include/dagnn_hip.h).
//
// Additive kinds (attn_h, attn_x, self_attn_h, self_attn_x): two launches for ALL (direction, stacked layer) cells.
//   1. attn_node_scores: one wave per (cell, kind, node) row: w . row[:dim] (+ vid[node mod vid_mod]) -> key_score / query_score.
//      float4 loads where base, pitch and weight vector are 16-byte aligned, a scalar tail / scalar rows otherwise.
//   2. attn_segment_softmax: one wave per (cell, rowrec slot): lanes over the row's CSR slots, score = key_score[col] + gain . feat,
//      PyG's softmax (running max / sum per lane beyond 64 slots, merged once), alpha / logit stored at eidx[slot].
// Multiplicative (mattn_h): one launch, attn_mult_softmax: the same walk, the score of a slot is an H-long dot of the target's
// projected query with the source's projected key (+ the edge term), one slot at a time by the whole wave.
// Every edge id is written exactly once; no atomics, no intermediate of E x H.
#include "common.h"

namespace {

constexpr int AT = 256;           // threads per workgroup: 4 waves, one row each
constexpr int AW = AT / DAGNN_WAVE;

struct AttnArgs {
    dagnn_attn_cell cell[DAGNN_ATTN_MAX_CELLS];
    int num_cells, vid_mod, N, E, R, want_query;
    float* key_score;
    float* query_score;
    float* alpha;
    float* logit;
};

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// one wave: w[:dim] . row[:dim], the same value in every lane
__device__ __forceinline__ float wave_dot(const float* __restrict__ row, const float* __restrict__ w, int dim, bool vec, int lane) {
    float acc = 0.f;
    int done = 0;
    if (vec) {
        const int d4 = dim >> 2;
        const float4* r4 = reinterpret_cast<const float4*>(row);
        const float4* w4 = reinterpret_cast<const float4*>(w);
        for (int c = lane; c < d4; c += DAGNN_WAVE) {
            const float4 a = r4[c], b = w4[c];
            acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
        }
        done = d4 << 2;
    }
    for (int k = done + lane; k < dim; k += DAGNN_WAVE) acc = fmaf(row[k], w[k], acc);
    return wave_sum(acc);
}

__global__ __launch_bounds__(AT) void attn_node_scores(AttnArgs A) {
    const int lane = threadIdx.x & (DAGNN_WAVE - 1);
    const int kinds = A.want_query ? 2 : 1;
    const int64_t total = (int64_t)A.num_cells * kinds * A.N;
    const int64_t stride = (int64_t)gridDim.x * AW;
    for (int64_t g = (int64_t)blockIdx.x * AW + (threadIdx.x >> 6); g < total; g += stride) {
        const int c = (int)(g / ((int64_t)kinds * A.N));
        const int64_t rem = g - (int64_t)c * kinds * A.N;
        const int kind = (int)(rem / A.N);
        const int u = (int)(rem - (int64_t)kind * A.N);
        const dagnn_attn_cell& C = A.cell[c];
        const float* src = kind ? C.query : C.key;
        float* out = (kind ? A.query_score : A.key_score) + (int64_t)c * A.N;
        if (!src) {   // (self-attention has no query part)
            if (lane == 0) out[u] = 0.f;
            continue;
        }
        const float* w = kind ? C.w_query : C.w_key;
        const int ld = kind ? C.ld_query : C.ld_key, dim = kind ? C.query_dim : C.key_dim;
        const bool vec = aligned16(src) && aligned16(w) && (ld & 3) == 0;
        float s = wave_dot(src + (int64_t)u * ld, w, dim, vec, lane);
        const float* vid = kind ? C.vid_query : C.vid_key;
        if (vid) s += vid[u % A.vid_mod];
        if (lane == 0) out[u] = s;
    }
}

// PyG's softmax over one segment [eb, ee) by one wave.  `score(base, lane)`: the score of slot base + lane in that lane
// (any value beyond ee); called by the whole wave, so it may be cooperative.  `extra`: what the logit adds to the score.
template <class ScoreFn>
__device__ __forceinline__ void segment_softmax(ScoreFn score, int eb, int ee, float extra, const int32_t* __restrict__ eidx,
                                                float* __restrict__ alpha, float* __restrict__ logit, int E, int lane) {
    const int deg = ee - eb;
    if (deg <= DAGNN_WAVE) {
        const bool on = lane < deg;
        const float sc = score(eb, lane);
        const float m = wave_max(on ? sc : -INFINITY);
        const float ex = on ? expf(sc - m) : 0.f;
        const float denom = wave_sum(ex) + 1e-16f;
        if (on) {
            const int e = eidx[eb + lane];
            if ((unsigned)e < (unsigned)E) {
                alpha[e] = ex / denom;
                if (logit) logit[e] = sc + extra;
            }
        }
        return;
    }
    // more than one wave of slots: running (max, sum) per lane, merged once, then a second walk that stores
    float m_l = -INFINITY, s_l = 0.f;
    for (int base = eb; base < ee; base += DAGNN_WAVE) {
        const float sc = score(base, lane);
        if (base + lane < ee) {
            const float m_new = fmaxf(m_l, sc);
            s_l = s_l * expf(m_l - m_new) + expf(sc - m_new);   // (first element: 0 * exp(-inf) = 0)
            m_l = m_new;
        }
    }
    const float m = wave_max(m_l);
    const float denom = wave_sum(m_l == -INFINITY ? 0.f : s_l * expf(m_l - m)) + 1e-16f;
    for (int base = eb; base < ee; base += DAGNN_WAVE) {
        const float sc = score(base, lane);
        if (base + lane < ee) {
            const int e = eidx[base + lane];
            if ((unsigned)e < (unsigned)E) {
                alpha[e] = expf(sc - m) / denom;
                if (logit) logit[e] = sc + extra;
            }
        }
    }
}

__global__ __launch_bounds__(AT) void attn_segment_softmax(const int32_t* __restrict__ plan, PlanLayout L, AttnArgs A) {
    const int lane = threadIdx.x & (DAGNN_WAVE - 1);
    const int64_t total = (int64_t)A.num_cells * A.N;
    const int64_t stride = (int64_t)gridDim.x * AW;
    for (int64_t g = (int64_t)blockIdx.x * AW + (threadIdx.x >> 6); g < total; g += stride) {
        const int c = (int)(g / A.N);
        const int slot = (int)(g - (int64_t)c * A.N);
        const dagnn_attn_cell& C = A.cell[c];
        const int4 rec = *reinterpret_cast<const int4*>(plan + L.rowrec[C.dir] + (int64_t)slot * 16);   // {node, e_begin, e_end, graph}
        const int node = rec.x, eb = rec.y, ee = rec.z;
        if (ee <= eb || eb < 0 || ee > A.E || (unsigned)node >= (unsigned)A.N) continue;
        const int32_t* col = plan + L.col[C.dir];
        const float* eattr = reinterpret_cast<const float*>(plan + L.eattr[C.dir]);
        const float* ks = A.key_score + (int64_t)c * A.N;
        const float* gain = C.edge_gain;
        const int R = gain ? A.R : 0, N = A.N;
        float extra = 0.f;
        if (A.logit) {
            if (A.want_query) extra = A.query_score[(int64_t)c * A.N + node];
            if (C.bias) extra += C.bias[0];
        }
        auto score = [&](int base, int ln) {
            const int s = base + ln;
            if (s >= ee) return 0.f;
            const int cj = col[s];
            float v = (unsigned)cj < (unsigned)N ? ks[cj] : 0.f;
            for (int r = 0; r < R; ++r) v = fmaf(gain[r], eattr[(int64_t)s * R + r], v);
            return v;
        };
        segment_softmax(score, eb, ee, extra, plan + L.eidx[C.dir], A.alpha + (int64_t)c * A.E,
                        A.logit ? A.logit + (int64_t)c * A.E : nullptr, A.E, lane);
    }
}

__global__ __launch_bounds__(AT) void attn_mult_softmax(const int32_t* __restrict__ plan, PlanLayout L, AttnArgs A) {
    const int lane = threadIdx.x & (DAGNN_WAVE - 1);
    const int64_t total = (int64_t)A.num_cells * A.N;
    const int64_t stride = (int64_t)gridDim.x * AW;
    for (int64_t g = (int64_t)blockIdx.x * AW + (threadIdx.x >> 6); g < total; g += stride) {
        const int c = (int)(g / A.N);
        const int slot = (int)(g - (int64_t)c * A.N);
        const dagnn_attn_cell& C = A.cell[c];
        const int4 rec = *reinterpret_cast<const int4*>(plan + L.rowrec[C.dir] + (int64_t)slot * 16);
        const int node = rec.x, eb = rec.y, ee = rec.z;
        if (ee <= eb || eb < 0 || ee > A.E || (unsigned)node >= (unsigned)A.N) continue;
        const int32_t* col = plan + L.col[C.dir];
        const float* eattr = reinterpret_cast<const float*>(plan + L.eattr[C.dir]);
        const float* q = C.query + (int64_t)node * C.ld_query;
        const float* emat = C.edge_gain;
        const int R = emat ? A.R : 0, N = A.N, K = C.key_dim;
        // what the target alone decides: q . edge_vec, and q . edge_mat[:, r] per feature (R <= 2 kept in registers, else recomputed)
        float qv = 0.f;
        if (C.edge_vec) qv = wave_dot(q, C.edge_vec, K, false, lane);
        auto score = [&](int base, int ln) {
            float mine = 0.f;
            const int cnt = min(DAGNN_WAVE, ee - base);
            for (int j = 0; j < cnt; ++j) {   // the whole wave, one slot at a time
                const int s = base + j;
                const int cj = col[s];
                float acc = 0.f;
                if ((unsigned)cj < (unsigned)N) {
                    const float* k = C.key + (int64_t)cj * C.ld_key;
                    for (int t = lane; t < K; t += DAGNN_WAVE) {
                        float kv = k[t];
                        for (int r = 0; r < R; ++r) kv = fmaf(emat[(int64_t)t * R + r], eattr[(int64_t)s * R + r], kv);
                        acc = fmaf(q[t], kv, acc);
                    }
                }
                const float v = wave_sum(acc) + qv;
                if (ln == j) mine = v;
            }
            return mine;
        };
        segment_softmax(score, eb, ee, 0.f, plan + L.eidx[C.dir], A.alpha + (int64_t)c * A.E,
                        A.logit ? A.logit + (int64_t)c * A.E : nullptr, A.E, lane);
    }
}

}  // namespace

extern "C" int dagnn_attention_weights(const dagnn_plan* pl, const dagnn_attn_args* a, void* stream) {
    if (!pl || !a) return DAGNN_EINVAL;
    if (a->num_cells < 1 || a->num_cells > DAGNN_ATTN_MAX_CELLS || (a->mode != 0 && a->mode != 1)) return DAGNN_EINVAL;
    if (pl->N < 0 || pl->E < 0 || pl->N >= (int64_t(1) << 31) || pl->E >= (int64_t(1) << 31) || pl->num_edge_feats < 0) return DAGNN_EINVAL;
    const bool work = pl->E > 0 && pl->N > 0;
    bool want_query = false;
    for (int c = 0; c < a->num_cells; ++c) {
        const dagnn_attn_cell& C = a->cell[c];
        if (C.dir < 0 || C.dir > 1) return DAGNN_EINVAL;
        if (C.key_dim < 1 || C.ld_key < C.key_dim) return DAGNN_EINVAL;
        if ((C.vid_key || C.vid_query) && a->vid_mod < 1) return DAGNN_EINVAL;
        if (work && !C.key) return DAGNN_EINVAL;
        if (a->mode == 0) {
            if (work && !C.w_key) return DAGNN_EINVAL;
            if (C.query && a->logit) {
                if (!C.w_query || C.query_dim < 1 || C.ld_query < C.query_dim) return DAGNN_EINVAL;
                want_query = true;
            }
        } else {
            if (work && !C.query) return DAGNN_EINVAL;
            if (C.query && (C.query_dim != C.key_dim || C.ld_query < C.query_dim)) return DAGNN_EINVAL;
        }
    }
    if (work && (!a->alpha || !pl->data)) return DAGNN_EINVAL;
    if (work && a->mode == 0 && (!a->key_score || (want_query && !a->query_score))) return DAGNN_EINVAL;
    if (!work) return DAGNN_OK;

    AttnArgs A;
    for (int c = 0; c < DAGNN_ATTN_MAX_CELLS; ++c) A.cell[c] = a->cell[c < a->num_cells ? c : 0];
    A.num_cells = a->num_cells; A.vid_mod = a->vid_mod > 0 ? a->vid_mod : 1;
    A.N = (int)pl->N; A.E = (int)pl->E; A.R = pl->num_edge_feats; A.want_query = want_query ? 1 : 0;
    A.key_score = a->key_score; A.query_score = a->query_score; A.alpha = a->alpha; A.logit = a->logit;
    const PlanLayout L = dagnn_plan_layout_words(pl->N, pl->E, pl->B, pl->num_edge_feats);
    hipStream_t st = (hipStream_t)stream;
    auto grid = [](int64_t rows) { return (unsigned)((rows + AW - 1) / AW < 65536 ? (rows + AW - 1) / AW : 65536); };
    if (a->mode == 0) {
        hipLaunchKernelGGL(attn_node_scores, dim3(grid((int64_t)A.num_cells * (want_query ? 2 : 1) * A.N)), dim3(AT), 0, st, A);
        DAGNN_CHECK_LAUNCH();
        hipLaunchKernelGGL(attn_segment_softmax, dim3(grid((int64_t)A.num_cells * A.N)), dim3(AT), 0, st,
                           (const int32_t*)pl->data, L, A);
    } else {
        hipLaunchKernelGGL(attn_mult_softmax, dim3(grid((int64_t)A.num_cells * A.N)), dim3(AT), 0, st, (const int32_t*)pl->data, L, A);
    }
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
