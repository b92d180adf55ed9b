// Sampling D-VAE decoder: `DVAE_PYG.decode(z, stochastic)` (dvae/models_pyg.py:338-396) for both decoders (NA: graph
// state = top state of the last vertex, edge head on [H_vi, H_v]; BN: graph state = sum of the top states, edge head on
// [H_vi, H_v, H0]), G independent groups of B rows in one call.
//
// Unlike teacher forcing (csrc/dvae_decode.hip), every edge decision changes the state the next decision reads, so the
// chain is one update at a time: per vertex idx the fresh update (no predecessors yet), then one update per earlier
// vertex vi = idx-1 .. 0 after that edge decision.  Each update is a fixed sequence of launches over all R rows:
//   decide  (one wave per row)   edge score from the previous update's product, the decision, the new predecessor mask,
//                                and the group's padding width P (integer atomicMax into a slot of its own per update);
//   agg     (one block per row)  padded soft-max over the precomputed keys, aggregate of the final layer-0 states;
//   gh      MFMA product         hagg * [W_hh of every layer]^T: the aggregate feeds every stacked cell;
//   cell l  (flat)               layer 0 gathers a W_ih column (one-hot input); layers above after an MFMA product.
// Work that is fixed within the chain runs once: W_ih0 * onehot is a gather, the keys and add_edge.0's H_vi part are
// formed once per vertex when its state is final, BN's H0 part once per decode.  At idx = n-1 every row is forced to
// END, which connects the loose ends at the first edge step and leaves nothing else to decide: the remaining updates of
// the reference recompute the same state from the same inputs and are skipped.
//
// States live in [R, n, HP] buffers, HP = hs rounded up to 4 with zero columns, so that every product runs the
// 16-byte-row MFMA path of dagnn_gemm_nt_bias; the weights are copied into the same padded layout inside `work`.
// No float atomics: every value is written by one thread in a fixed order, so results are bitwise repeatable.
//
// agg = gated_sum (NA): in place of its key, a vertex gets its message row once its layer-0 state is final (one
// product against the stacked state columns of the gate and the mapper, then the vertex-id columns, bg and the
// sigmoid-times), and the aggregate launch becomes a masked sum of message rows in ascending order, with no soft-max.
// The padding width P is still reduced but not read: the reference's zero padding rows contribute exactly 0.
//
// agg = attn_x (BN): the key of a vertex is one entry of the table key_type [nvt], looked up by its type when the vertex is
// final; the padded soft-max launch then serves unchanged.
#include "dvae_common.h"

namespace {

constexpr int DS_T = 256;

__host__ __device__ inline int64_t ds_pair(int idx, int vi) { return (int64_t)idx * (idx - 1) / 2 + (idx - 1 - vi); }

struct DSLayout {
    int64_t G, B, R, NE;
    int n, hs, HP, L, nvt, E1, V1, ein;
    // padded weights and inputs (float offsets into work)
    int64_t w_hh_all, b_hh_all, w_ih[DAGNN_MAX_STACKED], w_left, w_mid, w_h0, w_v1, h0p;
    // chain state
    int64_t h[DAGNN_MAX_STACKED], hagg, gh, gi, etmp, aedge, c0, key, hg, hidv, fin, succ, pbuf, end;
    // gated_sum: stacked padded state columns of Wg / Wm [2 hs, HP], the message pre-activations [R, 2 hs], messages [R, n, hs]
    int gated;
    int64_t wgm, mpre, msg;
};

bool ds_layout(const dagnn_dvae_sample_args* a, DSLayout& o) {
    if (!a || a->G <= 0 || a->B <= 0 || !dvae_decoder_ok(a) || a->end_type < 0 || a->end_type >= a->nvt ||
        (a->stochastic != 0 && a->stochastic != 1))
        return false;
    if (a->G > ((int64_t)1 << 31) || a->B > ((int64_t)1 << 31) || a->G * a->B > ((int64_t)1 << 30) || a->hs > (1 << 20) ||
        a->edge_hidden > (1 << 22) || a->vertex_hidden > (1 << 22))
        return false;
    o.G = a->G; o.B = a->B; o.R = a->G * a->B; o.n = a->n; o.hs = a->hs; o.HP = (a->hs + 3) / 4 * 4; o.L = a->L;
    o.nvt = a->nvt; o.E1 = a->edge_hidden; o.V1 = a->vertex_hidden; o.ein = (a->bn ? 3 : 2) * a->hs;
    o.NE = (int64_t)o.n * (o.n - 1) / 2;
    const int64_t R = o.R, HP = o.HP, H3 = 3 * (int64_t)o.hs, n = o.n;
    if (R * n * (HP > o.E1 ? HP : o.E1) >= ((int64_t)1 << 40) || R * H3 * o.L >= ((int64_t)1 << 40) ||
        (int64_t)n * HP > INT32_MAX || (int64_t)(n - 1) * o.E1 > INT32_MAX || H3 * o.L > INT32_MAX)
        return false;
    int64_t at = 0;
    o.w_hh_all = dvae_take(at, o.L * H3 * HP);
    o.b_hh_all = dvae_take(at, o.L * H3);
    for (int l = 0; l < o.L; ++l) o.w_ih[l] = l == 0 ? 0 : dvae_take(at, H3 * HP);
    o.w_left = dvae_take(at, (int64_t)o.E1 * HP);
    o.w_mid = dvae_take(at, (int64_t)o.E1 * HP);
    o.w_h0 = a->bn ? dvae_take(at, (int64_t)o.E1 * HP) : 0;
    o.w_v1 = dvae_take(at, (int64_t)o.V1 * HP);
    o.h0p = dvae_take(at, R * HP);
    for (int l = 0; l < o.L; ++l) o.h[l] = dvae_take(at, R * n * HP);
    o.hagg = dvae_take(at, R * HP);
    o.gh = dvae_take(at, R * H3 * o.L);
    o.gi = dvae_take(at, R * H3);
    o.etmp = dvae_take(at, R * o.E1);
    o.aedge = dvae_take(at, R * (n - 1) * o.E1);
    o.c0 = a->bn ? dvae_take(at, R * o.E1) : 0;
    o.key = dvae_take(at, R * n);
    o.hg = dvae_take(at, R * HP);
    o.hidv = dvae_take(at, R * o.V1);
    o.fin = dvae_take(at, R);
    o.succ = dvae_take(at, R);
    o.pbuf = dvae_take(at, o.NE * o.G);
    o.gated = a->agg == DAGNN_DVAE_AGG_GATED_SUM;
    if (o.gated) {
        o.wgm = dvae_take(at, 2 * (int64_t)o.hs * HP);
        o.mpre = dvae_take(at, R * 2 * o.hs);
        o.msg = dvae_take(at, R * n * o.hs);
    }
    o.end = at;
    return true;
}

inline unsigned ds_blocks(int64_t work, int per_block = DS_T) {
    const int64_t b = (work + per_block - 1) / per_block;
    return (unsigned)(b < 65536 * 16 ? b : 65536 * 16);   // flat kernels stride over the rest
}

// dst[r, c] = c < cols ? src[r * lds + c] : 0, for r < rows, c < ldd
__global__ void __launch_bounds__(DS_T) ds_pad_kernel(int64_t rows, int cols, const float* __restrict__ src, int64_t lds,
                                                      float* __restrict__ dst, int ldd) {
    const int64_t total = rows * ldd;
    for (int64_t e = (int64_t)blockIdx.x * DS_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * DS_T) {
        const int64_t r = e / ldd;
        const int c = (int)(e - r * ldd);
        dst[e] = c < cols ? src[r * lds + c] : 0.f;
    }
}

__global__ void __launch_bounds__(DS_T) ds_init_kernel(int64_t R, int n, int start_type, int32_t* __restrict__ types,
                                                       uint32_t* __restrict__ preds, int32_t* __restrict__ nv,
                                                       int32_t* __restrict__ fin, uint32_t* __restrict__ succ) {
    for (int64_t r = (int64_t)blockIdx.x * DS_T + threadIdx.x; r < R; r += (int64_t)gridDim.x * DS_T) {
        for (int v = 0; v < n; ++v) {
            types[r * n + v] = v == 0 ? start_type : -1;
            preds[r * n + v] = 0u;
        }
        nv[r] = 1;
        fin[r] = 0;
        succ[r] = 0u;
    }
}

// one stacked GRU cell of vertex idx for every row that has the vertex.  gh = NULL: the aggregate is zero (no
// predecessors in the whole group), so W_hh * 0 + b_hh is b_hh exactly; hagg = NULL: the hidden input is zero.
__global__ void __launch_bounds__(DS_T) ds_cell_kernel(int64_t R, int n, int hs, int HP, int idx, int l, int nvt,
                                                       const int32_t* __restrict__ types, const int32_t* __restrict__ nv,
                                                       const float* __restrict__ w_ih0, const float* __restrict__ b_ih0,
                                                       const float* __restrict__ gi, const float* __restrict__ gh, int64_t ld_gh,
                                                       const float* __restrict__ b_hh, const float* __restrict__ hagg,
                                                       float* __restrict__ h) {
    const int64_t total = R * hs;
    for (int64_t e = (int64_t)blockIdx.x * DS_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * DS_T) {
        const int64_t r = e / hs;
        const int c = (int)(e - r * hs);
        if (nv[r] <= idx) continue;
        float ir, iz, in_;
        if (l == 0) {
            int t = types[r * n + idx];
            t = t < 0 ? 0 : (t >= nvt ? nvt - 1 : t);   // (types are written by this file; never read outside W_ih)
            ir = w_ih0[(int64_t)c * nvt + t] + b_ih0[c];
            iz = w_ih0[(int64_t)(hs + c) * nvt + t] + b_ih0[hs + c];
            in_ = w_ih0[(int64_t)(2 * hs + c) * nvt + t] + b_ih0[2 * hs + c];
        } else {
            const float* g = gi + r * 3 * hs;
            ir = g[c]; iz = g[hs + c]; in_ = g[2 * hs + c];
        }
        float hr, hz, hn;
        if (gh) {
            const float* g = gh + r * ld_gh + (int64_t)l * 3 * hs;
            hr = g[c]; hz = g[hs + c]; hn = g[2 * hs + c];
        } else {
            hr = b_hh[c]; hz = b_hh[hs + c]; hn = b_hh[2 * hs + c];
        }
        const float rr = 1.0f / (1.0f + expf(-(ir + hr))), z = 1.0f / (1.0f + expf(-(iz + hz)));
        const float nn = tanhf(in_ + rr * hn);
        const float hp = hagg ? hagg[r * HP + c] : 0.f;
        h[(r * n + idx) * HP + c] = nn + z * (hp - nn);   // torch's GRUCell: (h - n) * z + n
    }
}

// key of vertex v once its layer-0 state is final: w_key . h + vid_bias[v] (one wave per row)
__global__ void __launch_bounds__(DS_T) ds_key_kernel(int64_t R, int n, int hs, int HP, int v, const float* __restrict__ h0l,
                                                      const float* __restrict__ w_key, const float* __restrict__ vid_bias,
                                                      float* __restrict__ key) {
    const int64_t r = (int64_t)blockIdx.x * (DS_T / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= R) return;
    const float* x = h0l + (r * n + v) * HP;
    float s = 0.f;
    for (int c = lane; c < hs; c += 64) s = fmaf(w_key[c], x[c], s);
    s = wave_sum(s);
    if (lane == 0) key[r * n + v] = s + (vid_bias ? vid_bias[v] : 0.f);
}

// attn_x: the key of vertex v is the table entry of its type (0 for a row that has no vertex v: never read)
__global__ void __launch_bounds__(DS_T) ds_type_key_kernel(int64_t R, int n, int nvt, int v, const int32_t* __restrict__ types,
                                                           const float* __restrict__ key_type, float* __restrict__ key) {
    for (int64_t r = (int64_t)blockIdx.x * DS_T + threadIdx.x; r < R; r += (int64_t)gridDim.x * DS_T) {
        const int t = types[r * n + v];
        key[r * n + v] = t < 0 ? 0.f : key_type[t < nvt ? t : nvt - 1];
    }
}

// graph state of every row (stride HP, zero pad): NA the top state of its last vertex, BN the sum of its top states
__global__ void __launch_bounds__(DS_T) ds_graph_state_kernel(int64_t R, int n, int hs, int HP, int bn, const int32_t* __restrict__ nv,
                                                              const float* __restrict__ htop, float* __restrict__ hg) {
    const int64_t total = R * HP;
    for (int64_t e = (int64_t)blockIdx.x * DS_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * DS_T) {
        const int64_t r = e / HP;
        const int c = (int)(e - r * HP);
        const int cnt = nv[r];
        float s = 0.f;
        if (c < hs) {
            if (bn) {
                for (int u = 0; u < cnt; ++u) s += htop[(r * n + u) * HP + c];
            } else {
                s = htop[(r * n + cnt - 1) * HP + c];
            }
        }
        hg[e] = s;
    }
}

// type of vertex idx (one wave per row): add_vertex.2 over relu(add_vertex.0 output), then argmax or the draw mapped
// through np.random.choice's rule (float64 cdf of the fp32 soft-max, normalised by its last entry, searchsorted right).
// forced >= 0: that type for every row (idx = n-1).  Rows already finished keep their vertex count.
__global__ void __launch_bounds__(DS_T) ds_type_kernel(int64_t R, int64_t B, int n, int V1, int nvt, int idx, int forced,
                                                       int stochastic, const float* __restrict__ hid, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, const float* __restrict__ u_type,
                                                       int32_t* __restrict__ types, int32_t* __restrict__ nv,
                                                       const int32_t* __restrict__ fin) {
    __shared__ float logit[DS_T / 64][DAGNN_DVAE_MAX_TYPES];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (DS_T / 64) + w;
    if (r >= R) return;
    int choice = forced;
    if (forced < 0) {
        const float* x = hid + r * V1;
        for (int t = 0; t < nvt; ++t) {
            float s = 0.f;
            for (int c = lane; c < V1; c += 64) s = fmaf(fmaxf(x[c], 0.f), w2[(int64_t)t * V1 + c], s);
            s = wave_sum(s);
            if (lane == 0) logit[w][t] = s + b2[t];
        }
        if (lane == 0) {
            float m = logit[w][0];
            int arg = 0;
            for (int t = 1; t < nvt; ++t)
                if (logit[w][t] > m) { m = logit[w][t]; arg = t; }
            if (stochastic) {
                float den = 0.f;
                for (int t = 0; t < nvt; ++t) den += expf(logit[w][t] - m);
                double tot = 0.0;
                for (int t = 0; t < nvt; ++t) tot += (double)(expf(logit[w][t] - m) / den);
                const int64_t g = r / B, b = r - g * B;
                const double u = (double)u_type[(g * n + idx) * B + b];
                double cum = 0.0;
                arg = nvt - 1;
                for (int t = 0; t < nvt; ++t) {
                    cum += (double)(expf(logit[w][t] - m) / den);
                    if (cum / tot > u) { arg = t; break; }
                }
            }
            choice = arg;
        }
    }
    if (lane == 0 && !fin[r]) {
        types[r * n + idx] = choice;
        nv[r] = idx + 1;
    }
}

// edge step (idx, vi), one wave per row that has vertex idx: a finished row decides nothing; a row whose new vertex is
// END connects every earlier vertex without successors at the first step and finishes; the others score
// sigmoid(add_edge(...)) and keep the edge on u < score (sampling) or score > 0.5.  Every row then raises its group's
// padding width P of the update that follows (integer max: order-free).
__global__ void __launch_bounds__(DS_T) ds_decide_kernel(int64_t R, int64_t B, int n, int E1, int idx, int vi, int end_type,
                                                         int score, int stochastic, const float* __restrict__ etmp,
                                                         const float* __restrict__ aedge, const float* __restrict__ c0,
                                                         const float* __restrict__ w2, const float* __restrict__ b2,
                                                         const float* __restrict__ u_edge, int64_t NE,
                                                         const int32_t* __restrict__ types, const int32_t* __restrict__ nv,
                                                         int32_t* __restrict__ fin, uint32_t* __restrict__ succ,
                                                         uint32_t* __restrict__ preds, int32_t* __restrict__ pslot) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (DS_T / 64) + (threadIdx.x >> 6);
    if (r >= R || nv[r] <= idx) return;
    const int64_t g = r / B, b = r - g * B;
    const int64_t p = ds_pair(idx, vi);
    uint32_t* pm = preds + r * n + idx;
    if (!fin[r]) {
        if (vi == idx - 1 && types[r * n + idx] == end_type) {
            if (lane == 0) {
                const uint32_t loose = ~succ[r] & ((1u << idx) - 1u);
                *pm |= loose;
                succ[r] |= loose;
                fin[r] = 1;
            }
        } else if (score) {
            const float* x = etmp + r * E1;
            const float* a = aedge + (r * (n - 1) + vi) * E1;
            const float* h0 = c0 ? c0 + r * E1 : nullptr;
            float s = 0.f;
            for (int c = lane; c < E1; c += 64) {
                float pre = x[c] + a[c];
                if (h0) pre += h0[c];
                s = fmaf(fmaxf(pre, 0.f), w2[c], s);
            }
            s = wave_sum(s);
            if (lane == 0) {
                const float prob = 1.0f / (1.0f + expf(-(s + b2[0])));
                const bool keep = stochastic ? (u_edge[(g * NE + p) * B + b] < prob) : (prob > 0.5f);
                if (keep) {
                    *pm |= 1u << vi;
                    succ[r] |= 1u << vi;
                }
            }
        }
    }
    if (lane == 0) atomicMax(pslot + p * (R / B) + g, __popc(*pm));
}

// the reference's padded soft-max aggregate of vertex idx (one block per row): P slots, the real predecessors in
// ascending order score their keys, the padding scores 0; the aggregate sums the final layer-0 states
__global__ void __launch_bounds__(DS_T) ds_agg_kernel(int64_t B, int n, int hs, int HP, int idx, int64_t p, int64_t G,
                                                      const int32_t* __restrict__ nv, const uint32_t* __restrict__ preds,
                                                      const int32_t* __restrict__ pslot, const float* __restrict__ key,
                                                      const float* __restrict__ h0l, float* __restrict__ hagg) {
    __shared__ float sc[DAGNN_DVAE_MAX_N];
    __shared__ int ids[DAGNN_DVAE_MAX_N];
    __shared__ int sCnt;
    const int64_t r = blockIdx.x;
    if (nv[r] <= idx) return;
    const int P = pslot[p * G + r / B];
    if (threadIdx.x == 0) {
        const uint32_t m = preds[r * n + idx];
        int c = 0;
        for (int u = 0; u < idx; ++u)
            if (m >> u & 1u) { ids[c] = u; sc[c] = key[r * n + u]; ++c; }
        float mx = -INFINITY, den = 0.f;
        for (int j = 0; j < P; ++j) mx = fmaxf(mx, j < c ? sc[j] : 0.f);
        for (int j = 0; j < P; ++j) den += expf((j < c ? sc[j] : 0.f) - mx);
        for (int j = 0; j < c; ++j) sc[j] = expf(sc[j] - mx) / den;   // padded slots score 0 and only take weight
        sCnt = c;
    }
    __syncthreads();
    const int cnt = sCnt;
    for (int c = threadIdx.x; c < hs; c += DS_T) {
        float a = 0.f;
        for (int j = 0; j < cnt; ++j) a = fmaf(sc[j], h0l[(r * n + ids[j]) * HP + c], a);
        hagg[r * HP + c] = a;
    }
}

// message of vertex v for every row, from its product row [gate | mapper]: vertex-id columns, bg, sigmoid-times
__global__ void __launch_bounds__(DS_T) ds_gated_msg_kernel(int64_t R, int n, int hs, int v, const float* __restrict__ mpre,
                                                            const float* __restrict__ gate_w, const float* __restrict__ gate_b,
                                                            const float* __restrict__ mapper_w, float* __restrict__ msg) {
    const int64_t total = R * hs;
    for (int64_t e = (int64_t)blockIdx.x * DS_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * DS_T) {
        const int64_t r = e / hs;
        const int c = (int)(e - r * hs);
        const float* p = mpre + r * 2 * hs;
        const float g = 1.0f / (1.0f + expf(-(p[c] + gate_w[(int64_t)c * (hs + n) + hs + v] + gate_b[c])));
        msg[(r * n + v) * hs + c] = g * (p[hs + c] + mapper_w[(int64_t)c * (hs + n) + hs + v]);
    }
}

// gated_sum aggregate of vertex idx: the messages of its predecessors so far, ascending (stride HP, zero pad)
__global__ void __launch_bounds__(DS_T) ds_gated_agg_kernel(int64_t R, int n, int hs, int HP, int idx, const int32_t* __restrict__ nv,
                                                            const uint32_t* __restrict__ preds, const float* __restrict__ msg,
                                                            float* __restrict__ hagg) {
    const int64_t total = R * HP;
    for (int64_t e = (int64_t)blockIdx.x * DS_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * DS_T) {
        const int64_t r = e / HP;
        const int c = (int)(e - r * HP);
        if (nv[r] <= idx) continue;
        float a = 0.f;
        if (c < hs) {
            const uint32_t m = preds[r * n + idx];
            for (int u = 0; u < idx; ++u)
                if (m >> u & 1u) a += msg[(r * n + u) * hs + c];
        }
        hagg[e] = a;
    }
}

__global__ void __launch_bounds__(DS_T) ds_states_kernel(int64_t R, int n, int hs, int HP, const int32_t* __restrict__ nv,
                                                         const float* __restrict__ htop, float* __restrict__ out) {
    const int64_t total = R * n * hs;
    for (int64_t e = (int64_t)blockIdx.x * DS_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * DS_T) {
        const int64_t rv = e / hs, r = rv / n;
        const int c = (int)(e - rv * hs), v = (int)(rv - r * n);
        out[e] = v < nv[r] ? htop[rv * HP + c] : 0.f;
    }
}

#define DS_TRY(x)                        \
    do {                                 \
        const int rc_ = (x);             \
        if (rc_ != DAGNN_OK) return rc_; \
    } while (0)

// C[M, Nc] (ldc) = A[M, K] (lda) * W[Nc, K]^T + bias on the MFMA product of gemm_f32.hip
int ds_gemm(hipStream_t st, int64_t M, int Nc, int K, const float* A, int lda, const float* W, const float* bias, float* C, int ldc) {
    dagnn_gemm_group g{A, W, bias, C};
    return dagnn_gemm_nt_bias(&g, 1, M, Nc, K, lda, K, ldc, st);
}

int ds_pad(hipStream_t st, int64_t rows, int cols, const float* src, int64_t lds, float* dst, int ldd) {
    hipLaunchKernelGGL(ds_pad_kernel, dim3(ds_blocks(rows * ldd)), dim3(DS_T), 0, st, rows, cols, src, lds, dst, ldd);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

bool ds_pointers_ok(const dagnn_dvae_sample_args* a) {
    return dvae_weights_ok(a) && a->types && a->preds && a->nv && a->work && (!a->stochastic || (a->u_type && a->u_edge));
}

}  // namespace

extern "C" size_t dagnn_dvae_sample_work_bytes(const dagnn_dvae_sample_args* a) {
    DSLayout o;
    return ds_layout(a, o) ? (size_t)o.end * sizeof(float) : 0;
}

extern "C" int dagnn_dvae_sample(const dagnn_dvae_sample_args* a, void* stream) {
    DSLayout o;
    if (!ds_layout(a, o) || !ds_pointers_ok(a)) return DAGNN_EINVAL;
    if (a->work_bytes < (size_t)o.end * sizeof(float)) return DAGNN_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    float* W = a->work;
    const int64_t R = o.R, B = o.B, G = o.G, H3 = 3 * (int64_t)o.hs;
    const int n = o.n, hs = o.hs, HP = o.HP, L = o.L, E1 = o.E1;
    int32_t* fin = reinterpret_cast<int32_t*>(W + o.fin);
    uint32_t* succ = reinterpret_cast<uint32_t*>(W + o.succ);
    int32_t* pslot = reinterpret_cast<int32_t*>(W + o.pbuf);
    float* htop = W + o.h[L - 1];
    const int ldh = n * HP;
    const unsigned row_waves = (unsigned)((R + DS_T / 64 - 1) / (DS_T / 64));

    // padded copies of the weights and of H0 (every product below then runs on 16-byte rows)
    for (int l = 0; l < L; ++l) {
        DS_TRY(ds_pad(st, H3, hs, a->w_hh[l], hs, W + o.w_hh_all + l * H3 * HP, HP));
        DS_TRY(ds_pad(st, 1, (int)H3, a->b_hh[l], H3, W + o.b_hh_all + l * H3, (int)H3));
        if (l > 0) DS_TRY(ds_pad(st, H3, hs, a->w_ih[l], hs, W + o.w_ih[l], HP));
    }
    DS_TRY(ds_pad(st, E1, hs, a->ae_w1, o.ein, W + o.w_left, HP));
    DS_TRY(ds_pad(st, E1, hs, a->ae_w1 + hs, o.ein, W + o.w_mid, HP));
    if (a->bn) DS_TRY(ds_pad(st, E1, hs, a->ae_w1 + 2 * hs, o.ein, W + o.w_h0, HP));
    DS_TRY(ds_pad(st, o.V1, hs, a->av_w1, hs, W + o.w_v1, HP));
    DS_TRY(ds_pad(st, R, hs, a->h0, hs, W + o.h0p, HP));
    if (o.gated) {
        DS_TRY(ds_pad(st, hs, hs, a->gate_w, hs + n, W + o.wgm, HP));
        DS_TRY(ds_pad(st, hs, hs, a->mapper_w, hs + n, W + o.wgm + (int64_t)hs * HP, HP));
    }
    for (int l = 0; l < L; ++l)
        if (hipMemsetAsync(W + o.h[l], 0, (size_t)R * n * HP * sizeof(float), st) != hipSuccess) return DAGNN_EHIP(hipGetLastError());
    if (hipMemsetAsync(pslot, 0, (size_t)o.NE * G * sizeof(int32_t), st) != hipSuccess) return DAGNN_EHIP(hipGetLastError());
    hipLaunchKernelGGL(ds_init_kernel, dim3(ds_blocks(R)), dim3(DS_T), 0, st, R, n, a->start_type, a->types, a->preds, a->nv,
                       fin, succ);
    DAGNN_CHECK_LAUNCH();
    if (a->bn) DS_TRY(ds_gemm(st, R, E1, HP, W + o.h0p, HP, W + o.w_h0, nullptr, W + o.c0, E1));

    // the stacked cells of one update of vertex idx; agg = NULL: no predecessors anywhere (the fresh update)
    auto cells = [&](int idx, const float* agg, bool from_agg) -> int {
        if (from_agg) DS_TRY(ds_gemm(st, R, (int)(L * H3), HP, agg, HP, W + o.w_hh_all, W + o.b_hh_all, W + o.gh, (int)(L * H3)));
        for (int l = 0; l < L; ++l) {
            if (l > 0)
                DS_TRY(ds_gemm(st, R, (int)H3, HP, W + o.h[l - 1] + (int64_t)idx * HP, ldh, W + o.w_ih[l], a->b_ih[l], W + o.gi,
                               (int)H3));
            hipLaunchKernelGGL(ds_cell_kernel, dim3(ds_blocks(R * hs)), dim3(DS_T), 0, st, R, n, hs, HP, idx, l, o.nvt, a->types,
                               a->nv, a->w_ih[0], a->b_ih[0], W + o.gi, from_agg ? W + o.gh : nullptr, L * H3, a->b_hh[l], agg,
                               W + o.h[l]);
            DAGNN_CHECK_LAUNCH();
        }
        return DAGNN_OK;
    };
    // vertex idx is final: its key (gated_sum: its message) and add_edge.0's H_vi part (+ bias) for every later edge step
    auto finalize = [&](int idx) -> int {
        if (o.gated) {
            DS_TRY(ds_gemm(st, R, 2 * hs, HP, W + o.h[0] + (int64_t)idx * HP, ldh, W + o.wgm, nullptr, W + o.mpre, 2 * hs));
            hipLaunchKernelGGL(ds_gated_msg_kernel, dim3(ds_blocks(R * hs)), dim3(DS_T), 0, st, R, n, hs, idx, W + o.mpre, a->gate_w,
                               a->gate_b, a->mapper_w, W + o.msg);
        } else if (a->agg == DAGNN_DVAE_AGG_ATTN_X) {
            hipLaunchKernelGGL(ds_type_key_kernel, dim3(ds_blocks(R)), dim3(DS_T), 0, st, R, n, o.nvt, idx, a->types, a->key_type,
                               W + o.key);
        } else {
            hipLaunchKernelGGL(ds_key_kernel, dim3(row_waves), dim3(DS_T), 0, st, R, n, hs, HP, idx, W + o.h[0], a->w_key, a->vid_bias,
                               W + o.key);
        }
        DAGNN_CHECK_LAUNCH();
        return ds_gemm(st, R, E1, HP, htop + (int64_t)idx * HP, ldh, W + o.w_left, a->ae_b1, W + o.aedge + (int64_t)idx * E1,
                       (n - 1) * E1);
    };

    // vertex 0: START with H0 as its aggregate
    DS_TRY(cells(0, W + o.h0p, true));
    DS_TRY(finalize(0));
    for (int idx = 1; idx < n; ++idx) {
        const bool last = idx == n - 1;
        if (!last) {
            hipLaunchKernelGGL(ds_graph_state_kernel, dim3(ds_blocks(R * HP)), dim3(DS_T), 0, st, R, n, hs, HP, a->bn, a->nv, htop,
                               W + o.hg);
            DAGNN_CHECK_LAUNCH();
            DS_TRY(ds_gemm(st, R, o.V1, HP, W + o.hg, HP, W + o.w_v1, a->av_b1, W + o.hidv, o.V1));
        }
        hipLaunchKernelGGL(ds_type_kernel, dim3(row_waves), dim3(DS_T), 0, st, R, B, n, o.V1, o.nvt, idx, last ? a->end_type : -1,
                           a->stochastic, W + o.hidv, a->av_w2, a->av_b2, a->u_type, a->types, a->nv, fin);
        DAGNN_CHECK_LAUNCH();
        DS_TRY(cells(idx, nullptr, false));
        for (int vi = idx - 1; vi >= 0; --vi) {
            if (last && vi < idx - 1) break;   // every row finished at the first step: the rest recomputes the same state
            if (!last) DS_TRY(ds_gemm(st, R, E1, HP, htop + (int64_t)idx * HP, ldh, W + o.w_mid, nullptr, W + o.etmp, E1));
            hipLaunchKernelGGL(ds_decide_kernel, dim3(row_waves), dim3(DS_T), 0, st, R, B, n, E1, idx, vi, a->end_type, last ? 0 : 1,
                               a->stochastic, W + o.etmp, W + o.aedge, a->bn ? W + o.c0 : nullptr, a->ae_w2, a->ae_b2, a->u_edge,
                               o.NE, a->types, a->nv, fin, succ, a->preds, pslot);
            DAGNN_CHECK_LAUNCH();
            if (o.gated)
                hipLaunchKernelGGL(ds_gated_agg_kernel, dim3(ds_blocks(R * HP)), dim3(DS_T), 0, st, R, n, hs, HP, idx, a->nv, a->preds,
                                   W + o.msg, W + o.hagg);
            else
                hipLaunchKernelGGL(ds_agg_kernel, dim3((unsigned)R), dim3(DS_T), 0, st, B, n, hs, HP, idx, ds_pair(idx, vi), G, a->nv,
                                   a->preds, pslot, W + o.key, W + o.h[0], W + o.hagg);
            DAGNN_CHECK_LAUNCH();
            DS_TRY(cells(idx, W + o.hagg, true));
        }
        if (!last) DS_TRY(finalize(idx));
    }
    if (a->states) {
        hipLaunchKernelGGL(ds_states_kernel, dim3(ds_blocks(R * n * hs)), dim3(DS_T), 0, st, R, n, hs, HP, a->nv, htop, a->states);
        DAGNN_CHECK_LAUNCH();
    }
    return DAGNN_OK;
}
