// Teacher-forced D-VAE decoder and its reverse pass: `DVAE_PYG.loss()` (dvae/models_pyg.py:398-456) minus the latent /
// KL part, for both decoders (NA: graph state = top state of the last vertex, edge head on [H_vi, H_v]; BN: graph state =
// sum of the top states, edge head on [H_vi, H_v, H0]).
//
// Teacher forcing makes the decoded prefix the true graph, so the states live in dense buffers.  Vertex v is updated
// v+1 times: update k (k = v .. 0) aggregates v's true predecessors >= k (k = v: none; k = 0: all of them, the FINAL
// state).  Update k >= 1 feeds exactly one edge score (vi = k-1); the final update feeds later vertices and the heads.
// Every update of v reads only the final layer-0 states of vertices < v, so all v+1 updates of v run in one launch per
// stacked layer.  The heads read nothing the chain needs: they run once, over all rows, after the chain.
//
// Row layouts (b = graph, fastest):
//   update rows   r = (U(v) + k) * B + b      U(0) = 0, U(v) = 1 + sum_{u=1}^{v-1} (u+1); NU = U(n) updates
//   edge rows     e = (v(v-1)/2 + k-1) * B + b    for k = 1..v (vi = k-1); NE = n(n-1)/2 pairs
//   vertex rows   q = (v-1) * B + b             for v = 1..n-1
//
// Gradients are pulled (each output element is written by one thread in a fixed order), so results are bitwise
// run-to-run deterministic.  No kernel waits on another workgroup.
//
// agg = gated_sum (NA): the message of vertex u, m_u = sigmoid(Wg [h_u ; e_u] + bg) * (Wm [h_u ; e_u]), depends on u's
// final layer-0 state only, so it is formed once, right after u's launches: one product [B, hs] x [hs, 2hs] (gate and
// mapper stacked), then an epilogue that adds the vertex-id columns and bg.  The aggregate of update (v, k) is the sum
// of the messages of v's predecessors >= k in ascending order (padding rows contribute exactly 0: the mapper has no
// bias).  In reverse, dm_u pulls d hagg from every update that read it, and one product turns it into u's layer-0
// state gradient before u's own cells run backwards.
//   message rows  q = u * B + b                 for u = 0..n-2 (vertex n-1 has no successors)
//
// agg = attn_x (BN): the keys are the predecessors' one-hot types (dvae/dagnn_bn.py:203-225), so the score of a real slot is
// one entry of the table key_type [nvt] and the values stay the layer-0 states: the same launches and saved records as
// attn_h with the score product replaced by a lookup.  In reverse the keys carry no state gradient, and d key_type[t]
// pulls the score gradients of every slot whose predecessor has type t (one workgroup per type, fixed order).
#include "dvae_common.h"

namespace {

constexpr int DD_T = 256;

__host__ __device__ inline int64_t dd_U(int v) { return v == 0 ? 0 : 1 + (int64_t)(v - 1) * (v + 2) / 2; }   // 1 + sum_{u=1}^{v-1}(u+1)
__host__ __device__ inline int64_t dd_E(int v) { return (int64_t)v * (v - 1) / 2; }

__device__ inline int dd_vertex_of_update(int64_t ui) {   // U(v) <= ui < U(v+1)
    int v = 0;
    while (dd_U(v + 1) <= ui) ++v;
    return v;
}
__device__ inline int dd_vertex_of_pair(int64_t p) {      // E(v) <= p < E(v+1), v >= 1
    int v = 1;
    while (dd_E(v + 1) <= p) ++v;
    return v;
}


// block-wide sum of one value per thread (DD_T threads), in a fixed order; every thread gets the result
__device__ inline float dd_block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < DD_T / 64; ++w) s += red[w];
    return s;
}

// ---- generic fp32 product  C[m,n] (+)= sum_k A(m,k) B(k,n) (+ bias[n]), A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk +
// n*sbn]; the strides express every transpose.  Optional epilogue: relu, or zero where gate[m*ldg + n] <= 0.  k runs in
// one fixed order per output element.
__global__ void __launch_bounds__(DD_T) dd_gemm_kernel(int M, int N, int K, const float* __restrict__ A, int64_t sam, int64_t sak,
                                                       const float* __restrict__ Bm, int64_t sbk, int64_t sbn,
                                                       const float* __restrict__ bias, float* __restrict__ C, int64_t ldc,
                                                       int accumulate, int relu, const float* __restrict__ gate, int64_t ldg) {
    __shared__ float As[16][65];
    __shared__ float Bs[16][65];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t m0 = (int64_t)blockIdx.y * 64, n0 = (int64_t)blockIdx.x * 64;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        for (int e = threadIdx.x; e < 16 * 64; e += DD_T) {
            int kk, mm;
            if (sak == 1) { kk = e & 15; mm = e >> 4; } else { mm = e & 63; kk = e >> 6; }
            const int64_t m = m0 + mm, k = k0 + kk;
            As[kk][mm] = (m < M && k < K) ? A[m * sam + k * sak] : 0.f;
            int nn;
            if (sbk == 1) { kk = e & 15; nn = e >> 4; } else { nn = e & 63; kk = e >> 6; }
            const int64_t n = n0 + nn, k2 = k0 + kk;
            Bs[kk][nn] = (n < N && k2 < K) ? Bm[k2 * sbk + n * sbn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[kk][ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[kk][tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + ty + 16 * i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t n = n0 + tx + 16 * j;
            if (n >= N) continue;
            float v = acc[i][j];
            if (bias) v += bias[n];
            if (accumulate) v += C[m * ldc + n];
            if (relu) v = fmaxf(v, 0.f);
            if (gate && !(gate[m * ldg + n] > 0.f)) v = 0.f;
            C[m * ldc + n] = v;
        }
    }
}

// out[n] = sum_r w[r] * A[r*lda + n]  (w = NULL: plain column sums), rows in ascending order
__global__ void __launch_bounds__(DD_T) dd_colsum_kernel(const float* __restrict__ A, int64_t lda, int64_t R, int N,
                                                         const float* __restrict__ w, float* __restrict__ out) {
    const int n = blockIdx.x * DD_T + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int64_t r = 0; r < R; ++r) s += w ? w[r] * A[r * lda + n] : A[r * lda + n];
    out[n] = s;
}

struct DDLayout {
    int64_t B, RU, RE, RV, NU;
    int n, H, L, nvt, ein, E1, V1;
    // saved by the forward pass (float offsets)
    int64_t hagg, h[DAGNN_MAX_STACKED], gates[DAGNN_MAX_STACKED], alpha, pid, pcount, gi, gh, xe, y_e, hid_e, s_e, ll_e, hg,
        hid_v, logit_v, ll_v, saved_end;
    // backward workspace
    int64_t dlog_e, dpre, dxe, dlog_v, dhid_v, dhg, dH[DAGNN_MAX_STACKED], dhagg, dGi[DAGNN_MAX_STACKED],
        dGh[DAGNN_MAX_STACKED], ds, work_end;
    // gated_sum (behind the attn_h layout): stacked weights [2H, H], message inputs / pre-activations / gate / mapper /
    // message per message row, and (backward) the pre-activation gradients
    int gated;
    int64_t RM, wgm, xmsg, mpre, mgate, mmap, msg, dmpre;
};

bool dd_layout(const dagnn_dvae_decode_args* a, DDLayout& o) {
    if (!a || a->B <= 0 || !dvae_decoder_ok(a)) return false;
    o.B = a->B; o.n = a->n; o.H = a->hs; o.L = a->L; o.nvt = a->nvt;
    o.gated = a->agg == DAGNN_DVAE_AGG_GATED_SUM;
    o.ein = (a->bn ? 3 : 2) * a->hs; o.E1 = a->edge_hidden; o.V1 = a->vertex_hidden;
    o.NU = dd_U(o.n);
    o.RU = o.NU * o.B; o.RE = dd_E(o.n) * o.B; o.RV = (int64_t)(o.n - 1) * o.B;
    const int64_t H = o.H, maxM = (int64_t)o.n * o.B;
    if (o.RU * 4 * H >= ((int64_t)1 << 40) || o.RE * (o.E1 > o.ein ? o.E1 : o.ein) >= ((int64_t)1 << 40)) return false;
    int64_t at = 0;
    o.hagg = dvae_take(at, o.RU * H);
    for (int l = 0; l < o.L; ++l) { o.h[l] = dvae_take(at, o.RU * H); o.gates[l] = dvae_take(at, o.RU * 4 * H); }
    o.alpha = dvae_take(at, o.RU * o.n);
    o.pid = dvae_take(at, o.RU * o.n);
    o.pcount = dvae_take(at, o.NU);
    o.gi = dvae_take(at, maxM * 3 * H);
    o.gh = dvae_take(at, maxM * 3 * H);
    o.xe = dvae_take(at, o.RE * o.ein);
    o.y_e = dvae_take(at, o.RE);
    o.hid_e = dvae_take(at, o.RE * o.E1);
    o.s_e = dvae_take(at, o.RE);
    o.ll_e = dvae_take(at, o.RE);
    o.hg = dvae_take(at, o.RV * H);
    o.hid_v = dvae_take(at, o.RV * o.V1);
    o.logit_v = dvae_take(at, o.RV * o.nvt);
    o.ll_v = dvae_take(at, o.RV);
    o.RM = (int64_t)(o.n - 1) * o.B;
    if (o.gated) {
        o.wgm = dvae_take(at, 2 * H * H);
        o.xmsg = dvae_take(at, o.RM * H);
        o.mpre = dvae_take(at, o.RM * 2 * H);
        o.mgate = dvae_take(at, o.RM * H);
        o.mmap = dvae_take(at, o.RM * H);
        o.msg = dvae_take(at, o.RM * H);
    }
    o.saved_end = at;
    at = 0;
    o.dlog_e = dvae_take(at, o.RE);
    o.dpre = dvae_take(at, o.RE * o.E1);
    o.dxe = dvae_take(at, o.RE * o.ein);
    o.dlog_v = dvae_take(at, o.RV * o.nvt);
    o.dhid_v = dvae_take(at, o.RV * o.V1);
    o.dhg = dvae_take(at, o.RV * H);
    for (int l = 0; l < o.L; ++l) o.dH[l] = dvae_take(at, o.RU * H);
    o.dhagg = dvae_take(at, o.RU * H);
    for (int l = 0; l < o.L; ++l) { o.dGi[l] = dvae_take(at, o.RU * 3 * H); o.dGh[l] = dvae_take(at, o.RU * 3 * H); }
    o.ds = dvae_take(at, o.RU * o.n);
    if (o.gated) o.dmpre = dvae_take(at, o.RM * 2 * H);
    o.work_end = at;
    return true;
}

__device__ inline int dd_type_of(const int32_t* __restrict__ types, int64_t b, int n, int u, int nvt, int start_type) {
    const int t = u == 0 ? start_type : types[b * n + u];
    return t < 0 ? 0 : (t >= nvt ? nvt - 1 : t);   // (the host validates the types; never read outside the table)
}

// ---- forward: the aggregate of every update of vertex v (grid [v+1, B]); v = 0: H0.  TYPE_KEY: a real slot scores
// key_type[type of its predecessor] (attn_x) instead of w_key . state + vid_bias
template <bool TYPE_KEY>
__global__ void __launch_bounds__(DD_T) dd_agg_kernel(int v, int n, int64_t B, int H, const uint32_t* __restrict__ preds,
                                                      const float* __restrict__ h0state, const float* __restrict__ w_key,
                                                      const float* __restrict__ vid_bias, const float* __restrict__ H0,
                                                      float* __restrict__ hagg, float* __restrict__ alpha, int32_t* __restrict__ pid,
                                                      int32_t* __restrict__ pcount, const float* __restrict__ key_type,
                                                      const int32_t* __restrict__ types, int nvt, int start_type) {
    __shared__ float red[DD_T / 64];
    __shared__ float sc[DAGNN_DVAE_MAX_N];
    __shared__ int ids[DAGNN_DVAE_MAX_N];
    __shared__ int sP, sCnt;
    const int k = blockIdx.x;
    const int64_t b = blockIdx.y;
    const int64_t ui = dd_U(v) + k, row = ui * B + b;
    if (v == 0) {
        for (int c = threadIdx.x; c < H; c += DD_T) hagg[row * H + c] = H0[b * H + c];
        if (threadIdx.x < n) { alpha[row * n + threadIdx.x] = 0.f; pid[row * n + threadIdx.x] = -1; }
        if (b == 0 && threadIdx.x == 0) pcount[ui] = 0;
        return;
    }
    if (threadIdx.x == 0) {
        const uint32_t keep = ~0u << k;   // predecessors >= k (k <= v < 32)
        int P = 0;
        for (int64_t g = 0; g < B; ++g) P = max(P, __popc(preds[g * n + v] & keep & ((1u << v) - 1u)));
        int c = 0;
        const uint32_t m = preds[b * n + v] & keep & ((1u << v) - 1u);
        for (int u = 0; u < v; ++u)
            if (m >> u & 1u) ids[c++] = u;
        sP = P; sCnt = c;
    }
    __syncthreads();
    const int P = sP, cnt = sCnt;
    if (TYPE_KEY) {
        if ((int)threadIdx.x < cnt) sc[threadIdx.x] = key_type[dd_type_of(types, b, n, ids[threadIdx.x], nvt, start_type)];
    } else {
        for (int j = 0; j < cnt; ++j) {
            const float* hv = h0state + (dd_U(ids[j]) * B + b) * H;
            float s = 0.f;
            for (int c = threadIdx.x; c < H; c += DD_T) s = fmaf(w_key[c], hv[c], s);
            s = dd_block_sum(s, red);
            if (threadIdx.x == 0) sc[j] = s + (vid_bias ? vid_bias[ids[j]] : 0.f);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = -INFINITY, den = 0.f;
        for (int j = 0; j < P; ++j) m = fmaxf(m, j < cnt ? sc[j] : 0.f);
        for (int j = 0; j < P; ++j) den += expf((j < cnt ? sc[j] : 0.f) - m);
        for (int j = 0; j < P; ++j) sc[j] = expf((j < cnt ? sc[j] : 0.f) - m) / den;   // padded slots score 0
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += DD_T) {
        alpha[row * n + j] = j < P ? sc[j] : 0.f;
        pid[row * n + j] = j < cnt ? ids[j] : -1;
    }
    if (b == 0 && threadIdx.x == 0) pcount[ui] = P;
    for (int c = threadIdx.x; c < H; c += DD_T) {
        float a = 0.f;
        for (int j = 0; j < cnt; ++j) a = fmaf(sc[j], h0state[(dd_U(ids[j]) * B + b) * H + c], a);
        hagg[row * H + c] = a;
    }
}

// ---- forward: one stacked GRU cell over the rows [r0, r0 + M) of vertex v; layer 0's input side is a column of W_ih
__global__ void __launch_bounds__(DD_T) dd_gru_kernel(int64_t r0, int v, int64_t B, int n, int H, int nvt, int start_type,
                                                      const int32_t* __restrict__ types, const float* __restrict__ w_ih0,
                                                      const float* __restrict__ b_ih0, const float* __restrict__ gi,
                                                      const float* __restrict__ gh, const float* __restrict__ hagg,
                                                      float* __restrict__ h, float* __restrict__ gates) {
    const int c = blockIdx.x * DD_T + threadIdx.x;
    if (c >= H) return;
    const int64_t i = blockIdx.y, row = r0 + i, b = row % B;
    float ir, iz, in_;
    if (w_ih0) {
        int t = v == 0 ? start_type : types[b * n + v];
        t = t < 0 ? 0 : (t >= nvt ? nvt - 1 : t);   // (the host validates the types; never read outside W_ih)
        ir = w_ih0[(int64_t)c * nvt + t] + b_ih0[c];
        iz = w_ih0[(int64_t)(H + c) * nvt + t] + b_ih0[H + c];
        in_ = w_ih0[(int64_t)(2 * H + c) * nvt + t] + b_ih0[2 * H + c];
    } else {
        ir = gi[i * 3 * H + c]; iz = gi[i * 3 * H + H + c]; in_ = gi[i * 3 * H + 2 * H + c];
    }
    const float hr = gh[i * 3 * H + c], hz = gh[i * 3 * H + H + c], hn = gh[i * 3 * H + 2 * H + c];
    const float r = sigm_div(ir + hr), z = sigm_div(iz + hz);
    const float nn = tanhf(in_ + r * hn);
    const float hp = hagg[row * H + c];
    h[row * H + c] = nn + z * (hp - nn);   // torch's GRUCell: (h - n) * z + n
    float* g4 = gates + row * 4 * H;
    g4[c] = r; g4[H + c] = z; g4[2 * H + c] = nn; g4[3 * H + c] = hn;
}

// ---- heads: inputs of every edge row [H_vi | H_v | (H0)] and its label
__global__ void __launch_bounds__(DD_T) dd_edge_gather_kernel(int64_t B, int n, int H, int L, int bn, const uint32_t* __restrict__ preds,
                                                              const float* __restrict__ htop, const float* __restrict__ H0,
                                                              float* __restrict__ xe, float* __restrict__ y) {
    const int64_t e = blockIdx.x, p = e / B, b = e % B;
    const int v = dd_vertex_of_pair(p);
    const int k = (int)(p - dd_E(v)) + 1, vi = k - 1;
    const int ein = (bn ? 3 : 2) * H;
    const float* hvi = htop + (dd_U(vi) * B + b) * H;
    const float* hv = htop + ((dd_U(v) + k) * B + b) * H;
    for (int c = threadIdx.x; c < H; c += DD_T) {
        xe[e * ein + c] = hvi[c];
        xe[e * ein + H + c] = hv[c];
        if (bn) xe[e * ein + 2 * H + c] = H0[b * H + c];
    }
    if (threadIdx.x == 0) y[e] = (preds[b * n + v] >> vi & 1u) ? 1.f : 0.f;
}

// sigmoid score of every edge row and its clamped log-likelihood (torch's binary_cross_entropy, log clamped at -100)
__global__ void __launch_bounds__(DD_T) dd_edge_head_kernel(int E1, const float* __restrict__ hid, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, const float* __restrict__ y,
                                                            float* __restrict__ s_out, float* __restrict__ ll) {
    __shared__ float red[DD_T / 64];
    const int64_t e = blockIdx.x;
    float s = 0.f;
    for (int c = threadIdx.x; c < E1; c += DD_T) s = fmaf(hid[e * E1 + c], w2[c], s);
    s = dd_block_sum(s, red) + b2[0];
    if (threadIdx.x == 0) {
        const float p = sigm_div(s);
        s_out[e] = p;
        ll[e] = y[e] > 0.5f ? fmaxf(logf(p), -100.f) : fmaxf(logf(1.0f - p), -100.f);
    }
}

// graph state of every vertex row: NA the top state of v-1, BN the sum of the top states of 0..v-1
__global__ void __launch_bounds__(DD_T) dd_vertex_gather_kernel(int64_t B, int H, int bn, const float* __restrict__ htop,
                                                                float* __restrict__ hg) {
    const int64_t q = blockIdx.x, b = q % B;
    const int v = (int)(q / B) + 1;
    for (int c = threadIdx.x; c < H; c += DD_T) {
        float s;
        if (bn) {
            s = 0.f;
            for (int u = 0; u < v; ++u) s += htop[(dd_U(u) * B + b) * H + c];
        } else {
            s = htop[(dd_U(v - 1) * B + b) * H + c];
        }
        hg[q * H + c] = s;
    }
}

// log-softmax of the type scores at the true type (one wave per vertex row)
__global__ void __launch_bounds__(64) dd_vertex_head_kernel(int64_t B, int n, int nvt, const int32_t* __restrict__ types,
                                                            const float* __restrict__ logit, float* __restrict__ ll) {
    const int64_t q = blockIdx.x, b = q % B;
    const int v = (int)(q / B) + 1;
    if (threadIdx.x != 0) return;
    const float* x = logit + q * nvt;
    float m = -INFINITY;
    for (int j = 0; j < nvt; ++j) m = fmaxf(m, x[j]);
    float den = 0.f;
    for (int j = 0; j < nvt; ++j) den += expf(x[j] - m);
    const int t = types[b * n + v];
    ll[q] = (t >= 0 && t < nvt) ? (x[t] - m) - logf(den) : NAN;
}

// per-graph partials and the total, in a fixed order: ll[b] vertex terms, ll[B + b] edge terms, ll[2B] = res
__global__ void __launch_bounds__(DD_T) dd_reduce_kernel(int64_t B, int n, const float* __restrict__ ll_v,
                                                         const float* __restrict__ ll_e, float* __restrict__ out) {
    for (int64_t b = threadIdx.x; b < B; b += DD_T) {
        float sv = 0.f, se = 0.f;
        for (int v = 1; v < n; ++v) sv += ll_v[(int64_t)(v - 1) * B + b];
        for (int64_t p = 0; p < dd_E(n); ++p) se += ll_e[p * B + b];
        out[b] = sv;
        out[B + b] = se;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = 0.f;
        for (int64_t b = 0; b < B; ++b) r += out[b] + out[B + b];
        out[2 * B] = -r;
    }
}

// ---- reverse: heads
__global__ void __launch_bounds__(DD_T) dd_edge_head_bwd_kernel(int E1, const float* __restrict__ g_res, const float* __restrict__ s,
                                                                const float* __restrict__ y, const float* __restrict__ hid,
                                                                const float* __restrict__ w2, float* __restrict__ dlog,
                                                                float* __restrict__ dpre) {
    const int64_t e = blockIdx.x;
    const float p = s[e];
    // d res / d p = d BCE / d p (torch: (p - y) / max((1 - p) p, 1e-12)), then the sigmoid's p (1 - p)
    const float d = g_res[0] * (p - y[e]) / fmaxf((1.0f - p) * p, 1e-12f) * ((1.0f - p) * p);
    if (threadIdx.x == 0) dlog[e] = d;
    for (int c = threadIdx.x; c < E1; c += DD_T) dpre[e * E1 + c] = hid[e * E1 + c] > 0.f ? d * w2[c] : 0.f;
}

__global__ void __launch_bounds__(64) dd_vertex_head_bwd_kernel(int64_t B, int n, int nvt, const float* __restrict__ g_res,
                                                                const int32_t* __restrict__ types, const float* __restrict__ logit,
                                                                float* __restrict__ dlog) {
    const int64_t q = blockIdx.x, b = q % B;
    const int v = (int)(q / B) + 1;
    const float* x = logit + q * nvt;
    float m = -INFINITY;
    for (int j = 0; j < nvt; ++j) m = fmaxf(m, x[j]);
    float den = 0.f;
    for (int j = 0; j < nvt; ++j) den += expf(x[j] - m);
    const float lse = logf(den);
    const int t = types[b * n + v];
    for (int j = threadIdx.x; j < nvt; j += 64) dlog[q * nvt + j] = g_res[0] * (expf((x[j] - m) - lse) - (j == t ? 1.f : 0.f));
}

// gradient reaching the TOP state of every update row from the heads (pulled: each (row, column) sums its sources in a
// fixed order); zeroes the lower layers' and the aggregate's accumulators of the same rows
__global__ void __launch_bounds__(DD_T) dd_seed_kernel(int64_t B, int n, int H, int L, int bn, const float* __restrict__ dxe,
                                                       const float* __restrict__ dhg, float* __restrict__ dHtop, float* __restrict__ dHlow, int64_t low_stride,
                                                       float* __restrict__ dhagg) {
    const int c = blockIdx.x * DD_T + threadIdx.x;
    if (c >= H) return;
    const int64_t row = blockIdx.y, ui = row / B, b = row % B;
    const int v = dd_vertex_of_update(ui);
    const int k = (int)(ui - dd_U(v));
    const int ein = (bn ? 3 : 2) * H;
    float val = 0.f;
    if (k >= 1) {
        val += dxe[((dd_E(v) + k - 1) * B + b) * ein + H + c];
    } else {
        for (int w = v + 1; w < n; ++w) val += dxe[((dd_E(w) + v) * B + b) * ein + c];   // v as vi of vertex w: k' = v + 1
        if (bn) {
            for (int w = v + 1; w < n; ++w) val += dhg[((int64_t)(w - 1) * B + b) * H + c];
        } else if (v + 1 < n) {
            val += dhg[((int64_t)v * B + b) * H + c];
        }
    }
    dHtop[row * H + c] = val;
    for (int l = 0; l + 1 < L; ++l) dHlow[l * low_stride + row * H + c] = 0.f;
    dhagg[row * H + c] = 0.f;
}

// reverse of one stacked GRU cell over rows [r0, r0 + M): gate gradients (kept for the weight products) and the direct
// part of the aggregate's gradient
__global__ void __launch_bounds__(DD_T) dd_gru_bwd_kernel(int64_t r0, int H, const float* __restrict__ dh, const float* __restrict__ gates,
                                                          const float* __restrict__ hagg, float* __restrict__ dgi,
                                                          float* __restrict__ dgh, float* __restrict__ dhagg) {
    const int c = blockIdx.x * DD_T + threadIdx.x;
    if (c >= H) return;
    const int64_t row = r0 + blockIdx.y;
    const float* g4 = gates + row * 4 * H;
    const float r = g4[c], z = g4[H + c], nn = g4[2 * H + c], hn = g4[3 * H + c];
    const float d = dh[row * H + c], hp = hagg[row * H + c];
    const float dn = d * (1.0f - z), dz = d * (hp - nn);
    const float dnp = dn * (1.0f - nn * nn);
    const float drp = dnp * hn * r * (1.0f - r), dzp = dz * z * (1.0f - z);
    float* gi = dgi + row * 3 * H;
    float* gh = dgh + row * 3 * H;
    gi[c] = drp; gi[H + c] = dzp; gi[2 * H + c] = dnp;
    gh[c] = drp; gh[H + c] = dzp; gh[2 * H + c] = dnp * r;
    dhagg[row * H + c] += d * z;
}

// reverse of the aggregates of vertex v >= 1 (one workgroup per graph): the score gradients `ds` (kept for the key
// gradient) and the predecessors' layer-0 state gradients, accumulated over the v+1 updates in a fixed order
__global__ void __launch_bounds__(DD_T) dd_agg_bwd_kernel(int v, int n, int64_t B, int H, const float* __restrict__ h0state,
                                                          const float* __restrict__ w_key, const float* __restrict__ alpha,
                                                          const int32_t* __restrict__ pid, const int32_t* __restrict__ pcount,
                                                          const float* __restrict__ dhagg, float* __restrict__ ds,
                                                          float* __restrict__ dH0) {
    __shared__ float red[DD_T / 64];
    __shared__ float da[DAGNN_DVAE_MAX_N];
    __shared__ float sds[DAGNN_DVAE_MAX_N][DAGNN_DVAE_MAX_N];   // [k][slot]
    const int64_t b = blockIdx.x;
    for (int k = 0; k <= v; ++k) {
        const int64_t ui = dd_U(v) + k, row = ui * B + b;
        const int P = pcount[ui];
        for (int j = 0; j < P; ++j) {
            const int u = pid[row * n + j];
            float s = 0.f;
            if (u >= 0) {
                const float* hv = h0state + (dd_U(u) * B + b) * H;
                for (int c = threadIdx.x; c < H; c += DD_T) s = fmaf(dhagg[row * H + c], hv[c], s);
                s = dd_block_sum(s, red);
            }
            if (threadIdx.x == 0) da[j] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float dot = 0.f;
            for (int j = 0; j < P; ++j) dot += alpha[row * n + j] * da[j];
            for (int j = 0; j < n; ++j) {
                const float d = (j < P && pid[row * n + j] >= 0) ? alpha[row * n + j] * (da[j] - dot) : 0.f;
                sds[k][j] = d;
                ds[row * n + j] = d;
            }
        }
        __syncthreads();
    }
    for (int c = threadIdx.x; c < H; c += DD_T) {
        for (int k = 0; k <= v; ++k) {
            const int64_t row = (dd_U(v) + k) * B + b;
            for (int j = 0; j < n; ++j) {
                const int u = pid[row * n + j];
                if (u < 0) break;
                float* d = dH0 + (dd_U(u) * B + b) * H + c;
                if (w_key) *d += alpha[row * n + j] * dhagg[row * H + c] + sds[k][j] * w_key[c];
                else *d += alpha[row * n + j] * dhagg[row * H + c];   // (attn_x: the keys are types, not states)
            }
        }
    }
}

// key / vertex-id gradients: dw_key[c] = sum ds * (layer-0 state of the predecessor), d vid_bias[u] = sum of ds at u
__global__ void __launch_bounds__(DD_T) dd_key_grad_kernel(int64_t B, int n, int H, int64_t NU, const float* __restrict__ h0state,
                                                           const int32_t* __restrict__ pid, const float* __restrict__ ds,
                                                           float* __restrict__ dkey, float* __restrict__ dvid) {
    const int c = blockIdx.x * DD_T + threadIdx.x;
    const int nkey = (H + DD_T - 1) / DD_T;
    if ((int)blockIdx.x < nkey) {
        if (c >= H) return;
        float s = 0.f;
        for (int64_t row = B; row < NU * B; ++row) {   // (update 0 has no predecessors)
            const int64_t b = row % B;
            for (int j = 0; j < n; ++j) {
                const int u = pid[row * n + j];
                if (u < 0) break;
                s = fmaf(ds[row * n + j], h0state[(dd_U(u) * B + b) * H + c], s);
            }
        }
        dkey[c] = s;
    } else if (dvid) {
        const int u = threadIdx.x;
        if (u >= n) return;
        float s = 0.f;
        for (int64_t row = B; row < NU * B; ++row)
            for (int j = 0; j < n; ++j) {
                const int w = pid[row * n + j];
                if (w < 0) break;
                if (w == u) s += ds[row * n + j];
            }
        dvid[u] = s;
    }
}

// attn_x: d key_type[t] = sum of ds over every (update row, real slot) whose predecessor has type t.  One workgroup per
// type: thread i sums the rows i, i + DD_T, .. in ascending order, then the block adds the partials in a fixed order
__global__ void __launch_bounds__(DD_T) dd_type_key_grad_kernel(int64_t B, int n, int nvt, int start_type, int64_t NU,
                                                                const int32_t* __restrict__ types, const int32_t* __restrict__ pid,
                                                                const float* __restrict__ ds, float* __restrict__ dkey) {
    __shared__ float red[DD_T / 64];
    const int t = blockIdx.x;
    float s = 0.f;
    for (int64_t row = B + threadIdx.x; row < NU * B; row += DD_T) {   // (update 0 has no predecessors)
        const int64_t b = row % B;
        for (int j = 0; j < n; ++j) {
            const int u = pid[row * n + j];
            if (u < 0) break;
            if (dd_type_of(types, b, n, u, nvt, start_type) == t) s += ds[row * n + j];
        }
    }
    s = dd_block_sum(s, red);
    if (threadIdx.x == 0) dkey[t] = s;
}

// d H0: vertex 0's aggregate IS H0, plus (BN) the H0 part of every edge row
__global__ void __launch_bounds__(DD_T) dd_h0_grad_kernel(int64_t B, int n, int H, int bn, const float* __restrict__ dhagg,
                                                          const float* __restrict__ dxe, float* __restrict__ dh0) {
    const int c = blockIdx.x * DD_T + threadIdx.x;
    if (c >= H) return;
    const int64_t b = blockIdx.y;
    float s = dhagg[b * H + c];
    if (bn)
        for (int64_t p = 0; p < dd_E(n); ++p) s += dxe[(p * B + b) * 3 * H + 2 * H + c];
    dh0[b * H + c] = s;
}

// d W_ih of layer 0: the input is one-hot, so column t sums the gate gradients of the rows whose vertex has type t
__global__ void __launch_bounds__(DD_T) dd_type_grad_kernel(int64_t B, int n, int H, int nvt, int start_type, int64_t RU,
                                                            const int32_t* __restrict__ types, const float* __restrict__ dgi,
                                                            float* __restrict__ dw) {
    const int m = blockIdx.x * DD_T + threadIdx.x;
    const int t = blockIdx.y;
    if (m >= 3 * H) return;
    float s = 0.f;
    for (int64_t row = 0; row < RU; ++row) {
        const int64_t ui = row / B, b = row % B;
        const int v = dd_vertex_of_update(ui);
        const int tt = v == 0 ? start_type : types[b * n + v];
        if (tt == t) s += dgi[row * 3 * H + m];
    }
    dw[(int64_t)m * nvt + t] = s;
}

// ---- gated_sum
// wgm [2H, H]: rows 0..H-1 the state columns of Wg, rows H..2H-1 those of Wm (both [H, H+n] row-major)
__global__ void __launch_bounds__(DD_T) dd_gated_stack_kernel(int H, int n, const float* __restrict__ gate_w,
                                                              const float* __restrict__ mapper_w, float* __restrict__ wgm) {
    const int64_t total = 2 * (int64_t)H * H;
    for (int64_t e = (int64_t)blockIdx.x * DD_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * DD_T) {
        const int64_t j = e / H, k = e - j * H;
        wgm[e] = j < H ? gate_w[j * (H + n) + k] : mapper_w[(j - H) * (H + n) + k];
    }
}

// epilogue of vertex u's message product (grid [hb, B]): vertex-id column and bias, sigmoid-times; keeps the input row,
// the gate and the mapper output for the reverse pass
__global__ void __launch_bounds__(DD_T) dd_gated_msg_kernel(int u, int n, int64_t B, int H, const float* __restrict__ h0state,
                                                            const float* __restrict__ pre, const float* __restrict__ gate_w,
                                                            const float* __restrict__ gate_b, const float* __restrict__ mapper_w,
                                                            float* __restrict__ xmsg, float* __restrict__ mgate,
                                                            float* __restrict__ mmap, float* __restrict__ msg) {
    const int c = blockIdx.x * DD_T + threadIdx.x;
    if (c >= H) return;
    const int64_t b = blockIdx.y, q = (int64_t)u * B + b;
    const float g = sigm_div(pre[q * 2 * H + c] + gate_w[(int64_t)c * (H + n) + H + u] + gate_b[c]);
    const float m = pre[q * 2 * H + H + c] + mapper_w[(int64_t)c * (H + n) + H + u];
    xmsg[q * H + c] = h0state[(dd_U(u) * B + b) * H + c];
    mgate[q * H + c] = g;
    mmap[q * H + c] = m;
    msg[q * H + c] = g * m;
}

// the aggregate of every update of vertex v (grid [hb, (v+1) B]): the messages of v's predecessors >= k, ascending; v = 0: H0
__global__ void __launch_bounds__(DD_T) dd_gated_agg_kernel(int v, int n, int64_t B, int H, const uint32_t* __restrict__ preds,
                                                            const float* __restrict__ msg, const float* __restrict__ H0,
                                                            float* __restrict__ hagg) {
    const int c = blockIdx.x * DD_T + threadIdx.x;
    if (c >= H) return;
    const int64_t i = blockIdx.y, k = i / B, b = i - k * B, row = dd_U(v) * B + i;
    if (v == 0) {
        hagg[row * H + c] = H0[b * H + c];
        return;
    }
    const uint32_t m = preds[b * n + v] & (~0u << k) & ((1u << v) - 1u);
    float a = 0.f;
    for (int u = 0; u < v; ++u)
        if (m >> u & 1u) a += msg[((int64_t)u * B + b) * H + c];
    hagg[row * H + c] = a;
}

// reverse of vertex u's message (grid [hb, B]): dm_u pulls d hagg from every update (v > u, k <= u) that read it, v then
// k ascending; then the gate / mapper pre-activation gradients [B, 2H]
__global__ void __launch_bounds__(DD_T) dd_gated_msg_bwd_kernel(int u, int n, int64_t B, int H, const uint32_t* __restrict__ preds,
                                                                const float* __restrict__ dhagg, const float* __restrict__ mgate,
                                                                const float* __restrict__ mmap, float* __restrict__ dmpre) {
    const int c = blockIdx.x * DD_T + threadIdx.x;
    if (c >= H) return;
    const int64_t b = blockIdx.y, q = (int64_t)u * B + b;
    float s = 0.f;
    for (int v = u + 1; v < n; ++v) {
        if (!(preds[b * n + v] >> u & 1u)) continue;
        for (int k = 0; k <= u; ++k) s += dhagg[((dd_U(v) + k) * B + b) * H + c];
    }
    const float g = mgate[q * H + c], m = mmap[q * H + c];
    dmpre[q * 2 * H + c] = s * m * g * (1.0f - g);
    dmpre[q * 2 * H + H + c] = s * g;
}

// vertex-id columns of d Wg / d Wm (grid [ceil(2H / DD_T), n]): column H+u sums the pre-activation gradients of u's
// message rows (zero for u = n-1, which sends none)
__global__ void __launch_bounds__(DD_T) dd_gated_vid_grad_kernel(int64_t B, int n, int H, const float* __restrict__ dmpre,
                                                                 float* __restrict__ d_gate_w, float* __restrict__ d_mapper_w) {
    const int j = blockIdx.x * DD_T + threadIdx.x;
    const int u = blockIdx.y;
    if (j >= 2 * H) return;
    float s = 0.f;
    if (u < n - 1)
        for (int64_t b = 0; b < B; ++b) s += dmpre[((int64_t)u * B + b) * 2 * H + j];
    if (j < H) d_gate_w[(int64_t)j * (H + n) + H + u] = s;
    else d_mapper_w[(int64_t)(j - H) * (H + n) + H + u] = s;
}

// ---- host helpers
int dd_gemm(hipStream_t st, int64_t M, int64_t N, int64_t K, const float* A, int64_t sam, int64_t sak, const float* Bm,
            int64_t sbk, int64_t sbn, const float* bias, float* C, int64_t ldc, int accumulate, int relu,
            const float* gate = nullptr, int64_t ldg = 0) {
    if (M <= 0 || N <= 0) return DAGNN_OK;
    if (M > INT32_MAX || N > INT32_MAX || K > INT32_MAX || (M + 63) / 64 > 65535) return DAGNN_EINVAL;
    hipLaunchKernelGGL(dd_gemm_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((M + 63) / 64)), dim3(DD_T), 0, st, (int)M,
                       (int)N, (int)K, A, sam, sak, Bm, sbk, sbn, bias, C, ldc, accumulate, relu, gate, ldg);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

int dd_colsum(hipStream_t st, const float* A, int64_t lda, int64_t R, int N, const float* w, float* out) {
    hipLaunchKernelGGL(dd_colsum_kernel, dim3((unsigned)((N + DD_T - 1) / DD_T)), dim3(DD_T), 0, st, A, lda, R, N, w, out);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

#define DD_TRY(x)                    \
    do {                             \
        const int rc_ = (x);         \
        if (rc_ != DAGNN_OK) return rc_; \
    } while (0)

// (after dd_layout, which has established key_type for attn_x)
bool dd_pointers_ok(const dagnn_dvae_decode_args* a) {
    return dvae_weights_ok(a) && a->types && a->preds && a->ll && a->saved;
}

}  // namespace

extern "C" size_t dagnn_dvae_decode_saved_bytes(const dagnn_dvae_decode_args* a) {
    DDLayout o;
    return dd_layout(a, o) ? (size_t)o.saved_end * sizeof(float) : 0;
}

extern "C" size_t dagnn_dvae_decode_work_bytes(const dagnn_dvae_decode_args* a) {
    DDLayout o;
    return dd_layout(a, o) ? (size_t)o.work_end * sizeof(float) : 0;
}

extern "C" int dagnn_dvae_decode_forward(const dagnn_dvae_decode_args* a, void* stream) {
    DDLayout o;
    if (!dd_layout(a, o) || !dd_pointers_ok(a)) return DAGNN_EINVAL;
    if (a->saved_bytes < (size_t)o.saved_end * sizeof(float)) return DAGNN_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    float* S = a->saved;
    const int64_t B = o.B, H = o.H;
    const int L = o.L, n = o.n;
    int32_t* pid = reinterpret_cast<int32_t*>(S + o.pid);
    int32_t* pcount = reinterpret_cast<int32_t*>(S + o.pcount);
    const unsigned hb = (unsigned)((H + DD_T - 1) / DD_T);
    if (o.gated) {
        hipLaunchKernelGGL(dd_gated_stack_kernel, dim3((unsigned)((2 * H * H + DD_T - 1) / DD_T)), dim3(DD_T), 0, st, (int)H, n,
                           a->gate_w, a->mapper_w, S + o.wgm);
        DAGNN_CHECK_LAUNCH();
    }
    // the chain: vertex by vertex, every update of the vertex at once, one launch per stacked layer
    for (int v = 0; v < n; ++v) {
        const int64_t r0 = dd_U(v) * B, M = (int64_t)(v == 0 ? 1 : v + 1) * B;
        if (o.gated) {
            hipLaunchKernelGGL(dd_gated_agg_kernel, dim3(hb, (unsigned)M), dim3(DD_T), 0, st, v, n, B, (int)H, a->preds, S + o.msg,
                               a->h0, S + o.hagg);
        } else if (a->agg == DAGNN_DVAE_AGG_ATTN_X) {
            hipLaunchKernelGGL(dd_agg_kernel<true>, dim3((unsigned)(v == 0 ? 1 : v + 1), (unsigned)B), dim3(DD_T), 0, st, v, n, B, (int)H,
                               a->preds, S + o.h[0], nullptr, nullptr, a->h0, S + o.hagg, S + o.alpha, pid, pcount, a->key_type,
                               a->types, o.nvt, a->start_type);
        } else {
            hipLaunchKernelGGL(dd_agg_kernel<false>, dim3((unsigned)(v == 0 ? 1 : v + 1), (unsigned)B), dim3(DD_T), 0, st, v, n, B, (int)H,
                               a->preds, S + o.h[0], a->w_key, a->vid_bias, a->h0, S + o.hagg, S + o.alpha, pid, pcount, nullptr,
                               nullptr, o.nvt, a->start_type);
        }
        DAGNN_CHECK_LAUNCH();
        for (int l = 0; l < L; ++l) {
            // gh = Hagg W_hh^T + b_hh; layers above 0: gi = h_{l-1} W_ih^T + b_ih
            DD_TRY(dd_gemm(st, M, 3 * H, H, S + o.hagg + r0 * H, H, 1, a->w_hh[l], 1, H, a->b_hh[l], S + o.gh, 3 * H, 0, 0));
            if (l > 0)
                DD_TRY(dd_gemm(st, M, 3 * H, H, S + o.h[l - 1] + r0 * H, H, 1, a->w_ih[l], 1, H, a->b_ih[l], S + o.gi, 3 * H, 0, 0));
            hipLaunchKernelGGL(dd_gru_kernel, dim3(hb, (unsigned)M), dim3(DD_T), 0, st, r0, v, B, n, (int)H, o.nvt, a->start_type,
                               a->types, l == 0 ? a->w_ih[0] : nullptr, a->b_ih[0], S + o.gi, S + o.gh, S + o.hagg, S + o.h[l],
                               S + o.gates[l]);
            DAGNN_CHECK_LAUNCH();
        }
        if (o.gated && v + 1 < n) {   // v's layer-0 state is final: its message to every later vertex
            DD_TRY(dd_gemm(st, B, 2 * H, H, S + o.h[0] + r0 * H, H, 1, S + o.wgm, 1, H, nullptr, S + o.mpre + v * B * 2 * H, 2 * H, 0, 0));
            hipLaunchKernelGGL(dd_gated_msg_kernel, dim3(hb, (unsigned)B), dim3(DD_T), 0, st, v, n, B, (int)H, S + o.h[0],
                               S + o.mpre, a->gate_w, a->gate_b, a->mapper_w, S + o.xmsg, S + o.mgate, S + o.mmap, S + o.msg);
            DAGNN_CHECK_LAUNCH();
        }
    }
    const float* htop = S + o.h[L - 1];
    // edge head over every (vertex, earlier vertex) pair
    hipLaunchKernelGGL(dd_edge_gather_kernel, dim3((unsigned)o.RE), dim3(DD_T), 0, st, B, n, (int)H, L, a->bn, a->preds, htop,
                       a->h0, S + o.xe, S + o.y_e);
    DAGNN_CHECK_LAUNCH();
    DD_TRY(dd_gemm(st, o.RE, o.E1, o.ein, S + o.xe, o.ein, 1, a->ae_w1, 1, o.ein, a->ae_b1, S + o.hid_e, o.E1, 0, 1));
    hipLaunchKernelGGL(dd_edge_head_kernel, dim3((unsigned)o.RE), dim3(DD_T), 0, st, o.E1, S + o.hid_e, a->ae_w2, a->ae_b2,
                       S + o.y_e, S + o.s_e, S + o.ll_e);
    DAGNN_CHECK_LAUNCH();
    // vertex head over every vertex 1..n-1
    hipLaunchKernelGGL(dd_vertex_gather_kernel, dim3((unsigned)o.RV), dim3(DD_T), 0, st, B, (int)H, a->bn, htop, S + o.hg);
    DAGNN_CHECK_LAUNCH();
    DD_TRY(dd_gemm(st, o.RV, o.V1, H, S + o.hg, H, 1, a->av_w1, 1, H, a->av_b1, S + o.hid_v, o.V1, 0, 1));
    DD_TRY(dd_gemm(st, o.RV, o.nvt, o.V1, S + o.hid_v, o.V1, 1, a->av_w2, 1, o.V1, a->av_b2, S + o.logit_v, o.nvt, 0, 0));
    hipLaunchKernelGGL(dd_vertex_head_kernel, dim3((unsigned)o.RV), dim3(64), 0, st, B, n, o.nvt, a->types, S + o.logit_v, S + o.ll_v);
    DAGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(dd_reduce_kernel, dim3(1), dim3(DD_T), 0, st, B, n, S + o.ll_v, S + o.ll_e, a->ll);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_dvae_decode_backward(const dagnn_dvae_decode_args* a, const dagnn_dvae_decode_grads* g, void* stream) {
    DDLayout o;
    if (!dd_layout(a, o) || !dd_pointers_ok(a) || !g || !g->g_res || !g->work || !g->d_h0 || (a->agg == DAGNN_DVAE_AGG_ATTN_H && !g->d_w_key) || (a->agg == DAGNN_DVAE_AGG_ATTN_X && !g->d_key_type) || !g->d_av_w1 ||
        !g->d_av_b1 || !g->d_av_w2 || !g->d_av_b2 || !g->d_ae_w1 || !g->d_ae_b1 || !g->d_ae_w2 || !g->d_ae_b2 ||
        (a->agg == DAGNN_DVAE_AGG_ATTN_H && a->vid_bias && !g->d_vid_bias) || (a->agg == DAGNN_DVAE_AGG_GATED_SUM && (!g->d_gate_w || !g->d_gate_b || !g->d_mapper_w)))
        return DAGNN_EINVAL;
    for (int l = 0; l < a->L; ++l)
        if (!g->d_w_ih[l] || !g->d_w_hh[l] || !g->d_b_ih[l] || !g->d_b_hh[l]) return DAGNN_EINVAL;
    if (a->saved_bytes < (size_t)o.saved_end * sizeof(float) || g->work_bytes < (size_t)o.work_end * sizeof(float))
        return DAGNN_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    const float* S = a->saved;
    float* W = g->work;
    const int64_t B = o.B, H = o.H, RU = o.RU;
    const int L = o.L, n = o.n;
    const int32_t* pid = reinterpret_cast<const int32_t*>(S + o.pid);
    const int32_t* pcount = reinterpret_cast<const int32_t*>(S + o.pcount);
    const unsigned hb = (unsigned)((H + DD_T - 1) / DD_T);
    // heads: local gradients, then what reaches their inputs
    hipLaunchKernelGGL(dd_edge_head_bwd_kernel, dim3((unsigned)o.RE), dim3(DD_T), 0, st, o.E1, g->g_res, S + o.s_e, S + o.y_e,
                       S + o.hid_e, a->ae_w2, W + o.dlog_e, W + o.dpre);
    DAGNN_CHECK_LAUNCH();
    DD_TRY(dd_gemm(st, o.RE, o.ein, o.E1, W + o.dpre, o.E1, 1, a->ae_w1, o.ein, 1, nullptr, W + o.dxe, o.ein, 0, 0));
    hipLaunchKernelGGL(dd_vertex_head_bwd_kernel, dim3((unsigned)o.RV), dim3(64), 0, st, B, n, o.nvt, g->g_res, a->types,
                       S + o.logit_v, W + o.dlog_v);
    DAGNN_CHECK_LAUNCH();
    DD_TRY(dd_gemm(st, o.RV, o.V1, o.nvt, W + o.dlog_v, o.nvt, 1, a->av_w2, o.V1, 1, nullptr, W + o.dhid_v, o.V1, 0, 0,
                   S + o.hid_v, o.V1));
    DD_TRY(dd_gemm(st, o.RV, H, o.V1, W + o.dhid_v, o.V1, 1, a->av_w1, H, 1, nullptr, W + o.dhg, H, 0, 0));
    // the chain in reverse
    hipLaunchKernelGGL(dd_seed_kernel, dim3(hb, (unsigned)RU), dim3(DD_T), 0, st, B, n, (int)H, L, a->bn, W + o.dxe, W + o.dhg,
                       W + o.dH[L - 1], W + o.dH[0], L > 1 ? o.dH[1] - o.dH[0] : 0, W + o.dhagg);
    DAGNN_CHECK_LAUNCH();
    for (int v = n - 1; v >= 0; --v) {
        const int64_t r0 = dd_U(v) * B, M = (int64_t)(v == 0 ? 1 : v + 1) * B;
        if (o.gated && v + 1 < n) {   // every reader of v's message is done: its gradient joins v's final layer-0 state
            hipLaunchKernelGGL(dd_gated_msg_bwd_kernel, dim3(hb, (unsigned)B), dim3(DD_T), 0, st, v, n, B, (int)H, a->preds,
                               W + o.dhagg, S + o.mgate, S + o.mmap, W + o.dmpre);
            DAGNN_CHECK_LAUNCH();
            DD_TRY(dd_gemm(st, B, H, 2 * H, W + o.dmpre + v * B * 2 * H, 2 * H, 1, S + o.wgm, H, 1, nullptr, W + o.dH[0] + r0 * H, H, 1, 0));
        }
        for (int l = L - 1; l >= 0; --l) {
            hipLaunchKernelGGL(dd_gru_bwd_kernel, dim3(hb, (unsigned)M), dim3(DD_T), 0, st, r0, (int)H, W + o.dH[l], S + o.gates[l],
                               S + o.hagg, W + o.dGi[l], W + o.dGh[l], W + o.dhagg);
            DAGNN_CHECK_LAUNCH();
            DD_TRY(dd_gemm(st, M, H, 3 * H, W + o.dGh[l] + r0 * 3 * H, 3 * H, 1, a->w_hh[l], H, 1, nullptr, W + o.dhagg + r0 * H, H, 1, 0));
            if (l > 0)
                DD_TRY(dd_gemm(st, M, H, 3 * H, W + o.dGi[l] + r0 * 3 * H, 3 * H, 1, a->w_ih[l], H, 1, nullptr,
                               W + o.dH[l - 1] + r0 * H, H, 1, 0));
        }
        if (v > 0 && !o.gated) {
            hipLaunchKernelGGL(dd_agg_bwd_kernel, dim3((unsigned)B), dim3(DD_T), 0, st, v, n, B, (int)H, S + o.h[0],
                               a->agg == DAGNN_DVAE_AGG_ATTN_X ? nullptr : a->w_key,
                               S + o.alpha, pid, pcount, W + o.dhagg, W + o.ds, W + o.dH[0]);
            DAGNN_CHECK_LAUNCH();
        }
    }
    // parameter gradients: ONE product (or column sum) over all saved rows each
    for (int l = 0; l < L; ++l) {
        DD_TRY(dd_gemm(st, 3 * H, H, RU, W + o.dGh[l], 1, 3 * H, S + o.hagg, H, 1, nullptr, g->d_w_hh[l], H, 0, 0));
        DD_TRY(dd_colsum(st, W + o.dGh[l], 3 * H, RU, (int)(3 * H), nullptr, g->d_b_hh[l]));
        DD_TRY(dd_colsum(st, W + o.dGi[l], 3 * H, RU, (int)(3 * H), nullptr, g->d_b_ih[l]));
        if (l > 0) {
            DD_TRY(dd_gemm(st, 3 * H, H, RU, W + o.dGi[l], 1, 3 * H, S + o.h[l - 1], H, 1, nullptr, g->d_w_ih[l], H, 0, 0));
        } else {
            hipLaunchKernelGGL(dd_type_grad_kernel, dim3((unsigned)((3 * H + DD_T - 1) / DD_T), (unsigned)o.nvt), dim3(DD_T), 0, st,
                               B, n, (int)H, o.nvt, a->start_type, RU, a->types, W + o.dGi[0], g->d_w_ih[0]);
            DAGNN_CHECK_LAUNCH();
        }
    }
    if (o.gated) {
        const int64_t ld = H + n;
        DD_TRY(dd_gemm(st, H, H, o.RM, W + o.dmpre, 1, 2 * H, S + o.xmsg, H, 1, nullptr, g->d_gate_w, ld, 0, 0));
        DD_TRY(dd_gemm(st, H, H, o.RM, W + o.dmpre + H, 1, 2 * H, S + o.xmsg, H, 1, nullptr, g->d_mapper_w, ld, 0, 0));
        hipLaunchKernelGGL(dd_gated_vid_grad_kernel, dim3((unsigned)((2 * H + DD_T - 1) / DD_T), (unsigned)n), dim3(DD_T), 0, st, B, n,
                           (int)H, W + o.dmpre, g->d_gate_w, g->d_mapper_w);
        DAGNN_CHECK_LAUNCH();
        DD_TRY(dd_colsum(st, W + o.dmpre, 2 * H, o.RM, (int)H, nullptr, g->d_gate_b));
    } else if (a->agg == DAGNN_DVAE_AGG_ATTN_X) {
        hipLaunchKernelGGL(dd_type_key_grad_kernel, dim3((unsigned)o.nvt), dim3(DD_T), 0, st, B, n, o.nvt, a->start_type, o.NU,
                           a->types, pid, W + o.ds, g->d_key_type);
        DAGNN_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL(dd_key_grad_kernel, dim3(hb + 1), dim3(DD_T), 0, st, B, n, (int)H, o.NU, S + o.h[0], pid, W + o.ds,
                           g->d_w_key, a->vid_bias ? g->d_vid_bias : nullptr);
        DAGNN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(dd_h0_grad_kernel, dim3(hb, (unsigned)B), dim3(DD_T), 0, st, B, n, (int)H, a->bn, W + o.dhagg, W + o.dxe,
                       g->d_h0);
    DAGNN_CHECK_LAUNCH();
    DD_TRY(dd_gemm(st, o.E1, o.ein, o.RE, W + o.dpre, 1, o.E1, S + o.xe, o.ein, 1, nullptr, g->d_ae_w1, o.ein, 0, 0));
    DD_TRY(dd_colsum(st, W + o.dpre, o.E1, o.RE, o.E1, nullptr, g->d_ae_b1));
    DD_TRY(dd_colsum(st, S + o.hid_e, o.E1, o.RE, o.E1, W + o.dlog_e, g->d_ae_w2));
    DD_TRY(dd_colsum(st, W + o.dlog_e, 1, o.RE, 1, nullptr, g->d_ae_b2));
    DD_TRY(dd_gemm(st, o.nvt, o.V1, o.RV, W + o.dlog_v, 1, o.nvt, S + o.hid_v, o.V1, 1, nullptr, g->d_av_w2, o.V1, 0, 0));
    DD_TRY(dd_colsum(st, W + o.dlog_v, o.nvt, o.RV, o.nvt, nullptr, g->d_av_b2));
    DD_TRY(dd_gemm(st, o.V1, H, o.RV, W + o.dhid_v, 1, o.V1, S + o.hg, H, 1, nullptr, g->d_av_w1, H, 0, 0));
    DD_TRY(dd_colsum(st, W + o.dhid_v, o.V1, o.RV, o.V1, nullptr, g->d_av_b1));
    return DAGNN_OK;
}
