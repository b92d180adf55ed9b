// Validity and selection over decoded D-VAE graphs: the post-processing of `decode_from_latent_space`
// (dvae/util.py:408-466) on the dense output of dagnn_dvae_sample, A attempts of B latent points.
//
// Row kernel (one thread per row): the reference's rules (is_valid_ENAS / is_valid_BN, util.py:599-649) read straight
// from the predecessor bitmasks.  Edges only run from lower to higher index, so every row is a DAG by construction;
// bits at or above v and rows past nv are masked off.  A valid row gets a canonical key: the content of its string,
// bit-packed into W 64-bit words, so that equal keys mean equal strings:
//   ENAS (decode_igraph_to_ENAS, util.py:168-180): the vertex count (6 bits), the type of every middle vertex (tb bits,
//        tb = bits of nvt-1), then for i = 2 .. nv-2 the row bits j < i-1 of vertex i;
//   BN (decode_igraph_to_BN_adj, util.py:388-394): the middle vertices' adjacency with rows and columns ordered by
//        type, (m)^2 bits, m = nvt-2 (a valid BN row has exactly nvt vertices of distinct types).
// The bits are appended in this order, low bit first, and each word is stored when it is complete.  Invalid rows get
// zero keys.  Types outside [0, nvt) and vertex counts outside [1, n] make a row invalid (the decoder writes neither).
//
// Selection kernel (one workgroup per latent point): the point's keys are staged in LDS a tile at a time; every valid
// attempt counts the valid attempts with an equal key (an O(A^2) compare in a fixed order).  From the counts: the
// first valid attempt (the reference's pick - np.argmax over a dict_values object is always 0) and the most frequent
// key, ties going to the earliest first occurrence (Counter.most_common(1)).  Integer work only, written with plain
// stores: results are bitwise repeatable.
#include "common.h"

namespace {

constexpr int SEL_T = 256;
constexpr int SEL_TILE_WORDS = 4096;   // 32 KB of keys in LDS per tile
constexpr int SEL_MAX_WORDS = 16;

__host__ __device__ inline int sel_type_bits(int nvt) {
    int b = 1;
    while ((1 << b) < nvt) ++b;
    return b;
}

__host__ __device__ inline int sel_key_words(int kind, int n, int nvt) {
    int64_t bits;
    if (kind == 0) {
        bits = 6 + (int64_t)(n - 2) * sel_type_bits(nvt) + (int64_t)(n - 2) * (n - 3) / 2;
    } else {
        int m = (nvt < n ? nvt : n) - 2;
        if (m < 0) m = 0;
        bits = (int64_t)m * m;
    }
    const int w = (int)((bits + 63) / 64);
    return w < 1 ? 1 : w;
}

// appends bit fields to a key, storing each 64-bit word once it is complete
struct KeyWriter {
    uint64_t* dst;
    int W, w, pos;
    uint64_t cur;
    __device__ void put(uint64_t v, int width) {   // width 1..63, v < 2^width
        cur |= v << pos;
        pos += width;
        if (pos >= 64) {
            if (w < W) dst[w] = cur;
            ++w;
            pos -= 64;
            cur = pos ? v >> (width - pos) : 0;
        }
    }
    __device__ void finish() {
        for (; w < W; ++w) {
            dst[w] = cur;
            cur = 0;
        }
    }
};

__global__ void __launch_bounds__(SEL_T) sel_row_kernel(int64_t A, int64_t B, int n, int nvt, int start_type, int end_type,
                                                        int kind, int n_nodes, int W, const int32_t* __restrict__ types,
                                                        const uint32_t* __restrict__ preds, const int32_t* __restrict__ nv,
                                                        int32_t* __restrict__ valid, uint64_t* __restrict__ keys) {
    const int64_t r = (int64_t)blockIdx.x * SEL_T + threadIdx.x;
    if (r >= A * B) return;
    const int64_t a = r / B, b = r - a * B;
    const int k = nv[r];
    const int32_t* trow = types + r * n;
    const uint32_t* prow = preds + r * n;
    int t[DAGNN_DVAE_MAX_N];
    uint32_t mk[DAGNN_DVAE_MAX_N];
    bool ok = k >= 1 && k <= n;
    int n_start = 0, n_end = 0;
    uint32_t has_succ = 0;
    uint64_t seen = 0, mid_types = 0;
#pragma unroll
    for (int v = 0; v < DAGNN_DVAE_MAX_N; ++v) {
        t[v] = -1;
        mk[v] = 0;
        if (v < k && v < n) {
            t[v] = trow[v];
            mk[v] = prow[v] & ((1u << v) - 1u);
            ok = ok && t[v] >= 0 && t[v] < nvt;
            if (t[v] == start_type) ++n_start;
            else if (t[v] == end_type) ++n_end;
            has_succ |= mk[v];
            if (t[v] >= 0 && t[v] < nvt) {
                seen |= 1ull << t[v];
                if (v >= 1 && v < k - 1) mid_types |= 1ull << t[v];
            }
        }
    }
    if (kind == 0) {
        // is_valid_DAG: one START, one END, no source but START, no sink but END; then the chain i -> i+1 for
        // i = 0 .. nv-3 and an END (last vertex) of in-degree 1; with n_nodes, exactly n_nodes vertices
        ok = ok && n_start == 1 && n_end == 1 && (n_nodes == 0 || k == n_nodes);
#pragma unroll
        for (int v = 0; v < DAGNN_DVAE_MAX_N; ++v) {
            if (v < k) {
                if (mk[v] == 0 && t[v] != start_type) ok = false;
                if (!(has_succ >> v & 1u) && t[v] != end_type) ok = false;
                if (v >= 1 && v <= k - 2 && !(mk[v] >> (v - 1) & 1u)) ok = false;
                if (v == k - 1 && __popc(mk[v]) != 1) ok = false;
            }
        }
    } else {
        // is_valid_BN: one START, one END, nvt distinct types on exactly nvt vertices
        ok = ok && n_start == 1 && n_end == 1 && k == nvt && __popcll(seen) == nvt;
    }
    valid[r] = ok ? 1 : 0;
    KeyWriter kw{keys + (b * A + a) * W, W, 0, 0, 0};
    if (ok) {
        if (kind == 0) {
            const int tb = sel_type_bits(nvt);
            kw.put((uint64_t)k, 6);
#pragma unroll
            for (int v = 1; v < DAGNN_DVAE_MAX_N - 1; ++v)
                if (v < k - 1) kw.put((uint64_t)t[v], tb);
#pragma unroll
            for (int v = 2; v < DAGNN_DVAE_MAX_N - 1; ++v)
                if (v < k - 1) kw.put((uint64_t)(mk[v] & ((1u << (v - 1)) - 1u)), v - 1);
        } else {
            // rank of a middle vertex = its position in the argsort of the middle types (all distinct here)
            const int m = k - 2;
            int rk[DAGNN_DVAE_MAX_N];
#pragma unroll
            for (int v = 0; v < DAGNN_DVAE_MAX_N; ++v)
                rk[v] = (v >= 1 && v < k - 1) ? __popcll(mid_types & ((1ull << t[v]) - 1ull)) : -1;
            for (int p = 0; p < m; ++p) {
                int up = 0;
#pragma unroll
                for (int v = 1; v < DAGNN_DVAE_MAX_N - 1; ++v)
                    if (rk[v] == p) up = v;
                uint64_t row = 0;
#pragma unroll
                for (int v = 1; v < DAGNN_DVAE_MAX_N - 1; ++v)
                    if (rk[v] >= 0 && (mk[v] >> up & 1u)) row |= 1ull << rk[v];
                kw.put(row, m);
            }
        }
    }
    kw.finish();
}

__global__ void __launch_bounds__(SEL_T) sel_pick_kernel(int64_t A, int64_t B, int W, int tile, int select,
                                                         const int32_t* __restrict__ valid, const uint64_t* __restrict__ keys,
                                                         int32_t* __restrict__ pick, int32_t* __restrict__ n_valid,
                                                         int32_t* __restrict__ n_same) {
    __shared__ uint64_t s_key[SEL_TILE_WORDS];
    __shared__ unsigned char s_ok[SEL_TILE_WORDS];
    __shared__ uint64_t s_first[SEL_T], s_best[SEL_T];
    __shared__ int s_count[SEL_T];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const uint64_t* pk = keys + b * A * W;
    uint64_t first = ~0ull, best = 0;   // (a << 32 | count) min; (count << 32 | ~a) max
    int count = 0;
    for (int64_t a0 = 0; a0 < A; a0 += SEL_T) {
        const int64_t a = a0 + tid;
        const bool own = a < A && valid[a * B + b] != 0;
        uint64_t mine[SEL_MAX_WORDS];
#pragma unroll
        for (int w = 0; w < SEL_MAX_WORDS; ++w) mine[w] = (own && w < W) ? pk[a * W + w] : 0;
        int same = 0;
        for (int64_t t0 = 0; t0 < A; t0 += tile) {
            const int tn = (int)(A - t0 < tile ? A - t0 : tile);
            __syncthreads();
            for (int j = tid; j < tn * W; j += SEL_T) s_key[j] = pk[t0 * W + j];
            for (int j = tid; j < tn; j += SEL_T) s_ok[j] = valid[(t0 + j) * B + b] != 0;
            __syncthreads();
            if (own) {
                for (int j = 0; j < tn; ++j) {
                    bool eq = s_ok[j] != 0;
#pragma unroll
                    for (int w = 0; w < SEL_MAX_WORDS; ++w)
                        if (w < W) eq = eq && s_key[j * W + w] == mine[w];
                    same += eq ? 1 : 0;
                }
            }
        }
        if (own) {
            ++count;
            const uint64_t f = (uint64_t)a << 32 | (uint32_t)same;
            const uint64_t m = (uint64_t)(uint32_t)same << 32 | (uint32_t)(0xFFFFFFFFu - (uint32_t)a);
            first = f < first ? f : first;
            best = m > best ? m : best;
        }
    }
    s_first[tid] = first;
    s_best[tid] = best;
    s_count[tid] = count;
    __syncthreads();
    for (int s = SEL_T / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_first[tid] = s_first[tid + s] < s_first[tid] ? s_first[tid + s] : s_first[tid];
            s_best[tid] = s_best[tid + s] > s_best[tid] ? s_best[tid + s] : s_best[tid];
            s_count[tid] += s_count[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int nvalid = s_count[0];
        n_valid[b] = nvalid;
        if (nvalid == 0) {
            pick[b] = -1;
            n_same[b] = 0;
        } else if (select == 0) {
            pick[b] = (int32_t)(s_first[0] >> 32);
            n_same[b] = (int32_t)(uint32_t)s_first[0];
        } else {
            pick[b] = (int32_t)(0xFFFFFFFFu - (uint32_t)s_best[0]);
            n_same[b] = (int32_t)(s_best[0] >> 32);
        }
    }
}

bool sel_args_ok(const dagnn_dvae_select_args* a) {
    return a && a->A >= 1 && a->B >= 1 && a->A <= ((int64_t)1 << 30) && a->B <= ((int64_t)1 << 30) &&
           a->A * a->B <= ((int64_t)1 << 30) && a->n >= 2 && a->n <= DAGNN_DVAE_MAX_N && a->nvt >= 1 &&
           a->nvt <= DAGNN_DVAE_MAX_TYPES && a->start_type >= 0 && a->start_type < a->nvt && a->end_type >= 0 &&
           a->end_type < a->nvt && (a->kind == DAGNN_DVAE_ENAS || a->kind == DAGNN_DVAE_BN) && a->n_nodes >= 0 &&
           a->n_nodes <= DAGNN_DVAE_MAX_N && (a->select == DAGNN_DVAE_FIRST_VALID || a->select == DAGNN_DVAE_MOST_FREQUENT);
}

}  // namespace

extern "C" int dagnn_dvae_select_key_words(int kind, int n, int nvt) {
    if ((kind != DAGNN_DVAE_ENAS && kind != DAGNN_DVAE_BN) || n < 2 || n > DAGNN_DVAE_MAX_N || nvt < 1 ||
        nvt > DAGNN_DVAE_MAX_TYPES)
        return 0;
    return sel_key_words(kind, n, nvt);
}

extern "C" size_t dagnn_dvae_select_work_bytes(const dagnn_dvae_select_args* a) {
    if (!sel_args_ok(a)) return 0;
    return (size_t)(a->A * a->B) * sel_key_words(a->kind, a->n, a->nvt) * sizeof(uint64_t);
}

extern "C" int dagnn_dvae_select(const dagnn_dvae_select_args* a, void* stream) {
    if (!sel_args_ok(a) || !a->types || !a->preds || !a->nv || !a->valid || !a->pick || !a->n_valid || !a->n_same || !a->work)
        return DAGNN_EINVAL;
    const int W = sel_key_words(a->kind, a->n, a->nvt);
    if (a->work_bytes < (size_t)(a->A * a->B) * W * sizeof(uint64_t)) return DAGNN_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    uint64_t* keys = reinterpret_cast<uint64_t*>(a->work);
    const int64_t R = a->A * a->B;
    hipLaunchKernelGGL(sel_row_kernel, dim3((unsigned)((R + SEL_T - 1) / SEL_T)), dim3(SEL_T), 0, st, a->A, a->B, a->n, a->nvt,
                       a->start_type, a->end_type, a->kind, a->kind == DAGNN_DVAE_ENAS ? a->n_nodes : 0, W, a->types,
                       a->preds, a->nv, a->valid, keys);
    DAGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sel_pick_kernel, dim3((unsigned)a->B), dim3(SEL_T), 0, st, a->A, a->B, W, SEL_TILE_WORDS / W, a->select,
                       a->valid, keys, a->pick, a->n_valid, a->n_same);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
