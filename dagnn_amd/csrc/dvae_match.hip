// Graph identity over decoded D-VAE graphs: what the reference's evaluation does after the decode, on the dense
// output of dagnn_dvae_sample and the canonical keys of dagnn_dvae_select.
//
//   same DAG (is_same_DAG, util.py:576-585): decode row (a, b) against true row b - equal vertex count, and for every
//        v < nv equal type and equal predecessor mask.  No isomorphism.
//   graph set (ratio_same_DAG's left-hand side, util.py:588-596): built once from N rows, membership = is_same_DAG
//        against any stored row.
//   distinct count (len(set(G_valid_str))): the number of different canonical keys among the masked rows of all calls
//        that added to one set.
//
// A row is compared as its RECORD, K 32-bit words: a graph row as {nv, type[v], preds[v] & bits below v} with every
// word of a vertex v >= nv zero (so entries past the end never take part), a key as its W 64-bit words.  A set is one
// caller-owned buffer: header, `cap` int32 slots (0: empty, else 1 + the index of a stored record) and a record store
// of max_rows records.  Adding R rows is two launches: the first writes the records of the masked rows to the store
// at base + r, the second inserts their indices by linear probing from hash(record) - a slot is claimed by one
// atomicCAS on global memory; a thread that finds a slot taken compares the two RECORDS word for word and only then
// treats its row as a duplicate, otherwise it moves on, so rows with equal hashes both end up in the table.  Every
// record a probe can meet was stored by an earlier launch, so no thread waits for another.  Slots only ever go from
// empty to taken and equal records walk the same slot sequence, so exactly one of them claims a slot whichever thread
// runs first: the distinct count, the flags and the counts are the same from run to run (which of several equal rows
// a slot names may differ; nothing returned depends on it).  Probes are bounded by cap; cap >= 2 * max_rows keeps an
// empty slot in reach, and a probe that still runs out sets the error word of the header.  Integer work only.
#include "common.h"

namespace {

constexpr int MT_T = 256;
constexpr uint32_t MT_MAGIC = 0x44534554u;   // "DSET"

struct SetLayout {
    int K;              // 32-bit words per record
    int64_t cap;        // slots, a power of two
    int64_t rec_off;    // first record word, in int32 words from the start of the buffer
    int64_t words;      // whole buffer, int32 words
};

__host__ __device__ inline int set_record_words(int form, int width) {
    return form == DAGNN_DVAE_SET_GRAPHS ? 2 * width + 1 : 2 * width;
}

inline bool set_desc_ok(int form, int width, int64_t max_rows) {
    if (max_rows < 1 || max_rows > DAGNN_DVAE_SET_MAX_ROWS) return false;
    if (form == DAGNN_DVAE_SET_GRAPHS) return width >= 2 && width <= DAGNN_DVAE_MAX_N;
    return form == DAGNN_DVAE_SET_KEYS && width >= 1 && width <= 16;
}

inline SetLayout set_layout(int form, int width, int64_t max_rows) {
    SetLayout L;
    L.K = set_record_words(form, width);
    L.cap = 64;
    while (L.cap < 2 * max_rows) L.cap <<= 1;
    L.rec_off = DAGNN_DVAE_SET_HEADER_WORDS + L.cap;
    L.words = L.rec_off + max_rows * L.K;
    return L;
}

// One row of a source, opened once (vertex count and row pointers are read a single time), then read word by word.
// Dense row r: {nv, types[0..n), masks[0..n)}, zero at and past the row's end.
struct GraphRows {
    const int32_t* types;
    const uint32_t* preds;
    const int32_t* nv;   // NULL: every row has n vertices
    int n;
    struct Row {
        const int32_t* t;
        const uint32_t* p;
        int cnt, n;
        __device__ uint32_t word(int k) const {
            if (k == 0) return (uint32_t)cnt;
            const int v = k <= n ? k - 1 : k - 1 - n;
            if (v >= cnt) return 0u;
            return k <= n ? (uint32_t)t[v] : p[v] & ((1u << v) - 1u);
        }
    };
    __device__ Row row(int64_t r) const { return Row{types + r * n, preds + r * n, nv ? nv[r] : n, n}; }
};

// the key of row r = a * B + b, stored at [b, a, :] (dagnn_dvae_select's layout)
struct KeyRows {
    const uint32_t* keys;
    int64_t A, B;
    int K;
    struct Row {
        const uint32_t* w;
        __device__ uint32_t word(int k) const { return w[k]; }
    };
    __device__ Row row(int64_t r) const {
        const int64_t a = r / B, b = r - a * B;
        return Row{keys + (b * A + a) * K};
    }
};

struct StoredRows {
    const uint32_t* rec;
    int K;
    struct Row {
        const uint32_t* w;
        __device__ uint32_t word(int k) const { return w[k]; }
    };
    __device__ Row row(int64_t r) const { return Row{rec + r * K}; }
};

template <class Row>
__device__ uint32_t record_hash(const Row& row, int K) {
    uint32_t h = 0x9E3779B9u;
    for (int k = 0; k < K; ++k) {
        h ^= row.word(k);
        h *= 0x85EBCA6Bu;
        h ^= h >> 15;
    }
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

template <class Row>
__device__ bool record_equal(const Row& row, const uint32_t* __restrict__ stored, int K) {
    for (int k = 0; k < K; ++k)
        if (row.word(k) != stored[k]) return false;
    return true;
}

__device__ bool header_ok(int32_t* hdr, int K, int64_t cap, int64_t max_rows) {
    if ((uint32_t)hdr[DAGNN_DVAE_SET_MAGIC] == MT_MAGIC && hdr[DAGNN_DVAE_SET_K] == K && hdr[DAGNN_DVAE_SET_CAP] == (int32_t)cap &&
        hdr[DAGNN_DVAE_SET_ROWS] == (int32_t)max_rows)
        return true;
    if (threadIdx.x == 0) atomicOr(&hdr[DAGNN_DVAE_SET_ERR], DAGNN_DVAE_SET_ERR_HEADER);
    return false;
}

__global__ void __launch_bounds__(64) set_header_kernel(int32_t* hdr, int K, int64_t cap, int64_t max_rows) {
    if (threadIdx.x == 0) {
        hdr[DAGNN_DVAE_SET_MAGIC] = (int32_t)MT_MAGIC;
        hdr[DAGNN_DVAE_SET_K] = K;
        hdr[DAGNN_DVAE_SET_CAP] = (int32_t)cap;
        hdr[DAGNN_DVAE_SET_ROWS] = (int32_t)max_rows;
    }
}

template <class Rows>
__global__ void __launch_bounds__(MT_T) set_store_kernel(Rows rows, int64_t R, const int32_t* __restrict__ mask, int K,
                                                         uint32_t* __restrict__ rec, int64_t base) {
    const int64_t r = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    if (r >= R || (mask && mask[r] == 0)) return;
    uint32_t* dst = rec + (base + r) * K;
    const auto row = rows.row(r);
    for (int k = 0; k < K; ++k) dst[k] = row.word(k);
}

__global__ void __launch_bounds__(MT_T) set_insert_kernel(int64_t R, const int32_t* __restrict__ mask, int K, int64_t cap,
                                                          int64_t max_rows, int32_t* hdr, int32_t* slots,
                                                          const uint32_t* __restrict__ rec, int64_t base) {
    if (!header_ok(hdr, K, cap, max_rows)) return;
    const int64_t r = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    int fresh = 0;
    if (r < R && (!mask || mask[r] != 0)) {
        const int64_t idx = base + r;
        const StoredRows::Row mine = StoredRows{rec, K}.row(idx);
        const uint32_t h = record_hash(mine, K);
        bool placed = false;
        for (int64_t p = 0; p < cap && !placed; ++p) {
            int32_t* slot = slots + ((h + p) & (uint64_t)(cap - 1));
            int32_t cur = *slot;   // a stale zero costs one failed compare-and-swap; a taken slot never changes again
            if (cur == 0) cur = atomicCAS(slot, 0, (int32_t)idx + 1);
            if (cur == 0) {
                fresh = 1;
                placed = true;
            } else if ((int64_t)cur - 1 < base + R && record_equal(mine, rec + ((int64_t)cur - 1) * K, K)) {
                placed = true;   // an equal record is in the table already
            }
        }
        if (!placed) atomicOr(&hdr[DAGNN_DVAE_SET_ERR], DAGNN_DVAE_SET_ERR_FULL);
    }
    const int n_fresh = __syncthreads_count(fresh);
    if (threadIdx.x == 0 && n_fresh) atomicAdd(&hdr[DAGNN_DVAE_SET_COUNT], n_fresh);
}

__global__ void __launch_bounds__(MT_T) set_query_kernel(GraphRows rows, int64_t R, const int32_t* __restrict__ mask, int K,
                                                         int64_t cap, int64_t max_rows, int32_t* hdr,
                                                         const int32_t* __restrict__ slots, const uint32_t* __restrict__ rec,
                                                         int32_t* __restrict__ member, int32_t* count) {
    const bool ok = header_ok(hdr, K, cap, max_rows);
    const int64_t r = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    int hit = 0;
    if (ok && r < R && (!mask || mask[r] != 0)) {
        const GraphRows::Row row = rows.row(r);
        const uint32_t h = record_hash(row, K);
        for (int64_t p = 0; p < cap; ++p) {
            const int32_t cur = slots[(h + p) & (uint64_t)(cap - 1)];
            if (cur == 0) break;
            if ((int64_t)cur - 1 < max_rows && record_equal(row, rec + ((int64_t)cur - 1) * K, K)) {
                hit = 1;
                break;
            }
        }
    }
    if (r < R) member[r] = hit;
    const int n_hit = __syncthreads_count(hit);
    if (threadIdx.x == 0 && n_hit) atomicAdd(count, n_hit);
}

__global__ void __launch_bounds__(MT_T) same_dag_kernel(GraphRows dec, GraphRows tru, int64_t A, int64_t B, int K,
                                                        int32_t* __restrict__ same, int32_t* per_graph, int32_t* total) {
    const int64_t r = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    int eq = 0;
    if (r < A * B) {
        const int64_t b = r % B;
        const GraphRows::Row x = dec.row(r), y = tru.row(b);
        eq = 1;
        for (int k = 0; k < K && eq; ++k) eq = x.word(k) == y.word(k);
        same[r] = eq;
        if (eq) atomicAdd(&per_graph[b], 1);
    }
    const int n_eq = __syncthreads_count(eq);
    if (threadIdx.x == 0 && n_eq) atomicAdd(total, n_eq);
}

bool rows_ok(const dagnn_dvae_set_rows_args* a) {
    return a && a->A >= 1 && a->B >= 1 && a->A <= DAGNN_DVAE_SET_MAX_ROWS && a->B <= DAGNN_DVAE_SET_MAX_ROWS &&
           a->A * a->B <= DAGNN_DVAE_SET_MAX_ROWS && a->base >= 0 && set_desc_ok(a->set.form, a->set.width, a->set.max_rows) &&
           a->set.data;
}

unsigned blocks_for(int64_t R) { return (unsigned)((R + MT_T - 1) / MT_T); }

}  // namespace

extern "C" size_t dagnn_dvae_set_bytes(int form, int width, int64_t max_rows) {
    if (!set_desc_ok(form, width, max_rows)) return 0;
    return (size_t)set_layout(form, width, max_rows).words * sizeof(int32_t);
}

extern "C" int dagnn_dvae_set_init(const dagnn_dvae_set* s, void* stream) {
    if (!s || !s->data || !set_desc_ok(s->form, s->width, s->max_rows)) return DAGNN_EINVAL;
    const SetLayout L = set_layout(s->form, s->width, s->max_rows);
    if (s->bytes < (size_t)L.words * sizeof(int32_t)) return DAGNN_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(s->data, 0, (size_t)L.rec_off * sizeof(int32_t), st);
    if (e != hipSuccess) return DAGNN_EHIP(e);
    hipLaunchKernelGGL(set_header_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<int32_t*>(s->data), L.K, L.cap, s->max_rows);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_dvae_set_add(const dagnn_dvae_set_rows_args* a, void* stream) {
    if (!rows_ok(a)) return DAGNN_EINVAL;
    const bool graphs = a->set.form == DAGNN_DVAE_SET_GRAPHS;
    if (graphs ? (!a->types || !a->preds) : !a->keys) return DAGNN_EINVAL;
    const SetLayout L = set_layout(a->set.form, a->set.width, a->set.max_rows);
    const int64_t R = a->A * a->B;
    if (a->set.bytes < (size_t)L.words * sizeof(int32_t) || a->base + R > a->set.max_rows) return DAGNN_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    int32_t* hdr = reinterpret_cast<int32_t*>(a->set.data);
    int32_t* slots = hdr + DAGNN_DVAE_SET_HEADER_WORDS;
    uint32_t* rec = reinterpret_cast<uint32_t*>(hdr + L.rec_off);
    if (graphs) {
        hipLaunchKernelGGL(set_store_kernel<GraphRows>, dim3(blocks_for(R)), dim3(MT_T), 0, st,
                           GraphRows{a->types, a->preds, a->nv, a->set.width}, R, a->mask, L.K, rec, a->base);
    } else {
        hipLaunchKernelGGL(set_store_kernel<KeyRows>, dim3(blocks_for(R)), dim3(MT_T), 0, st,
                           KeyRows{reinterpret_cast<const uint32_t*>(a->keys), a->A, a->B, L.K}, R, a->mask, L.K, rec, a->base);
    }
    DAGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(set_insert_kernel, dim3(blocks_for(R)), dim3(MT_T), 0, st, R, a->mask, L.K, L.cap, a->set.max_rows, hdr,
                       slots, rec, a->base);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_dvae_set_query(const dagnn_dvae_set_rows_args* a, void* stream) {
    if (!rows_ok(a) || a->set.form != DAGNN_DVAE_SET_GRAPHS || !a->types || !a->preds || !a->member || !a->count)
        return DAGNN_EINVAL;
    const SetLayout L = set_layout(a->set.form, a->set.width, a->set.max_rows);
    if (a->set.bytes < (size_t)L.words * sizeof(int32_t)) return DAGNN_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    int32_t* hdr = reinterpret_cast<int32_t*>(a->set.data);
    const hipError_t e = hipMemsetAsync(a->count, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return DAGNN_EHIP(e);
    const int64_t R = a->A * a->B;
    hipLaunchKernelGGL(set_query_kernel, dim3(blocks_for(R)), dim3(MT_T), 0, st, GraphRows{a->types, a->preds, a->nv, a->set.width},
                       R, a->mask, L.K, L.cap, a->set.max_rows, hdr, hdr + DAGNN_DVAE_SET_HEADER_WORDS,
                       reinterpret_cast<const uint32_t*>(hdr + L.rec_off), a->member, a->count);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_dvae_same_dag(const dagnn_dvae_same_dag_args* a, void* stream) {
    if (!a || a->A < 1 || a->B < 1 || a->A > DAGNN_DVAE_SET_MAX_ROWS || a->B > DAGNN_DVAE_SET_MAX_ROWS ||
        a->A * a->B > DAGNN_DVAE_SET_MAX_ROWS || a->n < 2 || a->n > DAGNN_DVAE_MAX_N || !a->types || !a->preds || !a->nv ||
        !a->types_true || !a->preds_true || !a->same || !a->per_graph || !a->total)
        return DAGNN_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(a->per_graph, 0, (size_t)a->B * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(a->total, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return DAGNN_EHIP(e);
    hipLaunchKernelGGL(same_dag_kernel, dim3(blocks_for(a->A * a->B)), dim3(MT_T), 0, st,
                       GraphRows{a->types, a->preds, a->nv, a->n}, GraphRows{a->types_true, a->preds_true, a->nv_true, a->n}, a->A,
                       a->B, 2 * a->n + 1, a->same, a->per_graph, a->total);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
