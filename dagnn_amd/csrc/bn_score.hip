// bn_score.hip - the BIC score of Bayesian-network structures on a table of discrete samples: the objective of the D-VAE's
// BN loops (the y column of the BN training file, and `eva.eval` of the BO loop).
//
// Reference path replaced, per structure: `Eval_BN.eval` (bayesian_optimization/evaluate_BN.py) writes the adjacency
// matrix to a file and starts an R process that calls bnlearn's `score(net, data)`.  The score is counting:
//
//   family_i = sum over cells (j, k) with N_ijk > 0 of N_ijk (log N_ijk - log N_ij) - 0.5 log(S) q_i (r_i - 1)
//   score    = sum over the nodes i of family_i
//
// with j the configuration of node i's parents (q_i = product of their cardinalities), k the value of x_i, N_ijk the
// number of samples in cell (j, k) and N_ij its sum over k (include/dagnn_hip.h has the full contract).
//
// Layout.  The samples live on the device column-major, one byte per value, every column `ld` bytes apart (ld a multiple
// of 16, zero padded).  A workgroup of 256 threads copies the whole table into LDS once (when it fits beside the count
// table) and then walks structures m = blockIdx.x, + gridDim.x, ...; the streaming form reads the same bytes from global
// memory instead and is otherwise the same code, so both give the same bits.
//
// Per family: every thread takes four consecutive samples at a time (one dword per column involved), forms the cell index
// cfg * r_i + x_i of each and adds 1 to an int32 count table in LDS with integer atomics - order-independent, so any
// permutation of the samples gives the same counts.  A small table is kept in R copies (the lane picks the copy, R = 32
// puts every lane of a half-wave on a bank of its own) that are added up afterwards, again in integers.  The float64 part
// has one fixed order: thread t owns configurations t, t + 256, ... in ascending order, inside a configuration k ascends,
// the 64 lanes of a wave are joined by an xor butterfly, the four waves as (w0 + w1) + (w2 + w3), and the families are
// added in node order.  No float atomics anywhere.
//
// The table is all zero between families: whoever reads a count also clears it, so there is no fill pass per family.
#include "common.h"

namespace {

constexpr int BN_T = 256;
constexpr int BN_WAVES = BN_T / DAGNN_WAVE;
constexpr int BN_CAP = DAGNN_BN_TABLE_CELLS;
constexpr int BN_MAXV = DAGNN_BN_MAX_VARS;
constexpr int BN_FIXED_LDS = BN_CAP * 4 + BN_MAXV * BN_WAVES * 8;   // count table + the families' wave partials
constexpr int BN_LDS_LIMIT = 160 * 1024;

struct BnCards { int32_t r[BN_MAXV]; };

// cells of family i (q_i * r_i), or BN_CAP + 1 as soon as the product passes the capacity
__device__ __forceinline__ int bn_family_cells(const BnCards& cards, int i, uint32_t mask) {
    int64_t cells = cards.r[i];
    for (uint32_t m = mask; m; m &= m - 1u) {
        cells *= cards.r[__ffs((int)m) - 1];
        if (cells > BN_CAP) return BN_CAP + 1;
    }
    return (int)cells;
}

template <bool STAGED>
__global__ void __launch_bounds__(BN_T) bn_score_kernel(const uint8_t* __restrict__ cols, int64_t ld, int64_t S, int n_var,
                                                        BnCards cards, const uint32_t* __restrict__ parents,
                                                        const int32_t* __restrict__ valid, int64_t M,
                                                        double* __restrict__ scores, int32_t* __restrict__ n_over) {
    extern __shared__ __align__(16) unsigned char bn_lds[];
    int32_t* table = reinterpret_cast<int32_t*>(bn_lds);
    double* fam = reinterpret_cast<double*>(bn_lds + BN_CAP * 4);
    const uint8_t* data = cols;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int c = tid; c < BN_CAP; c += BN_T) table[c] = 0;
    if (STAGED) {
        uint4* dst = reinterpret_cast<uint4*>(bn_lds + BN_FIXED_LDS);
        const uint4* src = reinterpret_cast<const uint4*>(cols);
        const int64_t words = (int64_t)n_var * ld / 16;
        for (int64_t w = tid; w < words; w += BN_T) dst[w] = src[w];
        data = bn_lds + BN_FIXED_LDS;
    }
    __syncthreads();

    const uint32_t var_mask = n_var >= 32 ? 0xFFFFFFFFu : ((1u << n_var) - 1u);
    const int64_t chunks = (S + 3) >> 2;   // groups of four samples (ld >= 4 * chunks)
    const double half_log_s = 0.5 * log((double)S);

    for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {
        const uint32_t* pm = parents + m * n_var;
        if (valid && valid[m] == 0) {   // (uniform over the workgroup)
            if (tid == 0) scores[m] = __longlong_as_double(0x7FF8000000000000ll);
            continue;
        }
        bool over = false;
        for (int i = 0; i < n_var; ++i) over = over || bn_family_cells(cards, i, pm[i] & var_mask) > BN_CAP;
        if (over) {
            if (tid == 0) {
                scores[m] = __longlong_as_double(0x7FF8000000000000ll);
                atomicAdd(n_over, 1);
            }
            continue;
        }
        for (int i = 0; i < n_var; ++i) {
            const uint32_t mask = pm[i] & var_mask;
            const int r = cards.r[i];
            const int cells = bn_family_cells(cards, i, mask);
            const int q = cells / r;
            int R = 1;   // copies of the table: the largest power of two <= 32 with cells * R <= BN_CAP / 2
            while (R < 32 && cells * (R * 2) <= BN_CAP / 2) R *= 2;
            const int rep = lane & (R - 1);

            // ---- counts
            const uint8_t* xi = data + (int64_t)i * ld;
            for (int64_t c = tid; c < chunks; c += BN_T) {
                const uint32_t xw = *reinterpret_cast<const uint32_t*>(xi + 4 * c);
                uint32_t cfg0 = 0, cfg1 = 0, cfg2 = 0, cfg3 = 0, mult = 1;
                for (uint32_t pmask = mask; pmask; pmask &= pmask - 1u) {
                    const int p = __ffs((int)pmask) - 1;
                    const uint32_t w = *reinterpret_cast<const uint32_t*>(data + (int64_t)p * ld + 4 * c);
                    cfg0 += (w & 0xFFu) * mult;
                    cfg1 += ((w >> 8) & 0xFFu) * mult;
                    cfg2 += ((w >> 16) & 0xFFu) * mult;
                    cfg3 += (w >> 24) * mult;
                    mult *= (uint32_t)cards.r[p];
                }
                const uint32_t cell[4] = {cfg0 * r + (xw & 0xFFu), cfg1 * r + ((xw >> 8) & 0xFFu),
                                          cfg2 * r + ((xw >> 16) & 0xFFu), cfg3 * r + (xw >> 24)};
                const int64_t s0 = 4 * c;
#pragma unroll
                for (int b = 0; b < 4; ++b)   // (a value outside its cardinality would leave the table: such a sample is skipped)
                    if (s0 + b < S && cell[b] < (uint32_t)cells) atomicAdd(&table[cell[b] * R + rep], 1);
            }
            __syncthreads();

            // ---- the R copies of every cell, added up into the upper half of the table (and cleared)
            int32_t* counts = table;
            if (R > 1) {
                const int total = cells * R, rounds = (total + BN_T - 1) / BN_T;
                for (int t = 0; t < rounds; ++t) {
                    const int idx = t * BN_T + tid;
                    int v = 0;
                    if (idx < total) {
                        v = table[idx];
                        table[idx] = 0;
                    }
                    for (int o = R >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                    if (idx < total && rep == 0) table[BN_CAP / 2 + idx / R] = v;
                }
                counts = table + BN_CAP / 2;
                __syncthreads();
            }

            // ---- float64 terms: a thread per configuration, k ascending
            double acc = 0.0;
            for (int j = tid; j < q; j += BN_T) {
                int32_t* cj = counts + j * r;
                int64_t nij = 0;
                for (int k = 0; k < r; ++k) nij += cj[k];
                if (nij > 0) {
                    const double lij = log((double)nij);
                    for (int k = 0; k < r; ++k) {
                        const int32_t nk = cj[k];
                        if (nk > 0) acc += (double)nk * (log((double)nk) - lij);
                    }
                }
                for (int k = 0; k < r; ++k) cj[k] = 0;
            }
            acc = wave_sum(acc);
            if (lane == 0) fam[i * BN_WAVES + wave] = acc;
            __syncthreads();   // the table is all zero again
        }
        if (tid == 0) {
            double score = 0.0;
            for (int i = 0; i < n_var; ++i) {
                const double* f = fam + i * BN_WAVES;
                const int r = cards.r[i];
                const int q = bn_family_cells(cards, i, pm[i] & var_mask) / r;
                score += ((f[0] + f[1]) + (f[2] + f[3])) - half_log_s * (double)q * (double)(r - 1);
            }
            scores[m] = score;
        }
        // (fam is rewritten only after the next structure's first family barrier, which thread 0 reaches after this read)
    }
}

// one thread per dense row: validity by the BN rules of dvae_select.hip, then the middle vertices' arcs renamed by the rank
// of their types
__global__ void __launch_bounds__(256) bn_rows_kernel(const int32_t* __restrict__ types, const uint32_t* __restrict__ preds,
                                                      const int32_t* __restrict__ nv, int64_t R, int n, int nvt, int start_type,
                                                      int end_type, uint32_t* __restrict__ parents, int32_t* __restrict__ valid) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= R) return;
    const int n_var = nvt - 2;
    const int k = nv[row];
    const int32_t* trow = types + row * n;
    const uint32_t* prow = preds + row * n;
    bool ok = k == nvt && k <= n;
    int n_start = 0, n_end = 0;
    uint64_t seen = 0;
    if (ok) {
        for (int v = 0; v < k; ++v) {
            const int t = trow[v];
            if (t < 0 || t >= nvt) { ok = false; break; }
            if (t == start_type) ++n_start;
            else if (t == end_type) ++n_end;
            seen |= 1ull << t;
        }
    }
    ok = ok && n_start == 1 && n_end == 1 && __popcll(seen) == nvt;
    valid[row] = ok ? 1 : 0;
    uint32_t* out = parents + row * n_var;
    for (int i = 0; i < n_var; ++i) out[i] = 0;
    if (!ok) return;
    // (types are distinct: the rank of a middle vertex's type among the middle types is its variable)
    for (int v = 1; v < k - 1; ++v) {
        int rv = 0;
        for (int u = 1; u < k - 1; ++u) rv += trow[u] < trow[v];
        uint32_t m = prow[v] & ((1u << v) - 1u) & ~1u, word = 0;   // predecessors among the middle vertices below v
        for (; m; m &= m - 1u) {
            const int u = __ffs((int)m) - 1;
            int ru = 0;
            for (int w = 1; w < k - 1; ++w) ru += trow[w] < trow[u];
            word |= 1u << ru;
        }
        out[rv] = word;
    }
}

bool bn_data_ok(const dagnn_bn_data* d) {
    if (!d || !d->cols) return false;
    if (d->n_var < 1 || d->n_var > BN_MAXV) return false;
    if (d->S < 1 || d->S >= (int64_t(1) << 31)) return false;
    if (d->ld < d->S || d->ld % 16 != 0 || d->ld > (int64_t(1) << 31) + 16) return false;
    if (reinterpret_cast<uintptr_t>(d->cols) % 16 != 0) return false;
    for (int i = 0; i < d->n_var; ++i)
        if (d->cards[i] < 1 || d->cards[i] > 255) return false;
    return true;
}

std::atomic<unsigned long long> g_bn_attr_staged{0};

}  // namespace

extern "C" int dagnn_bn_stage_fits(const dagnn_bn_data* d) {
    if (!bn_data_ok(d)) return DAGNN_EINVAL;
    return (int64_t)d->n_var * d->ld <= (int64_t)(BN_LDS_LIMIT - BN_FIXED_LDS) ? 1 : 0;
}

extern "C" int dagnn_bn_score(const dagnn_bn_data* d, const uint32_t* parents, const int32_t* valid, int64_t M, int stage,
                              double* scores, int32_t* n_over, void* stream) {
    if (!bn_data_ok(d)) return DAGNN_EINVAL;
    if (M < 0 || M >= (int64_t(1) << 31)) return DAGNN_EINVAL;
    if (stage != DAGNN_BN_STAGE_AUTO && stage != DAGNN_BN_STAGE_LDS && stage != DAGNN_BN_STAGE_GLOBAL) return DAGNN_EINVAL;
    const bool fits = (int64_t)d->n_var * d->ld <= (int64_t)(BN_LDS_LIMIT - BN_FIXED_LDS);
    if (stage == DAGNN_BN_STAGE_LDS && !fits) return DAGNN_EINVAL;
    if (M == 0) return DAGNN_OK;
    if (!parents || !scores || !n_over) return DAGNN_EINVAL;
    const bool staged = stage == DAGNN_BN_STAGE_LDS || (stage == DAGNN_BN_STAGE_AUTO && fits);
    BnCards cards;
    for (int i = 0; i < BN_MAXV; ++i) cards.r[i] = i < d->n_var ? d->cards[i] : 1;
    const int lds = BN_FIXED_LDS + (staged ? (int)(d->n_var * d->ld) : 0);
    const unsigned blocks = (unsigned)(M < 1024 ? M : 1024);   // (grid-stride beyond; a workgroup stages the table once)
    if (staged) {
        const hipError_t e = dagnn_lds_attr_once(g_bn_attr_staged, reinterpret_cast<const void*>(&bn_score_kernel<true>), BN_LDS_LIMIT);
        if (e != hipSuccess) return DAGNN_EHIP(e);
        hipLaunchKernelGGL(bn_score_kernel<true>, dim3(blocks), dim3(BN_T), lds, (hipStream_t)stream, d->cols, d->ld, d->S,
                           d->n_var, cards, parents, valid, M, scores, n_over);
    } else {
        hipLaunchKernelGGL(bn_score_kernel<false>, dim3(blocks), dim3(BN_T), lds, (hipStream_t)stream, d->cols, d->ld, d->S,
                           d->n_var, cards, parents, valid, M, scores, n_over);
    }
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_bn_rows_to_parents(const int32_t* types, const int32_t* preds, const int32_t* nv, int64_t R, int n, int nvt,
                                        int start_type, int end_type, uint32_t* parents, int32_t* valid, void* stream) {
    if (R < 0 || R >= (int64_t(1) << 31) || n < 3 || n > DAGNN_DVAE_MAX_N || nvt < 3 || nvt > n) return DAGNN_EINVAL;
    if (start_type < 0 || start_type >= nvt || end_type < 0 || end_type >= nvt || start_type == end_type) return DAGNN_EINVAL;
    if (R == 0) return DAGNN_OK;
    if (!types || !preds || !nv || !parents || !valid) return DAGNN_EINVAL;
    hipLaunchKernelGGL(bn_rows_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, types,
                       reinterpret_cast<const uint32_t*>(preds), nv, R, n, nvt, start_type, end_type, parents, valid);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
