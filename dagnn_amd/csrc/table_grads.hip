// table_grads.hip - the embedding-table gradients of a training step with ONE summation order (dagnn_table_grads).
//
// Reference path: autograd's accumulation behind the `nn.Embedding` lookups of ogbg-code/utils.py:26-28 (utils2.py:26-28):
// out_t[r] = sum of g[v] over the nodes v with key_t[v] == r.  torch's `index_add_` does it with float atomics (the order
// is the arrival order); here every row is summed in the order the header states: members ascending in v, chunks of
// TG_CHUNK consecutive members summed left to right, the chunks' partials added left to right onto +0.0.
//
// Two stages, six launches for up to three tables together:
//   index  tg_count    one wave per (table, node range b): zeroes its stripe M[b][0..R) and counts its nodes' keys into it
//          tg_ranges   one thread per (table, row): M[b][r] := members of r in ranges < b; the row's count
//          tg_offsets  one workgroup per table: exclusive scans of the counts -> segment offsets `off`, chunk offsets
//                      `coff`, partial-slot offsets `poff` (rows of >= 2 chunks only)
//          tg_place    the waves of tg_count again: node v goes to members[off[k] + M[b][k] + (rank among the equal keys of
//                      its 64-node tile)] - a stable placement, so every segment ascends in v; the node that opens a chunk
//                      writes the chunk's record {row, first member, members, partial slot}
//   sum    tg_partial  one group of lanes per chunk (lanes own float4 columns, a wave of 64 spans 256 columns; narrower
//                      rows put several chunks in a wave): walks the chunk's members in order; the partial goes to its
//                      slot, or - the row has this one chunk - as +0.0 + p straight to `out`
//          tg_rows     one group per row with 0 or >= 2 chunks: +0.0, plus the partials in chunk order
// The member lists and offsets are unique (a stable sort has one result), so integer atomics in their construction change
// no word; every float is added by exactly one lane in program order.  Compile without fast-math: `0.0f + p` must stay an add
// (p = -0.0 gives +0.0) and no add may be reassociated.
#include "common.h"

#define TG_CHUNK DAGNN_TABLE_GRADS_CHUNK
#define TG_MAX_TABLES DAGNN_TABLE_GRADS_MAX_TABLES
#define TG_MAX_RANGES 64          // node ranges (waves) per table
#define TG_MATRIX_WORDS (1 << 22) // cap of ranges x R: tables of more than 65536 rows get fewer ranges
#define TG_LIMIT (1 << 24)        // N, R below this
#define TG_BATCH 16               // row loads in flight per lane
#define TG_SCAN_ROWS 8            // rows per thread and tile of the offset scans (8 192 rows per tile)

static_assert(TG_CHUNK == 32, "the chunk arithmetic below shifts by 5");

struct TgTable {
    const long long* keys;
    long long kstride;
    float* out;
    long long ld_out4;     // row pitch of out in float4
    int* M;                // [nb][R]
    int* off;              // [R + 1] first member of each row (row counts between tg_ranges and tg_offsets)
    int* coff;             // [R + 1] first chunk of each row
    int* poff;             // [R + 1] first partial slot of each row (rows of >= 2 chunks own slots)
    int* members;          // [N]
    int4* crec;            // [max chunks] {row, first member position, members, partial slot or -1}
    float4* partial;       // [max slots][H4]
    int R, nb, span, bits; // rows; node ranges; nodes per range (a multiple of 64); bits of R - 1
    int wave0, rblk0, cblk0, oblk0;   // first block of this table in the grids of tg_count / tg_ranges / tg_partial / tg_rows
};

struct TgParams {
    TgTable t[TG_MAX_TABLES];
    const float4* g;
    long long ld_g4;
    int nt, N, H4, lpr;    // tables; nodes; float4 columns; lanes per row inside a wave (a power of two <= 64)
};

// table of a block: the last one whose first block is <= b
#define TG_FIND(field)                                                  \
    int ti = 0;                                                         \
    for (int q = 1; q < P.nt; ++q) if ((int)blockIdx.x >= P.t[q].field) ti = q; \
    const TgTable& T = P.t[ti];

// Among the active lanes of the wave that hold the same key: my position (ascending lane), their number, their first lane.
// One ballot per key bit (`bits` = bits of R - 1, wave-uniform): the lanes that agree with me on every bit.
static __device__ __forceinline__ void tg_peers(bool act, int key, int lane, int bits, int& rank, int& cnt, int& first) {
    unsigned long long m = __ballot(act);
    for (int b = 0; b < bits; ++b) {
        const bool one = (key >> b) & 1;
        const unsigned long long v = __ballot(one);
        m &= one ? v : ~v;
    }
    rank = __popcll(m & ((1ull << lane) - 1ull));
    cnt = __popcll(m);
    first = act ? __ffsll((long long)m) - 1 : lane;
}

// The key of node v as stored (-1: past the range), loaded one tile ahead of its use; then: is it a row of the table?
static __device__ __forceinline__ long long tg_load_key(const TgTable& T, int v, int end) {
    return v < end ? T.keys[(long long)v * T.kstride] : -1;
}
static __device__ __forceinline__ bool tg_key(const TgTable& T, long long k, int& key) {
    const bool act = k >= 0 && k < (long long)T.R;   // outside the table: contributes nothing, indexes nothing
    key = act ? (int)k : 0;
    return act;
}

__global__ void __launch_bounds__(64) tg_count(TgParams P) {
    TG_FIND(wave0)
    const int b = blockIdx.x - T.wave0, lane = threadIdx.x;
    int* Mb = T.M + (size_t)b * T.R;
    const int end = min(P.N, (b + 1) * T.span);
    long long next = tg_load_key(T, b * T.span + lane, end);
    for (int r = lane; r < T.R; r += 64) Mb[r] = 0;
    __threadfence();   // the zeros are in memory before the atomics below reach it
    for (int v0 = b * T.span; v0 < end; v0 += 64) {
        int key, rank, cnt, first;
        const bool act = tg_key(T, next, key);
        next = tg_load_key(T, v0 + 64 + lane, end);
        tg_peers(act, key, lane, T.bits, rank, cnt, first);
        if (act && first == lane) atomicAdd(&Mb[key], cnt);
    }
}

__global__ void __launch_bounds__(256) tg_ranges(TgParams P) {
    TG_FIND(rblk0)
    const int r = (blockIdx.x - T.rblk0) * 256 + threadIdx.x;
    if (r >= T.R) return;
    int* Mr = T.M + r;
    int run = 0;
    for (int b0 = 0; b0 < T.nb; b0 += 16) {   // (16 loads in flight, then their stores: a load behind a store to the same array waits for it)
        int x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = b0 + u < T.nb ? Mr[(size_t)(b0 + u) * T.R] : 0;
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (b0 + u < T.nb) { Mr[(size_t)(b0 + u) * T.R] = run; run += x[u]; }
    }
    T.off[r] = run;
}

__global__ void __launch_bounds__(1024) tg_offsets(TgParams P) {
    const TgTable& T = P.t[blockIdx.x];
    __shared__ int wsum[3][16];
    __shared__ int buf[1024 * (TG_SCAN_ROWS + 1)];   // a tile's rows, one pad word per TG_SCAN_ROWS: thread t's rows start at word (TG_SCAN_ROWS + 1) t
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int* const dst[3] = {T.off, T.coff, T.poff};
    int carry[3] = {0, 0, 0};
    // a thread scans TG_SCAN_ROWS consecutive rows of the tile; global memory is read and written with consecutive lanes on
    // consecutive rows, the tile turns in LDS (a lane that stores its own 8 rows touches 64 cache lines per instruction)
    for (int base = 0; base < T.R; base += 1024 * TG_SCAN_ROWS) {
#pragma unroll
        for (int u = 0; u < TG_SCAN_ROWS; ++u) {
            const int i = u * 1024 + tid;
            buf[i + i / TG_SCAN_ROWS] = base + i < T.R ? T.off[base + i] : 0;
        }
        __syncthreads();
        int n[TG_SCAN_ROWS];
        int x[3] = {0, 0, 0};
#pragma unroll
        for (int u = 0; u < TG_SCAN_ROWS; ++u) {
            n[u] = buf[tid * (TG_SCAN_ROWS + 1) + u];
            const int m = (n[u] + TG_CHUNK - 1) >> 5;
            x[0] += n[u]; x[1] += m; x[2] += m >= 2 ? m : 0;
        }
        int inc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int s = x[k];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(s, o, 64);
                if (lane >= o) s += up;
            }
            inc[k] = s;
            if (lane == 63) wsum[k][w] = s;
        }
        __syncthreads();
        int ex[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int before = 0, total = 0;
            for (int q = 0; q < 16; ++q) {
                const int s = wsum[k][q];
                if (q < w) before += s;
                total += s;
            }
            ex[k] = carry[k] + before + inc[k] - x[k];
            carry[k] += total;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            __syncthreads();   // (everybody has read the previous contents of buf)
            int e = ex[k];
#pragma unroll
            for (int u = 0; u < TG_SCAN_ROWS; ++u) {
                buf[tid * (TG_SCAN_ROWS + 1) + u] = e;
                const int m = (n[u] + TG_CHUNK - 1) >> 5;
                e += k == 0 ? n[u] : (k == 1 ? m : (m >= 2 ? m : 0));
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < TG_SCAN_ROWS; ++u) {
                const int i = u * 1024 + tid;
                if (base + i < T.R) dst[k][base + i] = buf[i + i / TG_SCAN_ROWS];
            }
        }
        __syncthreads();
    }
    if (tid == 0) { T.off[T.R] = carry[0]; T.coff[T.R] = carry[1]; T.poff[T.R] = carry[2]; }
}

__global__ void __launch_bounds__(64) tg_place(TgParams P) {
    TG_FIND(wave0)
    const int b = blockIdx.x - T.wave0, lane = threadIdx.x;
    int* Mb = T.M + (size_t)b * T.R;
    const int end = min(P.N, (b + 1) * T.span);
    long long next = tg_load_key(T, b * T.span + lane, end);
    for (int v0 = b * T.span; v0 < end; v0 += 64) {
        int key, rank, cnt, first;
        const bool act = tg_key(T, next, key);
        next = tg_load_key(T, v0 + 64 + lane, end);
        tg_peers(act, key, lane, T.bits, rank, cnt, first);
        // (key is 0 on the lanes without a node: the offsets are loaded next to the atomic's round trip, not behind it)
        const int o = T.off[key], n = T.off[key + 1] - o, c0 = T.coff[key], p0 = T.poff[key];
        int base = 0;
        if (act && first == lane) base = atomicAdd(&Mb[key], cnt);   // members of this key in earlier ranges and tiles
        base = __shfl(base, first, 64);
        if (!act) continue;
        const int q = base + rank;             // position inside the row's list
        T.members[o + q] = v0 + lane;
        if ((q & (TG_CHUNK - 1)) == 0) {       // this node opens chunk q / 32 of its row
            const int m = (n + TG_CHUNK - 1) >> 5;
            T.crec[c0 + (q >> 5)] = make_int4(key, o + q, min(TG_CHUNK, n - q), m >= 2 ? p0 + (q >> 5) : -1);
        }
    }
}

static __device__ __forceinline__ void tg_add(float4& a, const float4& x) {
    a.x = a.x + x.x; a.y = a.y + x.y; a.z = a.z + x.z; a.w = a.w + x.w;
}

__global__ void __launch_bounds__(256) tg_partial(TgParams P) {
    TG_FIND(cblk0)
    const int c = (blockIdx.x - T.cblk0) * (256 / P.lpr) + threadIdx.x / P.lpr;
    const int col = blockIdx.y * 64 + (threadIdx.x & (P.lpr - 1));
    if (c >= T.coff[T.R] || col >= P.H4) return;
    const int4 rec = T.crec[c];
    const int* mem = T.members + rec.y;
    const float4* gc = P.g + col;
    int id[TG_CHUNK];   // the chunk's members, all loads in flight at once (the same address in every lane of the group)
#pragma unroll
    for (int j = 0; j < TG_CHUNK; ++j) id[j] = mem[j < rec.z ? j : 0];   // (unconditional: a load under a branch is waited for at its join)
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j0 = 0; j0 < TG_CHUNK; j0 += TG_BATCH) {
        if (j0 >= rec.z) break;
        float4 x[TG_BATCH];
#pragma unroll
        for (int u = 0; u < TG_BATCH; ++u)
            x[u] = j0 + u < rec.z ? gc[(long long)id[j0 + u] * P.ld_g4] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j0 == 0) acc = x[0];   // the sum starts from the first member, not from zero
#pragma unroll
        for (int u = (j0 == 0 ? 1 : 0); u < TG_BATCH; ++u) if (j0 + u < rec.z) tg_add(acc, x[u]);
    }
    if (rec.w >= 0) {
        T.partial[(size_t)rec.w * P.H4 + col] = acc;
    } else {   // the row's only chunk
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        tg_add(o, acc);
        reinterpret_cast<float4*>(T.out)[(long long)rec.x * T.ld_out4 + col] = o;
    }
}

__global__ void __launch_bounds__(256) tg_rows(TgParams P) {
    TG_FIND(oblk0)
    const int r = (blockIdx.x - T.oblk0) * (256 / P.lpr) + threadIdx.x / P.lpr;
    const int col = blockIdx.y * 64 + (threadIdx.x & (P.lpr - 1));
    if (r >= T.R || col >= P.H4) return;
    const int m = P.N > 0 ? T.coff[r + 1] - T.coff[r] : 0;
    if (m == 1) return;   // written by tg_partial
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (m > 0) {
        const float4* pc = T.partial + (size_t)T.poff[r] * P.H4 + col;
        for (int j0 = 0; j0 < m; j0 += TG_BATCH) {
            const int nn = m - j0;
            float4 x[TG_BATCH];
#pragma unroll
            for (int u = 0; u < TG_BATCH; ++u) x[u] = u < nn ? pc[(size_t)(j0 + u) * P.H4] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int u = 0; u < TG_BATCH; ++u) if (u < nn) tg_add(acc, x[u]);
        }
    }
    reinterpret_cast<float4*>(T.out)[(long long)r * T.ld_out4 + col] = acc;
}

// ------------------------------------------------------------------ host side
struct TgLayout {
    size_t M[TG_MAX_TABLES], off[TG_MAX_TABLES], coff[TG_MAX_TABLES], poff[TG_MAX_TABLES], members[TG_MAX_TABLES],
        crec[TG_MAX_TABLES], partial[TG_MAX_TABLES], total;
    int nb[TG_MAX_TABLES], span[TG_MAX_TABLES];
    long long max_chunks[TG_MAX_TABLES];
};

static bool tg_layout(int64_t N, int H, const int64_t* rows, int nt, TgLayout& L) {
    if (N < 0 || N >= TG_LIMIT || H < 4 || H % 4 != 0 || !rows || nt < 1 || nt > TG_MAX_TABLES) return false;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 15) & ~size_t(15); return at; };
    for (int t = 0; t < nt; ++t) {
        const int64_t R = rows[t];
        if (R < 1 || R >= TG_LIMIT) return false;
        int64_t nb = TG_MATRIX_WORDS / R;
        nb = nb < 1 ? 1 : (nb > TG_MAX_RANGES ? TG_MAX_RANGES : nb);
        const int64_t tiles = (N + 63) / 64;
        if (nb > tiles) nb = tiles < 1 ? 1 : tiles;
        L.nb[t] = (int)nb;
        L.span[t] = (int)(((N + nb - 1) / nb + 63) / 64 * 64);
        // chunks: sum over rows of ceil(n_r / 32) <= N / 32 + (rows with members); slots: rows of >= 33 members only
        const int64_t chunks = N / TG_CHUNK + (R < N ? R : N);
        L.max_chunks[t] = chunks < N ? chunks : N;
        const int64_t slots = N / TG_CHUNK + N / (TG_CHUNK + 1);
        L.M[t] = take((size_t)nb * R * 4);
        L.off[t] = take((size_t)(R + 1) * 4);
        L.coff[t] = take((size_t)(R + 1) * 4);
        L.poff[t] = take((size_t)(R + 1) * 4);
        L.members[t] = take((size_t)N * 4);
        L.crec[t] = take((size_t)L.max_chunks[t] * 16);
        L.partial[t] = take((size_t)slots * H * 4);
    }
    L.total = o;
    return true;
}

extern "C" size_t dagnn_table_grads_workspace_bytes(int64_t N, int H, const int64_t* rows, int num_tables) {
    TgLayout L;
    return tg_layout(N, H, rows, num_tables, L) ? (L.total > 16 ? L.total : 16) : 0;
}

extern "C" int dagnn_table_grads(const dagnn_table_grads_args* a, void* stream) {
    if (!a || a->num_tables < 1 || a->num_tables > TG_MAX_TABLES || a->stages < 0 || a->stages > DAGNN_TABLE_GRADS_SUM) return DAGNN_EINVAL;
    const int64_t N = a->N;
    const int H = a->H, nt = a->num_tables;
    int64_t rows[TG_MAX_TABLES];
    for (int t = 0; t < nt; ++t) rows[t] = a->table[t].R;
    TgLayout L;
    if (!tg_layout(N, H, rows, nt, L)) return DAGNN_EINVAL;
    if (a->ld_g < H || a->ld_g % 4 != 0) return DAGNN_EINVAL;
    if (N > 0 && (!a->g || !a->workspace || ((uintptr_t)a->g & 15) || ((uintptr_t)a->workspace & 15))) return DAGNN_EINVAL;
    for (int t = 0; t < nt; ++t) {
        const dagnn_table_grads_table& u = a->table[t];
        if (!u.out || ((uintptr_t)u.out & 15) || u.ld_out < H || u.ld_out % 4 != 0 || u.key_stride < 0 || (N > 0 && !u.keys))
            return DAGNN_EINVAL;
    }
    if (N > 0 && a->workspace_bytes < L.total) return DAGNN_ENOSPC;

    TgParams P;
    P.g = reinterpret_cast<const float4*>(a->g);
    P.ld_g4 = a->ld_g / 4;
    P.nt = nt; P.N = (int)N; P.H4 = H / 4;
    P.lpr = 1;
    while (P.lpr < 64 && P.lpr < P.H4) P.lpr <<= 1;
    const int groups = 256 / P.lpr;                  // chunks (rows) per workgroup of the two sum kernels
    const int slabs = (P.H4 + 63) / 64;              // 256-column slabs (grid y)
    char* ws = static_cast<char*>(a->workspace);
    int waves = 0, rblk = 0, cblk = 0, oblk = 0;
    for (int t = 0; t < nt; ++t) {
        TgTable& T = P.t[t];
        const dagnn_table_grads_table& u = a->table[t];
        T.keys = reinterpret_cast<const long long*>(u.keys);
        T.kstride = u.key_stride;
        T.out = u.out;
        T.ld_out4 = u.ld_out / 4;
        T.R = (int)u.R; T.nb = L.nb[t]; T.span = L.span[t];
        T.bits = 0;
        while (((int64_t)1 << T.bits) < u.R) ++T.bits;
        T.M = reinterpret_cast<int*>(ws + L.M[t]);
        T.off = reinterpret_cast<int*>(ws + L.off[t]);
        T.coff = reinterpret_cast<int*>(ws + L.coff[t]);
        T.poff = reinterpret_cast<int*>(ws + L.poff[t]);
        T.members = reinterpret_cast<int*>(ws + L.members[t]);
        T.crec = reinterpret_cast<int4*>(ws + L.crec[t]);
        T.partial = reinterpret_cast<float4*>(ws + L.partial[t]);
        T.wave0 = waves; T.rblk0 = rblk; T.cblk0 = cblk; T.oblk0 = oblk;
        waves += T.nb;
        rblk += (T.R + 255) / 256;
        cblk += (int)((L.max_chunks[t] + groups - 1) / groups);
        oblk += (T.R + groups - 1) / groups;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool index = a->stages != DAGNN_TABLE_GRADS_SUM, sum = a->stages != DAGNN_TABLE_GRADS_INDEX;
    if (N > 0 && index) {
        hipLaunchKernelGGL(tg_count, dim3(waves), dim3(64), 0, s, P);
        hipLaunchKernelGGL(tg_ranges, dim3(rblk), dim3(256), 0, s, P);
        hipLaunchKernelGGL(tg_offsets, dim3(nt), dim3(1024), 0, s, P);
        hipLaunchKernelGGL(tg_place, dim3(waves), dim3(64), 0, s, P);
    }
    if (N > 0 && sum) hipLaunchKernelGGL(tg_partial, dim3(cblk, slabs), dim3(256), 0, s, P);
    if (sum) hipLaunchKernelGGL(tg_rows, dim3(oblk, slabs), dim3(256), 0, s, P);   // (N == 0: every row is empty, the zeros are all there is)
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
