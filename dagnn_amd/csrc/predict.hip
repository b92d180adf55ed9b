// predict.hip - the evaluation half of the TOK task's loop (ogbg-code/main_pyg.py:91-124): predicted tokens and the integer
// counts behind the F1 evaluator (ogb/graphproppred/evaluate.py:231-267).
//
// Reference path replaced, per batch: the S heads' GEMMs (dagnn.py:212-215), S torch.argmax launches and a cat
// (main_pyg.py:106-109), a copy to the host, decode_arr_to_seq per row (utils.py:166-179) and the evaluator's Python set
// arithmetic per graph.  An evaluation pass never needs the [B, S V] logits (12.8 MB at B = 128, S = 5, V = 5002), only each
// head's winner:
//   dagnn_heads_argmax   the GEMM of gemm_f32.hip (128 x 128 block tile, fp32 MFMA 32x32x2, both operands K-contiguous; the
//                        loaders and main loops below are that file's, stage for stage) whose epilogue reduces every row of
//                        the tile to (best, column, second) instead of storing C; column tiles never straddle two heads;
//                        one 16-byte partial per (graph, head, tile), merged in ascending tile order by a second launch;
//   dagnn_heads_score    the same two launches with a wider epilogue: the k best columns, the log-sum-exp and the row's
//                        negative log-likelihood ("heads + score" below);
//   dagnn_rows_argmax    the same answer from logits that exist (a training step needs them for the loss);
//   dagnn_seq_f1_counts  per graph (true_positive, n_pred, n_ref, len) in integers.
//
// The order of logits (rows_dev.h: logit_key / logit_pack / logit_col) makes "greatest value, lowest column" a single integer
// maximum, so the merges are exact, associative and independent of the order they run in.
#include "rows_dev.h"

namespace {

constexpr int KEY_NONE = INT_MIN;
constexpr int KEY_NEG_INF = -0x7f800000;

__device__ __forceinline__ float val_of(int k) {
    if (k == KEY_NAN) return __int_as_float(0x7fc00000);
    if (k < KEY_NEG_INF) return -INFINITY;   // (no such column: the runner-up of a one-column head)
    return __int_as_float(k >= 0 ? k : (int)(0x80000000u - (unsigned)k));
}
struct __attribute__((aligned(16))) Part {
    long long best;   // logit_pack(key, column) of the winner; logit_pack(KEY_NONE, ..) = nothing seen
    int second;       // key of the runner-up
    int pad;
};
__device__ __forceinline__ Part part_none() { return Part{LLONG_MIN, KEY_NONE, 0}; }
__device__ __forceinline__ void part_merge(Part& a, long long best, int second) {
    const long long lo = a.best < best ? a.best : best;
    a.best = a.best < best ? best : a.best;
    a.second = max(max(a.second, second), (int)(lo >> 32));
}

// ---------------------------------------------------------------------------------------------- heads + argmax
constexpr int BM = 128, BN = 128, BK = 16, LDT = BM + 4;
constexpr int GK = 32, GP = GK + 4;
constexpr int SP = 65;   // pitch of a wave's 32 x 64 staging tile: the 64 lanes of the row scan fall on 64 banks
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <bool VEC>
__device__ __forceinline__ void load_tile(const float* __restrict__ P, int64_t rows, int K, int64_t ld, int64_t row0, int k0,
                                          int tid, float4 (&v)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i;
        const int64_t r = row0 + (idx >> 2);
        const int k = k0 + (idx & 3) * 4;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows) {
            const float* p = P + r * ld + k;
            if (VEC && k + 3 < K) {
                t = *reinterpret_cast<const float4*>(p);
            } else {
                if (k < K) t.x = p[0];
                if (k + 1 < K) t.y = p[1];
                if (k + 2 < K) t.z = p[2];
                if (k + 3 < K) t.w = p[3];
            }
        }
        v[i] = t;
    }
}

__device__ __forceinline__ void store_tile(float* __restrict__ S, int tid, const float4 (&v)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i;
        const int r = idx >> 2, kq = (idx & 3) * 4;
        S[(kq + 0) * LDT + r] = v[i].x;
        S[(kq + 1) * LDT + r] = v[i].y;
        S[(kq + 2) * LDT + r] = v[i].z;
        S[(kq + 3) * LDT + r] = v[i].w;
    }
}

__device__ __forceinline__ void load_rows4(const float* __restrict__ P, int64_t rows, int64_t ld, int64_t row0, int k0, int tid,
                                           float4 (&v)[4]) {
    const int c = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int64_t r = row0 + (tid >> 3) + 32 * i;
        r = r < rows ? r : rows - 1;   // rows past the end repeat the last one (they never reach a maximum)
        v[i] = *reinterpret_cast<const float4*>(P + r * ld + k0 + 4 * c);
    }
}

__device__ __forceinline__ void store_rows4(float* __restrict__ S, int tid, const float4 (&v)[4]) {
    const int c = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(S + ((tid >> 3) + 32 * i) * GP + 4 * c) = v[i];
}

struct HeadsArgs {
    const float* out;
    const float* wcat;
    const float* bcat;
    Part* part;
    int64_t M, ld_out, ldw;
    int D, S, V, tph, tiles_m;
};

struct TileId { int64_t m0; int head, tile; };

// XCD-aware, bijective remap (hardware puts block b on XCD b % 8): the column tiles of one row tile run on one XCD and share
// `out` in its L2, as in gemm_f32.hip
__device__ __forceinline__ TileId tile_of(const HeadsArgs& a) {
    const int tiles_n = a.S * a.tph;
    const int nwg = a.tiles_m * tiles_n;
    const int bid = blockIdx.x;
    const int q = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const int swz = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (bid >> 3);
    const int tm = swz / tiles_n, tn = swz - tm * tiles_n;
    const int head = tn / a.tph;
    return TileId{(int64_t)tm * BM, head, tn - head * a.tph};
}

// The tile's 128 x 128 accumulators (C/D layout of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane
// >> 5)) -> one Part per row.  Each wave stages 32 rows x 64 columns at a time in LDS (bias added), two lanes scan a row's 64
// columns in ascending order, one shuffle joins them; the two waves that share the rows meet in `rowres`.  Columns at or
// beyond V (the head's partial last tile) are never looked at.
__device__ __forceinline__ void argmax_epilogue(const f32x16 (&acc)[2][2], float* __restrict__ stage, Part* __restrict__ rowres,
                                                const HeadsArgs& a, const TileId& t) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int fr = lane & 31, fk = lane >> 5;
    const int n0 = t.tile * BN;
    float* __restrict__ st = stage + wave * (32 * SP);
    float bv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn + j * 32 + fr;
        bv[j] = col < a.V ? a.bcat[(int64_t)t.head * a.V + col] : 0.f;
    }
    const int row = lane >> 1, c0 = (lane & 1) * 32;
    __syncthreads();   // (the main loop's last stage has been read by every wave)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) st[((e & 3) + 8 * (e >> 2) + 4 * fk) * SP + j * 32 + fr] = acc[i][j][e] + bv[j];
        __syncthreads();
        Part p = part_none();
        const int ncol = min(32, a.V - (n0 + wn + c0));   // live columns of this lane's half row (<= 0: none)
        for (int c = 0; c < ncol; ++c) part_merge(p, logit_pack(logit_key(st[row * SP + c0 + c]), n0 + wn + c0 + c), KEY_NONE);
        const long long ob = __shfl_xor(p.best, 1, 64);
        const int os = __shfl_xor(p.second, 1, 64);
        part_merge(p, ob, os);
        if ((lane & 1) == 0) rowres[(wave & 1) * BM + wm + i * 32 + row] = p;
        __syncthreads();
    }
    if (tid < BM && t.m0 + tid < a.M) {
        Part p = rowres[tid];
        const Part o = rowres[BM + tid];
        part_merge(p, o.best, o.second);
        a.part[((t.m0 + tid) * a.S + t.head) * a.tph + t.tile] = p;
    }
}

// the main loop of both generic kernels (argmax and score): the tile's 128 x 128 accumulators; `smem` = As[2] | Bs[2]
template <bool VEC>
__device__ __forceinline__ void heads_mainloop(f32x16 (&acc)[2][2], float* __restrict__ smem, const HeadsArgs& a, const TileId& t) {
    const float* __restrict__ A = a.out;
    const float* __restrict__ W = a.wcat + (int64_t)t.head * a.V * a.ldw;
    const int K = a.D, n0 = t.tile * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int fr = lane & 31, fk = lane >> 5;

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    float* As = smem;
    float* Bs = smem + 2 * BK * LDT;
    float4 ra[2], rb[2];
    load_tile<VEC>(A, a.M, K, a.ld_out, t.m0, 0, tid, ra);
    load_tile<VEC>(W, a.V, K, a.ldw, n0, 0, tid, rb);
    store_tile(As, tid, ra);
    store_tile(Bs, tid, rb);
    __syncthreads();

    const int nk = (K + BK - 1) / BK;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) {
            load_tile<VEC>(A, a.M, K, a.ld_out, t.m0, (kt + 1) * BK, tid, ra);
            load_tile<VEC>(W, a.V, K, a.ldw, n0, (kt + 1) * BK, tid, rb);
        }
        const float* as = As + cur * (BK * LDT);
        const float* bs = Bs + cur * (BK * LDT);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const int krow = (2 * kk + fk) * LDT;
            const float a0 = as[krow + wm + fr], a1 = as[krow + wm + 32 + fr];
            const float b0 = bs[krow + wn + fr], b1 = bs[krow + wn + 32 + fr];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (kt + 1 < nk) {
            store_tile(As + (cur ^ 1) * (BK * LDT), tid, ra);
            store_tile(Bs + (cur ^ 1) * (BK * LDT), tid, rb);
        }
        __syncthreads();
        cur ^= 1;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) heads_argmax_kernel(HeadsArgs a) {
    __shared__ float smem[4 * BK * LDT];   // As[2] | Bs[2]; the epilogue's staging tiles afterwards (4 x 32 x SP floats)
    __shared__ Part rowres[2 * BM];
    static_assert(4 * 32 * SP <= 4 * BK * LDT, "staging tiles must fit the operand buffers");
    const TileId t = tile_of(a);
    f32x16 acc[2][2];
    heads_mainloop<VEC>(acc, smem, a, t);
    argmax_epilogue(acc, smem, rowres, a, t);
}

// D a multiple of 32, 16-byte aligned rows (every model whose read-out width is: the headline's 1024): the 128-bit LDS
// traffic of gemm_nt_bias_k32_kernel
__device__ __forceinline__ void heads_mainloop_k32(f32x16 (&acc)[2][2], float* __restrict__ gsm, const HeadsArgs& a, const TileId& t) {
    const float* __restrict__ A = a.out;
    const float* __restrict__ W = a.wcat + (int64_t)t.head * a.V * a.ldw;
    const int K = a.D, n0 = t.tile * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int fr = lane & 31, fk = lane >> 5;

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    float4 ra[4], rb[4];
    load_rows4(A, a.M, a.ld_out, t.m0, 0, tid, ra);
    load_rows4(W, a.V, a.ldw, n0, 0, tid, rb);
    store_rows4(gsm, tid, ra);
    store_rows4(gsm + BM * GP, tid, rb);
    __syncthreads();
    const int nk = K / GK;
    for (int kt = 0; kt < nk; ++kt) {
        const int tn1 = min(kt + 1, nk - 1);   // unconditional (the last stage re-reads itself): no load behind a branch
        load_rows4(A, a.M, a.ld_out, t.m0, tn1 * GK, tid, ra);
        load_rows4(W, a.V, a.ldw, n0, tn1 * GK, tid, rb);
        const float* as = gsm + (kt & 1) * (2 * BM * GP);
        const float* bs = as + BM * GP;
#pragma unroll
        for (int kg = 0; kg < GK / 8; ++kg) {
            float4 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[i] = *reinterpret_cast<const float4*>(as + (wm + 32 * i + fr) * GP + 8 * kg + 4 * fk);
                bf[i] = *reinterpret_cast<const float4*>(bs + (wn + 32 * i + fr) * GP + 8 * kg + 4 * fk);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float av = q == 0 ? af[i].x : q == 1 ? af[i].y : q == 2 ? af[i].z : af[i].w;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const float bv = q == 0 ? bf[j].x : q == 1 ? bf[j].y : q == 2 ? bf[j].z : bf[j].w;
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i][j], 0, 0, 0);
                    }
                }
            }
        }
        float* ns = gsm + ((kt + 1) & 1) * (2 * BM * GP);
        store_rows4(ns, tid, ra);
        store_rows4(ns + BM * GP, tid, rb);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256, 2) heads_argmax_k32_kernel(HeadsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];   // [2][A: 128 x GP | B: 128 x GP]
    __shared__ Part rowres[2 * BM];
    static_assert(4 * 32 * SP <= 2 * 2 * BM * GP, "staging tiles must fit the operand buffers");
    const TileId t = tile_of(a);
    f32x16 acc[2][2];
    heads_mainloop_k32(acc, gsm, a, t);
    argmax_epilogue(acc, gsm, rowres, a, t);
}

// one thread per (graph, head): its tiles' partials in ascending tile order
__global__ void __launch_bounds__(256) heads_merge_kernel(const Part* __restrict__ part, int64_t rows, int tph,
                                                          long long* __restrict__ tok, float* __restrict__ top) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    Part p = part[r * tph];
    for (int k = 1; k < tph; ++k) {
        const Part o = part[r * tph + k];
        part_merge(p, o.best, o.second);
    }
    tok[r] = logit_col(p.best);
    if (top) {
        top[2 * r] = val_of((int)(p.best >> 32));
        top[2 * r + 1] = val_of(p.second);
    }
}

// ---------------------------------------------------------------------------------------------- heads + score
// The same two launches with a wider epilogue: per (graph, head, tile) the KT best packed keys in descending order, the tile's
// maximum m and sum of exp(x - m), and the logit at the target's column; the merge launch joins a row's tiles in ascending
// tile order (keys: exact and order-free; softmax: the order fixes the rounding) into the k best columns, their logits, the
// log-sum-exp and the row's negative log-likelihood.  KT in {1, 2, 4, 8}: every list lives in registers, insertion unrolled.
//
// A maximum of +-inf is replaced by 0 inside the exponentials, as torch.logsumexp does: a row with +inf sums to +inf, a row
// of -inf alone to 0 (log: -inf), a NaN poisons its sum, and nothing ever forms inf - inf.
template <int KT>
struct __attribute__((aligned(8))) SPart {
    long long top[KT];   // descending; LLONG_MIN (= logit_pack(KEY_NONE, -1)) where the tile has no further live column
    float m, s, xy;      // maximum, sum of exp(x - m) over the live columns; the target's logit if its column is in this tile
    int pad;
};

struct ScoreArgs {
    HeadsArgs h;
    const long long* y;   // [B, S] targets or null
    void* spart;          // SPart<KT> [B, S, tph]
    unsigned* ticket;     // the merge launch's arrival counter, zeroed by the first launch
};

template <int KT>
__device__ __forceinline__ void topk_insert(long long (&t)[KT], long long p) {
    if (p <= t[KT - 1]) return;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
        const long long hi = t[j] < p ? p : t[j];
        p = t[j] < p ? t[j] : p;
        t[j] = hi;
    }
}

__device__ __forceinline__ float finite_or_zero(float m) { return fabsf(m) == INFINITY ? 0.f : m; }

// (m, s) <- (m, s) joined with (om, os), in this order
__device__ __forceinline__ void soft_merge(float& m, float& s, float om, float os) {
    const float M = fmaxf(m, om), Mf = finite_or_zero(M);
    const float f0 = m == -INFINITY ? 1.f : __expf(finite_or_zero(m) - Mf);     // (a piece of -inf alone: s is 0 or NaN as it stands)
    const float f1 = om == -INFINITY ? 1.f : __expf(finite_or_zero(om) - Mf);
    s = s * f0 + os * f1;
    m = M;
}

// The staging of argmax_epilogue; each of a row's two lanes keeps the KT best of its 32 columns, their maximum and - in a
// second pass over the staged values - the sum of exponentials; lane pairs meet by shuffle, the wave of the upper 64 columns
// hands its rows over in `rtop` / `rms`, the wave of the lower 64 writes the partial.  Columns ascend through every join.
template <int KT>
__device__ __forceinline__ void score_epilogue(const f32x16 (&acc)[2][2], float* __restrict__ stage, long long* __restrict__ rtop,
                                               float2* __restrict__ rms, const ScoreArgs& sa, const TileId& t) {
    const HeadsArgs& a = sa.h;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int fr = lane & 31, fk = lane >> 5;
    const int n0 = t.tile * BN;
    float* __restrict__ st = stage + wave * (32 * SP);
    SPart<KT>* __restrict__ part = reinterpret_cast<SPart<KT>*>(sa.spart);
    float bv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn + j * 32 + fr;
        bv[j] = col < a.V ? a.bcat[(int64_t)t.head * a.V + col] : 0.f;
    }
    const int row = lane >> 1, c0 = (lane & 1) * 32;
    const int colbase = n0 + wn + c0;
    const int ncol = min(32, a.V - colbase);   // live columns of this lane's half row (<= 0: none)
    __syncthreads();   // (the main loop's last stage has been read by every wave)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) st[((e & 3) + 8 * (e >> 2) + 4 * fk) * SP + j * 32 + fr] = acc[i][j][e] + bv[j];
        __syncthreads();
        const int lrow = wm + i * 32 + row;              // row of the tile
        const int64_t grow = t.m0 + lrow;                // row of the batch
        const float* __restrict__ x = st + row * SP + c0;
        long long tk[KT];
#pragma unroll
        for (int j = 0; j < KT; ++j) tk[j] = LLONG_MIN;
        float m = -INFINITY, s = 0.f;
        for (int c = 0; c < ncol; ++c) {
            const float v = x[c];
            m = fmaxf(m, v);
            topk_insert(tk, logit_pack(logit_key(v), colbase + c));
        }
        const float mf = finite_or_zero(m);
        for (int c = 0; c < ncol; ++c) s += __expf(x[c] - mf);
        if (sa.y && grow < a.M) {
            const long long yc = sa.y[grow * a.S + t.head] - (long long)colbase;
            if (yc >= 0 && yc < ncol) part[(grow * a.S + t.head) * a.tph + t.tile].xy = x[yc];
        }
        {   // the row's other 32 columns of this wave
            const float om = __shfl_xor(m, 1, 64), os = __shfl_xor(s, 1, 64);
            long long ot[KT];
#pragma unroll
            for (int j = 0; j < KT; ++j) ot[j] = __shfl_xor(tk[j], 1, 64);
#pragma unroll
            for (int j = 0; j < KT; ++j) topk_insert(tk, ot[j]);
            soft_merge(m, s, om, os);   // (meaningful on the even lane: lower columns first)
        }
        if ((wave & 1) && (lane & 1) == 0) {
#pragma unroll
            for (int j = 0; j < KT; ++j) rtop[lrow * KT + j] = tk[j];
            rms[lrow] = make_float2(m, s);
        }
        __syncthreads();
        if (!(wave & 1) && (lane & 1) == 0 && grow < a.M) {
#pragma unroll
            for (int j = 0; j < KT; ++j) topk_insert(tk, rtop[lrow * KT + j]);
            const float2 o = rms[lrow];
            soft_merge(m, s, o.x, o.y);
            SPart<KT>* __restrict__ dst = part + (grow * a.S + t.head) * a.tph + t.tile;
#pragma unroll
            for (int j = 0; j < KT; ++j) dst->top[j] = tk[j];
            dst->m = m;
            dst->s = s;
        }
    }
}

template <bool VEC, int KT>
__global__ void __launch_bounds__(256) heads_score_kernel(ScoreArgs sa) {
    __shared__ float smem[4 * BK * LDT];   // As[2] | Bs[2]; the epilogue's staging tiles afterwards (4 x 32 x SP floats)
    __shared__ long long rtop[BM * KT];
    __shared__ float2 rms[BM];
    if (blockIdx.x == 0 && threadIdx.x == 0) *sa.ticket = 0u;
    const TileId t = tile_of(sa.h);
    f32x16 acc[2][2];
    heads_mainloop<VEC>(acc, smem, sa.h, t);
    score_epilogue<KT>(acc, smem, rtop, rms, sa, t);
}

// the row results live in the operand buffers behind the staging tiles: no static LDS, two blocks per CU as before
template <int KT>
__global__ void __launch_bounds__(256, 2) heads_score_k32_kernel(ScoreArgs sa) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];   // [2][A: 128 x GP | B: 128 x GP]
    constexpr int ROWRES = 4 * 32 * SP;   // floats: 16-byte aligned offset
    static_assert(ROWRES % 4 == 0 && (ROWRES + 2 * BM * KT + 2 * BM) <= 2 * 2 * BM * GP, "row results must fit the operand buffers");
    if (blockIdx.x == 0 && threadIdx.x == 0) *sa.ticket = 0u;
    const TileId t = tile_of(sa.h);
    f32x16 acc[2][2];
    heads_mainloop_k32(acc, gsm, sa.h, t);
    long long* rtop = reinterpret_cast<long long*>(gsm + ROWRES);
    score_epilogue<KT>(acc, gsm, rtop, reinterpret_cast<float2*>(rtop + BM * KT), sa, t);
}

// one thread per (graph, head): its tiles' partials in ascending tile order.  With `sums` the workgroup that arrives last adds
// the batch's row losses to the float64 in row order (one thread, 256 rows at a time through LDS) and the row count to the
// int64: no float atomics, bitwise repeatable.
constexpr int MT = 64;
template <int KT>
__global__ void __launch_bounds__(MT) heads_score_merge_kernel(const SPart<KT>* __restrict__ part, int64_t rows, int tph, int V, int k,
                                                               const long long* __restrict__ y, long long* __restrict__ tok,
                                                               float* __restrict__ logit, float* __restrict__ lse, float* __restrict__ nll,
                                                               double* __restrict__ sums, unsigned* __restrict__ ticket) {
    __shared__ float chunk[4 * MT];
    __shared__ unsigned last;
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * MT + tid;
    if (r < rows) {
        const SPart<KT>* __restrict__ p = part + r * tph;
        long long tk[KT];
#pragma unroll
        for (int j = 0; j < KT; ++j) tk[j] = p[0].top[j];
        float m = p[0].m, s = p[0].s;
        for (int q = 1; q < tph; ++q) {
#pragma unroll
            for (int j = 0; j < KT; ++j) topk_insert(tk, p[q].top[j]);
            soft_merge(m, s, p[q].m, p[q].s);
        }
        const float L = finite_or_zero(m) + __logf(s);
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (j < k) {
                tok[r * k + j] = logit_col(tk[j]);
                logit[r * k + j] = val_of((int)(tk[j] >> 32));
            }
        lse[r] = L;
        if (y) {
            const long long t = y[r];
            nll[r] = t >= 0 && t < V ? L - p[t / BN].xy : NAN;
        }
    }
    if (!sums) return;   // (uniform)
    __threadfence();
    __syncthreads();
    if (tid == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!last) return;   // (uniform per workgroup)
    __threadfence();
    double acc = sums[0];
    for (int64_t base = 0; base < rows; base += 4 * MT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t j = base + q * MT + tid;
            chunk[q * MT + tid] = j < rows ? __hip_atomic_load(nll + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
        }
        __syncthreads();
        if (tid == 0) {
            const int n = (int)min((int64_t)(4 * MT), rows - base);
            for (int j = 0; j < n; ++j) acc += (double)chunk[j];
        }
        __syncthreads();
    }
    if (tid == 0) {
        sums[0] = acc;
        reinterpret_cast<long long*>(sums)[1] += rows;
    }
}

// ---------------------------------------------------------------------------------------------- argmax of existing logits
// a workgroup per (graph, head): scalar reads up to the first 16-byte boundary of the head's V floats (V = 5002 puts the
// heads at every alignment), float4 reads behind it
__global__ void __launch_bounds__(256) rows_argmax_kernel(const float* __restrict__ logits, int64_t ld, int S, int V,
                                                          long long* __restrict__ tok) {
    __shared__ long long red[4];
    const int64_t r = blockIdx.x;
    const int64_t b = r / S;
    const int s = (int)(r - b * S);
    const float* __restrict__ x = logits + b * ld + (int64_t)s * V;
    const int tid = threadIdx.x;
    const int pre = min(V, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3));
    const int nvec = (V - pre) >> 2;
    long long best = LLONG_MIN;
    if (tid < pre) best = logit_pack(logit_key(x[tid]), tid);
    const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + pre);
    for (int q = tid; q < nvec; q += 256) {
        const float4 v = xv[q];
        const int c = pre + 4 * q;
        long long p = logit_pack(logit_key(v.x), c);
        best = p > best ? p : best;
        p = logit_pack(logit_key(v.y), c + 1);
        best = p > best ? p : best;
        p = logit_pack(logit_key(v.z), c + 2);
        best = p > best ? p : best;
        p = logit_pack(logit_key(v.w), c + 3);
        best = p > best ? p : best;
    }
    const int tail0 = pre + 4 * nvec;
    if (tail0 + tid < V) {   // (at most 3 columns)
        const long long p = logit_pack(logit_key(x[tail0 + tid]), tail0 + tid);
        best = p > best ? p : best;
    }
    best = wave_max(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) best = red[w] > best ? red[w] : best;
        tok[r] = logit_col(best);
    }
}

// ---------------------------------------------------------------------------------------------- the evaluator's counts
// a thread per graph (rows_dev.h: f1_counts_of_graph)
__global__ void __launch_bounds__(128) seq_f1_counts_kernel(const long long* __restrict__ tok, int64_t B, int S, long long eos,
                                                            const int* __restrict__ ref_ids, int R, const int* __restrict__ ref_extra,
                                                            int* __restrict__ counts) {
    const int64_t b = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (b >= B) return;
    const long long* __restrict__ t = tok + b * S;
    reinterpret_cast<int4*>(counts)[b] =
        f1_counts_of_graph([t](int i) { return t[i]; }, S, eos, ref_ids + b * R, R, ref_extra ? ref_extra[b] : 0);
}

bool heads_shape_ok(int64_t B, int S, int V) {
    return B >= 0 && S > 0 && V > 0 && (int64_t)S * V < (int64_t(1) << 31) && B * S < (int64_t(1) << 31);
}

}  // namespace

extern "C" size_t dagnn_heads_argmax_bytes(int64_t B, int S, int V) {
    if (!heads_shape_ok(B, S, V)) return 0;
    const int64_t tph = (V + BN - 1) / BN;
    return (size_t)(B > 0 ? B : 1) * S * tph * sizeof(Part);
}

extern "C" int dagnn_heads_argmax(const float* out, int64_t ld_out, const float* wcat, int64_t ldw, const float* bcat, int64_t B,
                                  int D, int S, int V, int64_t* tok, float* top, void* work, size_t work_bytes, void* stream) {
    if (!heads_shape_ok(B, S, V) || D <= 0 || ld_out < D || ldw < D) return DAGNN_EINVAL;
    if (B == 0) return DAGNN_OK;
    if (!out || !wcat || !bcat || !tok || !work || ((uintptr_t)work & 15)) return DAGNN_EINVAL;
    if (work_bytes < dagnn_heads_argmax_bytes(B, S, V)) return DAGNN_ENOSPC;
    HeadsArgs a;
    a.out = out; a.wcat = wcat; a.bcat = bcat; a.part = reinterpret_cast<Part*>(work);
    a.M = B; a.ld_out = ld_out; a.ldw = ldw; a.D = D; a.S = S; a.V = V;
    a.tph = (V + BN - 1) / BN;
    const int64_t tiles_m = (B + BM - 1) / BM;
    if (tiles_m * S * a.tph >= (int64_t(1) << 31)) return DAGNN_EINVAL;
    a.tiles_m = (int)tiles_m;
    const dim3 grid((unsigned)(tiles_m * S * a.tph));
    hipStream_t st = (hipStream_t)stream;
    const bool vec = ld_out % 4 == 0 && ldw % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)wcat & 15) == 0;
    if (vec && D % GK == 0) {
        constexpr size_t lds = (size_t)2 * 2 * BM * GP * sizeof(float);   // 72 KB: two blocks per CU
        static std::atomic<unsigned long long> attr_done{0ull};
        if (dagnn_lds_attr_once(attr_done, reinterpret_cast<const void*>(heads_argmax_k32_kernel), (int)lds) != hipSuccess)
            return DAGNN_EHIP(hipGetLastError());
        hipLaunchKernelGGL(heads_argmax_k32_kernel, grid, dim3(256), lds, st, a);
    } else if (vec)
        hipLaunchKernelGGL(heads_argmax_kernel<true>, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(heads_argmax_kernel<false>, grid, dim3(256), 0, st, a);
    DAGNN_CHECK_LAUNCH();
    const int64_t rows = B * S;
    hipLaunchKernelGGL(heads_merge_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, a.part, rows, a.tph,
                       reinterpret_cast<long long*>(tok), top);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

namespace {

constexpr size_t SCORE_HEAD_BYTES = 16;   // the merge launch's ticket, in front of the partials

int score_kt(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

template <int KT>
int launch_score(const ScoreArgs& sa, bool vec, int64_t rows, int k, int64_t* tok, float* logit, float* lse, float* nll, double* sums,
                 hipStream_t st) {
    const HeadsArgs& a = sa.h;
    const dim3 grid((unsigned)((int64_t)a.tiles_m * a.S * a.tph));
    if (vec && a.D % GK == 0) {
        constexpr size_t lds = (size_t)2 * 2 * BM * GP * sizeof(float);   // 72 KB: two blocks per CU
        static std::atomic<unsigned long long> attr_done{0ull};
        if (dagnn_lds_attr_once(attr_done, reinterpret_cast<const void*>(heads_score_k32_kernel<KT>), (int)lds) != hipSuccess)
            return DAGNN_EHIP(hipGetLastError());
        hipLaunchKernelGGL(heads_score_k32_kernel<KT>, grid, dim3(256), lds, st, sa);
    } else if (vec)
        hipLaunchKernelGGL((heads_score_kernel<true, KT>), grid, dim3(256), 0, st, sa);
    else
        hipLaunchKernelGGL((heads_score_kernel<false, KT>), grid, dim3(256), 0, st, sa);
    DAGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(heads_score_merge_kernel<KT>, dim3((unsigned)((rows + MT - 1) / MT)), dim3(MT), 0, st,
                       reinterpret_cast<const SPart<KT>*>(sa.spart), rows, a.tph, a.V, k, sa.y, reinterpret_cast<long long*>(tok), logit,
                       lse, nll, sums, sa.ticket);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

}  // namespace

extern "C" size_t dagnn_heads_score_bytes(int64_t B, int S, int V, int k) {
    if (!heads_shape_ok(B, S, V) || k < 1 || k > 8) return 0;
    const int64_t tph = (V + BN - 1) / BN;
    return SCORE_HEAD_BYTES + (size_t)(B > 0 ? B : 1) * S * tph * (8 * (size_t)score_kt(k) + 16);
}

extern "C" int dagnn_heads_score(const float* out, int64_t ld_out, const float* wcat, int64_t ldw, const float* bcat, int64_t B,
                                 int D, int S, int V, const int64_t* y, int k, int64_t* tok, float* logit, float* lse, float* nll,
                                 void* sums, void* work, size_t work_bytes, void* stream) {
    if (!heads_shape_ok(B, S, V) || D <= 0 || ld_out < D || ldw < D || k < 1 || k > 8) return DAGNN_EINVAL;
    if ((y != nullptr) != (nll != nullptr) || (sums && !y)) return DAGNN_EINVAL;
    if (B == 0) return DAGNN_OK;
    if (!out || !wcat || !bcat || !tok || !logit || !lse || !work || ((uintptr_t)work & 15) || ((uintptr_t)sums & 7))
        return DAGNN_EINVAL;
    if (work_bytes < dagnn_heads_score_bytes(B, S, V, k)) return DAGNN_ENOSPC;
    ScoreArgs sa;
    HeadsArgs& a = sa.h;
    a.out = out; a.wcat = wcat; a.bcat = bcat; a.part = nullptr;
    a.M = B; a.ld_out = ld_out; a.ldw = ldw; a.D = D; a.S = S; a.V = V;
    a.tph = (V + BN - 1) / BN;
    const int64_t tiles_m = (B + BM - 1) / BM;
    if (tiles_m * S * a.tph >= (int64_t(1) << 31)) return DAGNN_EINVAL;
    a.tiles_m = (int)tiles_m;
    sa.y = reinterpret_cast<const long long*>(y);
    sa.ticket = reinterpret_cast<unsigned*>(work);
    sa.spart = reinterpret_cast<char*>(work) + SCORE_HEAD_BYTES;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = ld_out % 4 == 0 && ldw % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)wcat & 15) == 0;
    double* sm = reinterpret_cast<double*>(sums);
    switch (score_kt(k)) {
        case 1: return launch_score<1>(sa, vec, B * S, k, tok, logit, lse, nll, sm, st);
        case 2: return launch_score<2>(sa, vec, B * S, k, tok, logit, lse, nll, sm, st);
        case 4: return launch_score<4>(sa, vec, B * S, k, tok, logit, lse, nll, sm, st);
        default: return launch_score<8>(sa, vec, B * S, k, tok, logit, lse, nll, sm, st);
    }
}

extern "C" int dagnn_rows_argmax(const float* logits, int64_t ld, int64_t B, int S, int V, int64_t* tok, void* stream) {
    if (!heads_shape_ok(B, S, V) || ld < (int64_t)S * V) return DAGNN_EINVAL;
    if (B == 0) return DAGNN_OK;
    if (!logits || !tok || ((uintptr_t)logits & 3)) return DAGNN_EINVAL;
    hipLaunchKernelGGL(rows_argmax_kernel, dim3((unsigned)(B * S)), dim3(256), 0, (hipStream_t)stream, logits, ld, S, V,
                       reinterpret_cast<long long*>(tok));
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

extern "C" int dagnn_seq_f1_counts(const int64_t* tok, int64_t B, int S, int64_t eos_id, const int32_t* ref_ids, int R,
                                   const int32_t* ref_extra, int32_t* counts, void* stream) {
    if (B < 0 || S <= 0 || R <= 0 || B >= (int64_t(1) << 31)) return DAGNN_EINVAL;
    if (B == 0) return DAGNN_OK;
    if (!tok || !ref_ids || !counts || ((uintptr_t)counts & 15)) return DAGNN_EINVAL;
    hipLaunchKernelGGL(seq_f1_counts_kernel, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(tok), B, S, (long long)eos_id, ref_ids, R, ref_extra, counts);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}
