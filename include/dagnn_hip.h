/*
 * dagnn_hip.h - C ABI of the MI355X (gfx950) DAGNN message-passing library (libdagnn_hip.so).
 *
 * The reference (vthost/DAGNN) is pure Python on PyTorch/PyG and has no FFI of its own; the
 * drop-in boundary it exposes is the nn.Module `DAGNN.forward(G)`
 * (ogbg-code/model/dagnn.py:128-215; dvae/dagnn.py:99-184; dvae/dagnn_bn.py:98-177).  The
 * Python mirror of that module lives in dagnn_amd/{model,dvae}.py; every device-side step it
 * takes goes through the entry points declared here, each of which replaces the reference lines
 * cited next to it.  INTEGRATION.md shows the ctypes binding a maintainer of the reference
 * would add.
 *
 * Conventions (all entry points):
 *   - every pointer is a BORROWED DEVICE pointer (e.g. torch.Tensor.data_ptr()) unless marked
 *     "host"; the library never allocates, frees or synchronises, so calls are stream-ordered
 *     and hipGraph-capturable (one caveat: a replayed graph repeats the `epoch` it was captured with, so a graph
 *     that contains dagnn_frontier_run / dagnn_backward_run with granule buffers must also contain the memset that
 *     re-zeroes those buffers - see dagnn_frontier_cell.granules);
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - return value: 0 on success, DAGNN_E* (<0) on bad arguments, -(1000+hipError_t) when a HIP
 *     call fails; nothing throws across the boundary;
 *   - no global mutable state: k threads / k ranks may call concurrently on different devices
 *     (ogbg-code/tg/data_parallel.py:59-62 runs one Python thread per device);
 *   - floats are IEEE fp32; hidden size H must be a multiple of 4 (the host pads otherwise).
 */
#ifndef DAGNN_HIP_H
#define DAGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAGNN_OK 0
#define DAGNN_EINVAL (-22)     /* bad argument (null pointer, H % 4 != 0, negative size ...) */
#define DAGNN_ENOSPC (-28)     /* workspace too small */
#define DAGNN_EHIP(e) (-(1000 + (int)(e)))

#define DAGNN_MAX_DIRS 2
#define DAGNN_MAX_GROUPS 4

/* Library / ABI version string, e.g. "dagnn_hip 0.1 gfx950". Host pointer, static storage. */
const char* dagnn_version(void);

/* ------------------------------------------------------------------------------------------
 * Plan: the layer-sorted, per-graph CSR the recurrence walks.
 * Replaces, per forward call, the reference's frontier selection (dagnn.py:146-147), its
 * per-node scan of the whole edge_index (dagnn.py:151-157) and the output-node selection
 * (dagnn.py:119-126).  Consumes the layer ids that src/utils_dag.py:39-52 attaches offline.
 * ---------------------------------------------------------------------------------------- */

/* Host-side descriptor of a plan: a device workspace plus the sizes it was laid out for. */
typedef struct dagnn_plan {
    void* data;          /* device workspace, >= dagnn_plan_bytes(N, E, B, num_edge_feats) bytes */
    size_t bytes;
    int64_t N, E, B;     /* nodes, edges, graphs in the batch */
    int num_edge_feats;  /* floats of edge_attr per edge carried into the plan (0 = none) */
    int flags;           /* 0, or DAGNN_PLAN_GENERAL_BUILD */
} dagnn_plan;

/* Batches of up to 2048 nodes, 4096 edges and 512 graphs (the D-VAE batches of dvae/dagnn.py:99-175) have their plan and
 * their dataflow schedule built by ONE workgroup each instead of 7 + 6 launches - the same words either way.  This flag
 * keeps a plan on the general kernels whatever its size (tests compare the two). */
#define DAGNN_PLAN_GENERAL_BUILD 1
/* 1 when dagnn_plan_build takes the one-workgroup path for these sizes (dagnn_dataflow_schedule: E does not matter, pass 0) */
int dagnn_plan_is_small(int64_t N, int64_t E, int64_t B);

/* Bytes of device workspace `dagnn_plan_build` needs for N nodes, E edges, B graphs and
 * `num_edge_feats` floats of edge_attr per edge (0 if the model has no edge features). */
size_t dagnn_plan_bytes(int64_t N, int64_t E, int64_t B, int num_edge_feats);

/* Build the plan for both directions.
 *   edge_index [2,E] int64 row-major: row 0 = source, row 1 = target (PyG layout)
 *   layer_fwd  [N] int64: longest-path layer of each node        (G._bi_layer_idx0)
 *   layer_bwd  [N] int64: same on the reversed graph             (G._bi_layer_idx1)
 *   batch      [N] int64: graph id of each node, non-decreasing  (G.batch)
 *   edge_attr  [E,num_edge_feats] fp32 or NULL
 * Edges must be grouped by graph in the same order as nodes (what PyG collation produces).
 * `status` [4] int32 device words, written by the kernels: status[0] != 0 flags a contract
 * violation (bit 0: edges not grouped by graph, bit 1: edge crosses graphs, bit 2: batch not
 * sorted, bit 3: layer id >= nodes of its graph).  The caller clears status[0] before the call (the
 * kernels OR into it); a batch for which dagnn_plan_is_small() holds has it written, cleared or not.
 * Read it back only when debugging: the forward path itself never synchronises. */
int dagnn_plan_build(const dagnn_plan* plan /* host */,
                     const int64_t* edge_index, const int64_t* layer_fwd, const int64_t* layer_bwd,
                     const int64_t* batch, const float* edge_attr, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * AST node encoder (ogbg-code/utils.py:26-28, called at dagnn.py:139):
 *   out[v,:] = type_emb[x[v,0]] + attr_emb[x[v,1]] + depth_emb[min(depth[v], max_depth)]
 * and clamps depth[v] IN PLACE to max_depth, as the reference does (utils.py:27).
 *   x [N,2] int64, depth [N] int64, tables [*,H] fp32, out [N,ld_out] fp32 (ld_out >= H).
 * depth_emb == NULL is the two-table encoder of the LP task (ogbg-code/utils2.py:26-28): out = type + attr, one fp32
 * add; depth is clamped all the same (utils2.py:27).
 * ---------------------------------------------------------------------------------------- */
int dagnn_encode_ast(const int64_t* x, int64_t* depth, const float* type_emb, const float* attr_emb,
                     const float* depth_emb, int max_depth, float* out, int ld_out,
                     int64_t N, int H, void* stream);

/* ------------------------------------------------------------------------------------------
 * Everything in front of the recurrence as ONE fused pipeline of 7 launches (instead of 13 + the encoder's): the plan
 * (dagnn_plan_build: dagnn.py:146-157), the dataflow schedule (dagnn_dataflow_schedule, groups > 0) and - riding on the
 * plan's longest kernel, which is latency-bound - the HBM-bound row work of forward() that does not depend on the plan:
 * the node encoder (utils.py:26-28, dagnn.py:139), up to three table sets at once (the embedding itself and, for an
 * evaluation pass, the tables folded through W_ih of stacked layer 0 of every direction: gi0 = (T W_ih^T)[type] +
 * (A W_ih^T)[attr] + (D W_ih^T + b_ih)[depth]), and side effect 1 (dagnn.py:130-133: four [N] index arrays stacked).
 * Launches: pointers | per-graph sorts + rows | batch-level layers + work items + LPT assignment + workspace fill |
 * first slots + group-layer counts | row records (+ seal) + group prefixes | group-layer bases | schedule records.
 * Same plan / schedule words as the separate calls (tests compare them); small batches (dagnn_plan_is_small) and empty
 * ones take the separate calls internally.
 * ---------------------------------------------------------------------------------------- */
#define DAGNN_PREPARE_MAX_TABLES 3
typedef struct dagnn_prepare_rows {
    const int64_t* x;            /* [N,2] (type, attribute) indices; NULL: no encoder rows */
    int64_t* depth;              /* [N], clamped IN PLACE to max_depth (utils.py:27) */
    int max_depth;
    int num_tables;              /* 1..DAGNN_PREPARE_MAX_TABLES */
    struct {
        const float *type_emb, *attr_emb, *depth_emb;   /* [*, width] each; depth_emb NULL: type + attr rows (utils2.py:28) */
        float* out;                                     /* [N, ld_out]: (type + attr) + depth rows */
        int width, ld_out;                              /* multiples of 4 */
    } table[DAGNN_PREPARE_MAX_TABLES];
    const int64_t* stack_src[4]; /* four [N] arrays ... */
    int64_t* stack_out;          /* ... copied to [4, N]; NULL: none */
} dagnn_prepare_rows;

int dagnn_prepare(const dagnn_plan* plan, const int64_t* edge_index, const int64_t* layer_fwd, const int64_t* layer_bwd,
                  const int64_t* batch, const float* edge_attr, int32_t* status,
                  void* schedule, size_t schedule_bytes, int groups, int cost_layer, int cost_row,   /* groups = 0: no schedule */
                  const dagnn_prepare_rows* rows /* or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input-side GRU GEMMs, batched over all nodes (the W_i* x + b_i* half of nn.GRUCell,
 * dagnn.py:181; independent of the recurrence, so done once per layer on the MFMA units):
 *   for g < num_groups:  C_g[M,Nc] = A_g[M,K] * W_g[Nc,K]^T + bias_g[Nc]
 * A row-major with leading dim lda, W row-major (torch weight layout) with leading dim ldw,
 * C row-major with leading dim ldc.  fp32 in, fp32 MFMA accumulate (bit-equal to an fmaf chain).
 * ---------------------------------------------------------------------------------------- */
typedef struct dagnn_gemm_group {
    const float* A;
    const float* W;
    const float* bias; /* may be NULL */
    float* C;
} dagnn_gemm_group;

int dagnn_gemm_nt_bias(const dagnn_gemm_group* groups /* host array */, int num_groups,
                       int64_t M, int Nc, int K, int lda, int ldw, int ldc, void* stream);

/* ------------------------------------------------------------------------------------------
 * Recurrent weights are consumed k-major: Wt[k, c] = W_hh[c, k]  ([H, 3H] from torch's [3H, H]).
 * ---------------------------------------------------------------------------------------- */
int dagnn_pack_whh(const float* w_hh /* [3H,H] */, float* w_hh_t /* [H,3H] */, int H, void* stream);

/* ------------------------------------------------------------------------------------------
 * One stacked GRU layer of the recurrence, all topological layers, for the directions in
 * `dir_mask` (bit d).  One workgroup walks one (graph, direction): for every topological layer
 * t of that graph and every frontier node v
 *     a_v  = sum_e softmax_e( score[u_e] + gain . edge_attr_e ) * h[u_e]     (t > 0, else 0)
 *     h[v] = GRU gates( gi[v], W_hh a_v + b_hh, a_v )
 *     score[v] = w_key . h[v] (+ vid_bias[v mod vid_mod])
 * Replaces AttnConv.forward/message + PyG propagate/softmax/scatter (dagnn.py:362-373), the
 * hidden half of nn.GRUCell (dagnn.py:181) and the state write (dagnn.py:182); the query half
 * of attn_lin and its bias cancel inside the segment softmax.
 * The dvae NA variant's `vids` one-hot on the keys (dvae/dagnn.py:130-139) is the vid_bias term.
 *
 * Per direction d (arrays indexed by d; entries for directions not in dir_mask are ignored):
 *   gi[d]       [N,3H]  W_ih u + b_ih for every node (from dagnn_gemm_nt_bias)
 *   w_hh_t[d]   [H,3H]  packed by dagnn_pack_whh
 *   b_hh[d]     [3H]
 *   w_key[d]    [H]     key half of attn_lin.weight (last H entries; dagnn.py:359,370)
 *   edge_gain[d][num_edge_feats]  = W_e^T w_key (edge_encoder folded onto the key vector), or NULL
 *   vid_bias[d] [vid_mod] or NULL
 *   h[d]        [N,ld_h] out: this layer's hidden states (rows are written exactly once)
 *   score[d]    [N]     scratch
 * ---------------------------------------------------------------------------------------- */
typedef struct dagnn_layer_args {
    const float* gi[DAGNN_MAX_DIRS];
    const float* w_hh_t[DAGNN_MAX_DIRS];
    const float* b_hh[DAGNN_MAX_DIRS];
    const float* w_key[DAGNN_MAX_DIRS];
    const float* edge_gain[DAGNN_MAX_DIRS];
    const float* vid_bias[DAGNN_MAX_DIRS];
    float* h[DAGNN_MAX_DIRS];
    float* score[DAGNN_MAX_DIRS];
    int vid_mod;
    int ld_h;
    int static_score;   /* 1: score[d] is an INPUT (w_key . x_v for the `*_x` aggregators whose keys are the node
                         * inputs, dagnn.py:175-177) and is not rewritten; w_key may then be NULL */
    void* debug_timing; /* NULL, or 8 uint64 device words: per-phase 100 MHz ticks of the deepest work item */
} dagnn_layer_args;

int dagnn_recurrence_layer(const dagnn_plan* plan /* host */, const dagnn_layer_args* args /* host */, int dir_mask,
                           int H, void* stream);

/* ------------------------------------------------------------------------------------------
 * Lock-step schedule of the same recurrence (the default path): one launch per batch-level
 * topological layer covering every (direction, stacked layer) cell; stacked layer i runs one
 * launch behind layer i-1, so the whole loop nest of dagnn.py:144-182 becomes T + L - 1 dependent
 * launches.  Each workgroup owns a 32-unit slice of one cell's GRU weights for a block of <= 8
 * frontier rows (see dagnn_amd/csrc/frontier.hip).  Requires H % 64 == 0 (the host pads).
 *
 * Weights are consumed in slice/lane order: pack W [3H, K] (torch layout) with dagnn_pack_slices for
 * both slice widths the launches use (16 hidden units for thin launches, 32 for fat ones); K = H for
 * weight_hh and for weight_ih of stacked layers > 0.  H % 32 == 0, K % 64 == 0.
 *
 * State rows carry their attention scores: h_out is [N, ld_h] with ld_h >= H + H/16 (multiple of 4);
 * floats [H, H + H/16) of row v are the partial dots w_key[16q:16q+16] . h[v, 16q:16q+16], written
 * by the producing workgroups and summed in index order by the consumers (deterministic).
 * ---------------------------------------------------------------------------------------- */
int dagnn_pack_slices(const float* w /* [3H,K] */, float* out /* 3H*K floats */, int H, int K, int slice_units,
                      void* stream);

/* W [3H,K] -> B-fragment order of v_mfma_f32_16x16x4_f32 for 32-unit slices (six 16-column blocks per slice, 16 k per
 * 1-KiB wave load; 3H*K floats out; K % 16 == 0); used by the 64-row tiles of the fat launches (csrc/fat.hip). */
int dagnn_pack_mfma(const float* w /* [3H,K] */, float* out, int H, int K, void* stream);

/* Both slice layouts and the MFMA layout of several matrices in ONE launch (a training step re-packs every cell's
 * weights: 18 launches at L = 2 otherwise).  Outputs that are NULL are skipped. */
#define DAGNN_MAX_PACK_JOBS 16
typedef struct dagnn_pack_job {
    const float* w;      /* [3H,K] torch layout */
    float* out_slices16; /* 3H*K floats each, as dagnn_pack_slices(.., 16) / (.., 32) / dagnn_pack_mfma would write them */
    float* out_slices32;
    float* out_mfma;
    int32_t H, K;
} dagnn_pack_job;
int dagnn_pack_batch(const dagnn_pack_job* jobs /* host */, int num_jobs, void* stream);

typedef struct dagnn_frontier_cell {
    const float* w_hh_pk16; /* weight_hh packed for 16-unit slices */
    const float* w_hh_pk32; /* ... and for 32-unit slices */
    const float* w_ih_pk16; /* weight_ih (stacked layers > 0), else NULL */
    const float* w_ih_pk32;
    const float* w_hh_mfma; /* weight_hh in MFMA fragment order (dagnn_pack_mfma), or NULL: no MFMA tiles */
    const float* w_ih_mfma; /* weight_ih likewise (stacked layers > 0) */
    const float* b_hh;      /* [3H] */
    const float* b_ih;      /* [3H] (stacked layers > 0; layer 0 has it folded into gi0) */
    const float* w_key;     /* [H] key half of attn_lin.weight (NULL when static_score is given) */
    const float* static_score; /* NULL, or [N]: attention score of every node when the keys are the node inputs
                             * (`attn_x`, `self_attn_x`: w_key . x_v, constant over the recurrence) */
    const float* edge_gain; /* [num_edge_feats] or NULL */
    const float* vid_bias;  /* [vid_mod] or NULL */
    const float* gi0;       /* [N,3H] W_ih x + b_ih (stacked layer 0 only), from dagnn_gemm_nt_bias */
    float* h_out;           /* [N,ld_h] hidden states + partial scores (every row written exactly once) */
    void* granules;         /* NULL, or uint64 [N, H + H/16]: tagged copies {epoch, fp32 bits} of the same row,
                             * the hand-off format of the persistent tail kernel.  The buffer must have been
                             * zero-initialised once and only ever used with strictly increasing epochs. */
} dagnn_frontier_cell;

#define DAGNN_MAX_STACKED 8
typedef struct dagnn_frontier_args {
    dagnn_frontier_cell cell[DAGNN_MAX_DIRS][DAGNN_MAX_STACKED];
    int num_stacked; /* L */
    int dir_mask;
    int H, ld_h, vid_mod;
    int num_cus;     /* compute units of the device (launch geometry heuristic), e.g. 256 */
    int rb4_max_wgs; /* streamed 32-unit slices: launches of up to this many 4-row-block workgroups use 4-row blocks,
                      * bigger ones 8-row blocks; 0 = default (1.5 per CU) */
    int mfma_min_rows;    /* launches with at least this many rows (all cells of both directions; a one-direction chain takes its
                           * share) run as 64-row MFMA tiles with the gather fused (csrc/fat.hip); 0 = never */
    void* agg_scratch;    /* NULL, or fp32 [agg_scratch_rows, H]: scratch rows for the aggregates of rows with more than two
                           * predecessors (the fat launches build them in their prologue; nothing else goes through memory) */
    int agg_scratch_rows; /* >= (largest number of rows of direction 0's cells in one launch) + (the same for direction 1): the two
                           * directions' launches may run concurrently (below) and keep their scratch rows apart */
    /* persistent tail: one dataflow launch for all layers after the fat head (needs every cell's
     * `granules`, epoch != 0 and H <= 256): */
    int tail_replicas;   /* workgroups per (cell, slice) in the tail kernel; 0 disables it */
    int tail_slice_units; /* 16 or 32 hidden units per tail workgroup (32 if anything else) */
    int tail_max_blocks; /* a layer may have up to 4 * tail_replicas * tail_max_blocks rows per cell in the tail */
    unsigned epoch;      /* tag of this forward pass in the granule buffers: nonzero, larger than any used before */
    void* tail_err;      /* device int32: set to 1 if a bounded wait in the tail kernel ever expires */
    void* debug_timing; /* NULL, or (T+L-1)*8 uint64 device words: 100 MHz stamps of workgroup 0 per launch */
    /* split mode (optional): with a second stream and the plan's per-layer split pointers (blsplit_d, read back with
     * the schedule) the persistent kernel walks the DEEP graphs (depth > thr_d) from layer 0 on `side_stream`,
     * concurrently with the per-layer launches, which then only cover the shallow graphs.  The call forks from and
     * joins back into `stream` with the caller's `fork_event` / `join_event` (capturable); results agree with the unsplit mode to rounding (a row may be
     * handled by a different kernel), each mode by itself is deterministic.  (CU-masked streams for the two
     * halves were measured and dropped: masked queues slowed every other launch of the process.) */
    void* side_stream;                              /* hipStream_t or NULL: runs the persistent kernel.  Without a persistent tail in
                                                     * the call (H > 256, or tail_replicas = 0) and with both directions, the same
                                                     * stream and events run direction 1's per-layer launches as a second chain next to
                                                     * direction 0's on `stream` (the directions share nothing; each chain's launches
                                                     * fill the CUs the other's leave idle while their last workgroups drain) */
    const int32_t* layer_split[DAGNN_MAX_DIRS];     /* HOST, num_layers[d] int32: first deep slot of every layer, or NULL */
    void* fork_event;                               /* hipEvent_t x 2, CALLER-OWNED (the library creates nothing): split */
    void* join_event;                               /* mode needs both, otherwise it is off */
} dagnn_frontier_args;

/* layer_ptr[d] (HOST, num_layers[d] + 1 int32): row offsets of the batch-level layers of direction
 * d, i.e. the first num_layers[d]+1 words of the plan's blptr_d array read back by the caller
 * (the one device->host read of the forward pass; the reference reads T back at dagnn.py:137). */
int dagnn_frontier_run(const dagnn_plan* plan /* host */, const dagnn_frontier_args* args /* host */,
                       const int32_t* const* layer_ptr /* host */, const int32_t* num_layers /* host [2] */,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Dataflow schedule of the same recurrence (the default path for H <= 256): ONE persistent launch for the whole loop
 * nest of dagnn.py:144-182, cut along graphs instead of layers (dagnn_amd/csrc/dataflow.hip).
 *
 *   1. dagnn_dataflow_groups: how many independent groups G the device hosts.  A workgroup SET has one workgroup
 *      (one CU) per (kernel cell, 32-unit slice); the kernel cells of a direction are its L GRU cells plus, for every
 *      stacked layer above the first, one PROJECTION cell (the input-side product W_ih u + b_ih, which leaves the
 *      dependent chain that way).  A set serves TWO groups (their blocks interleave: one group's dependent hop hides
 *      behind the other's work): G = 2 * floor(num_cus / (num_dirs * (2L - 1) * H/32)), capped at 64 and at B;
 *      0 = this shape is not supported (H > 256, H % 64 != 0, more than 16 kernel cells, or one set does not fit the
 *      device) - use dagnn_frontier_run.  Any 1 <= G <= 64 is valid for the calls below (ceil(G / 2) sets launch).
 *   2. dagnn_dataflow_schedule: deals the graphs of a plan to the G groups - longest-processing-time first on
 *      cost_layer * depth + cost_row * nodes, integer arithmetic, ties to the lowest group - and re-sorts the plan's
 *      64-byte row records by (group, topological layer, graph, node), every group-layer padded to whole blocks of 4
 *      records (padding records: node = -1).  The result depends on the plan and on (G, costs) only: build it once per
 *      batch (it also serves the backward pass).  Workspace: dagnn_dataflow_bytes(N, B, G), any contents; the record
 *      arrays are defined over the records the groups use (first record .. first record + 4 * blocks of every group).
 *   3. dagnn_dataflow_run: the launch.  Every (direction, stacked layer) cell needs `granules`: uint64 [N, gld]
 *      (gld >= H) tagged copies {epoch, fp32 bits} of its state rows - the hand-off format between workgroups.  The
 *      buffers must have been zero-initialised once and only ever used with strictly increasing `epoch`s (a replayed
 *      hipGraph must contain the memset).  `err` (device int32, zeroed by the caller) is set when a bounded wait
 *      expires (results are then invalid): bit 0 a granule poll, bit 1 an LDS flag; bit 2: the plan's status word
 *      (`plan_status`) was nonzero, nothing was computed - bits 8-15 then carry that status word; bit 3: `schedule` does not carry the header of a schedule
 *      built for `groups` groups (dagnn_dataflow_schedule), nothing was computed.
 *      State rows h_out [N, ld_h] receive the H states only; dagnn_score_parts adds the H/16 partial attention scores
 *      behind them (the format dagnn_backward_prepare reads) when a backward pass follows.
 * Weights: dagnn_pack_dataflow(W [3H,H] torch layout) -> 3*H*H floats in slice / lane order (the A operands of the
 * kernel's v_mfma_f32_4x4x1 products: lane = (unit quad, K slice of H/8, unit of the quad)).
 * ---------------------------------------------------------------------------------------- */
typedef struct dagnn_dataflow_cell {
    const float* w_hh;      /* weight_hh packed by dagnn_pack_dataflow */
    const float* w_ih;      /* weight_ih packed likewise (stacked layers > 0), else NULL */
    const float* b_hh;      /* [3H] */
    const float* b_ih;      /* [3H] (stacked layers > 0; layer 0 has it folded into gi0) */
    const float* w_key;     /* [H] key half of attn_lin.weight (ignored when static_score is given) */
    const float* static_score; /* NULL, or [N]: see dagnn_frontier_cell */
    const float* edge_gain; /* [num_edge_feats] or NULL */
    const float* vid_bias;  /* [vid_mod] or NULL */
    const float* gi0;       /* [N,3H] W_ih x + b_ih (stacked layer 0 only) */
    float* h_out;           /* [N,ld_h] */
    void* granules;         /* uint64 [N,gld] */
    void* proj_granules;    /* stacked layers > 0: 16-byte granules {tag, r, z, n} [N,pld] (pld >= H, 16-byte aligned), the hand-off
                             * buffer of the cell's input-side pre-activations W_ih u + b_ih, one granule per unit (same
                             * zero-init / epoch contract as `granules`); else NULL */
    float* gh_out;          /* NULL, or [N,3H]: the hidden-side pre-activations W_hh a + b_hh of every node as the gates saw them */
    float* gi_out;          /* NULL, or [N,3H] (stacked layers > 0): the input-side pre-activations as plain floats - what a
                             * training pass keeps for its reverse sweep instead of recomputing both with GEMMs */
    /* plain aggregators (AggConv `add` / `max`, ogbg-code/model/dagnn.py:232-251: messages h_j + edge_encoder(edge_attr_j)):
     * agg = DAGNN_DF_AGG_ATTN (0, the soft-max above), _ADD, _MAX, or _NONE (no message lands on these rows - the reference's one
     * shared AggConv in the reverse direction - the aggregate is zero).  agg_edge_w [H, num_edge_feats <= 2] / agg_edge_b [H]:
     * the edge encoder in torch layout, or NULL (no edge features).  H <= 256; w_key / edge_gain / static_score are ignored. */
    const float* agg_edge_w;
    const float* agg_edge_b;
    int agg;
} dagnn_dataflow_cell;
#define DAGNN_DF_AGG_ATTN 0
#define DAGNN_DF_AGG_ADD 1
#define DAGNN_DF_AGG_MAX 2
#define DAGNN_DF_AGG_NONE 3

typedef struct dagnn_dataflow_args {
    dagnn_dataflow_cell cell[DAGNN_MAX_DIRS][DAGNN_MAX_STACKED];
    int num_stacked, dir_mask;
    int H, ld_h, gld, pld, vid_mod;
    int groups;            /* G the schedule was built for */
    unsigned epoch;
    const void* schedule;  /* device workspace written by dagnn_dataflow_schedule */
    void* err;             /* device int32 */
    void* debug_timing;    /* NULL, or uint64 device words (100 MHz stamps): [workgroups][2] start / end of every
                            * workgroup, then [blocks][8] phase stamps of workgroup `debug_wg` */
    unsigned spin_limit;   /* polls before a wait gives up and raises `err`; 0 = default (1 << 22, seconds) */
    int debug_wg;          /* workgroup whose blocks are stamped (debug_timing) */
    /* XCD-aware placement (optional, a speed hint that is verified at run time): with `num_cus` (CUs of the device, one
     * workgroup per CU) and `xcc_table` (uint64 [num_cus], zero-initialised once, same epoch contract as `granules`) the
     * workgroups of a recurrent cell and of the projection cell reading its rows are given ids that the observed dispatch
     * rule (workgroup b -> XCD b % 8) puts on one XCD.  Every workgroup publishes the XCD it really runs on; a cell whose
     * readers all share its XCD hands its rows over through that XCD's L2 (plain stores) instead of write-through ones -
     * results are identical either way.  0 / NULL: linear ids, write-through stores. */
    int num_cus;
    void* xcc_table;
    const void* plan_status; /* NULL, or the device status word of dagnn_plan_build: if it is nonzero (the batch violates
                            * the layout contract) the launch walks nothing and raises bit 2 of `err` */
    int xcd_first;          /* XCD-aware placement: the XCD the packing starts with (0..7).  Launches that run next to each other
                            * (micro-batches in flight on several streams, each sized for a part of the device) pass different
                            * values, otherwise all of them pack their workgroups onto the same first XCDs and take turns */
    int stat_rows;          /* training passes whose reverse pass is dagnn_bwd_dataflow_run: nonzero = every cell's `gh_out` is that
                            * cell's static-record buffer `stat` (dagnn_bwd_dataflow_static_bytes_h; zero-filled by the caller when
                            * H is neither 256 nor 320) and the kernel writes the state and the six gate-coefficient rows of each
                            * node's record instead of the pre-activations; `gi_out` must be NULL.  The reverse pass then only
                            * adds the external-gradient row (dagnn_bwd_dataflow_args.stat_rows_written).  The records are
                            * addressed with 32-bit byte offsets: N x 4 x (8 x 256) bytes (H <= 256) or N x 4 x (8 x 320) bytes
                            * (H = 320) must stay below 2^32, otherwise the call returns DAGNN_EINVAL */
} dagnn_dataflow_args;

int dagnn_dataflow_groups(int num_cus, int num_dirs, int num_stacked, int H, int64_t B);
size_t dagnn_dataflow_bytes(int64_t N, int64_t B, int groups);
int dagnn_dataflow_schedule(const dagnn_plan* plan /* host */, void* workspace, size_t workspace_bytes, int groups,
                            int cost_layer, int cost_row, const int32_t* plan_status /* device, or NULL */, void* stream);
int dagnn_dataflow_run(const dagnn_plan* plan /* host */, const dagnn_dataflow_args* args /* host */, void* stream);
/* H = 320 (hidden sizes 257..320, zero-padded by the caller: the reference trains at emb_dim = 300, scripts/ogb_tok.sh:17): the
 * same launch, same workgroup shape, in a translation unit of its own (csrc/dataflow_w.hip).  Exactly two edge features, no static scores, no vertex-id
 * key biases (anything else: DAGNN_EINVAL - the caller keeps such models on the other paths).  dagnn_dataflow_run forwards
 * H > 256 here; dagnn_dataflow_groups / dagnn_pack_dataflow accept H = 320. */
int dagnn_dataflow_run_wide(const dagnn_plan* plan /* host */, const dagnn_dataflow_args* args /* host */, void* stream);
int dagnn_pack_dataflow(const float* w /* [3H,H] */, float* out /* 3H*H floats */, int H, void* stream);
/* the same order of the gate-wise transposed matrix W'[g H + j][u] = W[g H + u][j] (reverse sweep, dagnn_bwd_dataflow_run) */
int dagnn_pack_dataflow_transposed(const float* w /* [3H,H] */, float* out /* 3H*H floats */, int H, void* stream);
/* Both layouts of several [3H, H] matrices in ONE launch (a training step re-packs every cell's weights). */
typedef struct dagnn_df_pack_job {
    const float* w;       /* [3H, H] torch layout (mode 2: edge_encoder.weight [rows, cols]) */
    float* out;           /* 3H*H floats (mode 2: [cols]) */
    const float* aux;     /* mode 2: the key weights [rows]; else unused */
    int32_t transposed;   /* 0: as dagnn_pack_dataflow, 1: as dagnn_pack_dataflow_transposed, 2: edge gain out = w^T aux */
    int32_t rows, cols;   /* mode 2 only */
} dagnn_df_pack_job;
int dagnn_pack_dataflow_batch(const dagnn_df_pack_job* jobs /* host */, int njob, int H, void* stream);
int dagnn_score_parts(float* h /* [N,ld_h] */, int ld_h, int H, const float* w_key /* [H] */, int64_t N, void* stream);
/* ... of several cells (the same ld_h / H / N) in one launch: n <= DAGNN_MAX_PACK_JOBS host arrays of device pointers. */
int dagnn_score_parts_batch(float* const* h, const float* const* w_key, int n, int ld_h, int H, int64_t N, void* stream);
/* Introspection (tests, host-side mirror): byte offsets of the schedule workspace's arrays, 13 entries: [grp_of,
 * gdepth, gload, loff, gtab0, gtab1, lcnt0, lcnt1, glbase0, glbase1, grec0, grec1, total]. */
int dagnn_dataflow_layout(int64_t N, int64_t B, int groups, int64_t* offsets13 /* host */);

/* ------------------------------------------------------------------------------------------
 * Weight-stationary tile schedule of the same recurrence for WIDE hidden states (H = 512; dagnn_amd/csrc/tiles.hip): the
 * path of BASELINE.json's cfg 5 (batch 256, hidden 512, 5 stacked layers, bidirectional), where the GRU matrices (56.6 MB)
 * are too large to be streamed once per topological layer (dagnn_frontier_run) and the rows too many for the 4-row blocks
 * of dagnn_dataflow_run.  One persistent launch per CHUNK of stacked layers (all of them at once when 32 workgroups per cell
 * fit the device - up to 4 layers x 2 directions on 256 CUs; else chunk 0 = stacked layer 0, then as many layers at a time as fit): every workgroup keeps its 16-unit slice of one cell's
 * W_ih | W_hh (torch layouts, read once) in registers and walks the plan's batch-level layers in tiles of 16 rows
 * (v_mfma_f32_16x16x4_f32); rows are handed between workgroups by write-through stores + {epoch, tiles done} progress
 * counters.  Replaces the loop nest of dagnn.py:144-182 like the two schedules above; needs no device->host read.
 *   h_out [N, ld_h], ld_h >= H + H/16: states + the H/16 partial attention scores behind them (as dagnn_frontier_run);
 *   counters: uint64 [2 * DAGNN_MAX_STACKED * 8 * 32], zero-initialised once, only ever used with strictly increasing
 *             `epoch`s (the granule contract); err: device int32, zeroed by the caller - bit 0 / 1 a bounded wait expired,
 *             bit 2 (+ bits 8-15) the plan's status word was set and nothing was computed.
 * dagnn_tiles_launches: number of launches dagnn_tiles_run makes for this shape, 0 = shape not supported (H != 512, more
 * than 2 edge features, fewer than 32 * num_dirs CUs): use dagnn_frontier_run.  Static scores (the `*_x` aggregators)
 * are not supported either; the vertex-id key bias of the NA encoder (vid_bias / vid_mod) is.
 * ---------------------------------------------------------------------------------------- */
typedef struct dagnn_tiles_cell {
    const float* w_hh;      /* [3H,H] torch layout */
    const float* w_ih;      /* [3H,H] torch layout (stacked layers > 0), else NULL */
    const float* b_hh;      /* [3H] */
    const float* b_ih;      /* [3H] (stacked layers > 0; layer 0 has it folded into gi0) */
    const float* w_key;     /* [H] key half of attn_lin.weight */
    const float* edge_gain; /* [num_edge_feats] or NULL */
    const float* gi0;       /* [N,3H] W_ih x + b_ih (stacked layer 0 only), from dagnn_gemm_nt_bias */
    float* h_out;           /* [N,ld_h] */
    const float* vid_bias;  /* [vid_mod] or NULL: score bias by vertex id (NA variant), as in dagnn_frontier_cell */
} dagnn_tiles_cell;

typedef struct dagnn_tiles_args {
    dagnn_tiles_cell cell[DAGNN_MAX_DIRS][DAGNN_MAX_STACKED];
    int num_stacked, dir_mask;
    int H, ld_h;
    int num_cus;             /* compute units of the device: every workgroup of a launch must be resident */
    unsigned epoch;
    void* counters;
    void* err;
    unsigned spin_limit;     /* polls before a wait gives up and raises `err`; 0 = default (1 << 22) */
    const void* plan_status; /* NULL, or the device status word of dagnn_plan_build */
    int first_layer[DAGNN_MAX_DIRS]; /* per direction: walk the batch-level layers from this one on (0 = all).  The layers
                              * before it must be complete in every h_out (e.g. by dagnn_frontier_run called with num_layers =
                              * first_layer): the wide first layers on per-layer launches, the long thin tail on this kernel */
    void* debug_timing;      /* NULL, or uint64 [launches][1024][32] device words: per-workgroup phase sums in 100 MHz ticks,
                              * written by a -DT_STAMPS build only (scripts/tiles_stamps.py) */
    int vid_mod;             /* 0, or the node count per graph of the NA variant (node id % vid_mod selects vid_bias) */
} dagnn_tiles_args;

int dagnn_tiles_launches(int num_cus, int num_dirs, int num_stacked, int H, int num_edge_feats);
int dagnn_tiles_run(const dagnn_plan* plan /* host */, const dagnn_tiles_args* args /* host */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward pass of the recurrence (training: what `loss.backward()`, ogbg-code/main_pyg.py:62, does to
 * dagnn.py:144-182).  Additive attention with keys from the hidden states (`attn_h`), GRU cells.
 * The forward pass keeps only the lock-step state buffers h[d][i] ([N,ld_h], scores behind the rows).
 *
 *   1. dagnn_backward_prepare: a[c] [N,H] (attention aggregates) and alpha[c] [E] (attention weights,
 *      indexed by ORIGINAL edge id) of every cell, one parallel launch;
 *   2. caller: gh[c] = a[c] W_hh^T + b_hh and gi[c] = u W_ih^T + b_ih (dagnn_gemm_nt_bias), g_ext[c] [N,H]
 *      = gradient reaching h[c] from outside the recurrence (read-out; dagnn_readout_pool_backward_batch);
 *   3. dagnn_backward_run: T + L - 1 reverse lock-step launches.  Adds W_ih^T dgi of stacked layer i into
 *      g_ext of layer i-1 and writes, per cell: da [N,H], dgi, dgh [N,3H] (gradients of the GRU
 *      pre-activations, gate blocks r,z,n), sigma [N] (sum over a node's out-edges of the attention-logit
 *      gradients) and edge_feat_grad [N,R] (the same sum weighted by the edge features);
 *   4. caller (plain library GEMMs / reductions): dW_ih = dgi^T u, db_ih = colsum(dgi), dW_hh = dgh^T a,
 *      db_hh = colsum(dgh), dx = sum_d dgi[d][0] W_ih, d w_key = h^T sigma + W_e colsum(edge_feat_grad),
 *      dW_e = w_key (x) colsum(edge_feat_grad).  The attention query weights and biases get exact zeros
 *      (they cancel inside the segment softmax).
 * Deterministic: gradients are pulled (no atomics), sums run in a fixed order.  H % 64 == 0, H <= 1024.
 * ---------------------------------------------------------------------------------------- */
typedef struct dagnn_backward_cell {
    const float* w_hh;      /* [3H,H] torch layout (padded to H) */
    const float* w_ih;      /* [3H,H] (stacked layers > 0), else NULL */
    const float* w_key;     /* [H] */
    const float* edge_gain; /* [num_edge_feats] or NULL */
    const float* vid_bias;  /* [vid_mod] or NULL: score bias by vertex id (NA variant), as in dagnn_frontier_cell */
    const float* static_score; /* NULL, or [N]: the nodes' attention scores when the keys are the inputs (`attn_x`,
                             * `self_attn_x`); pass an all-zero w_key then (the scores do not depend on the states) */
    const float* h;         /* [N,ld_h] forward states + partial scores */
    float* a;               /* [N,H]  written by prepare, read by run */
    float* alpha;           /* [E]    written by prepare, read by run */
    const float* gi;        /* [N,3H] */
    const float* gh;        /* [N,3H] */
    float* g_ext;           /* [N,H] in; stacked layers below the top also receive the upper layer's du */
    float* da;              /* [N,H] out */
    float* dgi;             /* [N,3H] out */
    float* dgh;             /* [N,3H] out */
    float* sigma;           /* [N] out */
    float* edge_feat_grad;  /* [N,num_edge_feats] out, or NULL without edge features */
    /* persistent sweep (optional; all NULL = one launch per layer throughout): */
    void* da_granules;      /* uint64 [N,H]: tagged copies {epoch, fp32 bits} of da rows (zero-initialised once,
                             * strictly increasing epochs - the same contract as dagnn_frontier_cell.granules) */
    void* du_granules;      /* uint64 [N,H]: the upper stacked layer's du for THIS cell's rows (stacked layers below
                             * the top) */
    const float* g_ext_static; /* [N,H] copy of g_ext taken before the sweep (stacked layers below the top): inside
                             * the persistent launch a row's gradient is g_ext_static + its du granules */
} dagnn_backward_cell;

typedef struct dagnn_backward_args {
    dagnn_backward_cell cell[DAGNN_MAX_DIRS][DAGNN_MAX_STACKED];
    int num_stacked, dir_mask, H, ld_h;
    int vid_mod;    /* 0, or the node count per graph of the NA variant (node id % vid_mod selects vid_bias) */
    int num_cus;
    int thin_wgs;   /* launches of up to this many slice workgroups use the register-resident slice kernel, bigger ones
                     * the rows + MFMA-tile kernels; 0 = default (2 * num_cus) */
    /* persistent sweep over the thin head of the reverse order (needs the cells' granule buffers, H <= 256): */
    int tail_replicas;   /* workgroups per (cell, 16-unit slice); 0 disables it */
    int tail_max_blocks; /* a layer may have up to 4 * tail_replicas * tail_max_blocks rows per cell in it */
    unsigned epoch;      /* tag of this backward pass in the granule buffers: nonzero, larger than any used before */
    void* tail_err;      /* device int32: set to 1 if a bounded wait ever expires (results are then invalid) */
    /* split mode (optional): with a second stream and the plan's per-layer split pointers the sweep runs as two
     * independent chains - the shallow graphs' per-layer launches on `side_stream`, the deep graphs (persistent head,
     * then per-layer launches) on `stream`; forks from and joins back into `stream` with the caller's two events */
    void* side_stream;
    const int32_t* layer_split[DAGNN_MAX_DIRS];   /* HOST, num_layers[d] int32, or NULL */
    void* fork_event;                             /* hipEvent_t x 2, CALLER-OWNED; split mode needs both */
    void* join_event;
} dagnn_backward_args;

int dagnn_backward_prepare(const dagnn_plan* plan /* host */, const dagnn_backward_args* args /* host */, void* stream);
int dagnn_backward_run(const dagnn_plan* plan /* host */, const dagnn_backward_args* args /* host */,
                       const int32_t* const* layer_ptr /* host */, const int32_t* num_layers /* host */, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same reverse sweep as ONE persistent dataflow launch (csrc/bwd_dataflow.hip; H <= 256): the mirror image of
 * dagnn_dataflow_run on the same schedule workspace, replacing dagnn_backward_run's T + L - 1 launches.
 *   1. dagnn_backward_prepare (a, alpha) and the two pre-activation GEMMs (gi, gh) as before (no gi / gh when the forward
 *      launch wrote the static rows itself: stat_rows / stat_rows_written);
 *   2. dagnn_bwd_dataflow_prepare: successor records in schedule order (`records`, dagnn_bwd_dataflow_record_bytes: 256 bytes
 *      per record - the node, its successor row, the first four successors with their edge features and the attention weight
 *      of every stacked layer, so `alpha` of step 1 must be final) and the per-(cell, node) static rows `stat` (dagnn_bwd_dataflow_static_bytes each): Gext, h and the GRU-backward
 *      coefficients - the gate algebra is linear in the incoming gradient, so it leaves the dependent chain;
 *   3. dagnn_bwd_dataflow_run: the launch.  Hand-off buffers (uint64 granules {epoch, fp32 bits}, zero-initialised once,
 *      strictly increasing epochs): da [N,gld], q [N], dgi [N,3 gld] (stacked layers > 0), du [N,gld] (stacked layers
 *      below the top: the du arriving at THIS cell's rows).  Outputs for the weight-gradient epilogue: dgi, dgh [N,3H],
 *      sigma [N], edge_feat_grad [N,R].  `err` as for dagnn_dataflow_run.
 * Weights: dagnn_pack_dataflow_transposed(W): the forward kernel's slice / lane order of the gate-wise transposed matrix
 * W'[g H + j][u] = W[g H + u][j] (H x H blocks of the torch layout transposed in place). */
typedef struct dagnn_bwd_dataflow_cell {
    const float* w_hh_t;    /* packed gate-wise transposed W_hh */
    const float* w_ih_t;    /* ... W_ih (stacked layers > 0), else NULL */
    const float* w_key;     /* [H] (zeros when the scores are static) */
    const float* alpha;     /* [E] (dagnn_backward_prepare); read by dagnn_bwd_dataflow_prepare (into the successor records) and run */
    const float* gi;        /* prepare: [N,3H] */
    const float* gh;        /* prepare: [N,3H] */
    const float* a;         /* prepare: [N,H] */
    const float* b_hh;      /* prepare: [3H] */
    const float* h;         /* prepare: [N,ld_h] forward states */
    const float* g_ext;     /* prepare: [N,ld_g] gradient reaching h from outside the recurrence */
    float* stat;            /* [N, 8 * 256] static rows: written by prepare (or, all but the g_ext row, by the forward launch:
                             * stat_rows_written), read by run */
    void* da_granules;      /* uint64 [N,gld] */
    void* q_granules;       /* uint64 [N] */
    void* dgi_granules;     /* uint64 [N,3 gld] (stacked layers > 0) */
    void* du_granules;      /* uint64 [N,gld] (stacked layers below the top) */
    float* dgi;             /* out [N,3H] */
    float* dgh;             /* out [N,3H] */
    float* sigma;           /* out [N] */
    float* edge_feat_grad;  /* out [N,R] or NULL */
} dagnn_bwd_dataflow_cell;

typedef struct dagnn_bwd_dataflow_args {
    dagnn_bwd_dataflow_cell cell[DAGNN_MAX_DIRS][DAGNN_MAX_STACKED];
    int num_stacked, dir_mask, H, ld_h, ld_g, gld, groups;
    unsigned epoch, spin_limit;
    const void* schedule;     /* dagnn_dataflow_schedule workspace for `groups` groups */
    void* records;            /* dagnn_bwd_dataflow_record_bytes(N) */
    void* err;                /* device int32 */
    const void* plan_status;  /* or NULL */
    int num_cus;              /* XCD-aware placement, as in dagnn_dataflow_args (0 / NULL: off) */
    void* xcc_table;
    int xcd_first;            /* as in dagnn_dataflow_args */
    int stat_rows_written;    /* nonzero: the forward launch of this step wrote rows 1..7 of every `stat` record
                               * (dagnn_dataflow_args.stat_rows); prepare only scatters g_ext into row 0 and gi / gh / a / b_hh / h
                               * of the cells are not read */
    int pull_rows;            /* nonzero (agg = max of the constructor-string variants; H <= 256, not the wide entry): every cell's
                               * `alpha` is [E, DAGNN_PULL_ROW] - per original edge id a row of per-unit pull weights in the loaders'
                               * lane order (dagnn_plain_max_weights; all zeros for a cell that pulls nothing) - instead of one
                               * scalar per edge; `w_key` must be zeros, and sigma / edge_feat_grad come out as zeros */
} dagnn_bwd_dataflow_args;

size_t dagnn_bwd_dataflow_record_bytes(int64_t N);
size_t dagnn_bwd_dataflow_static_bytes(int64_t N);
size_t dagnn_bwd_dataflow_static_bytes_h(int64_t N, int H);   /* ... for a given H: 8 KB per (cell, node) up to H = 256, 10 KB at H = 320 */
int dagnn_bwd_dataflow_prepare(const dagnn_plan* plan /* host */, const dagnn_bwd_dataflow_args* args /* host */, void* stream);
int dagnn_bwd_dataflow_run(const dagnn_plan* plan /* host */, const dagnn_bwd_dataflow_args* args /* host */, void* stream);
/* H = 320: the same sweep with five column blocks per lane (csrc/bwd_dataflow_w.hip; 12 waves like H <= 256); dagnn_bwd_dataflow_run forwards H > 256 here */
int dagnn_bwd_dataflow_run_wide(const dagnn_plan* plan /* host */, const dagnn_bwd_dataflow_args* args /* host */, void* stream);

/* agg = add / max (AggConv, GRU cells) on the sweep above (csrc/variants_bwd.hip).  `add` is the sweep as it is with
 * alpha = 1 per edge (0 for a cell whose direction aggregates nothing) and w_key = 0; `max` is `pull_rows`.
 *   dagnn_plain_max_weights  before the sweep: weights[e, :] of every in-edge e of the rows in [row_begin, row_end) (row slots
 *      of direction `dir`, as for dagnn_variant_max_prepare): 0 where the message h_j + edge term of e is not the stored maximum
 *      a_w[k], else 1 / c with c the number of messages of (w, k) that are - the tie rule of dagnn_variant_max_prepare.
 *      `weights` is [E, DAGNN_PULL_ROW], zero-filled by the caller; column k of a row sits at 4 (k % 64) + k / 64.
 *   dagnn_plain_edge_grads   behind the sweep: esum[w, r, :] = sum over the in-edges e of w of weight_e (.) da_w f_e[r] (r < R)
 *      and esum[w, R, :] = sum_e weight_e (.) da_w, in CSR order (`weights` NULL: add, weight 1); da_w from the sweep's
 *      `da_granules` of this pass.  `esum` is [N, (R + 1) * H], zero-filled by the caller; its column sums are the gradients
 *      of edge_encoder.weight[:, r] and edge_encoder.bias.  No atomics: the same bits on every run.
 * Limits: H <= DAGNN_PULL_ROW, at most two edge features, ld_h / ld_a / gld >= H; violations return DAGNN_EINVAL before any launch. */
#define DAGNN_PULL_ROW 256
typedef struct dagnn_plain_pull {
    const float* h;            /* max_weights: [N, ld_h] forward states */
    const float* a;            /* max_weights: [N, ld_a] aggregates (dagnn_variant_aggregate of the same states) */
    const float* edge_mat;     /* [H, R] edge_encoder.weight, or NULL (no edge encoder) */
    const float* edge_vec;     /* [H] edge_encoder.bias, or NULL */
    float* weights;            /* [E, DAGNN_PULL_ROW]; edge_grads: NULL = add */
    const void* da_granules;   /* edge_grads: uint64 [N, gld] */
    float* esum;               /* edge_grads: out [N, (R + 1) * H] */
    int ld_h, ld_a, gld;
} dagnn_plain_pull;
int dagnn_plain_max_weights(const dagnn_plan* plan /* host */, const dagnn_plain_pull* c /* host */, int dir, int H,
                            int32_t row_begin, int32_t row_end, void* stream);
int dagnn_plain_edge_grads(const dagnn_plan* plan /* host */, const dagnn_plain_pull* c /* host */, int dir, int H,
                           int32_t row_begin, int32_t row_end, void* stream);

/* ------------------------------------------------------------------------------------------
 * Parameter gradients of the GRU cells from the sweep's outputs (csrc/wgrad.hip): for every job
 *     d_weight [3H, in_dim] = dg[:, real rows]^T in,      d_bias [3H] = column sums of dg          (both overwritten)
 * with dg [N, ld_dg] = dgi or dgh (three gate blocks of Hp columns, Hp >= H: padding units are dropped) and `in` [N, ld_in]
 * the product's input (u for W_ih, the aggregate a for W_hh).  The reduction over the nodes is split `splits` ways
 * (dagnn_wgrad_splits) into partial tiles in `workspace` (dagnn_wgrad_workspace_bytes) that a second kernel adds in
 * split order: deterministic, no atomics.  Replaces what autograd accumulates per `nn.GRUCell` call (dagnn.py:181). */
typedef struct dagnn_wgrad_job {
    const float* dg;     /* [N, ld_dg] */
    const float* in;     /* [N, ld_in] */
    float* d_weight;     /* [3H, in_dim] */
    float* d_bias;       /* [3H] or NULL */
    int ld_dg, ld_in, in_dim;   /* in_dim even; ld_dg % 4 == 0, ld_in % 2 == 0, rows 8-byte aligned */
} dagnn_wgrad_job;
/* Weighted column sums for the rest of the epilogue: out[k] = sum_n weight[n] x[n][k] (weight NULL: plain column sums) -
 * the attention-key gradients sum_v sigma_v keys_v, the edge-feature sums, sum_v sigma_v.  Rows are summed in a fixed
 * chunk order (deterministic). */
typedef struct dagnn_colsum_job {
    const float* x;        /* [N, ld_x] */
    const float* weight;   /* [N] or NULL */
    float* out;            /* [cols] */
    int ld_x, cols;
} dagnn_colsum_job;
size_t dagnn_colsum_workspace_bytes(int njob, int max_cols);
int dagnn_colsum_run(const dagnn_colsum_job* jobs /* host */, int njob, int64_t N, void* workspace, size_t workspace_bytes,
                     void* stream);
size_t dagnn_wgrad_workspace_bytes(int njob, int Hp, int max_in_dim, int splits);
int dagnn_wgrad_splits(int num_cus, int njob, int Hp, int max_in_dim, int64_t N);
int dagnn_wgrad_run(const dagnn_wgrad_job* jobs /* host */, int njob, int64_t N, int Hp, int H, int splits, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Embedding-table gradients with ONE summation order (csrc/table_grads.hip): what autograd accumulates behind the three
 * `nn.Embedding` lookups of ogbg-code/utils.py:26-28 (two for utils2.py:26-28), out_t[r] = sum of g[v] over the nodes v whose
 * key in table t is r, without a floating-point atomic.
 *
 * The order.  For a row r, list the nodes with key r in ascending v and cut the list into chunks of
 * DAGNN_TABLE_GRADS_CHUNK consecutive members BY POSITION IN THE LIST (the last chunk may be short):
 *     chunk partial  p_c    = ((g[v0] + g[v1]) + g[v2]) + ...      left to right from the chunk's first member,
 *     out[r]                = ((+0.0 + p_0) + p_1) + ...           left to right over the row's chunks,
 * plain IEEE fp32 adds, never reassociated, independent of grid and device; a row without members is exactly +0.0.  Keys
 * outside [0, R) contribute nothing and are never used as an index.  With n members and m = ceil(n / 32) chunks a term
 * passes at most k = min(n, 32) - 1 + max(m - 1, 0) rounding adds: |out - exact| <= k u / (1 - k u) sum |g|, u = 2^-24.
 * `autograd.table_grads_host` restates the order in numpy; the kernels' bits equal its bits.
 *
 *   g    [N, ld_g] fp32, ld_g >= H, 16-byte aligned rows (ld_g % 4 == 0); H % 4 == 0; 0 <= N < 2^24
 *   per table (1..DAGNN_TABLE_GRADS_MAX_TABLES): keys[v * key_stride] int64 (the two columns of one [N, 2] tensor have
 *        stride 2), 1 <= R < 2^24, out [R, ld_out] (ld_out >= H, ld_out % 4 == 0, 16-byte aligned).  `out` may arrive
 *        uninitialised: all R rows of columns [0, H) are written (zero rows too, there is no fill), columns [H, ld_out)
 *        are never touched.
 *   workspace: dagnn_table_grads_workspace_bytes(N, H, rows, num_tables) bytes, 16-byte aligned, any contents.
 * Six launches for all tables together: key counts per (node range, key) | their prefix over the ranges | segment
 * offsets | stable placement of the member lists + chunk records | chunk partials (rows of one chunk go straight to
 * `out`) | rows of several chunks and empty rows.  Integer atomics only.  N == 0: one launch that writes the zeros.
 * DAGNN_EINVAL: a NULL pointer (g / keys / workspace only when N > 0), H % 4 != 0, a pitch below H or not a multiple of
 * 4, a misaligned g / out, N >= 2^24, R < 1 or R >= 2^24, num_tables out of range; DAGNN_ENOSPC: workspace too small.
 * Borrowed pointers, the caller's stream, no allocation, no synchronisation, no host read-back.
 * ---------------------------------------------------------------------------------------- */
#define DAGNN_TABLE_GRADS_MAX_TABLES 3
#define DAGNN_TABLE_GRADS_CHUNK 32
typedef struct dagnn_table_grads_table {
    const int64_t* keys;     /* key of node v at keys[v * key_stride] */
    int64_t key_stride;      /* in elements, >= 0 */
    int64_t R;               /* rows of the table */
    float* out;              /* [R, ld_out] */
    int64_t ld_out;
} dagnn_table_grads_table;
typedef struct dagnn_table_grads_args {
    const float* g;          /* [N, ld_g] */
    int64_t ld_g, N;
    int32_t H, num_tables;
    dagnn_table_grads_table table[DAGNN_TABLE_GRADS_MAX_TABLES];
    void* workspace;
    size_t workspace_bytes;
    int32_t stages;          /* 0: the whole call; DAGNN_TABLE_GRADS_INDEX: the four index launches only; DAGNN_TABLE_GRADS_SUM:
                              * the two sum launches only, over the index an earlier call with the same N, H, keys and rows
                              * left in `workspace` (what scripts/bench_table_grads.py times apart) */
    int32_t reserved;        /* 0 */
} dagnn_table_grads_args;
#define DAGNN_TABLE_GRADS_INDEX 1
#define DAGNN_TABLE_GRADS_SUM 2
size_t dagnn_table_grads_workspace_bytes(int64_t N, int H, const int64_t* rows /* host */, int num_tables);   /* 0: out of range */
int dagnn_table_grads(const dagnn_table_grads_args* args /* host */, void* stream);

/* The small gradients of one cell's attention / edge encoder from the three column sums above, every cell in ONE launch
 * (replaces ~10 torch ops per cell behind `loss.backward()`, dagnn.py:362-373 under autograd):
 *   g_attn[j]      = 0 outside [dq, dq + kd);  g_attn[dq + k] = key_sum[k] + edge_w[k, :] . feat_sum + edge_b[k] * sigma_sum
 *   g_edge_w[k, r] = attn_w[dq + k] * feat_sum[r];   g_edge_b[k] = attn_w[dq + k] * sigma_sum        (edge_w != NULL only) */
#define DAGNN_ATTN_GRAD_MAX_JOBS 16
typedef struct dagnn_attn_grad_job {
    const float* key_sum;    /* [kd]  sum_v sigma_v keys_v */
    const float* feat_sum;   /* [R]   sum_v (edge-feature sums)_v, or NULL */
    const float* sigma_sum;  /* [1]   sum_v sigma_v, or NULL */
    const float* edge_w;     /* [kd, R] edge_encoder.weight, or NULL: no edge encoder */
    const float* edge_b;     /* [kd] */
    const float* attn_w;     /* [attn_len] attn_lin.weight row */
    float* g_attn;           /* [attn_len] */
    float* g_edge_w;         /* [kd, R] */
    float* g_edge_b;         /* [kd] */
    int32_t dq, kd, attn_len, R;
} dagnn_attn_grad_job;
int dagnn_attn_grads_run(const dagnn_attn_grad_job* jobs /* host */, int njob, void* stream);

/* ------------------------------------------------------------------------------------------
 * Read-out (dagnn.py:119-126,184-202: `global_max_pool` / `global_add_pool` / `global_mean_pool`; `P_ATTN`,
 * dagnn.py:114-117, is a softmax over a size-1 dimension and therefore add-pooling) and its backward, for several
 * matrices in ONE launch, grid (graph, job).  jobs: host arrays, n <= DAGNN_MAX_READOUT_JOBS (n == 0: nothing to do,
 * returns 0).  A job pools `width` columns of h [N,ld_h] per graph g into out[g, col_off .. col_off + width).
 *   scope:    0 / 1 = the output nodes of direction 0 / 1 (0: the sinks, 1: the sources): the layer-0 frontier of the
 *             OPPOSITE direction, { v in g : layer_{1-scope}(v) == 0 }, which the plan holds as a contiguous range of
 *             order[1 - scope];  2 = every node of the graph (`out_pool_all=1`).
 *   order:    scope 0 / 1 visit that range of order[1 - scope] front to back, scope 2 visits ascending node ids.  Sums
 *             are taken in this order, one fp32 addition per node from 0.f (the first node's value, but for -0); the
 *             maximum starts from the first node's value.
 *   empty:    a graph with nothing in scope reads 0 in the forward; the backward writes nothing for it.
 *   forward:  MAX: the maximum (fmaxf) in visiting order; ADD: the sum; MEAN: the sum times 1.f / (float)count, i.e.
 *             two roundings after the sum: one of the reciprocal, one of the product.
 *   backward: grad_h[v, j] += grad_out[g, col_off + j] for every node v of graph g in scope (ADD); the same addend times
 *             the forward's factor 1.f / (float)count, rounded once and applied with one multiply of its own (MEAN); the
 *             addend at the FIRST node in visiting order that attains the maximum of column j (MAX: a later node wins
 *             only if strictly greater, the single winner of scatter-max).  h is read for DAGNN_POOL_MAX only and may
 *             be NULL otherwise.  grad_h is initialised by the caller.  Jobs of one launch have distinct grad_h (equal
 *             pointers: DAGNN_EINVAL).
 * One thread owns a (graph, column) pair and every node belongs to one graph: no atomics, two runs agree bit for bit.
 * ---------------------------------------------------------------------------------------- */
#define DAGNN_MAX_READOUT_JOBS 24
enum { DAGNN_POOL_MAX = 0, DAGNN_POOL_ADD = 1, DAGNN_POOL_MEAN = 2 };
typedef struct dagnn_pool_job {
    const float* h;      /* [N, ld_h] */
    int32_t ld_h, width, scope, mode, col_off;
} dagnn_pool_job;
typedef struct dagnn_pool_bwd_job {
    const float* h;      /* [N, ld_h]; DAGNN_POOL_MAX only */
    float* grad_h;       /* [N, ld_g] */
    int32_t ld_h, ld_g, width, scope, mode, col_off;
} dagnn_pool_bwd_job;
int dagnn_readout_pool_batch(const dagnn_plan* plan /* host */, const dagnn_pool_job* jobs /* host */, int n, float* out,
                             int ld_out, void* stream);
int dagnn_readout_pool_backward_batch(const dagnn_plan* plan /* host */, const dagnn_pool_bwd_job* jobs /* host */, int n,
                                      const float* grad_out, int ld_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Constructor-string variants of the same loop (no BASELINE configuration selects
 * them): the aggregators `MultAttnConv` (dagnn.py:379-409), `GatedSumConv` (:254-276), `AggConv` add / max
 * (:232-251), the additive-attention convs when they meet `agg_x` (:159-169) or the Linear cell `recurr=0`
 * (:83-85,181).  Forward only; one lock-step pass of generic kernels: per step an aggregate launch (one wave per
 * frontier row), a cell launch (GRU or Linear over [input ; aggregate]) and - for the aggregators that project the
 * states - a launch of per-node linear maps over the rows just produced.  All operands are indexed by node id.
 *
 * Aggregate of frontier row v over its in-edges e = (j -> v) in original edge order, attr_e = the plan's edge
 * features (num_edge_feats = R floats; pointers marked "or NULL" drop their term):
 *   ATTN   logit_e = edge_vec0 . node0[j] + edge_mat0 . attr_e        (key score; the query half and the biases are
 *          out[v]  = sum_e softmax_e(logit) * vals[j]                   constant inside a softmax segment)
 *   MATTN  logit_e = node1[v] . (node0[j] + edge_mat0 attr_e + edge_vec0);  out[v] as for ATTN
 *          node1 = W_l q + b_l per node, node0 = W_r k + b_r per node, edge_mat0 = W_r W_e [aux_dim,R],
 *          edge_vec0 = W_r b_e
 *   GATED  out[v] = sum_e sigmoid(node0[j] + edge_mat0 attr_e + edge_vec0) * (node1[j] + edge_mat1 attr_e + edge_vec1)
 *          node0 = W_g h + b_g, node1 = W_m h (+ b_m) per node; edge_mat0 = W_g W_e, edge_vec0 = W_g b_e, ..1 for W_m
 *   ADD    out[v] = sum_e (vals[j] + edge_mat0 attr_e + edge_vec0)      edge_mat0 = W_e [val_dim,R], edge_vec0 = b_e
 *   MAX    out[v] = max_e (...)                                          (as ADD)
 *   GIVEN  out is an input: the aggregate of every node (zeros for the nodes of layer 0), computed beforehand
 *          (`agg_x`: the aggregator runs on the node inputs, dagnn.py:159-169, so dagnn_variant_aggregate does all
 *          layers in one launch; nothing then couples the layers, and the caller may pass the whole batch as ONE
 *          layer: layer_ptr = {0, N})
 * Segment softmax as PyG 1.6: exp(x - max) / (sum + 1e-16).  Columns val_dim..out_dim-1 of out[v] are zero-filled
 * (the reference pads the aggregate of the inputs up to the hidden size, dagnn.py:166-168).
 * ---------------------------------------------------------------------------------------- */
enum { DAGNN_AGG_ATTN = 0, DAGNN_AGG_MATTN = 1, DAGNN_AGG_GATED = 2, DAGNN_AGG_ADD = 3, DAGNN_AGG_MAX = 4,
       DAGNN_AGG_GIVEN = 5 };

typedef struct dagnn_variant_aggregator {
    int32_t mode;      /* DAGNN_AGG_* */
    int32_t lands;     /* 0: the messages do not land on the frontier and every row reads zeros - the reference builds ONE
                        * AggConv for both directions (dagnn.py:74-75), whose flow is source -> target in direction 1 too */
    int32_t val_dim;   /* width of a message (<= 1024) */
    int32_t aux_dim;   /* ATTN: key width; MATTN: width of the projected query / key */
    int32_t out_dim;   /* columns of out written per row (>= val_dim) */
    int32_t reserved;
    const float* vals; /* [N,ld_vals] rows summed (ATTN, MATTN, ADD, MAX) */
    int64_t ld_vals;
    const float* node0; /* [N,ld_node], see above */
    const float* node1;
    int64_t ld_node;
    const float* edge_mat0; /* row-major [dim,R], or NULL */
    const float* edge_vec0; /* [dim], or NULL (ATTN: the key weights, required) */
    const float* edge_mat1;
    const float* edge_vec1;
    float* out;        /* [N,ld_out] aggregate by node id */
    int64_t ld_out;
} dagnn_variant_aggregator;

/* Aggregate the rowrec slots [slot_begin, slot_end) of direction `dir` (any range of whole layers >= 1). */
int dagnn_variant_aggregate(const dagnn_plan* plan /* host */, const dagnn_variant_aggregator* agg /* host */, int dir,
                            int32_t slot_begin, int32_t slot_end, void* stream);

typedef struct dagnn_variant_map { /* out[v, 0:out_dim] = w_t^T h[v] + bias (+ vid_bias[v mod vid_mod]) for every row v the cell just produced */
    const float* w_t;  /* [H,out_dim]: the weight transposed (k-major) */
    const float* bias; /* [out_dim] or NULL */
    float* out;        /* [N,ld_out] */
    int64_t ld_out;
    int32_t out_dim;
    int32_t vid_mod;   /* > 0: the mapped vector is [state ; one-hot(v mod vid_mod)] (D-VAE NA, dvae/dagnn.py:124-137): the one-hot
                        * columns of the weight act as a per-vertex-id bias */
    const float* vid_bias; /* [vid_mod, out_dim] (the weight's one-hot columns, transposed) when vid_mod > 0 */
} dagnn_variant_map;

typedef struct dagnn_variant_cell {
    dagnn_variant_aggregator agg; /* agg.out: scratch [N,ld_out] with out_dim = H (GIVEN: the input aggregate) */
    int32_t recurrent; /* 1: GRUCell(input, aggregate) (gate order r,z,n); 0: Linear([input ; aggregate]) (dagnn.py:181) */
    int32_t in_dim;    /* width of the input: emb_dim for stacked layer 0, H above */
    const float* input; /* [N,ld_input]: node inputs (stacked layer 0) or the states of the cell below */
    int64_t ld_input;
    const float* w_in_t;  /* [in_dim, G*H] k-major (G = 3 gates, or 1): weight_ih^T, or weight[:, :in_dim]^T */
    const float* w_agg_t; /* [H, G*H]: weight_hh^T, or weight[:, in_dim:]^T */
    const float* b_in;    /* [G*H] bias_ih, or the Linear bias */
    const float* b_agg;   /* [3H] bias_hh, or NULL */
    float* h;          /* [N,ld_h] states, every row written exactly once */
    int64_t ld_h;
    dagnn_variant_map map[3];
    int32_t num_maps;
    int32_t reserved;
} dagnn_variant_cell;

typedef struct dagnn_variant_args {
    dagnn_variant_cell cell[DAGNN_MAX_DIRS][DAGNN_MAX_STACKED];
    int num_stacked, dir_mask, H;
} dagnn_variant_args;

/* layer_ptr / num_layers as for dagnn_frontier_run.  Layer t of stacked layer i runs in step t + i; at layer 0 the
 * aggregate is zero (GRUCell(x, None), dagnn.py:172-174,181) unless it is GIVEN. */
int dagnn_variant_run(const dagnn_plan* plan /* host */, const dagnn_variant_args* args /* host */,
                      const int32_t* const* layer_ptr /* host */, const int32_t* num_layers /* host [2] */, void* stream);

/* Reverse sweep of the variants `gated_sum`, `mattn_h`, `add`, `max` with GRU or Linear cells (csrc/variants_bwd.hip): what
 * `loss.backward()` does to dagnn.py:144-182 with GatedSumConv (:254-276), MultAttnConv (:379-409) or AggConv add / max (:232-251).
 * Every buffer is indexed by node id; weights are in their torch layouts.  Width and row pitch are separate for gated_sum,
 * add and max: with ld = args->ld (0: H; mattn and additive attention need ld == H) the state-like buffers h, a, g, da are
 * [N, ld], gi / gh / dgi / dgh are [N, 3 ld] with gate block q at column q * ld, gated node0 / dnode0 are [N, 2 ld] with the
 * mapper's half at column ld; esum keeps the widths below.  Only columns < H of a block are read or written, so padding the
 * caller zeroed stays zero (a pitch that is a multiple of 4 keeps dagnn_gemm_nt_bias / dagnn_wgrad_run on aligned rows).  The caller
 * provides the forward quantities (states h, aggregates a, pre-activations gi / gh, the per-node projections the forward
 * pass of dagnn_variant_run computed: node0 = [P | M] for gated_sum, Kr for mattn; node1 = Ql for mattn; mattn also the
 * attention weights alpha by original edge id - dagnn_variant_mattn_prepare computes a and alpha), `g` = the gradient
 * reaching h from outside (modified: the sweep accumulates into it), `g_in` = the gradient of the cell's input (the `g`
 * of the stacked layer below, or a zero-initialised dx buffer of ITS OWN per direction).  Outputs for the parallel
 * epilogue: dgi, dgh [N,3H], dnode0 (dP | dM, or dKr), dnode1 (dQl), and per-node edge-feature sums `esum` (gated:
 * [N, 2 R H], mattn: [N, R proj_dim], add / max: [N, (R + 1) H]; R <= 2; NULL without an edge encoder).  At most 8 cells. */
typedef struct dagnn_variant_bwd_cell {
    int32_t mode, lands, in_dim, proj_dim;
    int32_t recurrent;       /* 1: GRU cell; 0: the Linear cell of `recurr=0` (dagnn.py:83-85): h = W [u ; a] + b - then gi / gh / dgi /
                              * dgh are unused, w_ih = W[:, :in_dim] and w_hh = W[:, in_dim:] as contiguous [H, .] copies */
    int32_t reserved;        /* additive attention (DAGNN_AGG_ATTN): 1 = the keys are this cell's states (their gradient gets
                              * sigma w_k), 0 = the keys are the node inputs; node0 = keys [N, proj_dim], w_node = w_k [proj_dim],
                              * edge_mat0 = the folded edge gains [R]; outputs dnode0 = sigma [N], esum = sum_e ds_e attr_e [N, R];
                              * dlogit [E] (work space by edge id, as for mattn) is required */
    const float* h;  const float* a;  const float* gi;  const float* gh;
    const float* node0;  const float* node1;  const float* alpha;
    const float* edge_mat0;  const float* edge_vec0;  const float* edge_mat1;  const float* edge_vec1;
    const float* w_node;     /* gated: [W_g ; W_m] [2H, H] - or, with w_node2, W_g alone; mattn: W_r [proj_dim, H] */
    const float* w_query;    /* mattn: W_l [proj_dim, in_dim] */
    const float* w_hh;       /* [3H, H] */
    const float* w_ih;       /* [3H, in_dim] */
    float* g;  float* g_in;  float* da;  float* dgi;  float* dgh;
    float* dnode0;  float* dnode1;  float* dlogit;  float* esum;
    const float* w_node2;    /* gated: W_m [H, .] when gate and mapper are read in place as two matrices; NULL: stacked at w_node */
    int32_t w_ld;            /* gated: row stride of w_node / w_node2, of which the first H columns are read (D-VAE NA: H +
                              * num_nodes - the rest are the one-hot vertex-id columns); 0: H */
    int32_t ld_in;           /* row pitch of g_in; 0: in_dim */
    float* ties;             /* max: [N, ld] - how many messages of (w, k) equal the maximum a_w[k]; they share da_w[k] evenly.
                              * Written by dagnn_variant_max_prepare, read by the sweep; required when `lands` */
} dagnn_variant_bwd_cell;

typedef struct dagnn_variant_bwd_args {
    dagnn_variant_bwd_cell cell[DAGNN_MAX_DIRS][DAGNN_MAX_STACKED];
    int num_stacked, dir_mask, H;
    int ld;                  /* row pitch of the state-like buffers, >= H; 0: H */
} dagnn_variant_bwd_args;

/* (also the additive-attention aggregators: mode DAGNN_AGG_ATTN) */
int dagnn_variant_mattn_prepare(const dagnn_plan* plan /* host */, const dagnn_variant_bwd_cell* cell /* host */, int dir, int H,
                                int32_t row_begin, int32_t row_end, void* stream);
/* max: fills cell->ties [N, ld] for the rows [row_begin, row_end) of direction `dir` from h (the aggregated values, [N, ld]), a
 * (the stored maxima, [N, ld]) and the edge terms - one pass over the in-edges of every row, whole numbers, no atomics. */
int dagnn_variant_max_prepare(const dagnn_plan* plan /* host */, const dagnn_variant_bwd_cell* cell /* host */, int dir, int H,
                              int ld, int32_t row_begin, int32_t row_end, void* stream);
int dagnn_variant_backward_run(const dagnn_plan* plan /* host */, const dagnn_variant_bwd_args* args /* host */,
                               const int32_t* const* layer_ptr /* host */, const int32_t* num_layers /* host [2] */, void* stream);
/* `agg_x` (dagnn.py:159-169: the aggregator reads the node inputs only): the cells' sweep runs with mode DAGNN_AGG_GIVEN
 * (nothing is pulled) over ONE pseudo-layer holding all rows, then the aggregator's reverse pass is one shot over all rows:
 * `cell` with h = x [N, width], a = the aggregator's output, da = the gradient of that output summed over the stacked
 * cells, g = g_in = the gradient of x (accumulated into). */
int dagnn_variant_aggregator_backward(const dagnn_plan* plan /* host */, const dagnn_variant_bwd_cell* cell /* host */, int dir,
                                      int width, int32_t row_begin, int32_t row_end, void* stream);

/* D-VAE NA gated_sum (dvae/dagnn.py:124-137): gate and mapper read [state ; one-hot(v mod n)], so the gradient of their one-hot
 * column j is the sum of dP | dM over the nodes with v mod n == j:  out[j, 0:J] = sum_{v mod n == j} in[v, 0:J] for in [N, ld_in],
 * out [n, ld_out].  One thread per output element adds its rows in ascending order: no atomics, bitwise repeatable. */
int dagnn_vid_colsums(const float* in, int64_t ld_in, int64_t N, int J, int n, float* out, int64_t ld_out, void* stream);

/* D-VAE read-out (dvae/dagnn.py:147-161, dvae/dagnn_bn.py:138-152): every graph has exactly
 * `stride` nodes; gather row g*stride + node_off of h [N,ld_h] into out[g, col_off : col_off+width]. */
int dagnn_gather_rows(const float* h, int ld_h, int width, int64_t num_graphs, int stride, int node_off,
                      float* out, int ld_out, int col_off, void* stream);
/* ... for up to 16 (matrix, node offset, column offset) jobs in one launch: every (direction, stacked layer) of the read-out */
typedef struct dagnn_gather_job { const float* h; int ld_h, width, node_off, col_off; } dagnn_gather_job;
int dagnn_gather_rows_batch(const dagnn_gather_job* jobs /* host */, int n, int64_t num_graphs, int stride, float* out, int ld_out,
                            void* stream);

/* Decoder-side single-vertex step of the D-VAE models: `_ipropagate_to(G, v, propagator, H)` (dvae/dagnn.py:187-239,
 * dvae/dagnn_bn.py:179-238; called as `_update_iv` from models_pyg.py:247-250), for all B graphs that have vertex v, in
 * ONE launch.  values [B,P,hs]: layer-0 states of v's predecessors, lists padded to P with zero rows; pred_vid [B,P]:
 * vertex id of each predecessor, -1 for padding.  The reference's soft-max runs over the padding too (a padded key
 * scores w_q.q + b; that common term cancels, so padded slots score 0 and real ones w_key.h_j + vid_bias[j]); the
 * aggregate is computed once and feeds every stacked GRU cell; with `H_given` [B,hs] it replaces the aggregate.
 * x [B,in0]: one-hot vertex types.  states [L,B,hs]: the new state of v per stacked layer (states[L-1] is the return
 * value of the reference's function). */
typedef struct dagnn_iprop_layer {
    const float* w_ih;   /* [3hs, in_dim] torch GRUCell layout */
    const float* w_hh;   /* [3hs, hs] */
    const float* b_ih;   /* [3hs] */
    const float* b_hh;   /* [3hs] */
    int in_dim;          /* in0 for layer 0, hs above */
} dagnn_iprop_layer;
int dagnn_iprop_step(const float* values, const int32_t* pred_vid, int64_t B, int P, int hs, const float* w_key,
                     const float* vid_bias /* [max_n] or NULL */, const float* H_given /* or NULL */, const float* x, int in0,
                     const dagnn_iprop_layer* layers /* host [L] */, int L, float* states, void* stream);
/* ... with type-keyed attention (`attn_x` on the BN model, dvae/dagnn_bn.py:203-225): pred_type [B,P] holds the vertex
 * TYPE of each predecessor (-1 for padding; clamped to nvt-1), a real slot scores key_type[type] (key_type [nvt]: the key
 * half of attn_lin.weight), a padded one 0; the values are the predecessors' layer-0 states as above. */
int dagnn_iprop_step_typed(const float* values, const int32_t* pred_type, int64_t B, int P, int hs, const float* key_type,
                           int nvt, const float* H_given /* or NULL */, const float* x, int in0,
                           const dagnn_iprop_layer* layers /* host [L] */, int L, float* states, void* stream);

/* ------------------------------------------------------------------------------------------
 * Teacher-forced D-VAE decoder: `DVAE_PYG.loss()` (dvae/models_pyg.py:398-456) without the latent part - H0 =
 * tanh(fc3(z)) and the KL term stay with the caller - for graphs of exactly n vertices.  One call issues every launch
 * of the decode: the n-1 vertex steps with all v+1 updates of vertex v (`_update_iv`, dvae/dagnn.py:187-239 /
 * dvae/dagnn_bn.py:179-238, the padded soft-max quirk included) at once per stacked layer, then the vertex head
 * (log-softmax at the true type, models_pyg.py:410-414) and the edge head (sigmoid score and torch's
 * binary_cross_entropy with its log clamp at -100, :423-448) over all rows.  `bn` = 1: the graph state is the sum of
 * the top states of vertices 0..v-1 and the edge head reads [H_vi, H_v, H0] (models_pyg.py:591-614, 733-736); bn = 0:
 * the top state of v-1 and [H_vi, H_v].
 *   types [B,n] int32: true vertex types (vertex 0 is decoded as start_type whatever it holds);
 *   preds [B,n] uint32: bit u of preds[b,v] = the true edge u -> v (u < v);
 *   h0 [B,hs]; w_key [hs] and vid_bias [n] (NULL for BN): the key half of node_aggr_0[0].attn_lin.weight;
 *   grud cell l: torch GRUCell tensors (layer 0 reads nvt-wide one-hot inputs, the others hs);
 *   av_* / ae_*: add_vertex.{0,2} / add_edge.{0,2} weight and bias (edge_hidden = add_edge.0 rows,
 *   vertex_hidden = add_vertex.0 rows);
 *   ll [2B+1]: vertex log-likelihood per graph, edge log-likelihood per graph, then res = -(sum of both), all reduced
 *   in a fixed order;
 *   saved: the activations the reverse pass reads, >= dagnn_dvae_decode_saved_bytes(args) bytes.
 * dagnn_dvae_decode_backward reads the same args (and the saved activations of the forward call) and writes - not
 * accumulates - d res scaled by the device scalar *g_res for every input above; d_w_key / d_vid_bias may point into one
 * zeroed attn_lin.weight gradient.  `work` >= dagnn_dvae_decode_work_bytes(args) bytes.  Both are bitwise deterministic
 * (no float atomics).
 *
 * The decoder's description - the fields n, hs, L, nvt, start_type, bn, edge_hidden, vertex_hidden, the grud / av_* /
 * ae_* weights and `agg` with its tensors - is shared, name by name, with dagnn_dvae_sample_args, and one set of rules
 * (csrc/dvae_common.h) serves both: the ranges noted on the fields below; edge_hidden, vertex_hidden >= 1; bn 0 or 1;
 * agg one of DAGNN_DVAE_AGG_*; DAGNN_DVAE_AGG_GATED_SUM only with bn = 0 and all of gate_w / gate_b / mapper_w;
 * DAGNN_DVAE_AGG_ATTN_X only with bn = 1 and key_type.  The size queries return 0 for arguments that break one of
 * them (or an entry point's own size limits), and the entry points DAGNN_EINVAL; a missing pointer otherwise - h0, a
 * weight, DAGNN_DVAE_AGG_ATTN_H's w_key, an output, a workspace - is refused by the entry points alone.
 * agg = DAGNN_DVAE_AGG_GATED_SUM (`gated_sum`, NA only): the aggregate of vertex v is sum over its predecessors u of sigmoid(Wg x_u + bg) *
 * (Wm x_u), x_u = [layer-0 state of u ; one-hot(u, n)], from gate_w / gate_b / mapper_w (gate_forward.0.0 and
 * mapper_forward.0.0, [hs, hs+n] row-major); w_key / vid_bias are not read.  Their gradients go to d_gate_w / d_gate_b
 * / d_mapper_w, and d_w_key / d_vid_bias are not written.  The fields are appended: a zero-filled struct is
 * DAGNN_DVAE_AGG_ATTN_H.
 * agg = DAGNN_DVAE_AGG_ATTN_X (`attn_x`, BN only: dvae/dagnn_bn.py:203-225): the attention keys are the predecessors' one-hot TYPES, so a
 * real slot scores key_type[type of u] - key_type [nvt] is the key half of node_aggr_0[0].attn_lin.weight ([1, 2 nvt]:
 * columns nvt..2nvt-1) -, a padded slot 0, and the values stay the layer-0 states; w_key / vid_bias are not read.  In
 * reverse d_key_type[t] (written, not accumulated) is the sum of the score gradients of every (update, real slot) whose
 * predecessor has type t, in one fixed order; the keys do not depend on the states, so a predecessor's state gradient
 * is alpha * d hagg alone; d_w_key / d_vid_bias are not written.
 * key_type / d_key_type are appended behind the gated_sum fields and read only once agg = DAGNN_DVAE_AGG_ATTN_X with
 * bn = 1 is established, so a caller built against the earlier structs (attn_h / gated_sum) is served as before.
 * ---------------------------------------------------------------------------------------- */
#define DAGNN_DVAE_MAX_N 32
#define DAGNN_DVAE_MAX_TYPES 64
#define DAGNN_DVAE_AGG_ATTN_H 0      /* w_key / vid_bias */
#define DAGNN_DVAE_AGG_GATED_SUM 1   /* gate_w / gate_b / mapper_w; NA only */
#define DAGNN_DVAE_AGG_ATTN_X 2      /* key_type; BN only */
typedef struct dagnn_dvae_decode_args {
    int64_t B;               /* graphs */
    int n;                   /* vertices per graph (max_n), 2..DAGNN_DVAE_MAX_N */
    int hs;                  /* state width */
    int L;                   /* stacked grud cells, 1..DAGNN_MAX_STACKED */
    int nvt;                 /* vertex types, 1..DAGNN_DVAE_MAX_TYPES */
    int start_type;
    int bn;                  /* 0: D-VAE (NA), 1: D-VAE for Bayesian networks */
    int edge_hidden, vertex_hidden;
    const int32_t* types;
    const uint32_t* preds;
    const float* h0;
    const float* w_ih[DAGNN_MAX_STACKED];
    const float* w_hh[DAGNN_MAX_STACKED];
    const float* b_ih[DAGNN_MAX_STACKED];
    const float* b_hh[DAGNN_MAX_STACKED];
    const float* w_key;
    const float* vid_bias;
    const float *av_w1, *av_b1, *av_w2, *av_b2;
    const float *ae_w1, *ae_b1, *ae_w2, *ae_b2;
    float* ll;
    float* saved;
    size_t saved_bytes;
    int agg;                 /* DAGNN_DVAE_AGG_* */
    const float* gate_w;     /* [hs, hs+n] */
    const float* gate_b;     /* [hs] */
    const float* mapper_w;   /* [hs, hs+n] */
    const float* key_type;   /* DAGNN_DVAE_AGG_ATTN_X: [nvt] */
} dagnn_dvae_decode_args;
typedef struct dagnn_dvae_decode_grads {
    const float* g_res;      /* device scalar: d loss / d res */
    float* work;
    size_t work_bytes;
    float* d_h0;
    float* d_w_ih[DAGNN_MAX_STACKED];
    float* d_w_hh[DAGNN_MAX_STACKED];
    float* d_b_ih[DAGNN_MAX_STACKED];
    float* d_b_hh[DAGNN_MAX_STACKED];
    float* d_w_key;
    float* d_vid_bias;
    float *d_av_w1, *d_av_b1, *d_av_w2, *d_av_b2;
    float *d_ae_w1, *d_ae_b1, *d_ae_w2, *d_ae_b2;
    float *d_gate_w, *d_gate_b, *d_mapper_w;   /* DAGNN_DVAE_AGG_GATED_SUM */
    float* d_key_type;       /* DAGNN_DVAE_AGG_ATTN_X: [nvt] */
} dagnn_dvae_decode_grads;
size_t dagnn_dvae_decode_saved_bytes(const dagnn_dvae_decode_args* args /* host */);
size_t dagnn_dvae_decode_work_bytes(const dagnn_dvae_decode_args* args /* host */);
int dagnn_dvae_decode_forward(const dagnn_dvae_decode_args* args /* host */, void* stream);
int dagnn_dvae_decode_backward(const dagnn_dvae_decode_args* args /* host */, const dagnn_dvae_decode_grads* grads /* host */,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Sampling D-VAE decoder: `DVAE_PYG.decode(z, stochastic)` (dvae/models_pyg.py:338-396; BN through DVAE_BN_PYG, graph
 * state = sum of the vertex states, edge head on [H_vi, H_v, H0]) for G independent groups of B rows, R = G*B, in ONE
 * call with no host round trip.  Each group is decoded exactly as one reference call on its B rows: the padding width P
 * of every update and the set of rows still being updated are reduced per group, never across groups.
 *   h0 [R,hs] = tanh(fc3(z)); the decoder's description - dimensions, grud cells, add_vertex (av_*), add_edge (ae_*),
 *   agg and its tensors - is that of dagnn_dvae_decode_args, with its rules; end_type in [0, nvt); stochastic = 0: argmax types and score > 0.5 edges (the draws are not read);
 *   stochastic = 1: u_type [G,n,B] (row idx serves the type draw of vertex idx = 1..n-2, as np.random.choice maps
 *   its uniform: searchsorted(cumsum(p)/sum(p), u, 'right') in float64), u_edge [G,n(n-1)/2,B] (pair
 *   idx(idx-1)/2 + (idx-1-vi) serves the edge step (idx, vi) in the reference's call order; edge kept on u < score).
 *   Outputs: types [R,n] int32 (-1 past the graph's end), preds [R,n] uint32 (bit u of preds[r,v]: edge u -> v, the
 *   encoding of dagnn_dvae_decode_args), nv [R] int32 vertex counts, states [R,n,hs] (or NULL): the final top-layer
 *   state of every vertex, zero past the end.
 *   work >= dagnn_dvae_sample_work_bytes(args) bytes.  No allocation, no synchronisation, bitwise repeatable (no float
 *   atomics).  DAGNN_DVAE_AGG_ATTN_X: a vertex's key score is key_type[its type], written when the vertex is final.
 * ---------------------------------------------------------------------------------------- */
typedef struct dagnn_dvae_sample_args {
    int64_t G;               /* groups (independent decode calls) */
    int64_t B;               /* rows per group */
    int n;                   /* max_n, 2..DAGNN_DVAE_MAX_N */
    int hs;
    int L;                   /* stacked grud cells, 1..DAGNN_MAX_STACKED */
    int nvt;                 /* vertex types, 1..DAGNN_DVAE_MAX_TYPES */
    int start_type, end_type;
    int bn;                  /* 0: D-VAE (NA), 1: D-VAE for Bayesian networks */
    int stochastic;          /* 0: argmax, 1: sample with the given draws */
    int edge_hidden, vertex_hidden;
    const float* h0;
    const float* w_ih[DAGNN_MAX_STACKED];
    const float* w_hh[DAGNN_MAX_STACKED];
    const float* b_ih[DAGNN_MAX_STACKED];
    const float* b_hh[DAGNN_MAX_STACKED];
    const float* w_key;
    const float* vid_bias;   /* [n] or NULL */
    const float *av_w1, *av_b1, *av_w2, *av_b2;
    const float *ae_w1, *ae_b1, *ae_w2, *ae_b2;
    const float* u_type;
    const float* u_edge;
    int32_t* types;
    uint32_t* preds;
    int32_t* nv;
    float* states;           /* or NULL */
    float* work;
    size_t work_bytes;
    int agg;                 /* DAGNN_DVAE_AGG_*, as in dagnn_dvae_decode_args */
    const float* gate_w;
    const float* gate_b;
    const float* mapper_w;
    const float* key_type;   /* DAGNN_DVAE_AGG_ATTN_X: [nvt] */
} dagnn_dvae_sample_args;
size_t dagnn_dvae_sample_work_bytes(const dagnn_dvae_sample_args* args /* host */);
int dagnn_dvae_sample(const dagnn_dvae_sample_args* args /* host */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Validity and selection of decoded D-VAE graphs: the loop of `decode_from_latent_space` (dvae/util.py:408-466) over
 * A attempts of B latent points, on the dense output of dagnn_dvae_sample (G = A groups of B rows).
 *   types [A,B,n] int32 (-1 past the end), preds [A,B,n] uint32 (bit u of preds[a,b,v]: edge u -> v, u < v; other
 *   bits are ignored), nv [A,B] int32 vertex counts.
 *   kind = DAGNN_DVAE_ENAS: is_valid_ENAS (util.py:621-631), and with n_nodes > 0 exactly n_nodes vertices; kind =
 *   DAGNN_DVAE_BN: is_valid_BN (util.py:634-649) with nvt types, n_nodes not read.  A type outside [0, nvt) or a vertex
 *   count outside [1, n] makes a row invalid.
 *   Outputs: valid [A,B] int32 (0 / 1); per point b: pick [B] the chosen attempt or -1 when none is valid, n_valid [B],
 *   n_same [B] the valid attempts whose string equals the picked one.  select = DAGNN_DVAE_FIRST_VALID: the first valid
 *   attempt (what the reference returns: np.argmax over a dict_values object is always 0); DAGNN_DVAE_MOST_FREQUENT:
 *   the most frequent string, ties to the earliest first occurrence (Counter.most_common(1)), picked at that occurrence.
 *   work >= dagnn_dvae_select_work_bytes(args) bytes receives the canonical keys, uint64 [B,A,W] with
 *   W = dagnn_dvae_select_key_words(kind, n, nvt): the string's content bit-packed (equal keys <=> equal strings; zero
 *   for invalid rows).  No allocation, no synchronisation, integer work only: bitwise repeatable.  The size query
 *   returns 0 (the key query 0) for arguments the entry point refuses with DAGNN_EINVAL.
 * ---------------------------------------------------------------------------------------- */
#define DAGNN_DVAE_ENAS 0
#define DAGNN_DVAE_BN 1
#define DAGNN_DVAE_FIRST_VALID 0
#define DAGNN_DVAE_MOST_FREQUENT 1
typedef struct dagnn_dvae_select_args {
    int64_t A;               /* attempts */
    int64_t B;               /* latent points; A * B <= 2^30 */
    int n;                   /* max_n, 2..DAGNN_DVAE_MAX_N */
    int nvt;                 /* vertex types, 1..DAGNN_DVAE_MAX_TYPES */
    int start_type, end_type;
    int kind;                /* DAGNN_DVAE_ENAS or DAGNN_DVAE_BN */
    int n_nodes;             /* ENAS: 0 any vertex count, else exactly this many (0..DAGNN_DVAE_MAX_N) */
    int select;              /* DAGNN_DVAE_FIRST_VALID or DAGNN_DVAE_MOST_FREQUENT */
    const int32_t* types;
    const uint32_t* preds;
    const int32_t* nv;
    int32_t* valid;
    int32_t* pick;
    int32_t* n_valid;
    int32_t* n_same;
    void* work;
    size_t work_bytes;
} dagnn_dvae_select_args;
int dagnn_dvae_select_key_words(int kind, int n, int nvt);
size_t dagnn_dvae_select_work_bytes(const dagnn_dvae_select_args* args /* host */);
int dagnn_dvae_select(const dagnn_dvae_select_args* args /* host */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Graph identity of decoded D-VAE graphs (csrc/dvae_match.hip): what the reference's evaluation runs after the decode,
 * on the dense layout of dagnn_dvae_sample (types / preds [A,B,n], nv [A,B]; bits of preds[.,v] at or above v ignored).
 *
 * dagnn_dvae_same_dag: `is_same_DAG` (dvae/util.py:576-585) of decode row (a, b) against true row b (types_true /
 *   preds_true [B,n], nv_true [B] or NULL: n vertices each): equal vertex count, and for every v < nv equal type and
 *   equal predecessor mask; entries at v >= nv take no part, no isomorphism.  Outputs, all int32, from one call: same
 *   [A,B] (0 / 1), per_graph [B] (matching attempts of graph b), total [1].
 *
 * A SET of rows: `ratio_same_DAG`'s left-hand side (util.py:588-596; DAGNN_DVAE_SET_GRAPHS, width = n, membership =
 *   is_same_DAG against any stored row), or the distinct canonical keys of dagnn_dvae_select, `len(set(G_valid_str))`
 *   (DAGNN_DVAE_SET_KEYS, width = W 64-bit words).  Its storage is ONE caller-owned buffer of
 *   dagnn_dvae_set_bytes(form, width, max_rows) bytes that outlives the calls: DAGNN_DVAE_SET_HEADER_WORDS int32 header
 *   words, `cap` int32 slots, max_rows records.  Capacity rule: cap = the power of two >= 2 * max_rows (at least 64),
 *   so the load factor never exceeds 1/2; the host refuses with DAGNN_ENOSPC, before any launch, a buffer smaller than
 *   that and an add whose rows base .. base + A*B - 1 do not fit in max_rows.  Every probe loop runs at most cap steps;
 *   one that runs out (possible only with a damaged header or table) sets DAGNN_DVAE_SET_ERR_FULL in header word
 *   DAGNN_DVAE_SET_ERR, a header that does not match the descriptor DAGNN_DVAE_SET_ERR_HEADER; the caller reads the word
 *   with its results.  The set is EXACT: the hash only chooses the first slot, a hit or a duplicate is reported after all
 *   words of the row compared equal, and rows with equal hashes are all stored.  Header word DAGNN_DVAE_SET_COUNT is
 *   the number of distinct rows added so far.  Flags and counts are bitwise repeatable (integer atomics on global memory;
 *   which of several equal rows a slot names may differ, nothing returned shows it).
 *   dagnn_dvae_set_init: empties the set (once, before the first add).
 *   dagnn_dvae_set_add: adds the rows r = a * B + b with mask[r] != 0 (mask [A,B] int32 or NULL: all) as records
 *     base + r; the caller gives every add a `base` behind the rows of the earlier ones.  GRAPHS: types / preds / nv
 *     (nv NULL: n vertices each); KEYS: keys [B,A,W] as dagnn_dvae_select writes them (mask = its `valid`).
 *   dagnn_dvae_set_query (GRAPHS): member [A,B] = 1 where mask[r] != 0 and the row is in the set, else 0; count [1] =
 *     their number.  `base` is not read.
 * No allocation, no synchronisation.  The size query returns 0 for descriptors the entry points refuse (DAGNN_EINVAL).
 * ---------------------------------------------------------------------------------------- */
#define DAGNN_DVAE_SET_GRAPHS 0
#define DAGNN_DVAE_SET_KEYS 1
#define DAGNN_DVAE_SET_MAX_ROWS ((int64_t)1 << 20)   /* per set, and per call (A * B) */
#define DAGNN_DVAE_SET_HEADER_WORDS 16
#define DAGNN_DVAE_SET_MAGIC 0    /* header words */
#define DAGNN_DVAE_SET_K 1
#define DAGNN_DVAE_SET_CAP 2
#define DAGNN_DVAE_SET_ROWS 3
#define DAGNN_DVAE_SET_COUNT 4
#define DAGNN_DVAE_SET_ERR 5
#define DAGNN_DVAE_SET_ERR_FULL 1
#define DAGNN_DVAE_SET_ERR_HEADER 2
typedef struct dagnn_dvae_same_dag_args {
    int64_t A;               /* attempts */
    int64_t B;               /* true graphs; A * B <= DAGNN_DVAE_SET_MAX_ROWS */
    int n;                   /* max_n, 2..DAGNN_DVAE_MAX_N */
    const int32_t* types;
    const uint32_t* preds;
    const int32_t* nv;
    const int32_t* types_true;
    const uint32_t* preds_true;
    const int32_t* nv_true;  /* or NULL */
    int32_t* same;
    int32_t* per_graph;
    int32_t* total;
} dagnn_dvae_same_dag_args;
int dagnn_dvae_same_dag(const dagnn_dvae_same_dag_args* args /* host */, void* stream);

typedef struct dagnn_dvae_set {
    int form;                /* DAGNN_DVAE_SET_GRAPHS or DAGNN_DVAE_SET_KEYS */
    int width;               /* GRAPHS: n, 2..DAGNN_DVAE_MAX_N; KEYS: W, 1..16 */
    int64_t max_rows;        /* 1..DAGNN_DVAE_SET_MAX_ROWS */
    void* data;
    size_t bytes;
} dagnn_dvae_set;
typedef struct dagnn_dvae_set_rows_args {
    dagnn_dvae_set set;
    int64_t base;            /* add: index of the call's first record */
    int64_t A;
    int64_t B;               /* A * B <= DAGNN_DVAE_SET_MAX_ROWS */
    const int32_t* types;
    const uint32_t* preds;
    const int32_t* nv;       /* or NULL */
    const uint64_t* keys;
    const int32_t* mask;     /* or NULL */
    int32_t* member;         /* query */
    int32_t* count;          /* query */
} dagnn_dvae_set_rows_args;
size_t dagnn_dvae_set_bytes(int form, int width, int64_t max_rows);
int dagnn_dvae_set_init(const dagnn_dvae_set* set /* host */, void* stream);
int dagnn_dvae_set_add(const dagnn_dvae_set_rows_args* args /* host */, void* stream);
int dagnn_dvae_set_query(const dagnn_dvae_set_rows_args* args /* host */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Topological layering on the device: replaces `top_sort` / `add_order_info_01` (src/utils_dag.py:8-52) for a
 * whole collated batch.  layer_fwd[v] = longest-path distance of v from any source, layer_bwd[v] = the same on
 * the flipped edges; both int64 [N], i.e. `_bi_layer_idx0/1` (`_bi_layer_index0/1` is arange(N)).  `batch`
 * sorted, edges grouped by graph (the collation guarantees both).  A cyclic graph raises bit 16 of *status.
 * ---------------------------------------------------------------------------------------- */
int dagnn_topo_layers(const int64_t* edge_index /* [2,E] */, const int64_t* batch /* [N] */, int64_t N, int64_t E,
                      int64_t B, int64_t* layer_fwd, int64_t* layer_bwd, int32_t* status /* device int32 or NULL */,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * A whole encoder pass from ONE call (the evaluation pass of the D-VAE encoders, dvae/dagnn.py:99-161,
 * dvae/dagnn_bn.py:98-152: batches of 64 x 8 / 128 x 10 nodes are host-bound - the device needs ~95 us for what one call
 * at a time took the host 115-135 us to issue).  Issues, in this order, exactly the launches of dagnn_plan_build,
 * dagnn_gemm_nt_bias (stacked layer 0's input side, one group per direction: C = x W_ih^T + b_ih), dagnn_dataflow_schedule,
 * dagnn_dataflow_run (`df`: the cells' gi0 must point at the GEMM groups' outputs), dagnn_gather_rows_batch (the end /
 * start vertex of every graph into `hcat`) and - `w_out` given - the model's final Linear (out = hcat W_out^T + b_out).
 * Every buffer is the caller's; nothing is allocated or synchronised.
 * ---------------------------------------------------------------------------------------- */
typedef struct dagnn_encode_args {
    dagnn_plan plan;
    const int64_t* edge_index; const int64_t* layer_fwd; const int64_t* layer_bwd; const int64_t* batch;
    const float* edge_attr;          /* or NULL */
    int32_t* plan_status;            /* device int32[4] */
    dagnn_gemm_group gemm[2];        /* per direction: {x, W_ih [gemm_cols, in_dim], b_ih, gi0 [N, gemm_cols]} */
    int num_gemm, gemm_cols, in_dim, ld_x;
    void* schedule; size_t schedule_bytes; int cost_layer, cost_row;
    dagnn_dataflow_args df;
    dagnn_gather_job jobs[16]; int num_jobs, stride;
    float* hcat; int ld_hcat;        /* [B, ld_hcat] */
    const float* w_out; const float* b_out; float* out; int out_dim;   /* w_out [out_dim, ld_hcat] or NULL */
} dagnn_encode_args;
int dagnn_encode_forward(const dagnn_encode_args* args /* host */, void* stream);

/* out [M, K2] = A^T B with A [N, lda >= M rounded up to 4], B [N, ldb]: the reduction over N rows is SMALL, the output large -
 * the S vocabulary heads' weight gradient d logits^T x pooled vectors (dagnn.py:212-215 under main_pyg.py:62), where the
 * library GEMM's pick for 25 010 x 1 024 x 128 runs at a quarter of the matrix rate; colsum [M] (may be NULL) = column sums of
 * A (the heads' bias gradient).  fp32 MFMA, fixed summation order.  lda % 4 == 0, ldb and K2 even, A 16-byte aligned. */
int dagnn_tn_product(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t N, int M, int K2, float* out,
                     float* colsum, void* stream);

/* The TOK task's training loss and its gradient in one launch (csrc/loss.hip; replaces the caller-side loop of
 * ogbg-code/main_pyg.py:55-60: `loss += CrossEntropyLoss()(pred_list[i], y_arr[:, i])` over the S heads, `/ S`).
 * logits [B, ld >= S * V]: head s's V outputs of graph b at b * ld + s * V (how DAGNN lays its heads' outputs side by side);
 * y [B, S] int64 targets in [0, V) (no ignore_index: an out-of-range target makes the loss NaN); dlogits (same layout with its own row pitch, may be
 * NULL) receives d loss / d logits = (softmax - onehot) / (B S); row_loss [B * S] scratch; loss [1]; counter [1] device word,
 * zero before the first call (the kernel leaves it zero).  Sums in a fixed order: bitwise reproducible. */
int dagnn_seq_ce(const float* logits, int64_t ld, const int64_t* y, int B, int S, int V, float* dlogits, int64_t ld_dlogits,
                 float* row_loss, float* loss, unsigned* counter, void* stream);

/* ------------------------------------------------------------------------------------------
 * The TOK task's evaluation path (csrc/predict.hip; ogbg-code/main_pyg.py:91-124): predicted tokens and the integer
 * counts of the F1 evaluator (ogb/graphproppred/evaluate.py:231-267).
 *
 * Order of the logits everywhere below: a NaN is greater than every number and NaNs are equal to each other, -0 == +0,
 * and among equal values the LOWEST column wins - what torch.argmax gives on the CPU.
 *
 * dagnn_heads_argmax: the S vocabulary heads (dagnn.py:212-215) and their argmax (main_pyg.py:106-109) without the
 *   logits.  out [B, ld_out >= D] pooled graph vectors; wcat [S * V, ldw >= D] / bcat [S * V] the heads side by side
 *   (head s: rows s V .. (s + 1) V - 1); tok [B, S] int64 = argmax_c (out[b] . wcat[s V + c] + bcat[s V + c]);
 *   top [B, S, 2] (may be NULL) = that winning logit and the runner-up (the second in the order above, which EQUALS the
 *   winner when two columns tie; -inf when V = 1).  fp32 MFMA accumulate; the sum over D is the same set of exact fp32
 *   fmaf steps whatever B is.  `work` >= dagnn_heads_argmax_bytes(B, S, V) bytes: one 16-byte partial per (graph, head,
 *   128-column tile), merged in ascending tile order by a second launch.  B = 0 returns at once; D is free (rows that
 *   are not 16-byte aligned, or D % 4 != 0, take scalar loads).
 * dagnn_rows_argmax: tok [B, S] from logits that exist, [B, ld >= S * V] with head s's V outputs of graph b at
 *   b * ld + s * V (as dagnn_seq_ce reads them): one launch, a workgroup per (graph, head).
 * dagnn_seq_f1_counts: counts [B, 4] int32 = (true_positive, n_pred, n_ref, len) per graph.  len = position of the first
 *   eos_id in tok[b] (S if none: utils.py:166-179), n_pred = distinct ids in tok[b, :len], n_ref = distinct non-negative
 *   ids in ref_ids[b] ([B, R] int32, padded with -1: the graph's in-vocabulary label words) + ref_extra[b] (its distinct
 *   label words outside the vocabulary, which no prediction can match), true_positive = size of the intersection.
 *   false_positive = n_pred - tp, false_negative = n_ref - tp.  A thread per graph.
 * dagnn_heads_score: the same pass with a wider epilogue, for what an evaluation wants beyond the arg-max - still without
 *   the logits.  Per (graph, head): tok [B, S, k] int64 / logit [B, S, k] = the k best columns (1 <= k <= 8) and their
 *   logits, descending in the order above (tok[.., 0] and logit[.., 0] are dagnn_heads_argmax's tok and top[.., 0], bit for
 *   bit; ranks beyond V hold column -1 and -inf); lse [B, S] = log sum_c exp(logit_c) as torch.logsumexp defines it (any NaN:
 *   NaN; else any +inf: +inf; all -inf: -inf); with targets y [B, S] int64 (NULL: none), nll [B, S] = lse - logit at
 *   y[b, s] - CrossEntropyLoss per row; a target outside [0, V) makes that row's nll NaN and nothing else, as dagnn_seq_ce
 *   decides.  y and nll come together or not at all.  sums (NULL, or 16 device bytes {float64, int64}; needs y): the
 *   batch's B S row losses are added to the float64 one by one in row order by a single thread, B S to the int64, so an
 *   evaluation's mean loss is sums[0] / sums[1] after one read.  `work` >= dagnn_heads_score_bytes(B, S, V, k) bytes,
 *   16-byte aligned: per (graph, head, 128-column tile) the tile's best columns (k rounded up to 1, 2, 4 or 8), its maximum,
 *   its sum of exponentials and the target's logit, merged in ascending tile order by the second launch
 *   (M = max(m1, m2), s = s1 exp(m1 - M) + s2 exp(m2 - M), fast-math exp / log as dagnn_seq_ce).  B = 0 returns at once.
 * No allocation, no synchronisation, no float atomics: bitwise repeatable.  The size queries return 0 for arguments the
 * entry point refuses with DAGNN_EINVAL.
 * ---------------------------------------------------------------------------------------- */
size_t dagnn_heads_argmax_bytes(int64_t B, int S, int V);
size_t dagnn_heads_score_bytes(int64_t B, int S, int V, int k);
int dagnn_heads_score(const float* out, int64_t ld_out, const float* wcat, int64_t ldw, const float* bcat, int64_t B, int D,
                      int S, int V, const int64_t* y, int k, int64_t* tok, float* logit, float* lse, float* nll, void* sums,
                      void* work, size_t work_bytes, void* stream);
int dagnn_heads_argmax(const float* out, int64_t ld_out, const float* wcat, int64_t ldw, const float* bcat, int64_t B, int D,
                       int S, int V, int64_t* tok, float* top, void* work, size_t work_bytes, void* stream);
int dagnn_rows_argmax(const float* logits, int64_t ld, int64_t B, int S, int V, int64_t* tok, void* stream);
int dagnn_seq_f1_counts(const int64_t* tok, int64_t B, int S, int64_t eos_id, const int32_t* ref_ids, int R,
                        const int32_t* ref_extra, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * The LP task's tail (csrc/lp.hip; ogbg-code/main_pyg_lp.py): predict `len_longest_path` of every graph as a class.
 *
 * dagnn_graph_depth: depth [B] int64 = max over the nodes of graph g of layer[v] (`_bi_layer_idx0`: the target the
 *   reference's patched reader stores, ogb/io/read_graph_pyg.py:51-54); batch [N] int64 sorted ascending, so a graph is one
 *   contiguous range, found by bisection; ids outside [0, B) are ignored, a graph without nodes gives 0.  One launch, a
 *   wave per graph, no atomics.  B = 0 returns at once.
 * Targets below are int64, float32 or float64 [B] (`targ_kind`): what the reference concatenates and hands to
 *   `.to(torch.long)` / to the evaluator.
 * dagnn_class_ce: `CrossEntropyLoss()(pred, targ.to(torch.long))` (main_pyg_lp.py:56-58) = dagnn_seq_ce with S = 1 - the
 *   same kernel (csrc/loss.hip), so the same arguments, sums and counter protocol; with int64 targets the same bits - with
 *   the target truncated toward zero in the kernel.
 *   dlogits = (softmax - onehot) / B.  A target outside [0, C) (a NaN included) makes the loss NaN.
 * dagnn_class_hits: out [2] int64 = (hits, labelled) of `Evaluator._eval_acc` (ogb/graphproppred/evaluate.py:221-229) over
 *   one batch.  Predictions are EITHER logits [B, ld >= C] - argmax in the order stated above dagnn_heads_argmax: lowest
 *   column among equals, a NaN beats every number - OR tok [B] int64 (what DAGNN.predict returns); the other pointer is
 *   NULL.  A NaN target is unlabelled and counts in neither; target and prediction are compared as values (3.0 matches
 *   class 3, 3.5 nothing).  `work` >= dagnn_class_hits_bytes(B, logits != NULL) bytes, 8-byte aligned: one partial pair per
 *   workgroup, added by the last workgroup in (integers: exact in any order); counter [1] device word, zero before the first
 *   call (the kernel leaves it zero).  One launch.
 * No allocation, no synchronisation, no float atomics: bitwise repeatable.
 * ---------------------------------------------------------------------------------------- */
#define DAGNN_LP_INT64 0
#define DAGNN_LP_FLOAT32 1
#define DAGNN_LP_FLOAT64 2
int dagnn_graph_depth(const int64_t* layer, const int64_t* batch, int64_t N, int64_t B, int64_t* depth, void* stream);
int dagnn_class_ce(const float* logits, int64_t ld, const void* targ, int targ_kind, int B, int C, float* dlogits,
                   int64_t ld_dlogits, float* row_loss, float* loss, unsigned* counter, void* stream);
size_t dagnn_class_hits_bytes(int64_t B, int from_logits);
int dagnn_class_hits(const float* logits, int64_t ld, const int64_t* tok, int64_t B, int C, const void* targ, int targ_kind,
                     void* work, size_t work_bytes, unsigned* counter, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The loss launch of a training step with the epoch's bookkeeping in it (csrc/loss.hip; `train()` of
 * ogbg-code/main_pyg.py:39-88 and main_pyg_lp.py:43-74: `loss_accum += loss.item()`, the argmax of the training logits and
 * the evaluator's counts, per step).
 *
 * dagnn_seq_ce_step: dagnn_seq_ce - same arguments up to `loss`, the same kernel and row stage (csrc/rows_dev.h), same
 *   counter protocol: loss and dlogits are dagnn_seq_ce's bits - and in the same launch
 *     tok [B, S] int64: each row's argmax in the order stated above dagnn_heads_argmax (lowest column among equals, a NaN
 *       beats every number, -0 == +0): what dagnn_rows_argmax gives;
 *     epoch_sum [1] float64 += (double)loss and epoch_steps [1] int64 += 1, by one thread of the workgroup that finishes
 *       last: launches of one stream are ordered, so the sum is `loss_accum += loss.item()` in step order, bit for bit;
 *     with ref_ids != NULL: counts [graph_offset + g, 4] int32 = dagnn_seq_f1_counts of the B graphs from tok, eos_id,
 *       ref_ids [B, R >= 1] and ref_extra [B] (may be NULL), written by the last workgroup.  counts [counts_rows, 4] is
 *       16-byte aligned; graph_offset + B > counts_rows returns DAGNN_ENOSPC before anything is launched.  ref_ids == NULL
 *       skips the metric (R >= 1 and graph_offset >= 0 are still checked).
 * dagnn_class_ce_step: dagnn_class_ce likewise (targets int64 / float32 / float64 by `targ_kind`), plus tok [B] int64 (the
 *   row argmax), epoch_hits [2] int64 += (hits, labelled) by dagnn_class_hits' rules (a NaN target is unlabelled; target
 *   and prediction are compared as values), epoch_sum and epoch_steps as above.
 * The epoch words are the caller's: zero them to start an epoch, read them once at its end; 8-byte aligned.  counter [1]
 * device word, zero before the first call (the kernel leaves it zero).  No allocation, no synchronisation, no float
 * atomics: bitwise repeatable.
 * ---------------------------------------------------------------------------------------- */
int dagnn_seq_ce_step(const float* logits, int64_t ld, const int64_t* y, int B, int S, int V, float* dlogits, int64_t ld_dlogits,
                      float* row_loss, float* loss, int64_t* tok, int64_t eos_id, const int32_t* ref_ids, int R,
                      const int32_t* ref_extra, int32_t* counts, int64_t counts_rows, int64_t graph_offset, double* epoch_sum,
                      int64_t* epoch_steps, unsigned* counter, void* stream);
int dagnn_class_ce_step(const float* logits, int64_t ld, const void* targ, int targ_kind, int B, int C, float* dlogits,
                        int64_t ld_dlogits, float* row_loss, float* loss, int64_t* tok, int64_t* epoch_hits, double* epoch_sum,
                        int64_t* epoch_steps, unsigned* counter, void* stream);

/* ------------------------------------------------------------------------------------------
 * The device-resident graph store (csrc/store.hip; dagnn_amd/store.py): a dataset of raw ogbg-code2 graphs packed once
 * into int32 arrays, and any batch of it - the collation of ogbg-code/tg/dataloader.py:13-35 over graphs that went through
 * `augment_edge2` (utils2.py:31-79) and `add_order_info_01` (src/utils_dag.py:39-52) - written by ONE launch.
 *
 * Packed form (G graphs; every pointer a device pointer): node_ptr / edge_ptr / tok_ptr [G+1] int64 (offsets of a graph's
 * nodes, AST edges and attributed nodes); per node x [., 2], depth, layer_f, layer_b int32; per AST edge src, dst int32
 * (node ids inside the graph); per attributed node tok int32 (its id inside the graph, ascending) - next-token edge k of a
 * graph is (tok[k], tok[k+1]); per graph depth_max int32, y_arr [G, S] int32, ref_ids [G, R] int32, ref_extra [G] int32.
 *
 * The batch: idx [B] int64 graph ids (any order, repeats allowed; the CALLER has checked them against G) and
 * offsets [3, ld_offsets] int64, rows (node, AST edge, next-token edge) of B+1 exclusive prefix sums over the batch's
 * graphs: graph slot b owns nodes [node[b], node[b+1]) and edges [ast[b] + nxt[b], ast[b+1] + nxt[b+1]), its AST edges in
 * stored order first.  N = node[B], E = ast[B] + nxt[B].
 *
 * Outputs, each written exactly over its extent, every word by one thread (no atomics, no hand-offs; work is divided by
 * OUTPUT element, so a batch of one large graph uses as many threads as a batch of many small ones): out_x [N, 2] int64
 * (one 16-byte store per row), out_depth [N] int64 (`node_depth` [N, 1]), out_edge_index [2, E] int64 (shifted by the
 * slot's node offset), out_edge_attr [E, 2] fp32 (rows [0, 0] / [1, 0], one 8-byte store), out_batch [N] int64,
 * out_ptr [B+1] int64, out_index0 / out_index1 [N] int64 (= 0..N-1).  Optional, NULL = not written: out_layer_f /
 * out_layer_b [N] int64 (need layer_f / layer_b), out_llp [B] fp32 (`len_longest_path` = depth_max as a float),
 * out_y_arr [B, S] int64, out_ref_ids [B, R] int32 with out_ref_extra [B] int32 (both or neither).
 *
 * Arguments are validated before any HIP call: DAGNN_EINVAL for a NULL required pointer (the edge arrays only when
 * E > 0), a negative count, ld_offsets < B + 1, B = 0 with N > 0 or E > 0, an optional output without its source or with
 * S / R = 0, out_x not 16-byte or x / out_edge_attr not 8-byte aligned.  B = 0 returns at once.  No allocation, no
 * synchronisation.
 * ---------------------------------------------------------------------------------------- */
typedef struct dagnn_store_gather_args {
    const int64_t* node_ptr;
    const int64_t* edge_ptr;
    const int64_t* tok_ptr;
    const int32_t* x;
    const int32_t* depth;
    const int32_t* layer_f;
    const int32_t* layer_b;
    const int32_t* src;
    const int32_t* dst;
    const int32_t* tok;
    const int32_t* depth_max;
    const int32_t* y_arr;
    const int32_t* ref_ids;
    const int32_t* ref_extra;
    const int64_t* idx;
    const int64_t* offsets;
    int64_t ld_offsets;
    int64_t B;
    int64_t N;
    int64_t E;
    int64_t S;
    int64_t R;
    int64_t* out_x;
    int64_t* out_depth;
    int64_t* out_edge_index;
    float* out_edge_attr;
    int64_t* out_batch;
    int64_t* out_ptr;
    int64_t* out_index0;
    int64_t* out_index1;
    int64_t* out_layer_f;
    int64_t* out_layer_b;
    float* out_llp;
    int64_t* out_y_arr;
    int32_t* out_ref_ids;
    int32_t* out_ref_extra;
} dagnn_store_gather_args;
int dagnn_store_gather(const dagnn_store_gather_args* args /* host */, void* stream);

/* -------------------------------------------------------------------------------------------
 * The device-resident store of a D-VAE data set (csrc/dvae_store.hip; host side dagnn_amd/dvae_store.py): a batch of
 * ENAS / BN graphs - what `Batch.from_data_list` (dvae/batch.py:26-146) makes of the graphs of `decode_ENAS_to_pygraph` /
 * `decode_BN_to_pygraph` (dvae/util.py:290-385), plus the decoder's schedule of `loss()` (models_pyg.py:405-420) - written
 * by ONE launch.
 *
 * Packed form (M graphs of exactly n vertices, n <= 32, every edge u -> v with u < v; every pointer a device pointer;
 * [M, n] int32 row-major): types; preds (bit u of word v: the edge u -> v); succs, its transpose (bit v of word u: the same
 * edge); layer_f / layer_b (longest-path layer over the edges / the reversed edges); y [M] fp32 (optional).  Mask words are
 * read as UNSIGNED: with 32 vertices bit 31 is an edge.
 *
 * The batch: idx [B] int64 graph ids (any order, repeats allowed; the CALLER has checked them against M) and offsets [B+1]
 * int64, the exclusive prefix sums of the graphs' edge counts; E = offsets[B].  N = B * n.
 *
 * Outputs, each written exactly over its extent, every word by one thread (no atomics; work is divided by OUTPUT element):
 * out_x [N, nvt] fp32 one-hot of the types; out_edge_index [2, E] int64, per graph slot source-major (source ascending,
 * then target ascending), shifted by b * n; out_bi_layer_index [2, 2, N] int64 ([d][0] the layer of direction d, [d][1]
 * the node id 0..N-1); out_batch [N] int64; out_ptr [B+1] int64 (= b * n).  Optional, NULL = not written: out_types /
 * out_preds [B, n] int32 (the decoder's schedule), out_y [B] fp32 (needs y).
 *
 * dagnn_dag_store_layers: layer_f[v] = 1 + max(layer_f[u]) over the predecessors u < v of v (0 without one), walking v
 * ascending; layer_b the same over succs, descending.  Bits at or above v in preds[v] (at or below u, or from n up, in
 * succs[u]) are ignored.
 *
 * Arguments are validated before any HIP call: DAGNN_EINVAL for a NULL required pointer (succs / out_edge_index only when
 * E > 0), a negative count, n outside [1, 32], nvt < 1, B = 0 with E > 0, E > B n (n - 1) / 2, out_preds without preds,
 * out_y without y.  B = 0 / M = 0 returns at once.  No allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------- */
typedef struct dagnn_dag_store_gather_args {
    const int32_t* types;
    const int32_t* preds;
    const int32_t* succs;
    const int32_t* layer_f;
    const int32_t* layer_b;
    const float* y;
    const int64_t* idx;
    const int64_t* offsets;
    int64_t B;
    int64_t n;
    int64_t nvt;
    int64_t E;
    float* out_x;
    int64_t* out_edge_index;
    int64_t* out_bi_layer_index;
    int64_t* out_batch;
    int64_t* out_ptr;
    int32_t* out_types;
    int32_t* out_preds;
    float* out_y;
} dagnn_dag_store_gather_args;
int dagnn_dag_store_gather(const dagnn_dag_store_gather_args* args /* host */, void* stream);
int dagnn_dag_store_layers(const int32_t* preds, const int32_t* succs, int64_t M, int n, int32_t* layer_f, int32_t* layer_b,
                           void* stream);

/* -------------------------------------------------------------------------------------------
 * The D-VAE performance predictor (csrc/predictor.hip; dvae/train.py:184-191, 243-250, bayesian_optimization/bo.py:250-286):
 *   y_pred = W2 tanh(W1 mu + b1) + b2   with W1 [hs, nz], b1 [hs], W2 [1, hs], b2 [1], read in place on every call.
 * 1 <= nz <= DAGNN_PREDICTOR_MAX_NZ, 1 <= hs <= DAGNN_PREDICTOR_MAX_HS; any other width is DAGNN_EINVAL.
 *
 * dagnn_predictor_mse: ONE launch.  mu [B, nz] fp32 with row pitch ld_mu >= nz, y [B] fp32 -> y_pred [B] and
 *   want_grads == 0:  out [1] = loss = sum_b (y_pred_b - y_b)^2                                   (dmu must be NULL)
 *   want_grads != 0:  out [hs nz + 2 hs + 2] = d W1 [hs, nz] | d b1 [hs] | d W2 [hs] | d b2 | loss,  the gradients of the loss
 *                     for an upstream gradient of 1; dmu [B, nz] contiguous, or NULL to skip it.
 *   y_pred and the loss are the same bits in both forms.  A workgroup owns tiles of DAGNN_PREDICTOR_ROWS rows; `work` (4-byte
 *   aligned, >= dagnn_predictor_mse_bytes(B, nz, hs, want_grads) bytes, any content) takes one partial of `out` per workgroup,
 *   which the last workgroup in - an integer ticket on `counter` - adds in workgroup order.  counter [1]: device word, zero
 *   before the first call (the kernel leaves it zero).
 * dagnn_predictor_forward: pred [M] of the rows of Z [M, nz] (row pitch ld_z >= nz), many workgroups over the rows; a row has
 *   the arithmetic of dagnn_predictor_mse, in the same order: the same bits.  M = 0 returns at once.
 * dagnn_fit_sums: with p_i = (-pred_i - mean) / std (bo.py:253) in float64,
 *   out [6] float64 = sum p, sum y, sum p^2, sum y^2, sum p y, sum (p - y)^2   over pred [M] fp32 and y [M] (fp32, or float64
 *   with y_is_f64 != 0); `work`: 8-byte aligned, >= dagnn_fit_sums_bytes(M) bytes; counter as above.  One launch.
 * No allocation, no synchronisation, no float atomics, every sum in one fixed order: bitwise repeatable.
 * ---------------------------------------------------------------------------------------- */
#define DAGNN_PREDICTOR_MAX_NZ 128
#define DAGNN_PREDICTOR_MAX_HS 1024
#define DAGNN_PREDICTOR_ROWS 8
size_t dagnn_predictor_mse_bytes(int B, int nz, int hs, int want_grads);
int dagnn_predictor_mse(const float* mu, int64_t ld_mu, const float* y, int B, int nz, int hs, const float* W1, const float* b1,
                        const float* W2, const float* b2, float* y_pred, float* out, float* dmu, void* work, size_t work_bytes,
                        unsigned* counter, int want_grads, void* stream);
int dagnn_predictor_forward(const float* Z, int64_t ld_z, int64_t M, int nz, int hs, const float* W1, const float* b1,
                            const float* W2, const float* b2, float* pred, void* stream);
size_t dagnn_fit_sums_bytes(int64_t M);
int dagnn_fit_sums(const float* pred, const void* y, int y_is_f64, int64_t M, double mean, double std, double* out, void* work,
                   size_t work_bytes, unsigned* counter, void* stream);

/* The BIC score of Bayesian-network structures on a table of discrete samples (csrc/bn_score.hip): the target y of the
 * D-VAE's BN data set and the objective of its BO loop - what the reference obtains from one R process per structure
 * (bayesian_optimization/evaluate_BN.py: bnlearn's score(net, data), type "bic").
 *
 * Data: S samples of n_var <= DAGNN_BN_MAX_VARS discrete variables, variable i with values in [0, cards[i]), cards[i] in
 * 1..255, S < 2^31; on the device column-major, one byte per value: value (s, i) at cols[i * ld + s], ld >= S a multiple of
 * 16, cols 16-byte aligned, the padding bytes zero.  A structure is n_var parent masks: bit j of parents[m * n_var + i] is
 * the arc j -> i (bits at or above n_var are ignored; the masks of one structure must describe a DAG - this is NOT checked,
 * a cyclic structure gets the number the formula gives).  With q_i the product of the parents' cardinalities (1 without a
 * parent; every configuration counts, observed or not), N_ijk the samples with parent configuration j and x_i = k, and N_ij
 * the sum of N_ijk over k:
 *     family_i = sum over (j, k) with N_ijk > 0 of N_ijk (log N_ijk - log N_ij)  -  0.5 log(S) q_i (cards[i] - 1)
 *     score[m] = sum over i of family_i
 * Counts are int32, everything after them float64, added in one fixed order (cells ascending through a fixed tree, then the
 * families in node order; no float atomics): scores are bitwise equal from run to run, under any permutation of the samples
 * and on both staging paths.
 *
 * Capacity: a family's count table holds at most DAGNN_BN_TABLE_CELLS cells.  A structure with a family of q_i cards[i] cells
 * beyond that is NOT scored: its score is NaN and *n_over (device int32, zeroed by the caller) is incremented once for the
 * structure.  `valid` (may be NULL) marks structures to skip: valid[m] == 0 gives NaN and does not count in *n_over.
 *
 * stage: DAGNN_BN_STAGE_LDS - a workgroup copies the table (n_var * ld bytes) into LDS once and scores many structures from
 * it; refused (DAGNN_EINVAL) when the bn_stage_fits query says 0.  DAGNN_BN_STAGE_GLOBAL - the columns are read from global
 * memory.  DAGNN_BN_STAGE_AUTO - LDS when it fits.
 *
 * The rows_to_parents entry turns R dense decoder rows (types / preds [R, n] int32, preds as predecessor bitmasks, nv [R];
 * 3 <= nvt <= n <= 32) into parent masks [R, nvt - 2] and valid [R]: a row is valid under the reference's BN rules (exactly nvt
 * vertices, every type in [0, nvt) exactly once, one start and one end type); the first and last vertex are dropped and a
 * middle vertex becomes the variable given by the rank of its type among the middle types (np.argsort in
 * decode_igraph_to_BN_adj, dvae/util.py:388-394).  Invalid rows get zero masks and valid = 0.
 *
 * Borrowed pointers, the caller's stream, no allocation, no synchronisation; arguments are validated before any HIP call
 * (DAGNN_EINVAL). */
#define DAGNN_BN_TABLE_CELLS 8192
#define DAGNN_BN_MAX_VARS 30
#define DAGNN_BN_STAGE_AUTO 0
#define DAGNN_BN_STAGE_LDS 1
#define DAGNN_BN_STAGE_GLOBAL 2
typedef struct dagnn_bn_data {
    const uint8_t* cols;
    int64_t ld;
    int64_t S;
    int32_t n_var;
    int32_t reserved;
    int32_t cards[DAGNN_BN_MAX_VARS];
} dagnn_bn_data;
int dagnn_bn_stage_fits(const dagnn_bn_data* d);   /* 1 / 0, DAGNN_EINVAL for a bad descriptor */
int dagnn_bn_score(const dagnn_bn_data* d, const uint32_t* parents, const int32_t* valid, int64_t M, int stage, double* scores,
                   int32_t* n_over, void* stream);
int dagnn_bn_rows_to_parents(const int32_t* types, const int32_t* preds, const int32_t* nv, int64_t R, int n, int nvt,
                             int start_type, int end_type, uint32_t* parents, int32_t* valid, void* stream);

/* The sparse GP of the D-VAE BO loop (csrc/sgp.hip): what `SparseGP.predict` and `batched_greedy_ei` of
 * bayesian_optimization/sparse_gp.py evaluate on every grid row.  Kernel: k(x, z_m) = sf exp(-1/2 sum_c (x_c - z_mc)^2 / ls_c)
 * over M <= DAGNN_SGP_MAX_M inducing rows of d <= DAGNN_SGP_MAX_D columns.
 *
 * dagnn_sgp_project: for the N rows of X (fp32, row pitch ld_x >= d) the tile k(X, z) is built in LDS and multiplied on the
 * fp32 matrix cores by a matrix T [Mt, M], Mt <= 2 DAGNN_SGP_MAX_M; k never goes to memory.  Derived operands, all fp32:
 *     zt [d, ld_z]  the inducing rows transposed (zt[c * ld_z + m] = z[m][c]),   inv_ls [d] = 1 / ls,
 *     Tt [M, ld_t]  T transposed (Tt[k * ld_t + j] = T[j][k]),                   a [M].
 * With u = T k(x, z), each output may be NULL:
 *     U    [N, ld_u]: the columns j >= u_col0 of u at U[x * ld_u + j - u_col0]  (ld_u >= Mt - u_col0),
 *     var0 [N] = sf - sum over j <  split of u_j^2,      var1 [N] = sf - sum over split <= j < Mt of u_j^2,
 *     mean [N] = k(x, z) . a   (a may be NULL only with mean).
 * Every sum has one fixed order and there is no atomic: the outputs are bitwise repeatable, and a row's value does not
 * depend on N or on the other rows.
 *
 * dagnn_sgp_ei_step: one greedy step over the whole grid and the argmin behind it.  With U != NULL the launch first appends
 * a chosen point p [d] to the factor: for every row, w = (k(x, p) - U[x, 0:Me] . c) * inv_delta (c [Me] = L_e^-1 k(p, z_e) and
 * delta from the host, in fp32), U[x, Me] = w (ld_u > Me) and r[x] -= w^2.  Then per row, in float64 from the fp32 mean[x] and
 * r[x]: mode DAGNN_SGP_ARGMIN_MEAN: the key is mean[x]; mode DAGNN_SGP_ARGMIN_EI: with v = r[x], s = (incumbent - mean) / sqrt(v),
 *     log EI = log((incumbent - mean) ratio(s) + sqrt(v)) - 1/2 log(2 pi) - 1/2 s^2,
 *     ratio(s) = -(1/s - 1/s^3 + 3/s^5 - 15/s^7) for s < -10, else (1/2 erfc(-s / sqrt 2)) / (exp(-s^2 / 2) / sqrt(2 pi)),
 * the key is -log EI, NaN where v is not positive.  keys (may be NULL) [N] receives every key.  result [4] int64:
 * {argmin as numpy.argmin gives it - the lowest index wins a tie, the first NaN wins -, rows whose v is not positive (mode EI),
 *  the bits of the winning key, 0}.  Workgroup partials are merged by the last workgroup to draw a ticket on `counter` (a
 * zeroed device word, left zero); work: dagnn_sgp_ei_step_bytes(N) bytes, 8-byte aligned.
 *
 * Borrowed pointers, the caller's stream, no allocation, no synchronisation; arguments are validated before any HIP call. */
#define DAGNN_SGP_MAX_M 512
#define DAGNN_SGP_MAX_D 128
#define DAGNN_SGP_MAX_Q 128
#define DAGNN_SGP_ARGMIN_MEAN 0
#define DAGNN_SGP_ARGMIN_EI 1
int dagnn_sgp_project(const float* X, int64_t ld_x, int64_t N, int d, int M, const float* zt, int64_t ld_z, const float* inv_ls,
                      float sf, const float* Tt, int64_t ld_t, int Mt, int split, const float* a, float* U, int64_t ld_u,
                      int u_col0, float* var0, float* var1, float* mean, void* stream);
size_t dagnn_sgp_ei_step_bytes(int64_t N);
int dagnn_sgp_ei_step(int mode, int64_t N, const float* mean, float* r, double incumbent, const float* X, int64_t ld_x, int d,
                      const float* inv_ls, float sf, const float* p, float* U, int64_t ld_u, int Me, const float* c,
                      float inv_delta, double* keys, int64_t* result, void* work, size_t work_bytes, unsigned* counter,
                      void* stream);

/* One training step of that sparse GP (csrc/sgp_train.hip): the energy of a minibatch (getContributionToEnergy with the cavity
 * factor c = (n_points - 1) / n_points; `SparseGP.energy`) and its gradients, all float64, by analytic adjoints of the whitened
 * form: Kzz = k(z, z) + 1e-3 sf I = L L^T, C = Lp^T L, A = C^T C, S_c = I + c A, S_1 = I + A, t = L^T m, U = L^-1 k(X, z)^T,
 *     v_i = sf - |U_i|^2 + U_i^T S_c^-1 U_i,   mean_i = c U_i^T S_c^-1 t,   out_i = |v_i| + exp(lvar_noise),
 *     E = b (-1/2 logdet S_c + 1/2 c^2 t^T S_c^-1 t - c (-1/2 logdet S_1 + 1/2 t^T S_1^-1 t))
 *         + sum_i (-1/2 log(2 pi out_i) - 1/2 (y_i - mean_i)^2 / out_i).
 * X [b, d] (row pitch ld_x >= d), y [b], lls [d], lsf [1], z [M, d], mP [M], Lp [M, M], lvar_noise [1] are read in place;
 * E [1], g_lls [d], g_lsf [1], g_z [M, d], g_m [M], g_Lp [M, M], g_noise [1] are written.  M <= DAGNN_SGP_MAX_M,
 * d <= DAGNN_SGP_MAX_D, 1 <= b <= 2^24, n_points >= 1.  work: dagnn_sgp_energy_grad_bytes(M, d, b) bytes (0 for a shape out of
 * range), 8-byte aligned.  The three Cholesky factorisations run a fixed number of steps: a pivot that is not positive (or
 * NaN) becomes NaN - the outputs are then NaN - and adds one to *fail, a device word the caller zeroes and reads when it
 * likes.  The products run on v_mfma_f64_16x16x4_f64; every sum has one fixed order and there is no floating-point atomic:
 * two calls on the same inputs are bitwise equal.  Borrowed pointers, the caller's stream, no allocation, no synchronisation. */
size_t dagnn_sgp_energy_grad_bytes(int M, int d, int64_t b);
int dagnn_sgp_energy_grad(const double* X, int64_t ld_x, const double* y, int64_t b, int M, int d, double n_points,
                          const double* lls, const double* lsf, const double* z, const double* mP, const double* Lp,
                          const double* lvar_noise, double* E, double* g_lls, double* g_lsf, double* g_z, double* g_m,
                          double* g_Lp, double* g_noise, void* work, size_t work_bytes, unsigned* fail, void* stream);

/* The refinement of that sparse GP's greedy proposals (csrc/sgp_refine.hip; the reference's `global_optimization`,
 * sparse_gp.py:24-43, is one L-BFGS-B run of scipy from the best grid row): S <= DAGNN_SGP_REFINE_MAX_STARTS starts advanced
 * in lock-step by a projected L-BFGS with DAGNN_SGP_REFINE_HISTORY curvature pairs and a halving Armijo search, everything in
 * float64.  The objective at a column of points x_s, over the Me = M + j rows of ze [Me, d] (the inducing rows, then the chosen
 * points; zet [d, ld_zt >= Me] holds the same rows transposed, zet[c ld_zt + m] = ze[m][c]), with k_m = sf exp(-1/2 sum_c (x_c - ze_mc)^2 inv_ls_c):
 *     mean = sum_{m < M} a_m k_m,   v = sf - |T k|^2,   T [Me, Me] with row pitch ld_t (tri != 0: lower triangular, the tiles
 *     above the diagonal are skipped),
 * mode DAGNN_SGP_REFINE_MEAN: f = mean (T is not read); mode DAGNN_SGP_REFINE_EI: f = -log EI(mean, v, incumbent), the branch
 * expression of dagnn_sgp_ei_step with its partials (NaN where v or the argument of the logarithm is not positive, -inf where
 * exp(-s^2 / 2) underflows).  K = k(x, ze) [Me, S], U = T K and C = T^T U are tile products on v_mfma_f64_16x16x4_f64; every
 * sum has one fixed order and there is no floating-point atomic, no ticket and no spinning: two calls are bitwise equal.
 *
 * dagnn_sgp_refine_eval: one evaluation.  X [S, d]; out [S, 4 + 2 d]: f, mean, v, 0, d mean / dx [d], d v / dx [d].
 * dagnn_sgp_refine_run: X0 [S, d] (clipped into [lower, upper] on entry); nstart (a device word, may be NULL: S) - the starts
 * from *nstart on are dead.  max_evals ticks are enqueued without a look at the device, a tick being the two products (mode
 * EI only) and one launch that reduces, advances every start by one transition and builds the next column of K.  out
 * [2 + d + 3 S]: the best start (-1: no start has a finite objective), its objective, its point [d], then per start the status
 * (DAGNN_SGP_REFINE_*), the evaluations it used and its objective, as doubles; xs (may be NULL) [S, d]: every start's accepted
 * point (NaN for a dead start).
 * work: dagnn_sgp_refine_bytes(Me, d, S) bytes (0 for a shape out of range), 8-byte aligned.  Borrowed pointers, the caller's
 * stream, no allocation, no synchronisation; arguments are validated before any HIP call. */
#define DAGNN_SGP_REFINE_MAX_STARTS 32
#define DAGNN_SGP_REFINE_HISTORY 8
#define DAGNN_SGP_REFINE_MEAN 0
#define DAGNN_SGP_REFINE_EI 1
#define DAGNN_SGP_REFINE_RUNNING 0
#define DAGNN_SGP_REFINE_CONVERGED 1
#define DAGNN_SGP_REFINE_STALLED 2
#define DAGNN_SGP_REFINE_BUDGET 3
#define DAGNN_SGP_REFINE_DEAD 4
size_t dagnn_sgp_refine_bytes(int Me, int d, int S);
int dagnn_sgp_refine_eval(int mode, int S, int d, int M, int Me, const double* X, const double* ze, const double* zet,
                          int64_t ld_zt, const double* inv_ls, double sf, const double* a, const double* T, int64_t ld_t, int tri, double incumbent, double* out, void* work,
                          size_t work_bytes, void* stream);
int dagnn_sgp_refine_run(int mode, int S, int d, int M, int Me, const double* X0, const int* nstart, const double* lower,
                         const double* upper, const double* ze, const double* zet, int64_t ld_zt, const double* inv_ls, double sf,
                         const double* a, const double* T,
                         int64_t ld_t, int tri, double incumbent, int max_evals, double* out, double* xs, void* work,
                         size_t work_bytes, void* stream);

/* The tail of the reference's training step - `clip_grad_norm_(model.parameters(), clip)` + `optim.Adam.step()`
 * (ogbg-code/main_pyg.py:63-65,179) - over a table of fp32 tensors (csrc/optim.hip).  dagnn_grad_norm: the 2-norm of up to
 * DAGNN_MAX_OPT_TENSORS gradients (`partial`: scratch of dagnn_opt_chunks() floats; `accumulate` != 0 adds the tensors' sum of
 * squares to *norm_sq from an earlier call - tables beyond the limit) as a device float, summed in a fixed order.
 * dagnn_clip_adam: Adam's update (no amsgrad, L2 weight decay, bias-corrected moments; `step` = 1, 2, ... of this update) with
 * the gradient scaled by min(1, max_norm / (*norm + 1e-6)) as it is read (max_norm <= 0: no clipping, norm may be NULL);
 * gradients are not modified.  Nothing synchronises; every pointer is a borrowed device pointer. */
#define DAGNN_MAX_OPT_TENSORS 48
typedef struct { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t numel; } dagnn_opt_tensor;
int64_t dagnn_opt_chunks(const int64_t* numel /* host */, int n);
int dagnn_grad_norm(const float* const* grads /* host array of device pointers */, const int64_t* numel /* host */, int n,
                    float* partial, int64_t partial_len, float* norm_sq /* device [1] */, int accumulate, float* norm /* device [1] */,
                    void* stream);
int dagnn_clip_adam(const dagnn_opt_tensor* tensors /* host */, int n, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int64_t step, float max_norm, const float* norm /* device */, void* stream);

/* Guard of the host side's derived-weight caches (dagnn_amd/core.py: ParamGuard; nothing in the reference corresponds - its
 * modules read their parameters on every call).  A fingerprint of up to DAGNN_MAX_FP_TENSORS fp32 / int32 tensors: 1024 words
 * spread evenly over each, weighted by position, summed mod 2^64.  mode 0 writes fp[t]; mode 1 compares with fp[t] and ORs
 * `bit` into *err (device word) for every tensor whose fingerprint moved - read back with the pass's other error words, no
 * synchronisation.  One launch, one workgroup per tensor. */
#define DAGNN_MAX_FP_TENSORS 96
int dagnn_param_fingerprint(const void* const* ptrs /* host array of device pointers */, const int64_t* numel /* host */, int n,
                            uint64_t* fp /* device [n] */, int mode, int* err /* device */, int bit, void* stream);

/* Test utility for the co-residency rule of the persistent kernels (engine.reserved_cus): occupies `num_wgs` workgroups of
 * `threads` threads for `ticks` of the 100 MHz constant clock (bounded: at most 2^31 ticks) on `stream` - a stand-in for the
 * kernels of a collective that runs next to a training pass.  Touches no memory besides `sink` (one float, may be NULL). */
int dagnn_debug_occupy(int num_wgs, int threads, int64_t ticks, float* sink, void* stream);

/* ------------------------------------------------------------------------------------------
 * Attention weights of a finished evaluation pass, per ORIGINAL edge id (`DAGNN.attention`; what a hook on the reference's
 * conv modules would record: ogbg-code/model/dagnn.py:297-310, 366-373, 399-406, dvae/dagnn.py:109-145, dvae/dagnn_bn.py).
 * A cell is one (direction, stacked layer).  Every state is written exactly once by the recurrence, so the final states
 * are the states the aggregation saw.  For every CSR slot s of the plan's direction `dir` (target row t, source u = col[s],
 * edge id e = eidx[s], R = plan->num_edge_feats):
 *   additive (mode 0):        score_s = w_key . key[u, :key_dim] + vid_key[u mod vid_mod] + sum_r edge_gain[r] eattr[s, r]
 *                             logit_e = score_s + w_query . query[t, :query_dim] + vid_query[t mod vid_mod] + *bias
 *   multiplicative (mode 1):  logit_e = score_s = sum_k query[t, k] (key[u, k] + sum_r edge_mat[k, r] eattr[s, r] + edge_vec[k]),
 *                             k < key_dim, with `query` / `key` the PROJECTED rows (attn_linl / attn_linr incl. bias: one
 *                             dagnn_gemm_nt_bias each) - w_key, w_query, bias, vid_* are not read
 *   alpha_e = exp(score_s - max_seg) / (sum_seg exp(score - max_seg) + 1e-16)                      (PyG's softmax)
 * (mode 0: the query part and the bias are common to a segment and cancel in alpha; only `logit` needs them.)
 * Every edge lies in exactly one segment per direction, so alpha[c, e] (and logit[c, e]) is written exactly once for every
 * e < E: plain stores, no atomics, no [E, H] intermediate.  Launches: mode 0 - one kernel for the node scores of ALL cells
 * (a wave per row, float4 loads where pointer, pitch and width allow), one for the segment softmax of ALL cells (a wave per
 * target row, lanes over slots, running max / sum beyond 64 slots); mode 1 - one kernel (a wave per target row).
 * Limits (violations: DAGNN_EINVAL before any launch): 1 <= num_cells <= DAGNN_ATTN_MAX_CELLS, plan->N and plan->E below
 * 2^31, 1 <= key_dim <= ld_key, query_dim <= ld_query, NULL alpha / key_score (mode 0) / key / w_key (mode 0) with E > 0,
 * NULL query_score with `logit` and a query in mode 0, dir outside {0, 1}, vid pointers with vid_mod < 1.  E == 0 or N == 0:
 * returns 0 without a launch.  No allocation, no synchronisation; borrowed pointers; the caller's stream.
 * ---------------------------------------------------------------------------------------- */
#define DAGNN_ATTN_MAX_CELLS 16
typedef struct dagnn_attn_cell {
    const float* key;        /* [N, ld_key]: rows the keys are read from (states of this cell, node inputs, or projected keys) */
    const float* w_key;      /* [key_dim] (mode 0) */
    const float* query;      /* [N, ld_query] or NULL (self-attention; or no logit wanted) */
    const float* w_query;    /* [query_dim] (mode 0) */
    const float* vid_key;    /* [vid_mod] or NULL */
    const float* vid_query;  /* [vid_mod] or NULL */
    const float* edge_gain;  /* mode 0: [R] or NULL; mode 1: edge_mat [key_dim, R] row-major or NULL */
    const float* edge_vec;   /* mode 1: [key_dim] or NULL */
    const float* bias;       /* mode 0: [1] on the device, the constant of the logit, or NULL */
    int ld_key, key_dim, ld_query, query_dim, dir, pad_;
} dagnn_attn_cell;
typedef struct dagnn_attn_args {
    dagnn_attn_cell cell[DAGNN_ATTN_MAX_CELLS];
    int num_cells, mode, vid_mod, pad_;
    float* key_score;        /* scratch [num_cells, N] (mode 0) */
    float* query_score;      /* scratch [num_cells, N] (mode 0 with `logit`) */
    float* alpha;            /* [num_cells, E] */
    float* logit;            /* [num_cells, E] or NULL */
} dagnn_attn_args;
int dagnn_attention_weights(const dagnn_plan* plan /* host */, const dagnn_attn_args* args /* host */, void* stream);

/* Introspection (tests, and the host-side read-back of the lock-step schedule): byte offsets of the
 * plan's arrays from `plan->data`, into a host array of 26 entries: [node_ptr, edge_ptr, depth0,
 * depth1, order0, order1, lstart0, lstart1, rowptr0, rowptr1, col0, col1, eattr0, eattr1, items,
 * total, blptr0, blptr1, rowrec0, rowrec1, slot0, slot1, eidx0, eidx1, blsplit0, blsplit1].  slot_d [N]: rowrec
 * slot of every node; eidx_d [E]: original edge id (column of edge_index) of every CSR slot; blsplit_d [N+2]: per
 * batch-level layer the first slot of the rows of the DEEP graphs of direction d (depth > thr_d, int32 header word
 * 5 + d of the plan; thr_d = 1 + the last layer with more than 14 rows) - inside a layer the shallow graphs' rows
 * come first.  blptr_d holds N+2 int32: the offsets of the
 * batch-level topological layers of direction d (entries 0..T_d) and T_d itself at index N+1. */
int dagnn_plan_layout(int64_t N, int64_t E, int64_t B, int num_edge_feats, int64_t* offsets26 /* host */);

#ifdef __cplusplus
}
#endif
#endif /* DAGNN_HIP_H */
