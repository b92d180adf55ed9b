// loss.hip - the training loss of the TOK and LP tasks and its gradient in ONE launch, with or without the step's share of
// the epoch's bookkeeping: four entry points, one kernel template, one row stage (rows_dev.h: ce_row).
//
// Reference paths replaced:
//   dagnn_seq_ce         the caller-side loss loop of ogbg-code/main_pyg.py:55-60 -
//                            loss = 0;  for i in range(len(pred_list)): loss += multicls_criterion(pred_list[i].to(torch.float32), batch.y_arr[:, i])
//                            loss = loss / len(pred_list)
//                        with multicls_criterion = torch.nn.CrossEntropyLoss() (main_pyg.py:37): the mean over the batch of
//                        -log softmax(pred)[y], per head, then the mean over the S heads.  Under autograd that is 5 x
//                        (log-softmax, nll, their two backward kernels, a reduction, the additions) = ~50 launches of 2-7 us
//                        each on a step that is bound by the host's launch rate.
//   dagnn_class_ce       `CrossEntropyLoss()(pred, targ.to(torch.long))` on ONE [B, C] head (main_pyg_lp.py:56-58): the S = 1
//                        instance of the same kernel (same sums in the same order, same error analysis: DESIGN.md 4i), except
//                        that the target is read as what the reference hands over - int64, or the float tensor it
//                        concatenates - and truncated toward zero in the kernel instead of by a launch in front of it.
//   dagnn_seq_ce_step    per step of `train()` (main_pyg.py:39-88): the loss loop, `loss_accum += loss.item()` (a host
//   dagnn_class_ce_step  synchronisation), the S `torch.argmax` + `cat` over the training logits, `decode_arr_to_seq` per row
//                        and the evaluator's set arithmetic (TOK) / the two copies to the host and `_eval_acc` (LP,
//                        main_pyg_lp.py:43-74).  The loss kernel already reads every logit of the step and already computes
//                        every row's maximum; the workgroup that draws the last ticket already sees every row.  So the STEP
//                        instances also leave tok [B, S] / [B] - each row's argmax in the order of rows_dev.h, a by-product
//                        of the first pass over the row - and, in the last workgroup, the epoch's loss sum in float64, its
//                        step counter and the F1 counts of the B graphs (f1_counts_of_graph, a thread per graph) at their
//                        place in the epoch's table (TOK) / the (hits, labelled) pair of hits_compare added into the epoch's
//                        pair (LP).  One launch per step, one read per epoch.
//
// One workgroup per (graph, head) row of the [B, S * V] logits - the S heads' outputs side by side, as DAGNN._heads lays them
// out - computes the row's loss AND the row of d loss / d logits = (softmax - onehot) / (B S); the workgroup that finishes
// last adds the B S row losses in index order (no atomics on values: the loss is bitwise reproducible).  Every head sees the
// same B rows, so the mean of the per-head means is the mean over all B S rows.  Targets must lie in [0, V):
// CrossEntropyLoss's ignore_index (-100) does not occur in the reference's targets (y_arr holds vocabulary ids, utils.py:
// encode_seq_to_arr) and is not supported - an out-of-range target makes the loss NaN, loudly.  Tokens travel to the last
// workgroup as the row losses do: written before `__threadfence` and the ticket, read with agent-scope loads after it.
#include "rows_dev.h"

namespace {

enum { CE_SEQ = 0, CE_CLASS = 1 };   // TASK: how a row maps to (b, s), how its target is read, what the epoch keeps

struct CeArgs {
    const float* logits; long long ld;
    const void* targ; int kind;   // CE_SEQ: int64 y [B, S]; CE_CLASS: [B] of DAGNN_LP_* `kind`
    int B, S, V;                  // (CE_CLASS: S = 1, V = C)
    float* dlogits; long long ld_d;
    float* row_loss; float* loss;
    unsigned* counter;
    // STEP
    long long* tok;
    double* epoch_sum; long long* epoch_steps;
    long long eos; const int* ref_ids; int R; const int* ref_extra;   // CE_SEQ
    int* counts;                                                      // CE_SEQ: already moved to the step's first graph
    long long* epoch_hits;                                            // CE_CLASS
};

template <int TASK, bool STEP>
__global__ void __launch_bounds__(256) ce_kernel(CeArgs a) {
    __shared__ float red[4];
    __shared__ long long redp[4];       // (STEP)
    __shared__ long long redh[4][2];    // (STEP, CE_CLASS)
    __shared__ unsigned last;
    const int B = a.B, S = TASK == CE_SEQ ? a.S : 1, V = a.V, n = B * S;
    const int row = blockIdx.x, b = row / S, s = row - b * S;
    const int tid = threadIdx.x;
    const float* x = a.logits + (long long)b * a.ld + (long long)s * V;
    long long t;
    if constexpr (TASK == CE_SEQ) t = reinterpret_cast<const long long*>(a.targ)[row];
    else t = class_of(a.targ, a.kind, row);
    const float row_loss = ce_row<STEP>(x, V, t, 1.0f / ((float)B * (float)S), a.dlogits, (long long)b * a.ld_d + (long long)s * V,
                                        red, redp, STEP ? a.tok + row : nullptr);
    if (tid == 0) a.row_loss[row] = row_loss;
    if (!ce_finish(a.counter, n, &last)) return;
    // the last row in: every row's loss and token is visible
    if constexpr (STEP && TASK == CE_SEQ) {
        if (a.ref_ids)
            for (int g = tid; g < B; g += 256) {
                const long long* tk = a.tok + (long long)g * S;
                const auto load = [tk](int i) { return __hip_atomic_load(tk + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
                reinterpret_cast<int4*>(a.counts)[g] =
                    f1_counts_of_graph(load, S, a.eos, a.ref_ids + (long long)g * a.R, a.R, a.ref_extra ? a.ref_extra[g] : 0);
            }
    }
    long long hits = 0, labelled = 0;   // (STEP, CE_CLASS)
    const float l = ce_loss_sum(a.row_loss, n, red, [&](int j) {
        if constexpr (STEP && TASK == CE_CLASS)
            hits_compare(a.targ, a.kind, j, __hip_atomic_load(a.tok + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), hits,
                         labelled);
    });
    if constexpr (STEP && TASK == CE_CLASS) {
        hits = wave_sum(hits);
        labelled = wave_sum(labelled);
        if ((tid & 63) == 0) { redh[tid >> 6][0] = hits; redh[tid >> 6][1] = labelled; }
        __syncthreads();
    }
    if (tid == 0) {
        a.loss[0] = l;
        if constexpr (STEP) {
            a.epoch_sum[0] += (double)l;   // launches of one stream are ordered: `loss_accum += loss.item()` in step order
            a.epoch_steps[0] += 1;
        }
        if constexpr (STEP && TASK == CE_CLASS) {
            a.epoch_hits[0] += (redh[0][0] + redh[1][0]) + (redh[2][0] + redh[3][0]);   // (integers: exact in any order)
            a.epoch_hits[1] += (redh[0][1] + redh[1][1]) + (redh[2][1] + redh[3][1]);
        }
        a.counter[0] = 0u;   // ready for the next call
    }
}

// the checks the four entry points share, and the arguments they imply
int ce_args(CeArgs& a, const float* logits, int64_t ld, const void* targ, int kind, int B, int S, int V, float* dlogits, int64_t ld_d,
            float* row_loss, float* loss, unsigned* counter) {
    if (!logits || !targ || !row_loss || !loss || !counter || !lp_kind_ok(kind) || B <= 0 || S <= 0 || V <= 0 ||
        ld < (int64_t)S * V || (dlogits && ld_d < (int64_t)S * V))
        return DAGNN_EINVAL;
    if ((int64_t)B * S >= (1ll << 31)) return DAGNN_EINVAL;
    a = CeArgs{};
    a.logits = logits; a.ld = (long long)ld; a.targ = targ; a.kind = kind; a.B = B; a.S = S; a.V = V;
    a.dlogits = dlogits; a.ld_d = (long long)ld_d; a.row_loss = row_loss; a.loss = loss; a.counter = counter;
    return DAGNN_OK;
}

template <int TASK, bool STEP>
int ce_launch(const CeArgs& a, void* stream) {
    hipLaunchKernelGGL((ce_kernel<TASK, STEP>), dim3((unsigned)(a.B * a.S)), dim3(256), 0, (hipStream_t)stream, a);
    DAGNN_CHECK_LAUNCH();
    return DAGNN_OK;
}

}  // namespace

extern "C" int dagnn_seq_ce(const float* logits, int64_t ld, const int64_t* y, int B, int S, int V, float* dlogits, int64_t ld_d,
                            float* row_loss, float* loss, unsigned* counter, void* stream) {
    CeArgs a;
    if (const int rc = ce_args(a, logits, ld, y, DAGNN_LP_INT64, B, S, V, dlogits, ld_d, row_loss, loss, counter)) return rc;
    return ce_launch<CE_SEQ, false>(a, stream);
}

extern "C" int dagnn_class_ce(const float* logits, int64_t ld, const void* targ, int targ_kind, int B, int C, float* dlogits,
                              int64_t ld_d, float* row_loss, float* loss, unsigned* counter, void* stream) {
    CeArgs a;
    if (const int rc = ce_args(a, logits, ld, targ, targ_kind, B, 1, C, dlogits, ld_d, row_loss, loss, counter)) return rc;
    return ce_launch<CE_CLASS, false>(a, stream);
}

extern "C" int dagnn_seq_ce_step(const float* logits, int64_t ld, const int64_t* y, int B, int S, int V, float* dlogits,
                                 int64_t ld_d, float* row_loss, float* loss, int64_t* tok, int64_t eos_id, const int32_t* ref_ids,
                                 int R, const int32_t* ref_extra, int32_t* counts, int64_t counts_rows, int64_t graph_offset,
                                 double* epoch_sum, int64_t* epoch_steps, unsigned* counter, void* stream) {
    CeArgs a;
    if (const int rc = ce_args(a, logits, ld, y, DAGNN_LP_INT64, B, S, V, dlogits, ld_d, row_loss, loss, counter)) return rc;
    if (!tok || !epoch_sum || !epoch_steps || ((uintptr_t)epoch_sum & 7) || ((uintptr_t)epoch_steps & 7) || R < 1 || graph_offset < 0)
        return DAGNN_EINVAL;
    if (ref_ids) {
        if (!counts || ((uintptr_t)counts & 15) || counts_rows < 0) return DAGNN_EINVAL;
        if (graph_offset > counts_rows || (int64_t)B > counts_rows - graph_offset) return DAGNN_ENOSPC;
    }
    a.tok = reinterpret_cast<long long*>(tok); a.eos = (long long)eos_id;
    a.ref_ids = ref_ids; a.R = R; a.ref_extra = ref_extra;
    a.counts = ref_ids ? counts + 4 * graph_offset : nullptr;
    a.epoch_sum = epoch_sum; a.epoch_steps = reinterpret_cast<long long*>(epoch_steps);
    return ce_launch<CE_SEQ, true>(a, stream);
}

extern "C" int dagnn_class_ce_step(const float* logits, int64_t ld, const void* targ, int targ_kind, int B, int C, float* dlogits,
                                   int64_t ld_d, float* row_loss, float* loss, int64_t* tok, int64_t* epoch_hits, double* epoch_sum,
                                   int64_t* epoch_steps, unsigned* counter, void* stream) {
    CeArgs a;
    if (const int rc = ce_args(a, logits, ld, targ, targ_kind, B, 1, C, dlogits, ld_d, row_loss, loss, counter)) return rc;
    if (!tok || !epoch_hits || !epoch_sum || !epoch_steps || ((uintptr_t)epoch_hits & 7) || ((uintptr_t)epoch_sum & 7) ||
        ((uintptr_t)epoch_steps & 7))
        return DAGNN_EINVAL;
    a.tok = reinterpret_cast<long long*>(tok); a.epoch_hits = reinterpret_cast<long long*>(epoch_hits);
    a.epoch_sum = epoch_sum; a.epoch_steps = reinterpret_cast<long long*>(epoch_steps);
    return ce_launch<CE_CLASS, true>(a, stream);
}
