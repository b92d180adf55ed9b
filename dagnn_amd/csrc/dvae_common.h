// What the two D-VAE decoders (dvae_decode.hip: teacher forcing, dvae_sample.hip: sampling) ask of their argument
// structs alike.  dagnn_dvae_decode_args and dagnn_dvae_sample_args name the decoder's dimensions, aggregator and
// weights the same way, so each rule is written once over the struct type; what only one entry point has (B / G, the
// draws, outputs, workspaces, its own size limits) stays in its file.
#pragma once
#include "common.h"

// one 64-float-aligned region of a workspace: returns its offset and moves `at` past it
static inline int64_t dvae_take(int64_t& at, int64_t count) {
    const int64_t off = at;
    at += (count + 63) / 64 * 64;
    return off;
}

// The decoder's dimensions and the aggregator's admission rules (dagnn_dvae_decode_args in dagnn_hip.h).  A size query
// returns 0 and an entry point DAGNN_EINVAL where this fails.  The fields behind `agg` were appended one aggregator at
// a time: each is read only after the `agg` value that introduced it - and, for key_type, `bn` - has been
// established, so a caller's shorter, earlier struct never has memory behind it read.
template <typename Args>
static inline bool dvae_decoder_ok(const Args* a) {
    if (a->n < 2 || a->n > DAGNN_DVAE_MAX_N || a->hs <= 0 || a->L < 1 || a->L > DAGNN_MAX_STACKED || a->nvt <= 0 ||
        a->nvt > DAGNN_DVAE_MAX_TYPES || a->start_type < 0 || a->start_type >= a->nvt || (a->bn != 0 && a->bn != 1) ||
        a->edge_hidden <= 0 || a->vertex_hidden <= 0 || a->agg < DAGNN_DVAE_AGG_ATTN_H || a->agg > DAGNN_DVAE_AGG_ATTN_X)
        return false;
    if (a->agg == DAGNN_DVAE_AGG_GATED_SUM && (a->bn || !a->gate_w || !a->gate_b || !a->mapper_w)) return false;
    if (a->agg == DAGNN_DVAE_AGG_ATTN_X && (!a->bn || !a->key_type)) return false;
    return true;
}

// The weight pointers every launch dereferences (after dvae_decoder_ok: the aggregator's own tensors are checked there,
// but for attn_h's w_key, whose absence only the entry points refuse; vid_bias may be NULL).
template <typename Args>
static inline bool dvae_weights_ok(const Args* a) {
    if (!a->h0 || (a->agg == DAGNN_DVAE_AGG_ATTN_H && !a->w_key) || !a->av_w1 || !a->av_b1 || !a->av_w2 || !a->av_b2 ||
        !a->ae_w1 || !a->ae_b1 || !a->ae_w2 || !a->ae_b2)
        return false;
    for (int l = 0; l < a->L; ++l)
        if (!a->w_ih[l] || !a->w_hh[l] || !a->b_ih[l] || !a->b_hh[l]) return false;
    return true;
}
