"""ctypes binding of libdagnn_hip.so (the C ABI declared in include/dagnn_hip.h).

There is NO fallback: if the library cannot be loaded the product path raises.  Tensors are passed
as raw device pointers; torch only owns the memory and the stream.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

from . import build as _build

MAX_DIRS = 2
MAX_GROUPS = 4
MAX_READOUT_JOBS = 24      # DAGNN_MAX_READOUT_JOBS
ATTN_GRAD_MAX_JOBS = 16    # DAGNN_ATTN_GRAD_MAX_JOBS

DAGNN_OK = 0
EINVAL, ENOSPC = -22, -28
_ERRORS = {EINVAL: "DAGNN_EINVAL (bad argument)", ENOSPC: "DAGNN_ENOSPC (workspace too small)"}


class DagnnHipError(RuntimeError):
    pass


class OptTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_int64)]


class DfPackJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("out", C.c_void_p), ("aux", C.c_void_p), ("transposed", C.c_int32), ("rows", C.c_int32),
                ("cols", C.c_int32)]


class PoolJob(C.Structure):   # dagnn_pool_job
    _fields_ = [("h", C.c_void_p), ("ld_h", C.c_int32), ("width", C.c_int32), ("scope", C.c_int32), ("mode", C.c_int32),
                ("col_off", C.c_int32)]


class PoolBwdJob(C.Structure):   # dagnn_pool_bwd_job
    _fields_ = [("h", C.c_void_p), ("grad_h", C.c_void_p), ("ld_h", C.c_int32), ("ld_g", C.c_int32), ("width", C.c_int32),
                ("scope", C.c_int32), ("mode", C.c_int32), ("col_off", C.c_int32)]


class AttnGradJob(C.Structure):
    _fields_ = [("key_sum", C.c_void_p), ("feat_sum", C.c_void_p), ("sigma_sum", C.c_void_p), ("edge_w", C.c_void_p),
                ("edge_b", C.c_void_p), ("attn_w", C.c_void_p), ("g_attn", C.c_void_p), ("g_edge_w", C.c_void_p),
                ("g_edge_b", C.c_void_p), ("dq", C.c_int32), ("kd", C.c_int32), ("attn_len", C.c_int32), ("R", C.c_int32)]


class Plan(C.Structure):
    _fields_ = [("data", C.c_void_p), ("bytes", C.c_size_t), ("N", C.c_int64), ("E", C.c_int64),
                ("B", C.c_int64), ("num_edge_feats", C.c_int), ("flags", C.c_int)]


ATTN_MAX_CELLS = 16


class AttnCell(C.Structure):   # dagnn_attn_cell
    _fields_ = [("key", C.c_void_p), ("w_key", C.c_void_p), ("query", C.c_void_p), ("w_query", C.c_void_p),
                ("vid_key", C.c_void_p), ("vid_query", C.c_void_p), ("edge_gain", C.c_void_p), ("edge_vec", C.c_void_p),
                ("bias", C.c_void_p), ("ld_key", C.c_int), ("key_dim", C.c_int), ("ld_query", C.c_int),
                ("query_dim", C.c_int), ("dir", C.c_int), ("pad_", C.c_int)]


class AttnArgs(C.Structure):   # dagnn_attn_args
    _fields_ = [("cell", AttnCell * ATTN_MAX_CELLS), ("num_cells", C.c_int), ("mode", C.c_int), ("vid_mod", C.c_int),
                ("pad_", C.c_int), ("key_score", C.c_void_p), ("query_score", C.c_void_p), ("alpha", C.c_void_p),
                ("logit", C.c_void_p)]


class GemmGroup(C.Structure):
    _fields_ = [("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("C", C.c_void_p)]


class LayerArgs(C.Structure):
    _fields_ = [("gi", C.c_void_p * MAX_DIRS), ("w_hh_t", C.c_void_p * MAX_DIRS), ("b_hh", C.c_void_p * MAX_DIRS),
                ("w_key", C.c_void_p * MAX_DIRS), ("edge_gain", C.c_void_p * MAX_DIRS),
                ("vid_bias", C.c_void_p * MAX_DIRS), ("h", C.c_void_p * MAX_DIRS), ("score", C.c_void_p * MAX_DIRS),
                ("vid_mod", C.c_int), ("ld_h", C.c_int), ("static_score", C.c_int), ("debug_timing", C.c_void_p)]


MAX_STACKED = 8   # DAGNN_MAX_STACKED


class PackJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("out_slices16", C.c_void_p), ("out_slices32", C.c_void_p), ("out_mfma", C.c_void_p),
                ("H", C.c_int32), ("K", C.c_int32)]


MAX_PACK_JOBS = 16


class FrontierCell(C.Structure):
    _fields_ = [("w_hh_pk16", C.c_void_p), ("w_hh_pk32", C.c_void_p), ("w_ih_pk16", C.c_void_p),
                ("w_ih_pk32", C.c_void_p), ("w_hh_mfma", C.c_void_p), ("w_ih_mfma", C.c_void_p), ("b_hh", C.c_void_p), ("b_ih", C.c_void_p), ("w_key", C.c_void_p),
                ("static_score", C.c_void_p), ("edge_gain", C.c_void_p), ("vid_bias", C.c_void_p), ("gi0", C.c_void_p), ("h_out", C.c_void_p),
                ("granules", C.c_void_p)]


class FrontierArgs(C.Structure):
    _fields_ = [("cell", (FrontierCell * MAX_STACKED) * MAX_DIRS), ("num_stacked", C.c_int), ("dir_mask", C.c_int),
                ("H", C.c_int), ("ld_h", C.c_int), ("vid_mod", C.c_int), ("num_cus", C.c_int), ("rb4_max_wgs", C.c_int), ("mfma_min_rows", C.c_int),
                ("agg_scratch", C.c_void_p), ("agg_scratch_rows", C.c_int),
                ("tail_replicas", C.c_int), ("tail_slice_units", C.c_int), ("tail_max_blocks", C.c_int), ("epoch", C.c_uint),
                ("tail_err", C.c_void_p), ("debug_timing", C.c_void_p), ("side_stream", C.c_void_p),
                ("layer_split", C.POINTER(C.c_int32) * MAX_DIRS), ("fork_event", C.c_void_p), ("join_event", C.c_void_p)]


class DataflowCell(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("w_hh", "w_ih", "b_hh", "b_ih", "w_key", "static_score", "edge_gain",
                                          "vid_bias", "gi0", "h_out", "granules", "proj_granules", "gh_out", "gi_out",
                                          "agg_edge_w", "agg_edge_b")] + [("agg", C.c_int)]


class DataflowArgs(C.Structure):
    _fields_ = [("cell", (DataflowCell * MAX_STACKED) * MAX_DIRS), ("num_stacked", C.c_int), ("dir_mask", C.c_int),
                ("H", C.c_int), ("ld_h", C.c_int), ("gld", C.c_int), ("pld", C.c_int), ("vid_mod", C.c_int), ("groups", C.c_int),
                ("epoch", C.c_uint), ("schedule", C.c_void_p), ("err", C.c_void_p), ("debug_timing", C.c_void_p),
                ("spin_limit", C.c_uint), ("debug_wg", C.c_int), ("num_cus", C.c_int), ("xcc_table", C.c_void_p),
                ("plan_status", C.c_void_p), ("xcd_first", C.c_int), ("stat_rows", C.c_int)]


class TilesCell(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("w_hh", "w_ih", "b_hh", "b_ih", "w_key", "edge_gain", "gi0", "h_out", "vid_bias")]


class TilesArgs(C.Structure):
    _fields_ = [("cell", (TilesCell * MAX_STACKED) * MAX_DIRS), ("num_stacked", C.c_int), ("dir_mask", C.c_int),
                ("H", C.c_int), ("ld_h", C.c_int), ("num_cus", C.c_int), ("epoch", C.c_uint), ("counters", C.c_void_p),
                ("err", C.c_void_p), ("spin_limit", C.c_uint), ("plan_status", C.c_void_p), ("first_layer", C.c_int * MAX_DIRS),
                ("debug_timing", C.c_void_p), ("vid_mod", C.c_int)]


class BackwardCell(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("w_hh", "w_ih", "w_key", "edge_gain", "vid_bias", "static_score", "h", "a", "alpha", "gi", "gh", "g_ext",
                                          "da", "dgi", "dgh", "sigma", "edge_feat_grad", "da_granules", "du_granules",
                                          "g_ext_static")]


class BackwardArgs(C.Structure):
    _fields_ = [("cell", (BackwardCell * MAX_STACKED) * MAX_DIRS), ("num_stacked", C.c_int), ("dir_mask", C.c_int),
                ("H", C.c_int), ("ld_h", C.c_int), ("vid_mod", C.c_int), ("num_cus", C.c_int), ("thin_wgs", C.c_int),
                ("tail_replicas", C.c_int), ("tail_max_blocks", C.c_int), ("epoch", C.c_uint), ("tail_err", C.c_void_p),
                ("side_stream", C.c_void_p), ("layer_split", C.POINTER(C.c_int32) * MAX_DIRS),
                ("fork_event", C.c_void_p), ("join_event", C.c_void_p)]


class WgradJob(C.Structure):
    _fields_ = [("dg", C.c_void_p), ("inp", C.c_void_p), ("d_weight", C.c_void_p), ("d_bias", C.c_void_p),
                ("ld_dg", C.c_int), ("ld_in", C.c_int), ("in_dim", C.c_int)]


class ColsumJob(C.Structure):
    _fields_ = [("x", C.c_void_p), ("weight", C.c_void_p), ("out", C.c_void_p), ("ld_x", C.c_int), ("cols", C.c_int)]


class BwdDataflowCell(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("w_hh_t", "w_ih_t", "w_key", "alpha", "gi", "gh", "a", "b_hh", "h", "g_ext", "stat",
                                          "da_granules", "q_granules", "dgi_granules", "du_granules", "dgi", "dgh", "sigma",
                                          "edge_feat_grad")]


class BwdDataflowArgs(C.Structure):
    _fields_ = [("cell", (BwdDataflowCell * MAX_STACKED) * MAX_DIRS), ("num_stacked", C.c_int), ("dir_mask", C.c_int),
                ("H", C.c_int), ("ld_h", C.c_int), ("ld_g", C.c_int), ("gld", C.c_int), ("groups", C.c_int),
                ("epoch", C.c_uint), ("spin_limit", C.c_uint), ("schedule", C.c_void_p), ("records", C.c_void_p),
                ("err", C.c_void_p), ("plan_status", C.c_void_p), ("num_cus", C.c_int), ("xcc_table", C.c_void_p), ("xcd_first", C.c_int),
                ("stat_rows_written", C.c_int), ("pull_rows", C.c_int)]


PULL_ROW = 256   # DAGNN_PULL_ROW: floats per edge of the per-unit pull weights (`agg = max` on the reverse dataflow sweep)


class PlainPull(C.Structure):   # dagnn_plain_pull
    _fields_ = [(k, C.c_void_p) for k in ("h", "a", "edge_mat", "edge_vec", "weights", "da_granules", "esum")] + \
        [("ld_h", C.c_int), ("ld_a", C.c_int), ("gld", C.c_int)]


class GatherJob(C.Structure):   # dagnn_gather_job: dagnn_gather_rows_batch, and the jobs of dagnn_encode_args
    _fields_ = [("h", C.c_void_p), ("ld_h", C.c_int), ("width", C.c_int), ("node_off", C.c_int), ("col_off", C.c_int)]


class EncodeArgs(C.Structure):
    _fields_ = [("plan", Plan), ("edge_index", C.c_void_p), ("layer_fwd", C.c_void_p), ("layer_bwd", C.c_void_p),
                ("batch", C.c_void_p), ("edge_attr", C.c_void_p), ("plan_status", C.c_void_p),
                ("gemm", GemmGroup * 2), ("num_gemm", C.c_int), ("gemm_cols", C.c_int), ("in_dim", C.c_int), ("ld_x", C.c_int),
                ("schedule", C.c_void_p), ("schedule_bytes", C.c_size_t), ("cost_layer", C.c_int), ("cost_row", C.c_int),
                ("df", DataflowArgs), ("jobs", GatherJob * 16), ("num_jobs", C.c_int), ("stride", C.c_int),
                ("hcat", C.c_void_p), ("ld_hcat", C.c_int), ("w_out", C.c_void_p), ("b_out", C.c_void_p), ("out", C.c_void_p),
                ("out_dim", C.c_int)]


AGG_ATTN, AGG_MATTN, AGG_GATED, AGG_ADD, AGG_MAX, AGG_GIVEN = range(6)
POOL_MAX, POOL_ADD, POOL_MEAN = range(3)


class VariantAggregator(C.Structure):
    _fields_ = [("mode", C.c_int32), ("lands", C.c_int32), ("val_dim", C.c_int32), ("aux_dim", C.c_int32),
                ("out_dim", C.c_int32), ("reserved", C.c_int32), ("vals", C.c_void_p), ("ld_vals", C.c_int64),
                ("node0", C.c_void_p), ("node1", C.c_void_p), ("ld_node", C.c_int64), ("edge_mat0", C.c_void_p),
                ("edge_vec0", C.c_void_p), ("edge_mat1", C.c_void_p), ("edge_vec1", C.c_void_p), ("out", C.c_void_p),
                ("ld_out", C.c_int64)]


class VariantMap(C.Structure):
    _fields_ = [("w_t", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("ld_out", C.c_int64),
                ("out_dim", C.c_int32), ("vid_mod", C.c_int32), ("vid_bias", C.c_void_p)]


class VariantCell(C.Structure):
    _fields_ = [("agg", VariantAggregator), ("recurrent", C.c_int32), ("in_dim", C.c_int32), ("input", C.c_void_p),
                ("ld_input", C.c_int64), ("w_in_t", C.c_void_p), ("w_agg_t", C.c_void_p), ("b_in", C.c_void_p),
                ("b_agg", C.c_void_p), ("h", C.c_void_p), ("ld_h", C.c_int64), ("map", VariantMap * 3),
                ("num_maps", C.c_int32), ("reserved", C.c_int32)]


class IpropLayer(C.Structure):
    _fields_ = [("w_ih", C.c_void_p), ("w_hh", C.c_void_p), ("b_ih", C.c_void_p), ("b_hh", C.c_void_p), ("in_dim", C.c_int)]


DVAE_MAX_N = 32   # DAGNN_DVAE_MAX_N
DVAE_AGG_ATTN_H, DVAE_AGG_GATED_SUM, DVAE_AGG_ATTN_X = 0, 1, 2   # DAGNN_DVAE_AGG_*

# what dagnn_dvae_decode_args and dagnn_dvae_sample_args declare alike: the decoder's weights, and the block appended for gated_sum
_DVAE_WEIGHTS = [("w_ih", C.c_void_p * MAX_STACKED), ("w_hh", C.c_void_p * MAX_STACKED), ("b_ih", C.c_void_p * MAX_STACKED),
                 ("b_hh", C.c_void_p * MAX_STACKED), ("w_key", C.c_void_p), ("vid_bias", C.c_void_p),
                 ("av_w1", C.c_void_p), ("av_b1", C.c_void_p), ("av_w2", C.c_void_p), ("av_b2", C.c_void_p),
                 ("ae_w1", C.c_void_p), ("ae_b1", C.c_void_p), ("ae_w2", C.c_void_p), ("ae_b2", C.c_void_p)]
_DVAE_AGG = [("agg", C.c_int), ("gate_w", C.c_void_p), ("gate_b", C.c_void_p), ("mapper_w", C.c_void_p)]


class DvaeDecodeArgs(C.Structure):
    _fields_ = [("B", C.c_int64), ("n", C.c_int), ("hs", C.c_int), ("L", C.c_int), ("nvt", C.c_int), ("start_type", C.c_int),
                ("bn", C.c_int), ("edge_hidden", C.c_int), ("vertex_hidden", C.c_int),
                ("types", C.c_void_p), ("preds", C.c_void_p), ("h0", C.c_void_p)] + _DVAE_WEIGHTS + \
               [("ll", C.c_void_p), ("saved", C.c_void_p), ("saved_bytes", C.c_size_t)] + _DVAE_AGG


class DvaeDecodeArgsTyped(DvaeDecodeArgs):
    """dagnn_dvae_decode_args as the header has it today: the layout above (attn_h / gated_sum, which the library still takes - fields
    are only ever appended, and one is read only under the `agg` value that introduced it) plus the type-keyed table (DVAE_AGG_ATTN_X)."""
    _fields_ = [("key_type", C.c_void_p)]


class DvaeDecodeGrads(C.Structure):
    _fields_ = [("g_res", C.c_void_p), ("work", C.c_void_p), ("work_bytes", C.c_size_t), ("d_h0", C.c_void_p),
                ("d_w_ih", C.c_void_p * MAX_STACKED), ("d_w_hh", C.c_void_p * MAX_STACKED),
                ("d_b_ih", C.c_void_p * MAX_STACKED), ("d_b_hh", C.c_void_p * MAX_STACKED),
                ("d_w_key", C.c_void_p), ("d_vid_bias", C.c_void_p),
                ("d_av_w1", C.c_void_p), ("d_av_b1", C.c_void_p), ("d_av_w2", C.c_void_p), ("d_av_b2", C.c_void_p),
                ("d_ae_w1", C.c_void_p), ("d_ae_b1", C.c_void_p), ("d_ae_w2", C.c_void_p), ("d_ae_b2", C.c_void_p),
                ("d_gate_w", C.c_void_p), ("d_gate_b", C.c_void_p), ("d_mapper_w", C.c_void_p)]


class DvaeDecodeGradsTyped(DvaeDecodeGrads):
    _fields_ = [("d_key_type", C.c_void_p)]   # DVAE_AGG_ATTN_X


class DvaeSampleArgs(C.Structure):
    _fields_ = [("G", C.c_int64), ("B", C.c_int64), ("n", C.c_int), ("hs", C.c_int), ("L", C.c_int), ("nvt", C.c_int),
                ("start_type", C.c_int), ("end_type", C.c_int), ("bn", C.c_int), ("stochastic", C.c_int),
                ("edge_hidden", C.c_int), ("vertex_hidden", C.c_int), ("h0", C.c_void_p)] + _DVAE_WEIGHTS + \
               [("u_type", C.c_void_p), ("u_edge", C.c_void_p), ("types", C.c_void_p), ("preds", C.c_void_p),
                ("nv", C.c_void_p), ("states", C.c_void_p), ("work", C.c_void_p), ("work_bytes", C.c_size_t)] + _DVAE_AGG


class DvaeSampleArgsTyped(DvaeSampleArgs):
    _fields_ = [("key_type", C.c_void_p)]   # DVAE_AGG_ATTN_X; see DvaeDecodeArgsTyped


DVAE_ENAS, DVAE_BN = 0, 1                        # DAGNN_DVAE_ENAS / DAGNN_DVAE_BN
DVAE_FIRST_VALID, DVAE_MOST_FREQUENT = 0, 1      # DAGNN_DVAE_FIRST_VALID / DAGNN_DVAE_MOST_FREQUENT


class DvaeSelectArgs(C.Structure):
    _fields_ = [("A", C.c_int64), ("B", C.c_int64), ("n", C.c_int), ("nvt", C.c_int), ("start_type", C.c_int),
                ("end_type", C.c_int), ("kind", C.c_int), ("n_nodes", C.c_int), ("select", C.c_int),
                ("types", C.c_void_p), ("preds", C.c_void_p), ("nv", C.c_void_p), ("valid", C.c_void_p),
                ("pick", C.c_void_p), ("n_valid", C.c_void_p), ("n_same", C.c_void_p), ("work", C.c_void_p),
                ("work_bytes", C.c_size_t)]


LP_INT64, LP_FLOAT32, LP_FLOAT64 = 0, 1, 2         # DAGNN_LP_INT64 / DAGNN_LP_FLOAT32 / DAGNN_LP_FLOAT64
PREDICTOR_MAX_NZ, PREDICTOR_MAX_HS, PREDICTOR_ROWS = 128, 1024, 8   # DAGNN_PREDICTOR_MAX_NZ / _MAX_HS / _ROWS
DVAE_SET_GRAPHS, DVAE_SET_KEYS = 0, 1             # DAGNN_DVAE_SET_GRAPHS / DAGNN_DVAE_SET_KEYS
DVAE_SET_MAX_ROWS = 1 << 20                      # DAGNN_DVAE_SET_MAX_ROWS
DVAE_SET_HEADER_WORDS, DVAE_SET_COUNT, DVAE_SET_ERR = 16, 4, 5   # header words of a set's storage
DVAE_SET_ERR_FULL, DVAE_SET_ERR_HEADER = 1, 2


class DvaeSameDagArgs(C.Structure):
    _fields_ = [("A", C.c_int64), ("B", C.c_int64), ("n", C.c_int), ("types", C.c_void_p), ("preds", C.c_void_p),
                ("nv", C.c_void_p), ("types_true", C.c_void_p), ("preds_true", C.c_void_p), ("nv_true", C.c_void_p),
                ("same", C.c_void_p), ("per_graph", C.c_void_p), ("total", C.c_void_p)]


class DvaeSet(C.Structure):
    _fields_ = [("form", C.c_int), ("width", C.c_int), ("max_rows", C.c_int64), ("data", C.c_void_p), ("bytes", C.c_size_t)]


class DvaeSetRowsArgs(C.Structure):
    _fields_ = [("set", DvaeSet), ("base", C.c_int64), ("A", C.c_int64), ("B", C.c_int64), ("types", C.c_void_p),
                ("preds", C.c_void_p), ("nv", C.c_void_p), ("keys", C.c_void_p), ("mask", C.c_void_p),
                ("member", C.c_void_p), ("count", C.c_void_p)]


class VariantBwdCell(C.Structure):
    _fields_ = [("mode", C.c_int32), ("lands", C.c_int32), ("in_dim", C.c_int32), ("proj_dim", C.c_int32),
                ("recurrent", C.c_int32), ("reserved", C.c_int32)] + \
        [(k, C.c_void_p) for k in ("h", "a", "gi", "gh", "node0", "node1", "alpha", "edge_mat0", "edge_vec0", "edge_mat1",
                                   "edge_vec1", "w_node", "w_query", "w_hh", "w_ih", "g", "g_in", "da", "dgi", "dgh",
                                   "dnode0", "dnode1", "dlogit", "esum", "w_node2")] + \
        [("w_ld", C.c_int32), ("ld_in", C.c_int32), ("ties", C.c_void_p)]


class VariantBwdArgs(C.Structure):
    _fields_ = [("cell", (VariantBwdCell * MAX_STACKED) * MAX_DIRS), ("num_stacked", C.c_int), ("dir_mask", C.c_int),
                ("H", C.c_int), ("ld", C.c_int)]


class VariantArgs(C.Structure):
    _fields_ = [("cell", (VariantCell * MAX_STACKED) * MAX_DIRS), ("num_stacked", C.c_int), ("dir_mask", C.c_int),
                ("H", C.c_int)]


class PrepTable(C.Structure):
    _fields_ = [("type_emb", C.c_void_p), ("attr_emb", C.c_void_p), ("depth_emb", C.c_void_p), ("out", C.c_void_p),
                ("width", C.c_int), ("ld_out", C.c_int)]


PREPARE_MAX_TABLES = 3


class PrepareRows(C.Structure):
    _fields_ = [("x", C.c_void_p), ("depth", C.c_void_p), ("max_depth", C.c_int), ("num_tables", C.c_int),
                ("table", PrepTable * PREPARE_MAX_TABLES), ("stack_src", C.c_void_p * 4), ("stack_out", C.c_void_p)]


class StoreGatherArgs(C.Structure):   # dagnn_store_gather_args: every field 8 bytes, in the header's order
    _fields_ = [(k, C.c_void_p) for k in ("node_ptr", "edge_ptr", "tok_ptr", "x", "depth", "layer_f", "layer_b", "src", "dst",
                                          "tok", "depth_max", "y_arr", "ref_ids", "ref_extra", "idx", "offsets")] + \
        [(k, C.c_int64) for k in ("ld_offsets", "B", "N", "E", "S", "R")] + \
        [(k, C.c_void_p) for k in ("out_x", "out_depth", "out_edge_index", "out_edge_attr", "out_batch", "out_ptr",
                                   "out_index0", "out_index1", "out_layer_f", "out_layer_b", "out_llp", "out_y_arr",
                                   "out_ref_ids", "out_ref_extra")]


class DagStoreGatherArgs(C.Structure):   # dagnn_dag_store_gather_args: every field 8 bytes, in the header's order
    _fields_ = [(k, C.c_void_p) for k in ("types", "preds", "succs", "layer_f", "layer_b", "y", "idx", "offsets")] + \
        [(k, C.c_int64) for k in ("B", "n", "nvt", "E")] + \
        [(k, C.c_void_p) for k in ("out_x", "out_edge_index", "out_bi_layer_index", "out_batch", "out_ptr", "out_types",
                                   "out_preds", "out_y")]


BN_TABLE_CELLS, BN_MAX_VARS = 8192, 30             # DAGNN_BN_TABLE_CELLS / DAGNN_BN_MAX_VARS
BN_STAGE_AUTO, BN_STAGE_LDS, BN_STAGE_GLOBAL = 0, 1, 2   # DAGNN_BN_STAGE_*


class BnData(C.Structure):   # dagnn_bn_data
    _fields_ = [("cols", C.c_void_p), ("ld", C.c_int64), ("S", C.c_int64), ("n_var", C.c_int32), ("reserved", C.c_int32),
                ("cards", C.c_int32 * BN_MAX_VARS)]


TABLE_GRADS_MAX_TABLES, TABLE_GRADS_CHUNK = 3, 32   # DAGNN_TABLE_GRADS_MAX_TABLES / _CHUNK (the summation order's chunk length)


class TableGradsTable(C.Structure):   # dagnn_table_grads_table
    _fields_ = [("keys", C.c_void_p), ("key_stride", C.c_int64), ("R", C.c_int64), ("out", C.c_void_p), ("ld_out", C.c_int64)]


class TableGradsArgs(C.Structure):   # dagnn_table_grads_args
    _fields_ = [("g", C.c_void_p), ("ld_g", C.c_int64), ("N", C.c_int64), ("H", C.c_int32), ("num_tables", C.c_int32),
                ("table", TableGradsTable * TABLE_GRADS_MAX_TABLES), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stages", C.c_int32), ("reserved", C.c_int32)]


TABLE_GRADS_INDEX, TABLE_GRADS_SUM = 1, 2   # DAGNN_TABLE_GRADS_INDEX / _SUM (dagnn_table_grads_args.stages; 0 = both)


SGP_MAX_M, SGP_MAX_D, SGP_MAX_Q = 512, 128, 128   # DAGNN_SGP_MAX_M / _MAX_D / _MAX_Q
SGP_ARGMIN_MEAN, SGP_ARGMIN_EI = 0, 1             # DAGNN_SGP_ARGMIN_*
SGP_REFINE_MAX_STARTS, SGP_REFINE_HISTORY = 32, 8    # DAGNN_SGP_REFINE_MAX_STARTS / _HISTORY
SGP_REFINE_MEAN, SGP_REFINE_EI = 0, 1                # DAGNN_SGP_REFINE_MEAN / _EI (the objective)
SGP_REFINE_STATUS = ("running", "converged", "stalled", "budget", "dead")   # DAGNN_SGP_REFINE_RUNNING .. _DEAD

# The C type each mirror above stands for: "dagnn_" + the class's name in snake case, unless stated here.  tests/test_abi_cpu.py has
# the compiler check every mirror against it - size, each field's offset and type - and every entry of SYMBOLS and every upper-case
# constant X (against DAGNN_X) likewise: a mirror, an argtypes list or a constant that drifts from the header fails the CPU tests.
C_TYPES = {PrepTable: "std::remove_extent_t<decltype(dagnn_prepare_rows::table)>",   # the unnamed struct of dagnn_prepare_rows.table[]
           DvaeDecodeArgsTyped: "dagnn_dvae_decode_args", DvaeDecodeGradsTyped: "dagnn_dvae_decode_grads",
           DvaeSampleArgsTyped: "dagnn_dvae_sample_args"}
C_TYPES = {cls: C_TYPES.get(cls, "dagnn_" + re.sub("(?<!^)(?=[A-Z])", "_", cls.__name__).lower())
           for cls in list(globals().values()) if isinstance(cls, type) and issubclass(cls, C.Structure)}
C_FIELD_NAMES = {(WgradJob, "inp"): "in"}   # a field the header names with a Python keyword
# earlier generations of a struct, which the library still serves (fields are only ever appended): each field sits where the
# header has it and the class is no longer than the header's struct; the *Typed successor is the one checked whole
C_EARLIER = {DvaeDecodeArgs, DvaeDecodeGrads, DvaeSampleArgs}

# every symbol include/dagnn_hip.h declares: (restype, argtypes)
SYMBOLS = {
    "dagnn_version": (C.c_char_p, []),
    "dagnn_store_gather": (C.c_int, [C.POINTER(StoreGatherArgs), C.c_void_p]),
    "dagnn_dag_store_gather": (C.c_int, [C.POINTER(DagStoreGatherArgs), C.c_void_p]),
    "dagnn_dag_store_layers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_plan_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64, C.c_int]),
    "dagnn_plan_is_small": (C.c_int, [C.c_int64, C.c_int64, C.c_int64]),
    "dagnn_plan_layout": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int64)]),
    "dagnn_plan_build": (C.c_int, [C.POINTER(Plan), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "dagnn_prepare": (C.c_int, [C.POINTER(Plan), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(PrepareRows), C.c_void_p]),
    "dagnn_encode_ast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_int, C.c_int64, C.c_int, C.c_void_p]),
    "dagnn_gemm_nt_bias": (C.c_int, [C.POINTER(GemmGroup), C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p]),
    "dagnn_pack_whh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dagnn_recurrence_layer": (C.c_int, [C.POINTER(Plan), C.POINTER(LayerArgs), C.c_int, C.c_int, C.c_void_p]),
    "dagnn_pack_slices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dagnn_pack_batch": (C.c_int, [C.POINTER(PackJob), C.c_int, C.c_void_p]),
    "dagnn_pack_mfma": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dagnn_frontier_run": (C.c_int, [C.POINTER(Plan), C.POINTER(FrontierArgs), C.POINTER(C.POINTER(C.c_int32)),
                                     C.POINTER(C.c_int32), C.c_void_p]),
    "dagnn_dataflow_groups": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64]),
    "dagnn_dataflow_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "dagnn_dataflow_layout": (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int64)]),
    "dagnn_dataflow_schedule": (C.c_int, [C.POINTER(Plan), C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p]),
    "dagnn_dataflow_run": (C.c_int, [C.POINTER(Plan), C.POINTER(DataflowArgs), C.c_void_p]),
    "dagnn_dataflow_run_wide": (C.c_int, [C.POINTER(Plan), C.POINTER(DataflowArgs), C.c_void_p]),
    "dagnn_tiles_launches": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dagnn_tiles_run": (C.c_int, [C.POINTER(Plan), C.POINTER(TilesArgs), C.c_void_p]),
    "dagnn_pack_dataflow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dagnn_pack_dataflow_transposed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dagnn_score_parts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "dagnn_backward_prepare": (C.c_int, [C.POINTER(Plan), C.POINTER(BackwardArgs), C.c_void_p]),
    "dagnn_backward_run": (C.c_int, [C.POINTER(Plan), C.POINTER(BackwardArgs), C.POINTER(C.POINTER(C.c_int32)),
                                     C.POINTER(C.c_int32), C.c_void_p]),
    "dagnn_bwd_dataflow_record_bytes": (C.c_size_t, [C.c_int64]),
    "dagnn_bwd_dataflow_static_bytes": (C.c_size_t, [C.c_int64]),
    "dagnn_bwd_dataflow_static_bytes_h": (C.c_size_t, [C.c_int64, C.c_int]),
    "dagnn_bwd_dataflow_prepare": (C.c_int, [C.POINTER(Plan), C.POINTER(BwdDataflowArgs), C.c_void_p]),
    "dagnn_bwd_dataflow_run": (C.c_int, [C.POINTER(Plan), C.POINTER(BwdDataflowArgs), C.c_void_p]),
    "dagnn_bwd_dataflow_run_wide": (C.c_int, [C.POINTER(Plan), C.POINTER(BwdDataflowArgs), C.c_void_p]),
    "dagnn_colsum_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "dagnn_colsum_run": (C.c_int, [C.POINTER(ColsumJob), C.c_int, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dagnn_wgrad_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "dagnn_wgrad_splits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64]),
    "dagnn_wgrad_run": (C.c_int, [C.POINTER(WgradJob), C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    "dagnn_table_grads_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "dagnn_table_grads": (C.c_int, [C.POINTER(TableGradsArgs), C.c_void_p]),
    "dagnn_pack_dataflow_batch": (C.c_int, [C.POINTER(DfPackJob), C.c_int, C.c_int, C.c_void_p]),
    "dagnn_attn_grads_run": (C.c_int, [C.POINTER(AttnGradJob), C.c_int, C.c_void_p]),
    "dagnn_readout_pool_batch": (C.c_int, [C.POINTER(Plan), C.POINTER(PoolJob), C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dagnn_readout_pool_backward_batch": (C.c_int, [C.POINTER(Plan), C.POINTER(PoolBwdJob), C.c_int, C.c_void_p, C.c_int,
                                                    C.c_void_p]),
    "dagnn_topo_layers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "dagnn_variant_aggregate": (C.c_int, [C.POINTER(Plan), C.POINTER(VariantAggregator), C.c_int, C.c_int32, C.c_int32,
                                          C.c_void_p]),
    "dagnn_variant_run": (C.c_int, [C.POINTER(Plan), C.POINTER(VariantArgs), C.POINTER(C.POINTER(C.c_int32)),
                                    C.POINTER(C.c_int32), C.c_void_p]),
    "dagnn_variant_mattn_prepare": (C.c_int, [C.POINTER(Plan), C.POINTER(VariantBwdCell), C.c_int, C.c_int, C.c_int32,
                                              C.c_int32, C.c_void_p]),
    "dagnn_variant_max_prepare": (C.c_int, [C.POINTER(Plan), C.POINTER(VariantBwdCell), C.c_int, C.c_int, C.c_int, C.c_int32,
                                            C.c_int32, C.c_void_p]),
    "dagnn_plain_max_weights": (C.c_int, [C.POINTER(Plan), C.POINTER(PlainPull), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_void_p]),
    "dagnn_plain_edge_grads": (C.c_int, [C.POINTER(Plan), C.POINTER(PlainPull), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_void_p]),
    "dagnn_variant_aggregator_backward": (C.c_int, [C.POINTER(Plan), C.POINTER(VariantBwdCell), C.c_int, C.c_int, C.c_int32,
                                                    C.c_int32, C.c_void_p]),
    "dagnn_variant_backward_run": (C.c_int, [C.POINTER(Plan), C.POINTER(VariantBwdArgs), C.POINTER(C.POINTER(C.c_int32)),
                                             C.POINTER(C.c_int32), C.c_void_p]),
    "dagnn_vid_colsums": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "dagnn_iprop_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int, C.POINTER(IpropLayer), C.c_int, C.c_void_p, C.c_void_p]),
    "dagnn_iprop_step_typed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_int, C.POINTER(IpropLayer), C.c_int, C.c_void_p, C.c_void_p]),
    "dagnn_encode_forward": (C.c_int, [C.POINTER(EncodeArgs), C.c_void_p]),
    "dagnn_dvae_decode_saved_bytes": (C.c_size_t, [C.POINTER(DvaeDecodeArgs)]),
    "dagnn_dvae_decode_work_bytes": (C.c_size_t, [C.POINTER(DvaeDecodeArgs)]),
    "dagnn_dvae_decode_forward": (C.c_int, [C.POINTER(DvaeDecodeArgs), C.c_void_p]),
    "dagnn_dvae_decode_backward": (C.c_int, [C.POINTER(DvaeDecodeArgs), C.POINTER(DvaeDecodeGrads), C.c_void_p]),
    "dagnn_dvae_sample_work_bytes": (C.c_size_t, [C.POINTER(DvaeSampleArgs)]),
    "dagnn_dvae_sample": (C.c_int, [C.POINTER(DvaeSampleArgs), C.c_void_p]),
    "dagnn_dvae_select_key_words": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "dagnn_dvae_select_work_bytes": (C.c_size_t, [C.POINTER(DvaeSelectArgs)]),
    "dagnn_dvae_select": (C.c_int, [C.POINTER(DvaeSelectArgs), C.c_void_p]),
    "dagnn_dvae_same_dag": (C.c_int, [C.POINTER(DvaeSameDagArgs), C.c_void_p]),
    "dagnn_dvae_set_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int64]),
    "dagnn_dvae_set_init": (C.c_int, [C.POINTER(DvaeSet), C.c_void_p]),
    "dagnn_dvae_set_add": (C.c_int, [C.POINTER(DvaeSetRowsArgs), C.c_void_p]),
    "dagnn_dvae_set_query": (C.c_int, [C.POINTER(DvaeSetRowsArgs), C.c_void_p]),
    "dagnn_debug_occupy": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "dagnn_tn_product": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "dagnn_seq_ce": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_heads_argmax_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "dagnn_heads_argmax": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dagnn_heads_score_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "dagnn_heads_score": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.c_void_p]),
    "dagnn_rows_argmax": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dagnn_seq_f1_counts": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "dagnn_graph_depth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "dagnn_class_ce": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_class_hits_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "dagnn_class_hits": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_seq_ce_step": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_class_ce_step": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_predictor_mse_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "dagnn_predictor_mse": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                      C.c_void_p]),
    "dagnn_predictor_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_fit_sums_bytes": (C.c_size_t, [C.c_int64]),
    "dagnn_fit_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p, C.c_void_p]),
    "dagnn_bn_stage_fits": (C.c_int, [C.POINTER(BnData)]),
    "dagnn_bn_score": (C.c_int, [C.POINTER(BnData), C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_bn_rows_to_parents": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_sgp_project": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_float,
                                    C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "dagnn_sgp_ei_step_bytes": (C.c_size_t, [C.c_int64]),
    "dagnn_sgp_ei_step": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                    C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "dagnn_sgp_energy_grad_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int64]),
    "dagnn_sgp_energy_grad": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 14 +
                              [C.c_size_t, C.c_void_p, C.c_void_p]),
    "dagnn_sgp_refine_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "dagnn_sgp_refine_eval": (C.c_int, [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dagnn_sgp_refine_run": (C.c_int, [C.c_int] * 5 + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                       C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dagnn_opt_chunks": (C.c_int64, [C.c_void_p, C.c_int]),
    "dagnn_grad_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "dagnn_clip_adam": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_float,
                                  C.c_void_p, C.c_void_p]),
    "dagnn_score_parts_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "dagnn_param_fingerprint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dagnn_gather_rows_batch": (C.c_int, [C.POINTER(GatherJob), C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dagnn_gather_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                    C.c_int, C.c_void_p]),
    "dagnn_attention_weights": (C.c_int, [C.POINTER(Plan), C.POINTER(AttnArgs), C.c_void_p]),
}

_lock = threading.Lock()
_lib = None


def lib_path() -> str:
    return _build.LIB


def load():
    """Load (building first if the in-tree .so is missing or stale and hipcc is present)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = _build.LIB
        if _build.is_stale():
            try:
                _build.build()
            except Exception as exc:  # no hipcc and no prebuilt library: fail loudly
                if not os.path.exists(path):
                    raise DagnnHipError(
                        "libdagnn_hip.so is missing and could not be built (%s). There is no CPU or "
                        "PyTorch fallback for the DAGNN hot path." % exc) from exc
                # an OLDER library next to NEWER sources: its argument structs and plan layout may no longer match
                # the ctypes mirrors in this file - that is memory corruption, not an error message
                if os.environ.get("DAGNN_AMD_ALLOW_STALE", "0") != "1":
                    raise DagnnHipError(
                        "%s is older than its sources and the rebuild failed (%s); refusing to load a library whose "
                        "ABI may differ from this package (set DAGNN_AMD_ALLOW_STALE=1 to load it anyway)" % (path, exc)) from exc
        try:
            lib = C.CDLL(path)
        except OSError as exc:
            raise DagnnHipError("cannot load %s: %s (no fallback path exists)" % (path, exc)) from exc
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as exc:
                raise DagnnHipError("%s does not export %s" % (path, name)) from exc
            fn.restype, fn.argtypes = res, args
        _lib = lib
        return lib


def check(code: int, what: str) -> None:
    if code == DAGNN_OK:
        return
    if code <= -1000:
        msg = "hipError_t %d" % (-code - 1000)
    else:
        msg = _ERRORS.get(code, "error %d" % code)
    raise DagnnHipError("%s failed: %s" % (what, msg))
