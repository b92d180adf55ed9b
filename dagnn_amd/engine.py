"""Host-side driver of the HIP path: turns torch tensors into C-ABI calls (include/dagnn_hip.h).

PyTorch is plumbing here - device memory, the current stream, and the dense head GEMMs; every
step of the DAGNN hot path itself runs in libdagnn_hip.so.  Nothing in this module has a CPU
implementation: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (BackwardArgs, BwdDataflowArgs, DagnnHipError, DataflowArgs, FrontierArgs, GemmGroup, LayerArgs, Plan,
                   TilesArgs, check)


class KernelTimer(object):
    """Optional HIP-event timing of individual launches (bench.py): events are recorded on the
    stream the kernel is launched on (torch's current stream), so they bracket exactly that kernel."""

    def __init__(self, only=None):
        self.spans = {}
        self.only = set(only) if only else None   # every event pair costs the stream ~8 us: time only what is asked for

    def span(self, name, device):
        if self.only is not None and name not in self.only:
            return _NoSpan()
        return _Span(self, name, device)

    def summary(self):
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / max(len(v), 1)) for k, v in self.spans.items()}


class _Span(object):
    def __init__(self, timer, name, device):
        self.timer, self.name, self.device = timer, name, device

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record(torch.cuda.current_stream(self.device))

    def __exit__(self, *exc):
        self.b.record(torch.cuda.current_stream(self.device))
        self.timer.spans.setdefault(self.name, []).append((self.a, self.b))


class _NoSpan(object):
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


TIMER: Optional[KernelTimer] = None  # set by bench.py around its timed region

def _env_int(name: str, default: int) -> int:
    return int(os.environ.get(name, default))


# Launch-geometry knobs (read once at import; the defaults are the measured optima on MI355X).
# Tests flip some of them to force the less common code paths.
RB4_MAX_WGS = _env_int("DAGNN_AMD_RB4_MAX_WGS", 0)          # 4-row vs 8-row blocks of the streamed kernel; 0 = library default
DUAL_CHAINS = _env_int("DAGNN_AMD_DUAL_CHAINS", 1)         # the two directions' per-layer launches on two streams (H > 256)
MFMA_MIN_ROWS = _env_int("DAGNN_AMD_MFMA_MIN_ROWS", 300)    # launches with at least this many rows use MFMA tiles; 0 = never
TAIL_SLICE = _env_int("DAGNN_AMD_TAIL_SLICE", 32)           # hidden units per workgroup of the persistent kernel (16 | 32)
TAIL_REPLICAS = _env_int("DAGNN_AMD_TAIL_REPLICAS", 4)      # workgroups per (cell, slice); 0 = one launch per layer throughout
TAIL_MAX_BLOCKS = _env_int("DAGNN_AMD_TAIL_MAX_BLOCKS", 2)  # without split mode: layers of <= 4 * replicas * this rows go to it
SPLIT_DEEP = _env_int("DAGNN_AMD_SPLIT_DEEP", 1)            # 1: deep graphs on a side stream from layer 0 (forward and backward)
BWD_THIN_WGS = _env_int("DAGNN_AMD_BWD_THIN_WGS", 0)        # backward: slice kernel vs rows + MFMA kernels; 0 = library default
BWD_TAIL_REPLICAS = _env_int("DAGNN_AMD_BWD_TAIL_REPLICAS", 2)    # backward persistent kernel; 0 = one launch per layer
BWD_TAIL_MAX_BLOCKS = _env_int("DAGNN_AMD_BWD_TAIL_MAX_BLOCKS", 4)
# 1: plan / schedule kernels on a side stream next to the encoder + input GEMM.  Off by default - measured on MI355X: no
# gain (2.405 vs 2.413 ms per forward); the GEMM's workgroups hold the CUs' LDS, so the 33-KB-LDS plan kernels only get
# their turn as it drains (rocprofv3 timeline: plan_graph_kernel 101 us next to the GEMM, 60 us alone).
# Tried again with the plan kernels' LDS cut to 17 / 12 KB so that they fit next to the GEMM's four workgroups per CU:
# they then run concurrently but 2-4x slower (plan_ptr 61 us instead of 15, plan_graph 103 instead of 49), bench.py
# 2.302-2.312 against 2.3085 ms - nothing - and two processes sharing one GPU (the two-rank bench test) failed.
PLAN_OVERLAP = _env_int("DAGNN_AMD_PLAN_OVERLAP", 0)              # 1: training passes launch plan / schedule on the arena's side stream next to encoder + input GEMM (model._plan_of); measured: 13 separate launches 1.64 -> 1.59 ms per forward, the fused pipeline (csrc/prepare.hip) gains nothing from it (fork + join cost what it hides: training step 5.42 against 5.32 ms)
SIDE_PRIORITY = _env_int("DAGNN_AMD_SIDE_PRIORITY", 0)     # stream priority of an arena's side stream (-1: high)
VARIANT_DATAFLOW = _env_int("DAGNN_AMD_VARIANT_DATAFLOW", 1)  # 1: evaluation passes of agg = add / max (GRU cells, no agg_x, H <= 256) run on the persistent dataflow kernel (a plain fold in its loader) instead of the per-layer variant launches
PARAM_GUARD = _env_int("DAGNN_AMD_PARAM_GUARD", 1)            # 1: evaluation passes fingerprint the parameters behind the derived-weight caches (core.ParamGuard: one small launch per pass); a write the version counters missed is reported like a device-side failure
ERR_PARAMS_MOVED = 0x10000                                       # bit of the arena's error word the guard sets
FOLD_INPUT = _env_int("DAGNN_AMD_FOLD_INPUT", 1)              # 1: evaluation passes over an ASTNodeEncoder fold the embedding tables through W_ih of stacked layer 0 once per
                                                            # weight version (gi0 = three folded rows summed per node instead of the [N, emb] x [emb, 3H] GEMM; model._folded_tables)
PREPARE_FUSED = _env_int("DAGNN_AMD_PREPARE", 1)            # 1: evaluation passes build plan + schedule + encoder rows + side effect 1 as one pipeline of 7 launches (csrc/prepare.hip)
PLAN_SMALL = _env_int("DAGNN_AMD_PLAN_SMALL", 1)            # 1: batches of <= 2048 nodes / 4096 edges / 512 graphs build plan and schedule with one workgroup each (csrc/small.hip)
PLAN_GENERAL_BUILD = 1                                      # dagnn_plan.flags: keep the plan on the general kernels
DATAFLOW = _env_int("DAGNN_AMD_DATAFLOW", 1)                # 1: the persistent graph-affine dataflow kernel where it applies (H <= 256)
DF_COST_LAYER = _env_int("DAGNN_AMD_DF_COST_LAYER", 4)      # schedule cost of one dependent layer, in rows (hop latency / row cost;
                                                            # round 3: 4 -> 6 after the block got cheaper; round 4: back to 4 after the hop did (lean loader), scripts/df_cost_sweep.py)
DF_COST_ROW = _env_int("DAGNN_AMD_DF_COST_ROW", 1)
DF_GROUPS = _env_int("DAGNN_AMD_DF_GROUPS", 0)              # 0 = as many groups as the device hosts
DF_XCD = _env_int("DAGNN_AMD_DF_XCD", 1)                    # 1: XCD-aware workgroup ids + hand-offs through the shared L2 where the run-time check allows
TILES = _env_int("DAGNN_AMD_TILES", 1)                      # 1: the weight-stationary tile kernel (H = 512: csrc/tiles.hip) where it is the faster path
                                                            # (>= 2 stacked layers: alone up to TILES_MAX_NODES nodes, behind the per-layer launches of the wide first
                                                            # layers on larger batches); 2: alone wherever it is supported; 0: never
TILES_PAD = _env_int("DAGNN_AMD_TILES_PAD", 1)              # 1: hidden sizes in (256, 512) of stacked models are zero-padded to 512 so that the tile kernel takes them
TILES_TAIL_ROWS = _env_int("DAGNN_AMD_TILES_TAIL_ROWS", 32)
TILES_MAX_MEAN_ROWS = _env_int("DAGNN_AMD_TILES_MAX_MEAN_ROWS", 160)   # policy (TILES=1): batches above 1536 nodes with more rows per batch-level layer than this stay on the launches    # larger batches: per-layer launches for the wide first layers, the tile kernel from the
                                                            # first layer on behind which no layer has more rows than this (0: no such split)
TILES_MAX_NODES = _env_int("DAGNN_AMD_TILES_MAX_NODES", 10000)  # measured on MI355X at L = 5 (scripts/tiles_sweep.py, tiles_hybrid.py): the kernel alone takes
                                                            # 0.75-0.82x the per-layer launches' time up to 8 k nodes, 0.95x at 15 k, 1.04-1.10x at 30 k
                                                            # (cfg 5); split at the thin tail 0.86x at 15 k and 0.88x at 30 k: larger batches are split
BWD_DATAFLOW = _env_int("DAGNN_AMD_BWD_DATAFLOW", 1)        # 1: the reverse sweep as one persistent dataflow launch (H <= 256)
TABLE_GRADS = _env_int("DAGNN_AMD_TABLE_GRADS", 0)          # 1: the node encoder's embedding-table gradients in one fixed summation order (csrc/table_grads.hip: bitwise repeatable) instead of torch's atomic index_add_; read at call time
DEBUG_WG = _env_int("DAGNN_AMD_DEBUG_WG", 0)               # workgroup whose blocks scripts/df_stamps.py stamps
SPIN_LIMIT = _env_int("DAGNN_AMD_SPIN_LIMIT", 0)            # polls before a device-side wait gives up; 0 = library default
DEBUG_TIMING: Optional[torch.Tensor] = None  # int64[8] device tensor: phase ticks of the deepest work item
_NOSPAN = _NoSpan()


def _span(name, tensor):
    return TIMER.span(name, tensor.device) if TIMER is not None else _NOSPAN


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


import threading

_LAUNCH_TLS = threading.local()   # per thread: stack of `launch_on` streams (the reference's DataParallel runs one thread per
                                  # device, tg/data_parallel.py:59-62: one thread's override must not redirect another's launches)


def _launch_stack() -> list:
    st = getattr(_LAUNCH_TLS, "stack", None)
    if st is None:
        st = _LAUNCH_TLS.stack = []
    return st


def _stream_obj(device):
    """The stream library launches go to for `device`: the innermost `launch_on` stream of this thread, else torch's current
    stream.  `_stream` (raw handle) and `persistent_launch` (events) both resolve it here."""
    st = _launch_stack()
    if st and st[-1] is not None:
        return st[-1]
    return torch.cuda.current_stream(device)


class launch_on(object):
    """Library launches inside the block go to `stream`; torch's CURRENT stream - hence the caching allocator's pool and
    every torch op - stays the caller's.  Memory allocated inside is the caller stream's: no `record_stream`, no
    foreign-pool blocks that cannot be reused (a forward pass that allocated under a side stream cost seven `hipMalloc`
    calls per batch).  The caller orders the two streams itself (fork before, join after)."""

    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        _launch_stack().append(self.stream)
        return self

    def __exit__(self, *exc):
        _launch_stack().pop()
        return False


def _stream(t: torch.Tensor) -> int:
    """Raw hipStream_t of torch's current stream on the tensor's device (the Stream object costs ~1.5 us per call and
    the small-batch forward asks seven times)."""
    st = getattr(_LAUNCH_TLS, "stack", None)
    if st and st[-1] is not None:
        return st[-1].cuda_stream
    if _RAW_STREAM is not None:
        return _RAW_STREAM(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


_CUS = {}


class persistent_launch(object):
    """Device-wide rule for the all-resident persistent kernels (`dagnn_dataflow_run[_wide]`, `dagnn_bwd_dataflow_run[_wide]`,
    `dagnn_tiles_run`, the persistent tails of `dagnn_frontier_run` / `dagnn_backward_run`, `dagnn_encode_forward`): each of
    them sizes its grid to the whole device (one workgroup per CU, every workgroup resident, bounded spins on the others'
    granules), so two of them in flight on different streams would each hold part of the CUs and wait for workgroups
    that cannot be dispatched - the micro-batch experiment of round 4 DEADLOCKED exactly like that until the bounded
    waits expired.  Rule: inside one process, persistent launches on one device never overlap - a launch on stream B
    first waits (on the DEVICE: `hipStreamWaitEvent`, the host never blocks) for the previous persistent launch of
    another stream A to drain.  Everything else of a pass (plan, encoder, GEMMs, read-out, heads) still overlaps freely.
    Across processes nothing can enforce it: ranks must not share a GPU (multi-GPU section)."""
    _last = {}   # device index -> (event, stream handle) of the most recent persistent launch

    def __init__(self, tensor: torch.Tensor):
        self.dev = tensor.device

    def __enter__(self):
        if self.dev.type != "cuda":
            return self
        cur = _stream_obj(self.dev)   # (the stream the kernel really goes to: a `launch_on` override counts)
        rec = persistent_launch._last.get(self.dev.index)
        if rec is not None and rec[1] != cur.cuda_stream:
            cur.wait_event(rec[0])
        return self

    def __exit__(self, *exc):
        if self.dev.type != "cuda":
            return False
        cur = _stream_obj(self.dev)
        rec = persistent_launch._last.get(self.dev.index)
        ev = rec[0] if (rec is not None and rec[1] == cur.cuda_stream) else torch.cuda.Event()
        ev.record(cur)   # (a waiter that was queued on an earlier record of this event keeps that earlier record)
        persistent_launch._last[self.dev.index] = (ev, cur.cuda_stream)
        return False


def _num_cus(device) -> int:
    key = device.index if isinstance(device, torch.device) else device
    n = _CUS.get(key)
    if n is None:
        n = _CUS[key] = torch.cuda.get_device_properties(device).multi_processor_count
    return n


def _dev(t: torch.Tensor, what: str, dtype=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise DagnnHipError(
            "%s must be a tensor on a ROCm GPU: the DAGNN hot path is hand-written HIP for gfx950 and has no "
            "CPU fallback (got %s)" % (what, getattr(t, "device", type(t))))
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()


def _rows(t: torch.Tensor, what: str) -> torch.Tensor:
    """fp32 GPU matrix whose rows are contiguous; a row pitch larger than the width is kept (views of the
    lock-step state buffers, [:, :H] of [N, H + H/16]) instead of being copied."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        return _dev(t, what, torch.float32)
    if t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] \
            and t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0:
        return t
    return _dev(t, what, torch.float32)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_STATUS_POOL = {}


def _status_words(device) -> torch.Tensor:
    """Four zeroed int32 words (a plan's contract status).  They come from a pool zeroed 1024 plans at a time - a fill kernel
    per plan sat on the critical path of every forward (4.4 us + its launch gap) - and a slot is never handed out twice: the
    plan's view keeps its pool alive, an exhausted pool is simply dropped."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, _RAW_STREAM(idx) if _RAW_STREAM is not None else torch.cuda.current_stream(dev).cuda_stream)
    pool = _STATUS_POOL.get(key)   # one pool per (device, stream): zeroed on, and owned by, the stream whose passes use it
    if pool is None or pool[1] >= pool[0].shape[0]:
        pool = _STATUS_POOL[key] = [torch.zeros(1024, 4, dtype=torch.int32, device=dev), 0]
    pool[1] += 1
    return pool[0][pool[1] - 1]


class PlanHandle(object):
    """Device workspace holding the layer-sorted per-graph CSR of one batch (both directions)."""

    route = None   # what `route.before_plan` said (width, dataflow groups) where the plan's builder asked, for the pass to go on from

    def __init__(self, N: int, E: int, B: int, R: int, device):
        lib = _lib.load()
        self.N, self.E, self.B, self.R = int(N), int(E), int(B), int(R)
        nbytes = lib.dagnn_plan_bytes(self.N, self.E, self.B, self.R)
        self.ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)
        self.status = _status_words(device)
        self.desc = Plan(self.ws.data_ptr(), nbytes, self.N, self.E, self.B, self.R, 0 if PLAN_SMALL else PLAN_GENERAL_BUILD)
        self.ready = None   # event to wait for when the plan was built on another stream

    def launch_build(self) -> None:
        edge_index, layer_fwd, layer_bwd, batch, edge_attr = self._keep
        with _span("plan_build", edge_index):
            check(_lib.load().dagnn_plan_build(C.byref(self.desc), edge_index.data_ptr(), layer_fwd.data_ptr(),
                                               layer_bwd.data_ptr(), batch.data_ptr(), _ptr(edge_attr),
                                               self.status.data_ptr(), _stream(edge_index)), "dagnn_plan_build")

    def launch_prepare(self, groups: int = 0, enc=None, stack=None) -> None:
        """The fused pipeline (`dagnn_prepare`, csrc/prepare.hip): this plan, its dataflow schedule for `groups` groups
        (0: none) and the row work that rides along - `enc` = (x [N,2], depth [N], max_depth, [(type, attr, depth tables, out),
        ...]): encoder rows of up to three table sets (depth table None: type + attr); `stack` = (four [N] int64 tensors, out [4, N]): side effect 1."""
        lib = _lib.load()
        edge_index, layer_fwd, layer_bwd, batch, edge_attr = self._keep
        rows = _lib.PrepareRows()
        keep = []
        if enc is not None:
            x, depth, max_depth, tables = enc
            x = _dev(x, "x", torch.int64)
            if not (depth.is_cuda and depth.dtype == torch.int64 and depth.is_contiguous()):
                raise DagnnHipError("node_depth must be a contiguous int64 GPU tensor (it is clamped in place)")
            rows.x, rows.depth, rows.max_depth, rows.num_tables = x.data_ptr(), depth.data_ptr(), int(max_depth), len(tables)
            for k, (tw, aw, dw, out) in enumerate(tables):
                tw, aw = _dev(tw, "type table", torch.float32), _dev(aw, "attribute table", torch.float32)
                dw = None if dw is None else _dev(dw, "depth table", torch.float32)   # (None: the two-table encoder, utils2.py:28)
                keep += [tw, aw, dw]
                t = rows.table[k]
                t.type_emb, t.attr_emb, t.depth_emb, t.out = tw.data_ptr(), aw.data_ptr(), _ptr(dw), out.data_ptr()
                t.width, t.ld_out = tw.shape[1], out.stride(0)
            keep.append(x)
        if stack is not None:
            srcs, out = stack
            srcs = [_dev(t, "layer index", torch.int64) for t in srcs]
            keep += srcs
            for j in range(4):
                rows.stack_src[j] = srcs[j].data_ptr()
            rows.stack_out = out.data_ptr()
        ws, nbytes, key = None, 0, None
        if groups > 0:
            key = (int(groups), DF_COST_LAYER, DF_COST_ROW)
            ws = self.dataflow_schedule(groups, launch=False)
            if key in self._df:   # (it came with the plan from the loader)
                ws, groups, key = None, 0, None
            else:
                nbytes = lib.dagnn_dataflow_bytes(self.N, self.B, key[0])
        with _span("prepare", edge_index):
            check(lib.dagnn_prepare(C.byref(self.desc), edge_index.data_ptr(), layer_fwd.data_ptr(), layer_bwd.data_ptr(),
                                    batch.data_ptr(), _ptr(edge_attr), self.status.data_ptr(), _ptr(ws), nbytes, int(groups),
                                    DF_COST_LAYER, DF_COST_ROW, C.byref(rows) if (enc is not None or stack is not None) else None,
                                    _stream(edge_index)), "dagnn_prepare")
        if key is not None and key in self.__dict__.get("_df_pending", {}):
            self._df[key] = self._df_pending.pop(key)

    def wait_ready(self) -> None:
        """Order the caller's stream behind the plan's construction (no-op for a plan built on this stream)."""
        ev = getattr(self, "ready", None)
        if ev is not None:
            torch.cuda.current_stream(self.ws.device).wait_event(ev)
            self.ready = None

    @classmethod
    def from_words(cls, ws: torch.Tensor, meta: dict, dataflow_words: Optional[torch.Tensor] = None) -> "PlanHandle":
        """Wrap a plan built on the host (`dagnn_amd.host_plan.build_plan_host`, e.g. in a loader worker) and
        already moved to the GPU: no plan kernels and - the schedule being known on the host - no device->host
        read in `forward`."""
        lib = _lib.load()
        if not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.int32 and ws.is_contiguous()):
            raise DagnnHipError("a host-built plan must be a contiguous int32 tensor on the GPU (move the batch "
                                "with .to(device) first)")
        self = cls.__new__(cls)
        self.N, self.E, self.B, self.R = (int(meta[k]) for k in ("N", "E", "B", "R"))
        nbytes = lib.dagnn_plan_bytes(self.N, self.E, self.B, self.R)
        if ws.numel() * 4 < nbytes:
            raise DagnnHipError("host-built plan has %d bytes, the layout needs %d" % (ws.numel() * 4, nbytes))
        self.ws = ws
        self.status = _status_words(ws.device)
        self.desc = Plan(ws.data_ptr(), nbytes, self.N, self.E, self.B, self.R, 0 if PLAN_SMALL else PLAN_GENERAL_BUILD)
        self._schedule = [a for a in meta["schedule"]]
        self._splits = [a for a in meta["splits"]]
        if dataflow_words is not None and meta.get("dataflow_key") is not None and dataflow_words.is_cuda:
            self._df_host = {"key": tuple(meta["dataflow_key"]), "words": dataflow_words}
        return self

    def layout(self) -> dict:
        off = (C.c_int64 * 26)()
        check(_lib.load().dagnn_plan_layout(self.N, self.E, self.B, self.R, off), "dagnn_plan_layout")
        names = ["node_ptr", "edge_ptr", "depth0", "depth1", "order0", "order1", "lstart0", "lstart1", "rowptr0",
                 "rowptr1", "col0", "col1", "eattr0", "eattr1", "items", "total", "blptr0", "blptr1", "rowrec0",
                 "rowrec1", "slot0", "slot1", "eidx0", "eidx1", "blsplit0", "blsplit1"]
        return {k: int(v) // 4 for k, v in zip(names, off)}

    def read_schedule(self):
        """Batch-level layer offsets of both directions as host int32 arrays (ONE device->host read,
        the counterpart of the reference's `.item()` at dagnn.py:137).  Returns [ptr_fwd, ptr_bwd],
        ptr_d has T_d + 1 entries."""
        if getattr(self, "_schedule", None) is None:
            lay = self.layout()
            a, b, c, e = lay["blptr0"], lay["blptr1"], lay["blsplit0"], lay["blsplit1"]
            host = self.ws[a:e + self.N + 2].cpu().numpy()   # blptr0 .. blsplit1 in one copy
            out, spl = [], []
            for off, soff in ((0, c - a), (b - a, e - a)):
                T = int(host[off + self.N + 1])
                out.append(host[off:off + T + 1].copy())
                spl.append(host[soff:soff + T].copy())
            self._schedule, self._splits = out, spl
        return self._schedule

    def read_splits(self):
        """Per direction, per batch-level layer: first slot of the deep graphs' rows (see include/dagnn_hip.h);
        comes with the same device->host read as the schedule."""
        self.read_schedule()
        return self._splits

    def dataflow_schedule(self, groups: int, launch: bool = True) -> torch.Tensor:
        """The plan's rows dealt to `groups` independent groups (`dagnn_dataflow_schedule`), built once per plan.
        `launch=False` allocates the workspace only; the next call with the same key issues the kernels."""
        cache = self.__dict__.setdefault("_df", {})
        pending = self.__dict__.setdefault("_df_pending", {})
        key = (int(groups), DF_COST_LAYER, DF_COST_ROW)
        if key not in cache:
            meta = getattr(self, "_df_host", None)
            if meta is not None and meta.get("key") == key:   # built by the loader (host_plan.attach_plan)
                cache[key] = meta["words"]
            else:
                lib = _lib.load()
                nbytes = lib.dagnn_dataflow_bytes(self.N, self.B, key[0])
                ws = pending.pop(key, None)
                if ws is None:
                    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=self.ws.device)
                if not launch:
                    pending[key] = ws
                    return ws
                with _span("dataflow_schedule", self.ws):
                    check(lib.dagnn_dataflow_schedule(C.byref(self.desc), ws.data_ptr(), nbytes, key[0], key[1], key[2],
                                                      self.status.data_ptr(), _stream(self.ws)), "dagnn_dataflow_schedule")
                cache[key] = ws
        return cache[key]

    def dataflow_layout(self, groups: int) -> dict:
        off = (C.c_int64 * 13)()
        check(_lib.load().dagnn_dataflow_layout(self.N, self.B, int(groups), off), "dagnn_dataflow_layout")
        names = ["grp_of", "gdepth", "gload", "loff", "gtab0", "gtab1", "lcnt0", "lcnt1", "glbase0", "glbase1", "grec0",
                 "grec1", "total"]
        return {k: int(v) // 4 for k, v in zip(names, off)}

    def check_status(self) -> None:
        """Debug helper (synchronises): raises if the batch violated the layout contract."""
        s = int(self.status[0])
        if s:
            msgs = [m for b, m in ((1, "edges not grouped by graph"), (2, "edge crosses graphs / out of range"),
                                   (4, "batch vector not sorted"), (8, "layer id >= nodes of its graph")) if s & b]
            raise DagnnHipError("plan contract violated: " + ", ".join(msgs))


def build_plan(edge_index: torch.Tensor, layer_fwd: torch.Tensor, layer_bwd: torch.Tensor, batch: torch.Tensor,
               num_graphs: int, edge_attr: Optional[torch.Tensor] = None, launch: bool = True) -> PlanHandle:
    """`launch=False`: allocate and initialise only; `plan.launch_build()` issues the kernels (e.g. under `launch_on`)."""
    edge_index = _dev(edge_index, "edge_index", torch.int64)
    layer_fwd = _dev(layer_fwd, "layer ids", torch.int64)
    layer_bwd = _dev(layer_bwd, "layer ids", torch.int64)
    batch = _dev(batch, "batch", torch.int64)
    N, E = layer_fwd.numel(), edge_index.shape[1]
    R = 0
    if edge_attr is not None:
        edge_attr = _dev(edge_attr, "edge_attr", torch.float32)
        # (a batch without edges: `view(0, -1)` cannot infer the width)
        edge_attr = edge_attr.view(E, -1) if E else edge_attr.reshape(0, edge_attr.shape[-1] if edge_attr.dim() > 1 else 1)
        R = edge_attr.shape[1]
    plan = PlanHandle(N, E, num_graphs, R, edge_index.device)
    plan._keep = (edge_index, layer_fwd, layer_bwd, batch, edge_attr)
    if launch:
        plan.launch_build()
    return plan


def encode_ast(x: torch.Tensor, depth: torch.Tensor, type_w: torch.Tensor, attr_w: torch.Tensor,
               depth_w: Optional[torch.Tensor], max_depth: int) -> torch.Tensor:
    """out = type_emb[x0] + attr_emb[x1] + depth_emb[min(depth, max_depth)]; clamps `depth` in place.  `depth_w` None: the
    two-table encoder (ogbg-code/utils2.py:26-28), out = type_emb[x0] + attr_emb[x1]."""
    x = _dev(x, "x", torch.int64)
    if not (depth.is_cuda and depth.dtype == torch.int64 and depth.is_contiguous()):
        raise DagnnHipError("node_depth must be a contiguous int64 GPU tensor (it is clamped in place)")
    N, H = x.shape[0], type_w.shape[1]
    out = torch.empty(N, H, dtype=torch.float32, device=x.device)
    check(_lib.load().dagnn_encode_ast(x.data_ptr(), depth.data_ptr(), _dev(type_w, "type table").data_ptr(),
                                       _dev(attr_w, "attribute table").data_ptr(),
                                       None if depth_w is None else _dev(depth_w, "depth table").data_ptr(), int(max_depth), out.data_ptr(), H,
                                       N, H, _stream(x)), "dagnn_encode_ast")
    return out


def gemm_nt_bias(A: Sequence[torch.Tensor], W: Sequence[torch.Tensor], bias: Sequence[Optional[torch.Tensor]],
                 out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """C_g = A_g @ W_g^T + bias_g for up to 4 groups sharing M, K and Nc (one launch)."""
    n = len(A)
    A = [_rows(a, "A") for a in A]
    if len({a.stride(0) for a in A}) > 1:
        A = [a.contiguous() for a in A]
    lda = A[0].stride(0)
    W = [_dev(w, "W", torch.float32) for w in W]
    M, K = A[0].shape
    Nc = W[0].shape[0]
    for a, w in zip(A, W):
        if tuple(a.shape) != (M, K) or tuple(w.shape) != (Nc, K):
            raise DagnnHipError("grouped GEMM needs identical shapes per group")
    if out is None:
        out = [torch.empty(M, Nc, dtype=torch.float32, device=A[0].device) for _ in range(n)]
    groups = (GemmGroup * n)()
    keep = []
    for g in range(n):
        b = None if bias[g] is None else _dev(bias[g], "bias", torch.float32)
        keep.append(b)
        groups[g] = GemmGroup(A[g].data_ptr(), W[g].data_ptr(), _ptr(b), out[g].data_ptr())
    with _span("gemm_nt_bias", A[0]):
        check(_lib.load().dagnn_gemm_nt_bias(groups, n, M, Nc, K, lda, K, Nc, _stream(A[0])), "dagnn_gemm_nt_bias")
    return list(out)


def pack_whh(w_hh: torch.Tensor) -> torch.Tensor:
    """[3H, H] (torch GRUCell layout) -> k-major [H, 3H]."""
    w_hh = _dev(w_hh, "weight_hh", torch.float32)
    H = w_hh.shape[1]
    out = torch.empty(H, 3 * H, dtype=torch.float32, device=w_hh.device)
    check(_lib.load().dagnn_pack_whh(w_hh.data_ptr(), out.data_ptr(), H, _stream(w_hh)), "dagnn_pack_whh")
    return out


def pack_slices(w: torch.Tensor, H: int, slice_units: int) -> torch.Tensor:
    """[3H, K] (torch layout) -> slice/lane order consumed by the lock-step kernel."""
    w = _dev(w, "weight", torch.float32)
    K = w.shape[1]
    out = torch.empty(3 * H * K, dtype=torch.float32, device=w.device)
    check(_lib.load().dagnn_pack_slices(w.data_ptr(), out.data_ptr(), H, K, slice_units, _stream(w)),
          "dagnn_pack_slices")
    return out


def pack_mfma(w: torch.Tensor, H: int) -> torch.Tensor:
    """[3H, K] (torch layout) -> MFMA B-fragment order of the 32-row tile kernel."""
    w = _dev(w, "weight", torch.float32)
    out = torch.empty(3 * H * w.shape[1], dtype=torch.float32, device=w.device)
    check(_lib.load().dagnn_pack_mfma(w.data_ptr(), out.data_ptr(), H, w.shape[1], _stream(w)), "dagnn_pack_mfma")
    return out


def pack_batch(mats: Sequence[torch.Tensor], H: int):
    """All three lock-step layouts ({16: .., 32: .., "mfma": ..}) of every [3H, K] matrix in `mats`, one launch per 16
    matrices (`dagnn_pack_batch`)."""
    mats = [_dev(w, "weight", torch.float32) for w in mats]
    outs = []
    for base in range(0, len(mats), _lib.MAX_PACK_JOBS):
        chunk = mats[base:base + _lib.MAX_PACK_JOBS]
        jobs = (_lib.PackJob * len(chunk))()
        for j, w in zip(jobs, chunk):
            o = {k: torch.empty(3 * H * w.shape[1], dtype=torch.float32, device=w.device) for k in (16, 32, "mfma")}
            outs.append(o)
            j.w, j.out_slices16, j.out_slices32, j.out_mfma = w.data_ptr(), o[16].data_ptr(), o[32].data_ptr(), \
                o["mfma"].data_ptr()
            j.H, j.K = H, w.shape[1]
        check(_lib.load().dagnn_pack_batch(jobs, len(chunk), _stream(chunk[0])), "dagnn_pack_batch")
    return outs


def pack_dataflow(w: torch.Tensor, H: int) -> torch.Tensor:
    """[3H, H] (torch layout) -> slice / lane order of the dataflow kernel."""
    w = _dev(w, "weight", torch.float32)
    if tuple(w.shape) != (3 * H, H):
        raise DagnnHipError("pack_dataflow needs a [3H, H] matrix, got %s" % (tuple(w.shape),))
    out = torch.empty(3 * H * H, dtype=torch.float32, device=w.device)
    check(_lib.load().dagnn_pack_dataflow(w.data_ptr(), out.data_ptr(), H, _stream(w)), "dagnn_pack_dataflow")
    return out


def pack_dataflow_batch(mats, H: int, gains=()):
    """`pack_dataflow` / `pack_dataflow_transposed` of several [3H, H] matrices in ONE launch per 16: `mats` = list of (w,
    transposed); returns the packed tensors in order.  `gains`: (edge_w [kd, R], key [kd], out [R]) triples - the cells' edge
    gains `W_e^T w_key` ride in the same launch (their outputs are written in place)."""
    lib = _lib.load()
    outs, jobs, keep = [], [], []
    for w, tr in mats:
        w = _dev(w, "weight", torch.float32)
        if tuple(w.shape) != (3 * H, H):
            raise DagnnHipError("pack_dataflow_batch needs [3H, H] matrices, got %s" % (tuple(w.shape),))
        o = torch.empty(3 * H * H, dtype=torch.float32, device=w.device)
        keep.append(w)
        outs.append(o)
        jobs.append(_lib.DfPackJob(w.data_ptr(), o.data_ptr(), None, 1 if tr else 0, 0, 0))
    for ew, key, out in gains:
        ew, key = _dev(ew, "edge_encoder.weight", torch.float32), _dev(key, "key weights", torch.float32)
        keep += [ew, key]
        jobs.append(_lib.DfPackJob(ew.data_ptr(), out.data_ptr(), key.data_ptr(), 2, ew.shape[0], ew.shape[1]))
    for k0 in range(0, len(jobs), _lib.MAX_PACK_JOBS):
        part = jobs[k0:k0 + _lib.MAX_PACK_JOBS]
        arr = (_lib.DfPackJob * len(part))(*part)
        check(lib.dagnn_pack_dataflow_batch(arr, len(part), H, _stream(keep[0])), "dagnn_pack_dataflow_batch")
    return outs


RESERVED_CUS = _env_int("DAGNN_AMD_RESERVED_CUS", -1)   # CUs the persistent kernels of a TRAINING pass leave free; -1 = automatic (below)
RCCL_MAX_WORKGROUPS = 64   # upper bound of RCCL's channel count (one workgroup per channel) when NCCL_MAX_NCHANNELS does not pin it
_COLLECTIVE = {"registered": False, "group": None}


def register_collective(group=None) -> None:
    """The process group the gradient exchange of this process runs on (`train.GradBucket` / `OverlappedGradReducer` /
    `DataParallel` call this): `reserved_cus` then looks at THAT group's size instead of the default group's - a model trained
    under a one-rank sub-group overlaps no collective and keeps every CU."""
    _COLLECTIVE["registered"] = True
    _COLLECTIVE["group"] = group


def reserved_cus_info(training: bool):
    """(CUs a training pass leaves free, why) - see `reserved_cus`."""
    if RESERVED_CUS >= 0:
        return (RESERVED_CUS if training else 0), "DAGNN_AMD_RESERVED_CUS=%d" % RESERVED_CUS
    if not training:
        return 0, "inference passes overlap no collective"
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0, "no communicator"
    try:
        world = dist.get_world_size(_COLLECTIVE["group"]) if _COLLECTIVE["registered"] else dist.get_world_size()
    except (RuntimeError, ValueError):   # (this rank is not a member of the registered group)
        world = 1
    if world <= 1:
        return 0, "the gradient exchange's group has one rank"
    pinned = _env_int("NCCL_MAX_NCHANNELS", 0)
    ch = pinned if pinned > 0 else RCCL_MAX_WORKGROUPS
    r = min((ch + 7) // 8 * 8, RCCL_MAX_WORKGROUPS)   # whole CUs per XCD: the launches are spread evenly over the 8 XCDs
    return r, ("NCCL_MAX_NCHANNELS=%d pins RCCL's workgroups" % pinned if pinned > 0 else
               "RCCL may run up to %d channels (one workgroup each); NCCL_MAX_NCHANNELS pins fewer" % RCCL_MAX_WORKGROUPS)


def reserved_cus(training: bool) -> int:
    """The dataflow kernels need EVERY workgroup resident (one per CU, the whole register file of the CU each: 240 of 256
    CUs at the headline shape).  In a data-parallel training step the heads' gradient bucket is all-reduced WHILE the
    reverse sweep runs (`train.OverlappedGradReducer`): the collective's kernels (RCCL: one workgroup per channel) were
    launched first and hold CUs the sweep counts on - the resident part of the sweep then spins on granules of workgroups
    that cannot be dispatched before the collective drains: a serialisation at best, an expired bounded wait at worst.  So
    a training pass whose gradient exchange runs on a group of more than one rank (`register_collective`; the default group
    when nothing registered) sizes its persistent launches - forward and reverse share one schedule - for `num_cus - r`,
    spread evenly over the XCDs, where r = RCCL's channel count rounded up to whole CUs per XCD: `NCCL_MAX_NCHANNELS` when
    the launcher pins it (16 leaves 240 CUs = all five workgroup sets of the headline shape), else RCCL's upper bound of 64
    (24 of 32 CUs per XCD: four sets).  `DAGNN_AMD_RESERVED_CUS=n` overrides the rule in both directions (0: never
    reserve; n: always, also in a single process - what the GPU tests of the rule use).  Inference passes overlap no
    collective and keep every CU.  Reserving changes which group a graph is dealt to, never a result (GPU test)."""
    return reserved_cus_info(training)[0]


def effective_cus(device, training: bool = False) -> int:
    n = _num_cus(device)
    r = reserved_cus(training)
    return max(n - r, 8) if r > 0 else n


def dataflow_groups(device, num_dirs: int, num_stacked: int, H: int, B: int, training: bool = False) -> int:
    """Groups the dataflow kernel runs on this device for this model shape; 0 = not applicable.  `training`: a pass
    whose reverse sweep may overlap a gradient collective (`reserved_cus`)."""
    if not DATAFLOW or not (H <= 256 or (H == 320 and DF_WIDE)):   # (320: `dagnn_dataflow_run_wide`, for the models `route.width` names)
        return 0
    cus = effective_cus(device, training)
    g = _lib.load().dagnn_dataflow_groups(cus, int(num_dirs), int(num_stacked), int(H), int(B))
    return min(g, DF_GROUPS) if DF_GROUPS > 0 else g


class PassRecord(object):
    """What a training pass's forward hands its reverse sweep: the raw state buffers `h_buf[d][i]`, `gi0[d]`, the width `Hp`, the
    `route` and, per cell (d, i), what the dataflow launch left: the sweep's static rows `stat`, or `gh` (`gi` above layer 0).
    `handover()`: "stat" - it wrote static rows; "preact" - it kept gh / gi; None - neither, the reverse sweep recomputes them."""
    __slots__ = ("h_buf", "gi0", "Hp", "route", "gh", "gi", "stat")

    def __init__(self, route=None):
        self.h_buf = self.gi0 = self.Hp = None
        self.route, self.gh, self.gi, self.stat = route, {}, {}, {}

    def handover(self) -> Optional[str]:
        return "stat" if self.stat else "preact" if self.gh else None


def dataflow_run(plan: PlanHandle, dirs: Sequence[int], L: int, H: int, cells, gi0, h, groups: int, vid_mod: int = 0,
                 arena: Optional["GranuleArena"] = None, static_score=None, score_parts: bool = False,
                 record: Optional[PassRecord] = None, training: bool = False, stat_rows: bool = False) -> None:
    """The whole recurrence as one persistent launch (csrc/dataflow.hip).  Same operands as `frontier_run`;
    `score_parts` adds the partial attention scores behind the state rows (what the backward pass reads); `record`
    (training passes) receives the pre-activations the kernel computed anyway - `gh` [N,3H] of every cell, `gi` of the stacked
    layers above the first - or, with `stat_rows` (`Route.stat_rows`), the static rows of the reverse sweep it wrote itself."""
    if arena is None:
        raise DagnnHipError("the dataflow kernel needs a GranuleArena (persistent, zero-initialised granule buffers)")
    lib = _lib.load()
    args = dataflow_args(plan, dirs, L, H, cells, gi0, h, groups, vid_mod, arena, static_score, record, training, None, stat_rows)
    with persistent_launch(plan.ws), _span("dataflow_run", plan.ws):
        check(lib.dagnn_dataflow_run(C.byref(plan.desc), C.byref(args), _stream(plan.ws)), "dagnn_dataflow_run")
    if score_parts and static_score is None:
        pairs = [(h[d][i], cells[(d, i)].w_key) for d in dirs for i in range(L)]   # (same row pitch, width and N: one launch per 16)
        for o in range(0, len(pairs), 16):
            part = pairs[o:o + 16]
            hp = (C.c_void_p * len(part))(*[t.data_ptr() for t, _ in part])
            wp = (C.c_void_p * len(part))(*[w.data_ptr() for _, w in part])
            check(lib.dagnn_score_parts_batch(hp, wp, len(part), part[0][0].shape[1], H, plan.N, _stream(plan.ws)), "dagnn_score_parts_batch")
    arena.watch(plan, folded=True)


def lib_static_floats(N: int, H: int) -> int:
    return int(_lib.load().dagnn_bwd_dataflow_static_bytes_h(int(N), int(H))) // 4


STAT_FWD = _env_int("DAGNN_AMD_STAT_FWD", 1)   # 1: a training pass's forward launch writes the reverse sweep's static rows itself


def dataflow_args(plan: PlanHandle, dirs: Sequence[int], L: int, H: int, cells, gi0, h, groups: int, vid_mod: int = 0,
                  arena: Optional["GranuleArena"] = None, static_score=None, record: Optional[PassRecord] = None,
                  training: bool = False, args=None, stat_rows: bool = False):
    """The argument struct of `dagnn_dataflow_run` for this pass (a fresh epoch of `arena`'s granule buffers, the plan's
    schedule for `groups`); `args`: fill this struct instead of a new one (the `df` member of `EncodeArgs`)."""
    if args is None:
        args = DataflowArgs()
    gld = H + H // 16
    keys = [(d, i) for d in dirs for i in range(L)] + [("p", d, i) for d in dirs for i in range(1, L)]
    # (projection granules: 16 bytes {tag, r, z, n} per unit = 2 H words of 8 bytes per node)
    gran, epoch, err = arena.get(keys, plan.N, gld, plan.ws.device, widths={k: 2 * H for k in keys if k[0] == "p"})
    mask = 0
    for d in dirs:
        mask |= 1 << d
        for i in range(L):
            c, fc = cells[(d, i)], args.cell[d][i]
            fc.w_hh = c.w_hh_df.data_ptr()
            fc.w_ih = c.w_ih_df.data_ptr() if c.w_ih_df is not None else None
            fc.b_hh, fc.b_ih = c.b_hh.data_ptr(), _ptr(c.b_ih_dev)
            if static_score is not None:
                fc.static_score = _dev(static_score[(d, i)], "static score", torch.float32).data_ptr()
            else:
                fc.w_key = c.w_key.data_ptr()
            fc.edge_gain = _ptr(c.edge_gain) if plan.R > 0 else None
            fc.vid_bias = _ptr(c.vid_bias) if vid_mod > 0 else None
            agg = getattr(c, "agg", 0)
            if agg:   # a plain aggregator (add / max / none): no keys, no gains - the edge encoder itself
                fc.agg, fc.agg_edge_w, fc.agg_edge_b = int(agg), _ptr(getattr(c, "agg_w", None)), _ptr(getattr(c, "agg_b", None))
                fc.w_key = fc.static_score = fc.edge_gain = None
            fc.gi0 = gi0[d].data_ptr() if i == 0 else None
            fc.h_out = h[d][i].data_ptr()
            fc.granules = gran[(d, i)].data_ptr()
            fc.proj_granules = gran[("p", d, i)].data_ptr() if i > 0 else None
            if record is not None and stat_rows:
                # the reverse sweep's static record of every node, rows 1..7 written by this launch (bwd_dataflow_sweep adds
                # row 0); widths other than 256 / 320 leave the columns >= H to the fill
                nfl = lib_static_floats(plan.N, H)
                record.stat[(d, i)] = (torch.empty if H in (256, 320) else torch.zeros)(nfl, dtype=torch.float32, device=plan.ws.device)
                fc.gh_out = record.stat[(d, i)].data_ptr()
                args.stat_rows = 1
            elif record is not None:
                record.gh[(d, i)] = torch.empty(plan.N, 3 * H, dtype=torch.float32, device=plan.ws.device)
                fc.gh_out = record.gh[(d, i)].data_ptr()
                if i > 0:
                    record.gi[(d, i)] = torch.empty(plan.N, 3 * H, dtype=torch.float32, device=plan.ws.device)
                    fc.gi_out = record.gi[(d, i)].data_ptr()
    args.num_stacked, args.dir_mask, args.H, args.ld_h, args.gld = L, mask, H, h[dirs[0]][0].shape[1], gld
    args.pld = H   # (row pitch of the projection granules, in 16-byte granules)
    args.vid_mod, args.groups, args.epoch = int(vid_mod), int(groups), epoch
    sched = plan.dataflow_schedule(groups)
    args.schedule, args.err = sched.data_ptr(), err.data_ptr()
    args.debug_timing = DEBUG_TIMING.data_ptr() if DEBUG_TIMING is not None else None
    args.spin_limit = SPIN_LIMIT
    args.debug_wg = DEBUG_WG
    if DF_XCD:
        args.num_cus = effective_cus(plan.ws.device, training)   # (the placement spreads the workgroups over num_cus / 8 per XCD)
        args.xcc_table = arena.xcc_table(plan.ws.device).data_ptr()
        args.xcd_first = arena.xcd_first
    args.plan_status = plan.status.data_ptr()
    return args


DF_WIDE = _env_int("DAGNN_AMD_DF_WIDE", 1)   # 1: hidden sizes 257..320 run 320 wide on the dataflow kernel (csrc/dataflow_w.hip)


def state_width(H: int, num_stacked: int = 1, num_edge_feats: int = 0, wide_ok: bool = False) -> int:
    """Padded width of a state row on the lock-step path: the next multiple of 64 - except that 256 < H < 512 is padded
    to 512 for a stacked model (and 384 < H for a single-layer one).  512 is the one width the tile kernel (csrc/tiles.hip)
    is built for and the one above 256 whose per-layer kernels, forward and reverse, run on MFMA tiles; padded units stay
    exactly 0 (zero weight rows and biases give r = z = 1/2, n = 0, h' = z * a = 0).  Measured (scripts/tiles_pad.py;
    DESIGN 4f): L >= 2 forward 0.46-0.98x and training step 0.46-0.99x of the unpadded width, one case of 1.06x
    (H = 300, L = 5, B = 32 forward); L = 1 wins from 448 up only, hence the second rule.  `DAGNN_AMD_TILES_PAD=0`
    keeps the next multiple of 64, `=2` pads every 256 < H < 512."""
    Hp = (int(H) + 63) // 64 * 64
    if Hp == 320 and wide_ok and DATAFLOW and DF_WIDE and num_edge_feats == 2:
        # hidden sizes 257..320 (the reference trains at 300, scripts/ogb_tok.sh:17): the dataflow kernel at H = 320 -
        # measured (round 4, B = 160, L = 2): forward 8.7 ms padded to 512 on the tile kernel / launches
        return 320
    if TILES and TILES_PAD and 256 < Hp < 512 and num_edge_feats <= 2 and (num_stacked >= 2 or Hp > 384 or TILES_PAD >= 2):
        Hp = 512
    return Hp


def tiles_launches(device, num_dirs: int, num_stacked: int, H: int, num_edge_feats: int, num_nodes: int = 0) -> int:
    """Launches the weight-stationary tile kernel makes for this model shape on this device; 0 = not applicable, or (with
    the default `DAGNN_AMD_TILES=1`) not the faster path for this depth / batch size."""
    if not TILES:
        return 0
    if TILES == 1 and (num_stacked < 2 or num_nodes > TILES_MAX_NODES):
        return 0
    return _lib.load().dagnn_tiles_launches(_num_cus(device), int(num_dirs), int(num_stacked), int(H), int(num_edge_feats))


def tiles_batch_too_flat(plan: PlanHandle, dirs: Sequence[int]) -> bool:
    """Policy (`DAGNN_AMD_TILES=1`): True for a batch of few, wide layers, which the per-layer launches' 32-row MFMA tiles
    take faster than the tile kernel's 16-row tiles gathered by all 32 slices - D-VAE BN batches at the reference's default
    width, 10 layers deep (scripts/dvae_wide.py, hs = 501, L = 2, both directions, tile kernel : launches): 32 rows per layer
    0.23 : 0.36 ms, 128: 0.46 : 0.50, 192: 0.62 : 0.61, 256: 0.77 : 0.66, 512: 1.42 : 0.99; code2 batches have ~40 rows per
    layer.  Batches of up to 1536 nodes are never too flat (and cost no read of the schedule: the tile kernel walks the
    plan's layers on the device)."""
    if TILES != 1 or TILES_MAX_MEAN_ROWS <= 0 or plan.N <= 1536:
        return False
    sched = plan.read_schedule()
    T = max([len(sched[d]) - 1 for d in dirs] + [1])
    return plan.N > TILES_MAX_MEAN_ROWS * T


def tiles_tail_split(plan: PlanHandle, dirs: Sequence[int]):
    """Where the tile kernel takes over from the per-layer launches on a large batch: per direction the first batch-level
    layer behind which no layer has more than `TILES_TAIL_ROWS` rows - the long thin tail, where a launch per layer costs
    30-50 us and a layer of the tile kernel 12.  None: no tail worth a second kernel (or the split is switched off)."""
    if TILES_TAIL_ROWS <= 0:
        return None
    import numpy as np
    sched = plan.read_schedule()
    first, tail = [0, 0], 0
    for d in dirs:
        rows = np.diff(sched[d].astype(np.int64))
        wide = np.nonzero(rows > TILES_TAIL_ROWS)[0]
        first[d] = int(wide[-1]) + 1 if len(wide) else 0
        tail = max(tail, len(rows) - first[d])
    return first if tail >= 32 else None


def tiles_run(plan: PlanHandle, dirs: Sequence[int], L: int, H: int, cells, gi0, h, arena: "GranuleArena",
              first_layer: Optional[Sequence[int]] = None, vid_mod: int = 0) -> None:
    """The whole recurrence at H = 512 as one persistent launch per chunk of stacked layers (csrc/tiles.hip): the
    weights stay in registers, the rows pass in tiles of 16.  Same operands as `frontier_run` (raw torch-layout
    matrices: nothing is packed); writes the states and the partial attention scores behind them; no device->host
    read."""
    if arena is None:
        raise DagnnHipError("the tile kernel needs a GranuleArena (persistent, zero-initialised progress counters)")
    args = TilesArgs()
    bufs, epoch, err = arena.get(["tiles"], 4096, 1, plan.ws.device)
    mask = 0
    for d in dirs:
        mask |= 1 << d
        for i in range(L):
            c, fc = cells[(d, i)], args.cell[d][i]
            fc.w_hh = c.w_hh_raw.data_ptr()
            fc.b_hh = c.b_hh.data_ptr()
            if i > 0:
                fc.w_ih, fc.b_ih = c.w_ih.data_ptr(), c.b_ih.data_ptr()
            fc.w_key = c.w_key.data_ptr()
            fc.edge_gain = _ptr(c.edge_gain) if plan.R > 0 else None
            fc.gi0 = gi0[d].data_ptr() if i == 0 else None
            fc.h_out = h[d][i].data_ptr()
            fc.vid_bias = _ptr(c.vid_bias) if vid_mod > 0 else None
    args.num_stacked, args.dir_mask, args.H, args.ld_h = L, mask, H, h[dirs[0]][0].shape[1]
    args.num_cus, args.vid_mod = _num_cus(plan.ws.device), int(vid_mod)
    args.epoch, args.counters, args.err = epoch, bufs["tiles"].data_ptr(), err.data_ptr()
    args.spin_limit = SPIN_LIMIT
    args.plan_status = plan.status.data_ptr()
    if first_layer is not None:   # the layers before these are complete already (`frontier_run(stop_layer=...)`)
        for d in dirs:
            args.first_layer[d] = int(first_layer[d])
    args.debug_timing = DEBUG_TIMING.data_ptr() if DEBUG_TIMING is not None else None
    with persistent_launch(plan.ws), _span("tiles_run", plan.ws):
        check(_lib.load().dagnn_tiles_run(C.byref(plan.desc), C.byref(args), _stream(plan.ws)), "dagnn_tiles_run")
    arena.watch(plan, folded=True)


def frontier_ld(H: int) -> int:
    """Row pitch of the lock-step state buffers: H states + H/16 partial scores, 16-byte multiple."""
    return H + (H // 16 + 3) // 4 * 4


class GranuleArena(object):
    """Persistent, zero-initialised granule buffers (tagged 8-byte copies of the state rows) of one
    module on one device, plus the strictly increasing epoch that tags a forward pass.  They must
    outlive single calls: a tag is only meaningful against memory that never held a larger one."""

    def __init__(self):
        self.bufs = {}
        self.cap = 0
        self.gld = 0
        self.epoch = 0
        self.err = None
        self.side = None   # second stream: the persistent kernel runs next to the per-layer launches (split mode)
        self.xcd_first = 0   # XCD the dataflow launches of this arena pack their workgroups from (arenas of further streams: 2, 4, ..)

    def get(self, keys, N: int, gld: int, device, widths=None):
        """`widths`: row pitch (granules) of the buffers that differ from `gld`."""
        widths = widths or {}
        if N > self.cap or gld != self.gld or self.err is None or self.err.device != device or \
                set(keys) != set(self.bufs) or self.epoch >= 0x7FFFFFF0:
            self.cap, self.gld, self.epoch = max(N, int(self.cap * 1.5)), gld, 0
            self.bufs = {k: torch.zeros(self.cap * widths.get(k, gld), dtype=torch.int64, device=device) for k in keys}
            self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self.epoch += 1
        return self.bufs, self.epoch, self.err

    def error_word(self, device) -> torch.Tensor:
        """`err`, made here when no persistent launch has made it yet: the parameter guard of passes that run no persistent
        kernel (the constructor-string variants, the D-VAE `add` / `max` encoders) reports through it too."""
        if self.err is None or self.err.device != device:
            self.err = torch.zeros(1, dtype=torch.int32, device=device)
        return self.err

    def scratch(self, nbytes: int, device) -> torch.Tensor:
        """At least `nbytes` of untyped device scratch (int64 words, 16-byte aligned by the allocator) that kernels of this
        arena's stream fill and consume within one call: grown geometrically, never shrunk, contents undefined."""
        t = getattr(self, "_scratch", None)
        words = (int(nbytes) + 7) // 8
        if t is None or t.device != device or t.numel() < words:
            t = self._scratch = torch.empty(max(words, 0 if t is None or t.device != device else int(t.numel() * 1.5), 1),
                                            dtype=torch.int64, device=device)
        return t

    def xcc_table(self, device):
        """Tagged table the workgroups of a dataflow launch publish their XCD in (zero-initialised once, tagged with the
        arena's epochs like the granule buffers; re-created with them)."""
        t = getattr(self, "_xcc", None)
        if t is None or t.device != device or getattr(self, "_xcc_gen", None) is not self.err:
            t = self._xcc = torch.zeros(1024, dtype=torch.int64, device=device)
            self._xcc_gen = self.err   # (the arena restarts its epochs whenever it re-creates `err`)
        return t

    def side_stream(self, device):
        """Second stream for the split mode (created once): the persistent kernel runs on it next to the per-layer
        launches of the caller's stream."""
        if self.side is None or self.side.device != device:
            self.side = torch.cuda.Stream(device, priority=SIDE_PRIORITY)
        return self.side

    def fork_join_events(self, device):
        """The two events a split-mode call forks and joins with (raw hipEvent_t handles).  They belong to the arena:
        the library itself creates and destroys nothing (include/dagnn_hip.h, conventions)."""
        evs = getattr(self, "_fj", None)
        if evs is None or evs[2] != device:
            a, b = torch.cuda.Event(), torch.cuda.Event()
            st = torch.cuda.current_stream(device)
            a.record(st)   # (torch creates the underlying event at the first record)
            b.record(st)
            evs = self._fj = (a, b, device)
        return evs[0].cuda_event, evs[1].cuda_event

    WATCH_SLOTS = 64   # read-backs in flight before the oldest one is waited for

    def watch(self, plan=None, folded: bool = False) -> None:
        """Queue an asynchronous read-back of the device-side error words (the kernels' bounded-wait flag and the
        plan's contract status) behind the work just launched; `poll()` looks at the finished ones without
        synchronising.  Every watch owns a slot of a pinned ring and an event: an async evaluation loop that issues
        many passes before anything synchronises loses none of their reports (one shared buffer would let a later clean
        pass overwrite a violation).  `folded`: the launch was one of the dataflow kernels, which carry the plan's status
        in bits 8-15 of the error word themselves - one copy instead of two."""
        import collections
        dev = self.err.device
        if getattr(self, "_host", None) is None:
            self._host = torch.zeros(self.WATCH_SLOTS, 2, dtype=torch.int32).pin_memory()
            self._host_err = [self._host[k, 0:1] for k in range(self.WATCH_SLOTS)]
            self._host_status = [self._host[k, 1:2] for k in range(self.WATCH_SLOTS)]
            self._events = [None] * self.WATCH_SLOTS
            self._pending = collections.deque()
            self._seq = 0
        if len(self._pending) >= self.WATCH_SLOTS:
            self._drain(block_first=True)   # (raises if that oldest pass failed)
        slot = self._seq % self.WATCH_SLOTS
        self._seq += 1
        self._host_err[slot].copy_(self.err, non_blocking=True)
        if plan is not None and not folded:
            self._host_status[slot].copy_(plan.status[0:1], non_blocking=True)
        else:
            self._host_status[slot].zero_()
        ev = self._events[slot]   # (the slot's previous watch has been drained: its event is free again)
        if ev is None:
            ev = self._events[slot] = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._pending.append((ev, slot))

    def _drain(self, block: bool = False, block_first: bool = False) -> None:
        pend = getattr(self, "_pending", None)
        failed = None
        while pend:
            ev, slot = pend[0]
            if block or block_first:
                ev.synchronize()
                block_first = False
            elif not ev.query():
                break
            pend.popleft()
            e, s = int(self._host[slot, 0]), int(self._host[slot, 1])
            if e & 0xff00:   # a dataflow kernel found the plan's status word set and reported it in bits 8-15
                s, e = s | ((e >> 8) & 0xff), e & ~0xff00
            if (e or s) and failed is None:
                failed = (e, s)
        if failed is None:
            return
        e, s = failed
        if self.err is not None:
            self.err.zero_()   # the flag is sticky on the device (a lost pass makes later ones give up early): consumed here
        msgs = []
        if e & ERR_PARAMS_MOVED:
            msgs.append("a parameter changed without its version counter moving (a fused optimizer step, a write through "
                        ".data) while the module was in evaluation mode: the pass read derived weights cached from the OLD "
                        "values - call module.train() / .eval() (or .invalidate_caches()) after such an update")
            e &= ~ERR_PARAMS_MOVED
            if not e and not s:
                raise DagnnHipError("results of an earlier DAGNN pass are invalid: " + msgs[0])
        if e & 3:
            msgs.append("a bounded device-side wait expired (code %d): the persistent kernel's workgroups were not "
                        "co-resident, or a producer failed" % e)
        if e & 8:
            msgs.append("the dataflow schedule handed to the kernel was built for another group count (or not built)")
        if (e & 4) and not s:
            msgs.append("the persistent kernel found the plan's status word set (the batch violates the plan contract)")
        if s:
            msgs.append("the batch violates the plan contract (status %d: 1 edges not grouped by graph, 2 edge "
                        "crosses graphs / out of range, 4 batch vector not sorted, 8 layer id out of range)" % s)
        if not msgs:
            msgs.append("device-side error word %d" % e)
        raise DagnnHipError("results of an earlier DAGNN pass are invalid: " + "; ".join(msgs))

    def poll(self, block: bool = False) -> None:
        """Raise `DagnnHipError` if a finished earlier pass reported a device-side failure.  Without `block` this only
        looks at read-backs that have already completed (no synchronisation); with it, at every pass launched so far."""
        self._drain(block=block)

    def check(self) -> None:
        """Synchronising check of every pass launched so far (bounded waits and plan contract)."""
        self._drain(block=True)
        if self.err is not None and int(self.err[0]):
            e = int(self.err[0])
            self.err.zero_()
            if e == ERR_PARAMS_MOVED:
                raise DagnnHipError("a parameter changed without its version counter moving while the module was in evaluation "
                                    "mode: the last pass read stale derived weights (call module.train() / .eval() after such an update)")
            raise DagnnHipError("persistent kernel: a bounded wait expired (results are invalid)")


def frontier_run(plan: PlanHandle, dirs: Sequence[int], L: int, H: int, cells, gi0, h, vid_mod: int = 0,
                 arena: Optional[GranuleArena] = None, static_score=None, stop_layer: Optional[Sequence[int]] = None,
                 chains: Optional[GranuleArena] = None) -> None:
    """Lock-step recurrence over all batch-level layers.  `cells[(d, i)]` are kernel-ready parameter
    holders (core.CellParams); gi0[d] [N,3H]; h[d][i] [N, frontier_ld(H)] outputs.  `chains`: an arena whose side stream
    and events the call may use to run the two directions' launches as two independent chains (no persistent tail in
    the call: `arena` is None or the width has no tail kernel)."""
    args = FrontierArgs()
    mask = 0
    use_tail = arena is not None and TAIL_REPLICAS > 0 and H <= 256
    gran, epoch, err = arena.get([(d, i) for d in dirs for i in range(L)], plan.N, H + H // 16, plan.ws.device) \
        if use_tail else ({}, 0, None)
    for d in dirs:
        mask |= 1 << d
        for i in range(L):
            c, fc = cells[(d, i)], args.cell[d][i]
            fc.granules = gran[(d, i)].data_ptr() if use_tail else None
            fc.w_hh_pk16, fc.w_hh_pk32 = c.w_hh_pk[16].data_ptr(), c.w_hh_pk[32].data_ptr()
            fc.w_hh_mfma = c.w_hh_pk["mfma"].data_ptr()
            if c.w_ih_pk is not None:
                fc.w_ih_pk16, fc.w_ih_pk32 = c.w_ih_pk[16].data_ptr(), c.w_ih_pk[32].data_ptr()
                fc.w_ih_mfma = c.w_ih_pk["mfma"].data_ptr()
            fc.b_hh, fc.b_ih = c.b_hh.data_ptr(), _ptr(c.b_ih_dev)
            if static_score is not None:
                fc.static_score = _dev(static_score[(d, i)], "static score", torch.float32).data_ptr()
            else:
                fc.w_key = c.w_key.data_ptr()
            fc.edge_gain = _ptr(c.edge_gain) if plan.R > 0 else None
            fc.vid_bias = _ptr(c.vid_bias) if vid_mod > 0 else None
            fc.gi0 = gi0[d].data_ptr() if i == 0 else None
            fc.h_out = h[d][i].data_ptr()
    args.num_stacked, args.dir_mask, args.H, args.ld_h, args.vid_mod = L, mask, H, h[dirs[0]][0].shape[1], int(vid_mod)
    args.debug_timing = DEBUG_TIMING.data_ptr() if DEBUG_TIMING is not None else None
    args.num_cus = _num_cus(plan.ws.device)
    args.rb4_max_wgs = RB4_MAX_WGS
    # everything above is independent of the schedule: the one device->host read of the forward pass comes
    # last, so the host-side argument marshalling overlaps the plan / GEMM kernels still in flight
    sched = plan.read_schedule()
    if stop_layer is not None:   # only the batch-level layers before these (the rest: `tiles_run(first_layer=...)`)
        sched = [s_[:min(len(s_), int(stop_layer[d]) + 1)] for d, s_ in enumerate(sched)]
    args.mfma_min_rows = MFMA_MIN_ROWS
    if MFMA_MIN_ROWS > 0:  # fat launches (csrc/fat.hip): scratch rows for the aggregates of rows with more than 4 predecessors
        import numpy as np
        nst = max(len(sched[0]), len(sched[1])) - 1 + L
        widest = 0
        for d in dirs:   # per direction: the two directions' launches may run as two chains, each with its own rows
            width = np.zeros(nst, dtype=np.int64)
            w = np.diff(sched[d].astype(np.int64))
            for i in range(L):  # layer t of stacked layer i runs in launch t + i
                width[i:i + len(w)] += w
            widest += int(width.max())
        plan.agg_scratch = torch.empty(max(widest, 1) * H, dtype=torch.float32, device=plan.ws.device)
        args.agg_scratch, args.agg_scratch_rows = plan.agg_scratch.data_ptr(), widest
    args.tail_replicas, args.tail_max_blocks = (TAIL_REPLICAS if use_tail else 0), TAIL_MAX_BLOCKS
    args.tail_slice_units = TAIL_SLICE
    args.epoch, args.tail_err = epoch, _ptr(err)
    ptrs, nl = _schedule_ptrs(sched)
    if chains is not None and not use_tail and len(dirs) == 2 and DUAL_CHAINS and DEBUG_TIMING is None:
        args.side_stream = chains.side_stream(plan.ws.device).cuda_stream
        args.fork_event, args.join_event = chains.fork_join_events(plan.ws.device)
    if use_tail and SPLIT_DEEP and DEBUG_TIMING is None:
        splits = plan.read_splits()
        args.side_stream = arena.side_stream(plan.ws.device).cuda_stream
        args.fork_event, args.join_event = arena.fork_join_events(plan.ws.device)
        for d in dirs:
            args.layer_split[d] = splits[d].ctypes.data_as(C.POINTER(C.c_int32))
    with persistent_launch(plan.ws), _span("frontier_run", plan.ws):
        check(_lib.load().dagnn_frontier_run(C.byref(plan.desc), C.byref(args), ptrs, nl, _stream(plan.ws)),
              "dagnn_frontier_run")
    if arena is not None and arena.err is not None:
        arena.watch(plan)   # the persistent tail's bounded waits and the plan's status word, like the dataflow path


def recurrence_layer(plan: PlanHandle, dirs: Sequence[int], H: int, gi, w_hh_t, b_hh, w_key, edge_gain=None,
                     vid_bias=None, vid_mod: int = 0, out=None, score=None,
                     static_score: bool = False) -> List[Optional[torch.Tensor]]:
    """One stacked GRU layer over all topological layers.  Per-direction lists indexed by d."""
    dev = plan.ws.device
    h = [None, None]
    args = LayerArgs()
    keep = []
    mask = 0
    for d in dirs:
        mask |= 1 << d
        h[d] = out[d] if out is not None else torch.empty(plan.N, H, dtype=torch.float32, device=dev)
        sc = score[d] if score is not None else torch.empty(plan.N, dtype=torch.float32, device=dev)
        ts = [_dev(gi[d], "gi", torch.float32), _dev(w_hh_t[d], "w_hh_t", torch.float32),
              _dev(b_hh[d], "b_hh", torch.float32),
              sc if static_score else _dev(w_key[d], "w_key", torch.float32)]
        eg = _dev(edge_gain[d], "edge_gain", torch.float32) if (edge_gain is not None and plan.R > 0) else None
        vb = _dev(vid_bias[d], "vid_bias", torch.float32) if (vid_bias is not None and vid_mod > 0) else None
        keep += ts + [eg, vb, sc]
        args.gi[d], args.w_hh_t[d], args.b_hh[d], args.w_key[d] = (t.data_ptr() for t in ts)
        args.edge_gain[d], args.vid_bias[d] = _ptr(eg), _ptr(vb)
        args.h[d], args.score[d] = h[d].data_ptr(), sc.data_ptr()
    args.vid_mod, args.ld_h, args.static_score = int(vid_mod), H, int(static_score)
    args.debug_timing = DEBUG_TIMING.data_ptr() if DEBUG_TIMING is not None else None
    with _span("recurrence_layer", plan.ws):
        check(_lib.load().dagnn_recurrence_layer(C.byref(plan.desc), C.byref(args), mask, H, _stream(plan.ws)),
              "dagnn_recurrence_layer")
    return h


_POOL_MODES = {"max": _lib.POOL_MAX, "add": _lib.POOL_ADD, "sum": _lib.POOL_ADD, "mean": _lib.POOL_MEAN}


def readout_pool_batch(plan: PlanHandle, jobs, out: torch.Tensor) -> None:
    """(h, scope, how, col_off) jobs in ONE launch (`dagnn_readout_pool_batch`): out[:, col_off : col_off + width] = max /
    add / mean pool of h over scope 0 / 1 (output nodes of that direction) or 2 (all nodes of the graph).  Longer job
    lists go in chunks of `MAX_READOUT_JOBS`."""
    if not jobs:
        return
    lib = _lib.load()
    for k0 in range(0, len(jobs), _lib.MAX_READOUT_JOBS):
        part = jobs[k0:k0 + _lib.MAX_READOUT_JOBS]
        arr = (_lib.PoolJob * len(part))()
        keep = []
        for q, (h, scope, how, col) in enumerate(part):
            h = _rows(h, "hidden states")
            keep.append(h)
            arr[q] = _lib.PoolJob(h.data_ptr(), h.stride(0), h.shape[1], int(scope), _POOL_MODES[how], int(col))
        check(lib.dagnn_readout_pool_batch(C.byref(plan.desc), arr, len(part), out.data_ptr(), out.stride(0), _stream(out)),
              "dagnn_readout_pool_batch")


def readout_pool_backward_batch(plan: PlanHandle, jobs, grad_out: torch.Tensor) -> None:
    """The backward of `readout_pool_batch`: (h, scope, how, col_off, grad_h) jobs, `grad_h[v] +=` node v's share of
    `grad_out[:, col_off : col_off + width]`, ONE launch per `MAX_READOUT_JOBS` jobs (distinct `grad_h` each; `grad_h`
    [N, >= width] is initialised by the caller and may be row-pitched).  `h` is read for 'max' only: None otherwise is fine,
    the width is `h`'s or, without it, `grad_h`'s."""
    if not jobs:
        return
    grad_out = _dev(grad_out, "grad_out", torch.float32)
    lib = _lib.load()
    for k0 in range(0, len(jobs), _lib.MAX_READOUT_JOBS):
        part = jobs[k0:k0 + _lib.MAX_READOUT_JOBS]
        arr = (_lib.PoolBwdJob * len(part))()
        keep = []
        for q, (h, scope, how, col, gh) in enumerate(part):
            mode = _POOL_MODES[how]
            if mode == _lib.POOL_MAX:
                h = _rows(h, "h")
                keep.append(h)
            width = h.shape[1] if h is not None else gh.shape[1]
            if gh.dtype != torch.float32 or gh.stride(1) != 1 or gh.shape[1] < width:
                raise DagnnHipError("readout_pool_backward_batch: grad_h must be fp32 rows of at least the pooled width")
            arr[q] = _lib.PoolBwdJob(h.data_ptr() if mode == _lib.POOL_MAX else None, gh.data_ptr(),
                                     h.stride(0) if mode == _lib.POOL_MAX else 0, gh.stride(0), width, int(scope), mode, int(col))
        check(lib.dagnn_readout_pool_backward_batch(C.byref(plan.desc), arr, len(part), grad_out.data_ptr(), grad_out.stride(0),
                                                    _stream(grad_out)), "dagnn_readout_pool_backward_batch")


def attn_grads(jobs):
    """Gradients of attn_lin.weight / edge_encoder.{weight, bias} of every cell from the epilogue's column sums, ONE launch
    (`dagnn_attn_grads_run`).  `jobs`: list of dicts {key_sum [kd], feat_sum [R] | None, sigma_sum [1] | None, edge_w [kd, R] |
    None, edge_b, attn_w [1, attn_len], dq}; returns a list of (g_attn [1, attn_len], g_edge_w | None, g_edge_b | None) - views of
    one buffer."""
    lib = _lib.load()
    dev = jobs[0]["attn_w"].device
    sizes = []
    for j in jobs:
        kd = j["key_sum"].numel()
        R = j["edge_w"].shape[1] if j["edge_w"] is not None else 0
        sizes.append((j["attn_w"].shape[1], kd * R, kd if R else 0))
    buf = torch.empty(sum(a + b + c for a, b, c in sizes), dtype=torch.float32, device=dev)
    out, off = [], 0
    arr = (_lib.AttnGradJob * len(jobs))()
    keep = []
    for q, (j, (a, b, c)) in enumerate(zip(jobs, sizes)):
        g_attn = buf[off:off + a].view(1, a); off += a
        g_ew = buf[off:off + b].view(-1, j["edge_w"].shape[1]) if b else None; off += b
        g_eb = buf[off:off + c] if c else None; off += c
        t = {k: (None if j[k] is None else j[k].detach().contiguous()) for k in ("key_sum", "feat_sum", "sigma_sum", "edge_w", "edge_b", "attn_w")}
        keep.append(t)
        kd = t["key_sum"].numel()
        arr[q] = _lib.AttnGradJob(t["key_sum"].data_ptr(), _ptr(t["feat_sum"]), _ptr(t["sigma_sum"]), _ptr(t["edge_w"]), _ptr(t["edge_b"]),
                                  t["attn_w"].data_ptr(), g_attn.data_ptr(), _ptr(g_ew), _ptr(g_eb), int(j["dq"]), kd, a,
                                  0 if t["edge_w"] is None else t["edge_w"].shape[1])
        out.append((g_attn, g_ew, g_eb))
    for k0 in range(0, len(jobs), _lib.ATTN_GRAD_MAX_JOBS):
        n = min(_lib.ATTN_GRAD_MAX_JOBS, len(jobs) - k0)
        sub = (_lib.AttnGradJob * n)(*[arr[k0 + i] for i in range(n)])
        check(lib.dagnn_attn_grads_run(sub, n, _stream(buf)), "dagnn_attn_grads_run")
    return out


def _schedule_ptrs(sched):
    """(ptrs, nl) of a lock-step launch: per direction the schedule's layer offsets (arrays the caller keeps) and layer count."""
    ptrs = (C.POINTER(C.c_int32) * 2)(*[sched[d].ctypes.data_as(C.POINTER(C.c_int32)) for d in (0, 1)])
    return ptrs, (C.c_int32 * 2)(*[len(sched[d]) - 1 for d in (0, 1)])


def _key_side(bc, c, o, h, score, H: int, R: int, vid_mod: int, keep: list) -> torch.Tensor:
    """Key-side fields of one `BackwardCell`; returns the key in use (`score`: keys from the inputs - a zero key, held by `keep`)."""
    key = c.w_key
    if score is not None:
        key = torch.zeros(H, dtype=torch.float32, device=h.device)
        keep.append(key)
        bc.static_score = _dev(score, "static score", torch.float32).data_ptr()
    bc.w_key = key.data_ptr()
    bc.edge_gain = _ptr(c.edge_gain) if R > 0 else None
    bc.vid_bias = _ptr(c.vid_bias) if vid_mod > 0 else None
    bc.h, bc.a, bc.alpha = h.data_ptr(), o["a"].data_ptr(), o["alpha"].data_ptr()
    return key


def _recompute_preact(keys, cells, out, h, H: int, gi: dict) -> dict:
    """gh of every cell (returned) and gi above layer 0 (into `gi`), recomputed by batched MFMA GEMMs: every h is known."""
    gh = {}
    for k0 in range(0, len(keys), 4):
        grp = keys[k0:k0 + 4]
        gh.update(zip(grp, gemm_nt_bias([out[k]["a"] for k in grp], [cells[k].w_hh_raw for k in grp], [cells[k].b_hh for k in grp])))
    up = [k for k in keys if k[1] > 0]
    for k0 in range(0, len(up), 4):
        grp = up[k0:k0 + 4]
        gi.update(zip(grp, gemm_nt_bias([h[d][i - 1][:, :H] for d, i in grp], [cells[k].w_ih for k in grp], [cells[k].b_ih for k in grp])))
    return gh


def backward_sweep(plan: PlanHandle, dirs: Sequence[int], L: int, H: int, cells, h, gi0, g_ext,
                   arena: Optional[GranuleArena] = None, vid_mod: int = 0, static_score=None):
    """Reverse pass of the lock-step recurrence (csrc/backward.hip).  `h[d][i]` [N, frontier_ld(H)] are the
    forward state buffers, `gi0[d]` [N,3H] the input-side pre-activations of stacked layer 0, `g_ext[d][i]`
    [N,H] the gradients reaching the states from outside (modified: stacked layers below the top receive the
    upper layer's input gradient).  Returns per cell (d, i) a dict with a, dgi, dgh, sigma, edge_feat_grad."""
    dev = plan.ws.device
    N, E, R = plan.N, plan.E, plan.R
    args = BackwardArgs()
    out = {}
    mask = 0
    f32 = dict(dtype=torch.float32, device=dev)
    use_tail = arena is not None and BWD_TAIL_REPLICAS > 0 and H <= 256
    gkeys = [("da", d, i) for d in dirs for i in range(L)] + [("du", d, i) for d in dirs for i in range(L - 1)]
    gran, epoch, err = arena.get(gkeys, N, H, dev) if use_tail else ({}, 0, None)
    keep = []
    if arena is not None:
        arena.poll()
    for d in dirs:
        mask |= 1 << d
        for i in range(L):
            c, bc = cells[(d, i)], args.cell[d][i]
            if use_tail:
                bc.da_granules = gran[("da", d, i)].data_ptr()
                if i + 1 < L:   # the sweep adds the upper layer's du into g_ext: keep what it was before
                    static = g_ext[d][i].clone()
                    keep.append(static)
                    bc.du_granules, bc.g_ext_static = gran[("du", d, i)].data_ptr(), static.data_ptr()
            o = dict(a=torch.empty(N, H, **f32), alpha=torch.empty(max(E, 1), **f32), da=torch.empty(N, H, **f32),
                     dgi=torch.empty(N, 3 * H, **f32), dgh=torch.empty(N, 3 * H, **f32), sigma=torch.empty(N, **f32),
                     edge_feat_grad=torch.empty(N, R, **f32) if R > 0 else None)
            out[(d, i)] = o
            bc.w_hh, bc.w_ih = c.w_hh_raw.data_ptr(), (c.w_ih.data_ptr() if i > 0 else None)
            _key_side(bc, c, o, h[d][i], None if static_score is None else static_score[(d, i)], H, R, vid_mod, keep)
            bc.g_ext, bc.da, bc.dgi, bc.dgh = g_ext[d][i].data_ptr(), o["da"].data_ptr(), o["dgi"].data_ptr(), o["dgh"].data_ptr()
            bc.sigma, bc.edge_feat_grad = o["sigma"].data_ptr(), _ptr(o["edge_feat_grad"])
    args.num_stacked, args.dir_mask, args.H, args.ld_h = L, mask, H, h[dirs[0]][0].shape[1]
    args.vid_mod = int(vid_mod)
    args.num_cus = _num_cus(dev)
    args.thin_wgs = BWD_THIN_WGS
    args.tail_replicas, args.tail_max_blocks = (BWD_TAIL_REPLICAS if use_tail else 0), BWD_TAIL_MAX_BLOCKS
    args.epoch, args.tail_err = epoch, _ptr(err)
    lib = _lib.load()
    with _span("backward_prepare", plan.ws):
        check(lib.dagnn_backward_prepare(C.byref(plan.desc), C.byref(args), _stream(plan.ws)), "dagnn_backward_prepare")
    keys = [(d, i) for d in dirs for i in range(L)]
    gi = {(d, 0): gi0[d] for d in dirs}
    gh = _recompute_preact(keys, cells, out, h, H, gi)
    for k in keys:
        args.cell[k[0]][k[1]].gi, args.cell[k[0]][k[1]].gh = gi[k].data_ptr(), gh[k].data_ptr()
        out[k]["gi"], out[k]["gh"] = gi[k], gh[k]
    sched = plan.read_schedule()
    ptrs, nl = _schedule_ptrs(sched)
    if use_tail and SPLIT_DEEP:
        splits = plan.read_splits()
        args.side_stream = arena.side_stream(dev).cuda_stream
        args.fork_event, args.join_event = arena.fork_join_events(dev)
        for d in dirs:
            args.layer_split[d] = splits[d].ctypes.data_as(C.POINTER(C.c_int32))
    with persistent_launch(plan.ws), _span("backward_run", plan.ws):
        check(lib.dagnn_backward_run(C.byref(plan.desc), C.byref(args), ptrs, nl, _stream(plan.ws)),
              "dagnn_backward_run")
    if use_tail:
        arena.watch()
    return out


def pack_dataflow_transposed(w: torch.Tensor, H: int) -> torch.Tensor:
    """[3H, H] (torch layout) -> the dataflow kernel's slice / lane order of the GATE-WISE TRANSPOSED matrix
    (out[g H + j][u] = W[g H + u][j]): the A operands of the reverse products W^T dg."""
    w = _dev(w, "weight", torch.float32)
    if tuple(w.shape) != (3 * H, H):
        raise DagnnHipError("pack_dataflow_transposed needs a [3H, H] matrix, got %s" % (tuple(w.shape),))
    out = torch.empty(3 * H * H, dtype=torch.float32, device=w.device)
    check(_lib.load().dagnn_pack_dataflow_transposed(w.data_ptr(), out.data_ptr(), H, _stream(w)),
          "dagnn_pack_dataflow_transposed")
    return out


# cap on what the reverse dataflow sweep may keep: unset (-1) = a third of the device's memory (96 GB on an MI355X); a value is
# taken as it is - 0 switches the reverse dataflow sweep off (every training pass then takes the reverse lock-step launches)
BWD_DF_MAX_BYTES = _env_int("DAGNN_AMD_BWD_DF_MAX_BYTES", -1)


_TOTAL_MEMORY = {}


def _total_memory(device) -> int:
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _TOTAL_MEMORY:
        _TOTAL_MEMORY[key] = int(torch.cuda.get_device_properties(key).total_memory)
    return _TOTAL_MEMORY[key]


def bwd_dataflow_fits(device, N: int, cells: int) -> bool:
    """The persistent reverse sweep keeps ONE 8 KB (H = 320: 10 KB) static record per (cell, node)
    (`dagnn_bwd_dataflow_static_bytes`) whatever H is, plus - about as much again, twice at H = 256 - the 256-byte
    successor records, the hand-off granules (`da`, `dgi`, `du`) and the forward pass's pre-activations: ~1.5 GB for the
    headline batch, tens of GB for a very large batch at H = 64.  The choice between the sweep and the reverse
    lock-step launches (`backward_sweep`, which need none of it) is a pure function of (device model, N, cells): the byte cap
    is a third of the device's TOTAL memory (96 GB on an MI355X; `DAGNN_AMD_BWD_DF_MAX_BYTES` overrides it, 0 = never) - not
    of the memory that happens to be free - so every rank and every step takes the same reverse path and gradients stay
    bitwise reproducible run to run, and a smaller device falls back to the launches instead of running out of memory."""
    need = int(_lib.load().dagnn_bwd_dataflow_static_bytes(int(N))) * int(cells) * 3   # records x 1.25 (H = 320) + granules + preact
    cap = BWD_DF_MAX_BYTES
    if cap < 0:
        cap = _total_memory(device) // 3
    return need <= cap


def bwd_dataflow_sweep(plan: PlanHandle, dirs: Sequence[int], L: int, H: int, cells, h, gi0, g_ext, groups: int,
                       arena: "GranuleArena", vid_mod: int = 0, static_score=None, record: Optional[PassRecord] = None,
                       plain: Optional[dict] = None):
    """Reverse pass of the recurrence as ONE persistent dataflow launch (csrc/bwd_dataflow.hip).  Same operands as
    `backward_sweep`, returns (its result dictionary, the buffers the launch reads); `groups` must be the group count of the
    forward pass's schedule, `record` says what the forward launch handed over (`PassRecord.handover`).
    `plain` (agg = add / max, `variants.PlainRecurrence`): {(d, i): (a [N, H] contiguous, pull)} - the aggregates and the
    pull weights the caller prepared instead of `dagnn_backward_prepare`'s: `pull` is [E] (add: ones, or zeros for a cell
    that aggregates nothing), or with `plain["pull_rows"]` (max) [E, _lib.PULL_ROW] per-unit weight rows; the keys are
    zeros, and every cell's result also carries its `da_granules` [N, H] (the edge encoder's gradient reads them)."""
    dev = plan.ws.device
    N, E, R = plan.N, plan.E, plan.R
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=dev)
    arena.poll()
    out, keep, wkey = {}, [], {}
    pargs = BackwardArgs()
    mask = 0
    for d in dirs:
        mask |= 1 << d
        for i in range(L):
            o = dict(a=plain[(d, i)][0] if plain else torch.empty(N, H, **f32),
                     alpha=plain[(d, i)][1] if plain else torch.empty(max(E, 1), **f32),
                     dgi=torch.empty(N, 3 * H, **f32), dgh=torch.empty(N, 3 * H, **f32), sigma=torch.empty(N, **f32),
                     edge_feat_grad=torch.empty(N, R, **f32) if R > 0 else None)
            out[(d, i)] = o
            if plain:
                wkey[(d, i)] = torch.zeros(H, **f32)
                keep.append(wkey[(d, i)])
            else:
                wkey[(d, i)] = _key_side(pargs.cell[d][i], cells[(d, i)], o, h[d][i],
                                         None if static_score is None else static_score[(d, i)], H, R, vid_mod, keep)
    pargs.num_stacked, pargs.dir_mask, pargs.H, pargs.ld_h = L, mask, H, h[dirs[0]][0].shape[1]
    pargs.vid_mod = int(vid_mod)
    with _span("backward_prepare", plan.ws):
        if not plain:
            check(lib.dagnn_backward_prepare(C.byref(plan.desc), C.byref(pargs), _stream(plan.ws)), "dagnn_backward_prepare")
        keys = [(d, i) for d in dirs for i in range(L)]
        kept = record.handover() if record is not None else None
        stat_fwd = kept == "stat"   # the forward launch wrote rows 1..7 (`Route.stat_rows`)
        gh, gi = {}, ({} if stat_fwd else {(d, 0): gi0[d] for d in dirs})
        if kept == "preact":   # the forward kernel kept the pre-activations of this pass
            gh = record.gh
            gi.update(record.gi)
        elif not stat_fwd:
            gh = _recompute_preact(keys, cells, out, h, H, gi)
        gkeys = [("da", d, i) for d in dirs for i in range(L)] + [("q", d, i) for d in dirs for i in range(L)] + \
                [("dgi", d, i) for d in dirs for i in range(1, L)] + [("du", d, i) for d in dirs for i in range(L - 1)]
        widths = {k: (1 if k[0] == "q" else 3 * H) for k in gkeys if k[0] in ("q", "dgi")}
        gran, epoch, err = arena.get(gkeys, N, H, dev, widths=widths)
        args = BwdDataflowArgs()
        stat_bytes = lib.dagnn_bwd_dataflow_static_bytes_h(N, H)
        for k in keys:
            d, i = k
            c, bc, o = cells[k], args.cell[d][i], out[k]
            o["gi"], o["gh"] = gi.get(k), gh.get(k)
            if getattr(c, "w_hh_bt", None) is None:
                c.w_hh_bt = pack_dataflow_transposed(c.w_hh_raw, H)
                c.w_ih_bt = pack_dataflow_transposed(c.w_ih, H) if i > 0 else None
            stat = record.stat[k] if stat_fwd else torch.empty(stat_bytes // 4, **f32)
            keep.append(stat)
            bc.w_hh_t, bc.w_ih_t = c.w_hh_bt.data_ptr(), _ptr(c.w_ih_bt)
            bc.w_key, bc.alpha = wkey[k].data_ptr(), o["alpha"].data_ptr()
            bc.gi, bc.gh, bc.a, bc.b_hh = _ptr(gi.get(k)), _ptr(gh.get(k)), o["a"].data_ptr(), c.b_hh.data_ptr()
            bc.h, bc.g_ext, bc.stat = h[d][i].data_ptr(), g_ext[d][i].data_ptr(), stat.data_ptr()
            bc.da_granules, bc.q_granules = gran[("da", d, i)].data_ptr(), gran[("q", d, i)].data_ptr()
            bc.dgi_granules = gran[("dgi", d, i)].data_ptr() if i > 0 else None
            bc.du_granules = gran[("du", d, i)].data_ptr() if i + 1 < L else None
            bc.dgi, bc.dgh, bc.sigma = o["dgi"].data_ptr(), o["dgh"].data_ptr(), o["sigma"].data_ptr()
            bc.edge_feat_grad = _ptr(o["edge_feat_grad"])
        args.num_stacked, args.dir_mask, args.H = L, mask, H
        args.ld_h, args.ld_g, args.gld, args.groups = h[dirs[0]][0].shape[1], g_ext[dirs[0]][0].shape[1], H, int(groups)
        args.epoch, args.spin_limit = epoch, SPIN_LIMIT
        args.stat_rows_written = 1 if stat_fwd else 0
        args.pull_rows = 1 if (plain and plain.get("pull_rows")) else 0
        sched = plan.dataflow_schedule(groups)
        recs = torch.empty(lib.dagnn_bwd_dataflow_record_bytes(N) // 4, dtype=torch.int32, device=dev)
        keep.append(recs)
        args.schedule, args.records, args.err = sched.data_ptr(), recs.data_ptr(), err.data_ptr()
        args.plan_status = plan.status.data_ptr()
        if DF_XCD:
            args.num_cus = effective_cus(dev, True)
            args.xcc_table = arena.xcc_table(dev).data_ptr()
            args.xcd_first = arena.xcd_first
        check(lib.dagnn_bwd_dataflow_prepare(C.byref(plan.desc), C.byref(args), _stream(plan.ws)), "dagnn_bwd_dataflow_prepare")
    with persistent_launch(plan.ws), _span("backward_run", plan.ws):
        check(lib.dagnn_bwd_dataflow_run(C.byref(plan.desc), C.byref(args), _stream(plan.ws)), "dagnn_bwd_dataflow_run")
    arena.watch(plan, folded=True)
    if plain:
        for k, o in out.items():
            o["da_granules"] = gran[("da",) + k]
    return out, keep   # (`keep`: buffers the launch reads - the caller holds them until its backward returns)


_WGRAD_WS = {}   # per (kind, device, stream): the partial-tile workspaces of `wgrad` / `colsums` (grown on demand, reused by
                 # every step of that stream; backward passes on different streams of one device never share a buffer)
WGRAD_MAX_JOBS = 32   # jobs one `dagnn_wgrad_run` / `dagnn_colsum_run` call takes (WG_MAX_JOBS / CS_MAX_JOBS in csrc/wgrad.hip)


def _wgrad_ws(kind: str, ref: torch.Tensor, nbytes: int) -> torch.Tensor:
    key = (kind, ref.device, _stream(ref))
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        # (a grown buffer replaces one that launches already queued on this stream may still read: stream-ordered
        # allocation keeps the old block alive until they have run)
        ws = _WGRAD_WS[key] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=ref.device)
    return ws


def wgrad(jobs, N: int, Hp: int, H: int):
    """Weight / bias gradients of GRU cells in one batch (`dagnn_wgrad_run`).  `jobs`: list of (dg [N, >= 3 Hp], inp
    [N, in_dim] (row pitch kept), want_bias); returns a list of (d_weight [3H, in_dim], d_bias [3H] or None).  More than
    WGRAD_MAX_JOBS jobs (bidirectional models of more than 8 stacked layers) go in several launches."""
    if len(jobs) > WGRAD_MAX_JOBS:
        out = []
        for k in range(0, len(jobs), WGRAD_MAX_JOBS):
            out += wgrad(jobs[k:k + WGRAD_MAX_JOBS], N, Hp, H)
        return out
    lib = _lib.load()
    dev = jobs[0][0].device
    arr = (_lib.WgradJob * len(jobs))()
    outs, keep = [], []
    kmax = 0
    for q, (dg, inp, want_bias) in enumerate(jobs):
        dg, inp = _rows(dg, "dg"), _rows(inp, "wgrad input")
        K0 = K2 = inp.shape[1]
        if K2 % 2:   # the kernel reads input columns in pairs (an odd width: the reference's default hs = 501, dvae/train.py:55)
            if inp.stride(0) > K2 and inp.stride(0) % 2 == 0:   # a view of wider rows: take the next word of each row along (its
                inp = inp.as_strided((inp.shape[0], K2 + 1), inp.stride())   # column of d_weight is dropped below)
            else:
                inp = torch.nn.functional.pad(inp, (0, 1))
            K2 += 1
        keep += [dg, inp]
        kmax = max(kmax, K2)
        dW = torch.empty(3 * H, K2, dtype=torch.float32, device=dev)
        db = torch.empty(3 * H, dtype=torch.float32, device=dev) if want_bias else None
        outs.append((dW if K2 == K0 else dW[:, :K0], db))
        arr[q] = _lib.WgradJob(dg.data_ptr(), inp.data_ptr(), dW.data_ptr(), _ptr(db), dg.stride(0), inp.stride(0), K2)
    cus = _num_cus(dev)
    splits = max(lib.dagnn_wgrad_splits(cus, len(jobs), Hp, kmax, max(N, 1)), 1)
    nbytes = lib.dagnn_wgrad_workspace_bytes(len(jobs), Hp, kmax, splits)
    ws = _wgrad_ws("wg", jobs[0][0], nbytes)
    check(lib.dagnn_wgrad_run(arr, len(jobs), N, Hp, H, splits, ws.data_ptr(), ws.numel() * 4, _stream(jobs[0][0])),
          "dagnn_wgrad_run")
    return [(dW if dW.is_contiguous() else dW.contiguous(), db) for dW, db in outs]


def colsums(jobs, N: int):
    """Weighted column sums in one batch (`dagnn_colsum_run`).  `jobs`: list of (x [N, cols] (row pitch kept; a 1-d
    tensor counts as [N, 1]), weight [N] or None); returns the list of [cols] sums.  More than WGRAD_MAX_JOBS jobs (a
    bidirectional model with edge features has three per cell: 12 cells = 36) go in several launches."""
    if len(jobs) > WGRAD_MAX_JOBS:
        out = []
        for k in range(0, len(jobs), WGRAD_MAX_JOBS):
            out += colsums(jobs[k:k + WGRAD_MAX_JOBS], N)
        return out
    lib = _lib.load()
    dev = jobs[0][0].device
    arr = (_lib.ColsumJob * len(jobs))()
    outs, keep = [], []
    kmax = 0
    for q, (x, w) in enumerate(jobs):
        x = x.view(-1, 1) if x.dim() == 1 else x
        if not (x.is_cuda and x.dtype == torch.float32 and x.stride(1) == 1):
            x = _dev(x, "colsum input", torch.float32)
        w = None if w is None else _dev(w, "colsum weight", torch.float32)
        keep += [x, w]
        o = torch.empty(x.shape[1], dtype=torch.float32, device=dev)
        outs.append(o)
        kmax = max(kmax, x.shape[1])
        arr[q] = _lib.ColsumJob(x.data_ptr(), _ptr(w), o.data_ptr(), x.stride(0) if x.shape[0] > 1 else x.shape[1], x.shape[1])
    nbytes = lib.dagnn_colsum_workspace_bytes(len(jobs), kmax)
    ws = _wgrad_ws("cs", jobs[0][0], nbytes)
    check(lib.dagnn_colsum_run(arr, len(jobs), N, ws.data_ptr(), ws.numel() * 4, _stream(jobs[0][0])), "dagnn_colsum_run")
    return outs


def table_grads(g: torch.Tensor, keys: Sequence[torch.Tensor], rows: Sequence[int], stages: int = 0,
                workspace: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """Embedding-table gradients in the one summation order of `dagnn_table_grads` (include/dagnn_hip.h; the host mirror
    is `autograd.table_grads_host`): out_t[r] = sum of g[v] over the nodes with keys[t][v] == r, bitwise repeatable, no float
    atomics.  g [N, H] fp32 (row pitch kept), H % 4 == 0; keys: int64 [N] tensors, strided views allowed (the columns of one
    [N, 2] tensor); rows: the tables' row counts.  Returns one [rows[t], H] tensor per table.
    `stages` / `workspace` (at most three tables): the index launches (`_lib.TABLE_GRADS_INDEX`) or the sum launches
    (`_lib.TABLE_GRADS_SUM`) alone, over a workspace the caller keeps between the two (scripts/bench_table_grads.py)."""
    lib = _lib.load()
    g = _rows(g, "g")
    N, H = g.shape
    outs = []
    if (stages or workspace is not None) and len(keys) > _lib.TABLE_GRADS_MAX_TABLES:
        raise DagnnHipError("table_grads: stages / workspace take at most %d tables" % _lib.TABLE_GRADS_MAX_TABLES)
    with _span("table_grads", g):
        for t0 in range(0, len(keys), _lib.TABLE_GRADS_MAX_TABLES):
            ks, rs = list(keys[t0:t0 + _lib.TABLE_GRADS_MAX_TABLES]), [int(r) for r in rows[t0:t0 + _lib.TABLE_GRADS_MAX_TABLES]]
            a = _lib.TableGradsArgs()
            a.g, a.ld_g, a.N, a.H, a.num_tables = g.data_ptr(), g.stride(0) if N > 1 else max(g.stride(0), H), N, H, len(ks)
            for t, (k, R) in enumerate(zip(ks, rs)):
                if not isinstance(k, torch.Tensor) or not k.is_cuda or k.dim() != 1 or k.shape[0] != N:
                    raise DagnnHipError("table_grads: keys[%d] must be a GPU tensor of %d entries (got %s)" % (
                        t0 + t, N, getattr(k, "shape", type(k))))
                if k.dtype != torch.int64 or (N > 1 and k.stride(0) < 0):
                    k = k.to(torch.int64).contiguous()
                    ks[t] = k   # (keeps the copy alive until the launches are queued: stream-ordered allocation does the rest)
                out = torch.empty(R, H, dtype=torch.float32, device=g.device)
                outs.append(out)
                a.table[t] = _lib.TableGradsTable(k.data_ptr(), k.stride(0) if N > 1 else 1, R, out.data_ptr(), H)
            nbytes = lib.dagnn_table_grads_workspace_bytes(N, H, (C.c_int64 * len(rs))(*rs), len(rs))
            if nbytes == 0:
                raise DagnnHipError("table_grads: shape out of range (N = %d, H = %d, rows = %s)" % (N, H, rs))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device) if workspace is None else workspace
            a.workspace, a.workspace_bytes, a.stages = ws.data_ptr(), ws.numel() * ws.element_size(), stages
            check(lib.dagnn_table_grads(C.byref(a), _stream(g)), "dagnn_table_grads")
    return outs


def gather_rows(h: torch.Tensor, num_graphs: int, stride: int, node_off: int, out: torch.Tensor,
                col_off: int) -> None:
    h = _dev(h, "h", torch.float32)
    check(_lib.load().dagnn_gather_rows(h.data_ptr(), h.shape[1], h.shape[1], num_graphs, stride, node_off,
                                        out.data_ptr(), out.shape[1], col_off, _stream(h)), "dagnn_gather_rows")


def iprop_step(values: Optional[torch.Tensor], pred_vid: Optional[torch.Tensor], w_key: Optional[torch.Tensor],
               vid_bias: Optional[torch.Tensor], H_given: Optional[torch.Tensor], x: torch.Tensor, cells,
               key_type: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`_ipropagate_to` for all graphs of a decoder step in one launch (`dagnn_iprop_step`).  values [B,P,hs] /
    pred_vid [B,P] int32 (or None with `H_given` [B,hs]); x [B,in0]; cells: the propagator's GRUCells.  Returns the
    new states [L,B,hs].  `key_type` [nvt] (attn_x, `dagnn_iprop_step_typed`): `pred_vid` then holds the predecessors'
    vertex TYPES and w_key / vid_bias are not read."""
    x = _dev(x, "x", torch.float32)
    B, in0 = x.shape
    hs = cells[0].weight_hh.shape[1]
    L = len(cells)
    P = 0
    if H_given is not None:
        H_given = _dev(H_given, "H", torch.float32)
    elif values is not None:
        values = _dev(values, "predecessor states", torch.float32)
        pred_vid = _dev(pred_vid, "predecessor ids", torch.int32)
        P = values.shape[1]
    layers = (_lib.IpropLayer * L)()
    keep = []
    for l, c in enumerate(cells):
        ts = [_dev(t.detach(), "GRU parameter", torch.float32) for t in (c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh)]
        keep.append(ts)
        layers[l] = _lib.IpropLayer(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), ts[0].shape[1])
    states = torch.empty(L, B, hs, dtype=torch.float32, device=x.device)
    if H_given is None and P == 0:   # no graph has a predecessor: the aggregate is zero (`_get_zero_hidden`)
        H_given = torch.zeros(B, hs, dtype=torch.float32, device=x.device)
    if key_type is not None:
        kt = _dev(key_type.detach(), "key_type", torch.float32)
        check(_lib.load().dagnn_iprop_step_typed(_ptr(values), _ptr(pred_vid), B, P, hs, kt.data_ptr(), kt.shape[0], _ptr(H_given),
                                                 x.data_ptr(), in0, layers, L, states.data_ptr(), _stream(x)),
              "dagnn_iprop_step_typed")
        return states
    wk = _dev(w_key.detach(), "w_key", torch.float32)
    vb = None if vid_bias is None else _dev(vid_bias.detach(), "vid_bias", torch.float32)
    check(_lib.load().dagnn_iprop_step(_ptr(values), _ptr(pred_vid), B, P, hs, wk.data_ptr(), _ptr(vb), _ptr(H_given),
                                       x.data_ptr(), in0, layers, L, states.data_ptr(), _stream(x)), "dagnn_iprop_step")
    return states


def gather_rows_batch(jobs, num_graphs: int, stride: int, out: torch.Tensor) -> None:
    """`gather_rows` for several (h, node_off, col_off) in one launch."""
    arr = (_lib.GatherJob * len(jobs))()
    keep = []
    for k, (h, node_off, col_off) in enumerate(jobs):
        h = _rows(h, "h")
        keep.append(h)
        arr[k] = _lib.GatherJob(h.data_ptr(), h.stride(0), h.shape[1], int(node_off), int(col_off))
    check(_lib.load().dagnn_gather_rows_batch(arr, len(jobs), num_graphs, stride, out.data_ptr(), out.shape[1], _stream(out)),
          "dagnn_gather_rows_batch")


def topo_layers(edge_index: torch.Tensor, batch: torch.Tensor, num_graphs: int):
    """(layer_fwd, layer_bwd, status): longest-path layer ids of both orientations for a collated batch, on the
    device (`src/utils_dag.py:8-52` without the per-graph numpy pass).  `status` is a device int32[1]: bit 16 =
    some graph has a cycle (check it with `int(status)` when the input is not trusted - that synchronises)."""
    edge_index = _dev(edge_index, "edge_index", torch.int64)
    batch = _dev(batch, "batch", torch.int64)
    N, E = batch.numel(), edge_index.shape[1]
    lf = torch.empty(N, dtype=torch.int64, device=batch.device)
    lb = torch.empty(N, dtype=torch.int64, device=batch.device)
    status = torch.zeros(1, dtype=torch.int32, device=batch.device)
    check(_lib.load().dagnn_topo_layers(edge_index.data_ptr(), batch.data_ptr(), N, E, int(num_graphs), lf.data_ptr(),
                                        lb.data_ptr(), status.data_ptr(), _stream(batch)), "dagnn_topo_layers")
    return lf, lb, status


# ------------------------------------------------------------------ the D-VAE decoders (csrc/dvae_decode.hip, csrc/dvae_sample.hip)
def decoder_shapes(d) -> list:
    """[(tensor, shape it must have)] for every weight of a decoder description `d` (`dvae._Decoder`: n, nvt, hs, bn, agg,
    cells, av, ae and the aggregator's views).  The library reads all of them through bare pointers."""
    n, nvt, hs = d.n, d.nvt, d.hs
    av, ae = d.av, d.ae
    V1, E1, ein = av[0].shape[0], ae[0].shape[0], (3 if d.bn else 2) * hs
    want = [(av[0], (V1, hs)), (av[1], (V1,)), (av[2], (nvt, V1)), (av[3], (nvt,)),
            (ae[0], (E1, ein)), (ae[1], (E1,)), (ae[2], (1, E1)), (ae[3], (1,))]
    if d.agg == _lib.DVAE_AGG_GATED_SUM:
        want += [(d.gate[0], (hs, hs + n)), (d.gate[1], (hs,)), (d.gate[2], (hs, hs + n))]
    elif d.agg == _lib.DVAE_AGG_ATTN_X:
        want.append((d.key_type, (nvt,)))
    else:
        want.append((d.w_key, (hs,)))
        if d.vid_bias is not None:
            want.append((d.vid_bias, (n,)))
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(d.cells):
        want += [(w_ih, (3 * hs, nvt if l == 0 else hs)), (w_hh, (3 * hs, hs)), (b_ih, (3 * hs,)), (b_hh, (3 * hs,))]
    return want


def check_shapes(entry: str, want) -> None:
    for t, shape in want:
        if tuple(t.shape) != shape:
            raise ValueError("%s: a tensor of shape %s where %s is needed" % (entry, tuple(t.shape), shape))


def _marshal_decoder(a, d, entry: str, also=()):
    """The decoder fields of `a` - dagnn_dvae_decode_args or dagnn_dvae_sample_args, which name them alike - from the
    description `d`: every weight on the device as float32, every shape checked (`also`: the entry point's own
    (tensor, shape) pairs), then dimensions, `agg` and pointers.  Returns `d` with the tensors the pointers borrow."""
    if not 1 <= d.L <= _lib.MAX_STACKED:
        raise DagnnHipError("%s: 1 to %d stacked cells" % (entry, _lib.MAX_STACKED))
    f = lambda t, what: None if t is None else _dev(t.detach(), what, torch.float32)  # noqa: E731
    d = d._replace(cells=[[f(t, "grud parameter") for t in c] for c in d.cells],
                   gate=None if d.gate is None else [f(t, "gate / mapper parameter") for t in d.gate],
                   key_type=f(d.key_type, "key_type"), w_key=f(d.w_key, "w_key"), vid_bias=f(d.vid_bias, "vid_bias"),
                   av=[f(t, "add_vertex parameter") for t in d.av], ae=[f(t, "add_edge parameter") for t in d.ae])
    check_shapes(entry, list(also) + decoder_shapes(d))
    a.n, a.hs, a.L, a.nvt, a.start_type, a.bn, a.agg = d.n, d.hs, d.L, d.nvt, int(d.start_type), int(bool(d.bn)), d.agg
    a.vertex_hidden, a.edge_hidden = d.av[0].shape[0], d.ae[0].shape[0]
    for l, c in enumerate(d.cells):
        a.w_ih[l], a.w_hh[l], a.b_ih[l], a.b_hh[l] = (t.data_ptr() for t in c)
    a.w_key, a.vid_bias, a.key_type = _ptr(d.w_key), _ptr(d.vid_bias), _ptr(d.key_type)
    if d.gate is not None:
        a.gate_w, a.gate_b, a.mapper_w = (t.data_ptr() for t in d.gate)
    a.av_w1, a.av_b1, a.av_w2, a.av_b2 = (t.data_ptr() for t in d.av)
    a.ae_w1, a.ae_b1, a.ae_w2, a.ae_b2 = (t.data_ptr() for t in d.ae)
    return d


class DvaeDecode(object):
    """One teacher-forced decode (`dagnn_dvae_decode_forward` / `_backward`): the argument struct, the tensors its pointers
    borrow, and the saved activations of the forward call.  `d`: the decoder description (`dvae._Decoder`); h0 [B,hs],
    types / preds [B,n] int32."""

    def __init__(self, d, types: torch.Tensor, preds: torch.Tensor, h0: torch.Tensor):
        h0 = _dev(h0, "H0", torch.float32)
        dev = h0.device
        B = h0.shape[0]
        types = _dev(types, "types", torch.int32)
        preds = _dev(preds, "predecessor masks", torch.int32)
        a = _lib.DvaeDecodeArgsTyped()
        d = _marshal_decoder(a, d, "dagnn_dvae_decode", [(h0, (B, d.hs)), (types, (B, d.n)), (preds, (B, d.n))])
        a.B = B
        a.types, a.preds, a.h0 = types.data_ptr(), preds.data_ptr(), h0.data_ptr()
        self.ll = torch.empty(2 * B + 1, dtype=torch.float32, device=dev)
        a.ll = self.ll.data_ptr()
        lib = _lib.load()
        nbytes = lib.dagnn_dvae_decode_saved_bytes(C.byref(a))
        if nbytes == 0:
            raise DagnnHipError("dagnn_dvae_decode: unsupported shape (B=%d, n=%d, hs=%d, L=%d, nvt=%d)" % (B, d.n, d.hs, d.L, d.nvt))
        self.saved = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        a.saved, a.saved_bytes = self.saved.data_ptr(), nbytes
        self.args, self.d, self.tensors, self.h0 = a, d, (types, preds), h0

    def forward(self) -> torch.Tensor:
        """Runs the decode; returns ll [2B+1]: per-graph vertex and edge log-likelihoods, then res."""
        check(_lib.load().dagnn_dvae_decode_forward(C.byref(self.args), _stream(self.h0)), "dagnn_dvae_decode_forward")
        return self.ll

    def backward(self, g_res: torch.Tensor, d_attn: Optional[torch.Tensor], key_off: int, vid_off: Optional[int]):
        """Gradients of res (scaled by the device scalar g_res) for h0, the cells, the add_vertex / add_edge tensors;
        the key / vertex-id parts are written into the zeroed `d_attn` (a [1, D] attn_lin.weight gradient) at the given
        column offsets (attn_x: the [nvt] table gradient at `key_off`).  Returns (d_h0, [per cell (d_w_ih, d_w_hh, d_b_ih,
        d_b_hh)], d_av, d_ae); gated_sum (d_attn = None): (d_h0, d_cells, d_av, d_ae, [d_gate_w, d_gate_b, d_mapper_w])."""
        lib = _lib.load()
        g_res = _dev(g_res.reshape(1), "grad", torch.float32)
        nbytes = lib.dagnn_dvae_decode_work_bytes(C.byref(self.args))
        work = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.h0.device)
        g = _lib.DvaeDecodeGradsTyped()
        g.g_res, g.work, g.work_bytes = g_res.data_ptr(), work.data_ptr(), nbytes
        d_h0 = torch.empty_like(self.h0)
        g.d_h0 = d_h0.data_ptr()
        d = self.d
        d_cells = []
        for l, c in enumerate(d.cells):
            ts = [torch.empty_like(t) for t in c]
            d_cells.append(ts)
            g.d_w_ih[l], g.d_w_hh[l], g.d_b_ih[l], g.d_b_hh[l] = (t.data_ptr() for t in ts)
        d_av = [torch.empty_like(t) for t in d.av]
        d_ae = [torch.empty_like(t) for t in d.ae]
        g.d_av_w1, g.d_av_b1, g.d_av_w2, g.d_av_b2 = (t.data_ptr() for t in d_av)
        g.d_ae_w1, g.d_ae_b1, g.d_ae_w2, g.d_ae_b2 = (t.data_ptr() for t in d_ae)
        if d.agg == _lib.DVAE_AGG_GATED_SUM:
            d_gate = [torch.empty_like(t) for t in d.gate]
            g.d_gate_w, g.d_gate_b, g.d_mapper_w = (t.data_ptr() for t in d_gate)
            check(lib.dagnn_dvae_decode_backward(C.byref(self.args), C.byref(g), _stream(self.h0)), "dagnn_dvae_decode_backward")
            return d_h0, d_cells, d_av, d_ae, d_gate
        if not d_attn.is_contiguous():
            raise DagnnHipError("dagnn_dvae_decode_backward: the attn_lin gradient must be contiguous")
        if d.agg == _lib.DVAE_AGG_ATTN_X:
            g.d_key_type = d_attn.data_ptr() + 4 * key_off
        else:
            g.d_w_key = d_attn.data_ptr() + 4 * key_off
        g.d_vid_bias = None if vid_off is None else d_attn.data_ptr() + 4 * vid_off
        check(lib.dagnn_dvae_decode_backward(C.byref(self.args), C.byref(g), _stream(self.h0)), "dagnn_dvae_decode_backward")
        return d_h0, d_cells, d_av, d_ae


# ------------------------------------------------------------------ sampling D-VAE decoder (csrc/dvae_sample.hip)
def dvae_sample(h0: torch.Tensor, groups: int, d, u_type: Optional[torch.Tensor] = None, u_edge: Optional[torch.Tensor] = None,
                states: bool = False):
    """One call of `dagnn_dvae_sample` over `groups` groups of h0.shape[0] // groups rows.  `d`: the decoder description
    (`dvae._Decoder`).  u_type [G,n,B] and u_edge [G,n(n-1)/2,B] (both or neither): the draws of a sampled decode; None:
    argmax.  Returns (types [R,n] int32, preds [R,n] int32 bitmasks, nv [R] int32, states [R,n,hs] or None) on h0's
    device, without synchronising."""
    h0 = _dev(h0, "H0", torch.float32)
    dev = h0.device
    R, n, hs = h0.shape[0], d.n, d.hs
    if groups <= 0 or R % groups:
        raise ValueError("dagnn_dvae_sample: %d rows do not split into %d groups" % (R, groups))
    B = R // groups
    also = [(h0, (R, hs))]
    stochastic = u_type is not None or u_edge is not None
    if stochastic:
        if u_type is None or u_edge is None:
            raise ValueError("dagnn_dvae_sample: give both u_type and u_edge, or neither")
        u_type = _dev(u_type, "u_type", torch.float32)
        u_edge = _dev(u_edge, "u_edge", torch.float32)
        also += [(u_type, (groups, n, B)), (u_edge, (groups, n * (n - 1) // 2, B))]
    a = _lib.DvaeSampleArgsTyped()
    d = _marshal_decoder(a, d, "dagnn_dvae_sample", also)
    a.G, a.B, a.end_type, a.stochastic = groups, B, int(d.end_type), int(stochastic)
    a.h0 = h0.data_ptr()
    a.u_type, a.u_edge = _ptr(u_type), _ptr(u_edge)
    types = torch.empty(R, n, dtype=torch.int32, device=dev)
    preds = torch.empty(R, n, dtype=torch.int32, device=dev)
    nv = torch.empty(R, dtype=torch.int32, device=dev)
    st = torch.empty(R, n, hs, dtype=torch.float32, device=dev) if states else None
    a.types, a.preds, a.nv, a.states = types.data_ptr(), preds.data_ptr(), nv.data_ptr(), _ptr(st)
    lib = _lib.load()
    nbytes = lib.dagnn_dvae_sample_work_bytes(C.byref(a))
    if nbytes == 0:
        raise DagnnHipError("dagnn_dvae_sample: unsupported shape (G=%d, B=%d, n=%d, hs=%d, L=%d, nvt=%d)"
                            % (groups, B, n, hs, d.L, d.nvt))
    work = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    a.work, a.work_bytes = work.data_ptr(), nbytes
    check(lib.dagnn_dvae_sample(C.byref(a), _stream(h0)), "dagnn_dvae_sample")
    return types, preds, nv, st


def dvae_select(types: torch.Tensor, preds: torch.Tensor, nv: torch.Tensor, nvt: int, start_type: int, end_type: int,
                kind: int, n_nodes: int = 0, select: int = 0):
    """One call of `dagnn_dvae_select` on the dense decode of A attempts of B points: types / preds [A,B,n] int32 (preds
    as bitmasks), nv [A,B] int32.  kind: _lib.DVAE_ENAS / DVAE_BN; n_nodes: 0 or the ENAS vertex count required;
    select: _lib.DVAE_FIRST_VALID / DVAE_MOST_FREQUENT.  Returns (valid [A,B], pick [B], n_valid [B], n_same [B], all
    int32, and keys [B,A,W] int64, the canonical keys) on types' device, without synchronising."""
    types = _dev(types, "types", torch.int32)
    preds = _dev(preds, "preds", torch.int32)
    nv = _dev(nv, "nv", torch.int32)
    if types.dim() != 3 or tuple(preds.shape) != tuple(types.shape) or tuple(nv.shape) != tuple(types.shape[:2]):
        raise ValueError("dagnn_dvae_select: types / preds [A,B,n] and nv [A,B] (got %s, %s, %s)"
                         % (tuple(types.shape), tuple(preds.shape), tuple(nv.shape)))
    A, B, n = types.shape
    dev = types.device
    a = _lib.DvaeSelectArgs()
    a.A, a.B, a.n, a.nvt, a.start_type, a.end_type = A, B, n, int(nvt), int(start_type), int(end_type)
    a.kind, a.n_nodes, a.select = int(kind), int(n_nodes), int(select)
    valid = torch.empty(A, B, dtype=torch.int32, device=dev)
    out = torch.empty(3, B, dtype=torch.int32, device=dev)
    a.types, a.preds, a.nv, a.valid = types.data_ptr(), preds.data_ptr(), nv.data_ptr(), valid.data_ptr()
    a.pick, a.n_valid, a.n_same = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
    lib = _lib.load()
    nbytes = lib.dagnn_dvae_select_work_bytes(C.byref(a))
    if nbytes == 0:
        raise ValueError("dagnn_dvae_select: unsupported arguments (A=%d, B=%d, n=%d, nvt=%d, kind=%d, n_nodes=%d, select=%d)"
                         % (A, B, n, nvt, kind, n_nodes, select))
    W = lib.dagnn_dvae_select_key_words(int(kind), n, int(nvt))
    keys = torch.empty(B, A, W, dtype=torch.int64, device=dev)
    a.work, a.work_bytes = keys.data_ptr(), nbytes
    check(lib.dagnn_dvae_select(C.byref(a), _stream(types)), "dagnn_dvae_select")
    return valid, out[0], out[1], out[2], keys


def _dense_rows(types, preds, nv, what):
    """types / preds [..., n] int32 and nv [...] int32 (or None) on one GPU, with equal leading shapes of 1 or 2 dims."""
    types = _dev(types, "types", torch.int32)
    preds = _dev(preds, "preds", torch.int32)
    nv = None if nv is None else _dev(nv, "nv", torch.int32)
    if types.dim() not in (2, 3) or tuple(preds.shape) != tuple(types.shape) or \
            (nv is not None and tuple(nv.shape) != tuple(types.shape[:-1])):
        raise ValueError("%s: types / preds [A,B,n] or [R,n] and nv [A,B] or [R] (got %s, %s, %s)"
                         % (what, tuple(types.shape), tuple(preds.shape), None if nv is None else tuple(nv.shape)))
    return types, preds, nv


def dvae_same_dag(types: torch.Tensor, preds: torch.Tensor, nv: torch.Tensor, types_true: torch.Tensor,
                  preds_true: torch.Tensor, nv_true: Optional[torch.Tensor] = None):
    """One call of `dagnn_dvae_same_dag`: decode rows types / preds [A,B,n], nv [A,B] against true rows types_true /
    preds_true [B,n], nv_true [B] (None: n vertices each).  Returns (same [A,B], per_graph [B], total [1]), int32 on the
    rows' device, without synchronising."""
    types, preds, nv = _dense_rows(types, preds, nv, "dagnn_dvae_same_dag")
    tt, pt, nt = _dense_rows(types_true, preds_true, nv_true, "dagnn_dvae_same_dag")
    if types.dim() != 3 or nv is None or tt.dim() != 2 or tuple(tt.shape) != tuple(types.shape[1:]) or tt.device != types.device:
        raise ValueError("dagnn_dvae_same_dag: decode rows [A,B,n] with nv [A,B] against true rows [B,n] on one device "
                         "(got %s and %s)" % (tuple(types.shape), tuple(tt.shape)))
    A, B, n = types.shape
    a = _lib.DvaeSameDagArgs()
    a.A, a.B, a.n = A, B, n
    same = torch.empty(A, B, dtype=torch.int32, device=types.device)
    out = torch.empty(B + 1, dtype=torch.int32, device=types.device)
    a.types, a.preds, a.nv = types.data_ptr(), preds.data_ptr(), nv.data_ptr()
    a.types_true, a.preds_true, a.nv_true = tt.data_ptr(), pt.data_ptr(), _ptr(nt)
    a.same, a.per_graph, a.total = same.data_ptr(), out.data_ptr(), out[B:].data_ptr()
    check(_lib.load().dagnn_dvae_same_dag(C.byref(a), _stream(types)), "dagnn_dvae_same_dag")
    return same, out[:B], out[B:]


def dvae_set_words(form: int, width: int, max_rows: int) -> int:
    """int32 words of a set's storage (dagnn_dvae_set_bytes / 4)."""
    nbytes = _lib.load().dagnn_dvae_set_bytes(int(form), int(width), int(max_rows))
    if nbytes == 0:
        raise ValueError("dagnn_dvae_set: unsupported set (form=%d, width=%d, max_rows=%d; at most %d rows)"
                         % (form, width, max_rows, _lib.DVAE_SET_MAX_ROWS))
    return nbytes // 4


def _set_desc(storage: torch.Tensor, form: int, width: int, max_rows: int) -> _lib.DvaeSet:
    storage = _dev(storage, "set storage", torch.int32)
    s = _lib.DvaeSet()
    s.form, s.width, s.max_rows = int(form), int(width), int(max_rows)
    s.data, s.bytes = storage.data_ptr(), storage.numel() * 4
    return s


def dvae_set_init(storage: torch.Tensor, form: int, width: int, max_rows: int) -> None:
    """`dagnn_dvae_set_init` on `storage` (int32, at least dvae_set_words(...) words): an empty set."""
    check(_lib.load().dagnn_dvae_set_init(C.byref(_set_desc(storage, form, width, max_rows)), _stream(storage)),
          "dagnn_dvae_set_init")


def _set_rows_args(storage, form, width, max_rows, A, B, mask, what):
    a = _lib.DvaeSetRowsArgs()
    a.set = _set_desc(storage, form, width, max_rows)
    a.A, a.B = A, B
    if mask is not None:
        mask = _dev(mask, "mask", torch.int32)
        if mask.numel() != A * B or mask.device != storage.device:
            raise ValueError("%s: mask must hold one int32 per row (%d) on the set's device" % (what, A * B))
    a.mask = _ptr(mask)
    return a, mask


def dvae_set_add(storage: torch.Tensor, form: int, width: int, max_rows: int, base: int, rows, mask=None) -> None:
    """One call of `dagnn_dvae_set_add`.  form DVAE_SET_GRAPHS: rows = (types, preds, nv or None), [A,B,n] or [R,n];
    DVAE_SET_KEYS: rows = keys [B,A,W] int64 (dagnn_dvae_select's).  mask: int32 per row ([A,B] / [R]) or None.  The rows
    become records base .. base + A*B - 1; a storage that is too small, or rows beyond max_rows, raise DagnnHipError
    before anything is launched.  Nothing synchronises."""
    if form == _lib.DVAE_SET_GRAPHS:
        types, preds, nv = _dense_rows(*rows, "dagnn_dvae_set_add")
        if types.shape[-1] != width or types.device != storage.device:
            raise ValueError("dagnn_dvae_set_add: rows of %d vertices on the set's device needed (got %s)" % (width, tuple(types.shape)))
        A, B = (1, types.shape[0]) if types.dim() == 2 else tuple(types.shape[:2])
        a, mask = _set_rows_args(storage, form, width, max_rows, A, B, mask, "dagnn_dvae_set_add")
        a.types, a.preds, a.nv = types.data_ptr(), preds.data_ptr(), _ptr(nv)
    else:
        keys = _dev(rows, "keys", torch.int64)
        if keys.dim() != 3 or keys.shape[2] != width or keys.device != storage.device:
            raise ValueError("dagnn_dvae_set_add: keys [B,A,%d] on the set's device needed (got %s)" % (width, tuple(keys.shape)))
        B, A = keys.shape[:2]
        a, mask = _set_rows_args(storage, form, width, max_rows, A, B, mask, "dagnn_dvae_set_add")
        a.keys = keys.data_ptr()
    a.base = int(base)
    check(_lib.load().dagnn_dvae_set_add(C.byref(a), _stream(storage)), "dagnn_dvae_set_add")


def dvae_set_query(storage: torch.Tensor, width: int, max_rows: int, types: torch.Tensor, preds: torch.Tensor,
                   nv: Optional[torch.Tensor], mask=None):
    """One call of `dagnn_dvae_set_query` on a DVAE_SET_GRAPHS set: (member, count [1]) int32, member shaped as the
    rows' leading dims, 1 where the masked row is_same_DAG-equal to a stored row.  Nothing synchronises."""
    types, preds, nv = _dense_rows(types, preds, nv, "dagnn_dvae_set_query")
    if types.shape[-1] != width or types.device != storage.device:
        raise ValueError("dagnn_dvae_set_query: rows of %d vertices on the set's device needed (got %s)" % (width, tuple(types.shape)))
    A, B = (1, types.shape[0]) if types.dim() == 2 else tuple(types.shape[:2])
    a, mask = _set_rows_args(storage, _lib.DVAE_SET_GRAPHS, width, max_rows, A, B, mask, "dagnn_dvae_set_query")
    a.types, a.preds, a.nv = types.data_ptr(), preds.data_ptr(), _ptr(nv)
    member = torch.empty(types.shape[:-1], dtype=torch.int32, device=types.device)
    count = torch.empty(1, dtype=torch.int32, device=types.device)
    a.member, a.count = member.data_ptr(), count.data_ptr()
    check(_lib.load().dagnn_dvae_set_query(C.byref(a), _stream(storage)), "dagnn_dvae_set_query")
    return member, count


# ----------------------------------------------------------------------------- attention weights of a finished pass (csrc/attention.hip)
def attention_weights(plan: PlanHandle, cells: Sequence[dict], E: int, mode: int = 0, vid_mod: int = 0, logits: bool = False):
    """`dagnn_attention_weights`: (alpha [len(cells), E], logit [len(cells), E] or None) of the cells of a finished pass, one
    launch pair for all of them (`mode` 1, mattn_h: one launch).  A cell is a dict: `dir`, `key` (fp32 GPU rows, any pitch),
    `key_dim`, `w_key`, and optionally `query`, `query_dim`, `w_query`, `vid_key`, `vid_query`, `edge_gain` (mode 1: the
    [key_dim, R] edge matrix), `edge_vec`, `bias` (a one-element device tensor).  Nothing synchronises; E == 0: no launch."""
    n = len(cells)
    if not 1 <= n <= _lib.ATTN_MAX_CELLS:
        raise DagnnHipError("attention_weights: 1..%d cells (directions x stacked layers) per call (got %d)" % (_lib.ATTN_MAX_CELLS, n))
    if int(E) != plan.E:
        raise DagnnHipError("attention_weights: the plan holds %d edges, the batch %d" % (plan.E, int(E)))
    dev = plan.ws.device
    alpha = torch.empty(n, plan.E, dtype=torch.float32, device=dev)
    logit = torch.empty(n, plan.E, dtype=torch.float32, device=dev) if logits else None
    if plan.E == 0 or plan.N == 0:
        return alpha, logit
    a = _lib.AttnArgs()
    a.num_cells, a.mode, a.vid_mod = n, int(mode), int(vid_mod)
    keep = []

    def vec(t, what, numel=None):
        if t is None:
            return None
        t = _dev(t, what, torch.float32)
        if numel is not None and t.numel() < numel:
            raise DagnnHipError("attention_weights: %s holds %d floats, %d needed" % (what, t.numel(), numel))
        keep.append(t)
        return t.data_ptr()

    def rows(t, what, dim):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1
                and t.shape[0] == plan.N and t.shape[1] >= dim and t.stride(0) >= dim):
            raise DagnnHipError("attention_weights: %s must be fp32 GPU rows [%d, >= %d] with unit column stride" % (what, plan.N, dim))
        keep.append(t)
        return t.data_ptr(), t.stride(0)

    want_query = False
    for k, c in enumerate(cells):
        ac = a.cell[k]
        ac.dir, ac.key_dim = int(c["dir"]), int(c["key_dim"])
        ac.key, ac.ld_key = rows(c["key"], "key rows", ac.key_dim)
        ac.w_key = vec(c.get("w_key"), "w_key", ac.key_dim)
        if c.get("query") is not None and (logits or mode == 1):
            ac.query_dim = int(c["query_dim"])
            ac.query, ac.ld_query = rows(c["query"], "query rows", ac.query_dim)
            ac.w_query = vec(c.get("w_query"), "w_query", ac.query_dim)
            want_query = True
        ac.vid_key, ac.vid_query = vec(c.get("vid_key"), "vid_key", vid_mod), vec(c.get("vid_query"), "vid_query", vid_mod)
        ac.edge_gain = vec(c.get("edge_gain"), "edge term", plan.R * (ac.key_dim if mode == 1 else 1))
        ac.edge_vec = vec(c.get("edge_vec"), "edge_vec", ac.key_dim)
        ac.bias = vec(c.get("bias"), "bias", 1)
    if mode == 0:
        ks = torch.empty(n * (2 if (logits and want_query) else 1), plan.N, dtype=torch.float32, device=dev)
        a.key_score = ks.data_ptr()
        if logits and want_query:
            a.query_score = ks.data_ptr() + 4 * n * plan.N
    a.alpha, a.logit = alpha.data_ptr(), _ptr(logit)
    plan.wait_ready()
    with _span("attention_weights", alpha):
        check(_lib.load().dagnn_attention_weights(C.byref(plan.desc), C.byref(a), _stream(alpha)), "dagnn_attention_weights")
    del keep
    return alpha, logit


# ----------------------------------------------------------------------------- the TOK task's evaluation path (csrc/predict.hip)
def heads_argmax(out: torch.Tensor, wcat: torch.Tensor, bcat: torch.Tensor, S: int, V: int,
                 arena: Optional[GranuleArena] = None):
    """`dagnn_heads_argmax`: (tok [B, S] int64, top [B, S, 2] float32 = winning logit and runner-up) of the S heads kept as one
    matrix `wcat` [S V, D] / `bcat` [S V] on the pooled vectors `out` [B, D], without the logits.  The per-tile partials live
    in `arena`'s scratch (a fresh tensor without one).  Nothing synchronises."""
    out = _rows(out, "pooled graph vectors")
    wcat, bcat = _rows(wcat, "head weights"), _dev(bcat, "head biases", torch.float32)
    B, D = out.shape
    if tuple(wcat.shape) != (S * V, D) or bcat.numel() != S * V or wcat.device != out.device or bcat.device != out.device:
        raise DagnnHipError("heads_argmax: heads of shape [%d, %d] / [%d] on the device of `out` needed (got %s / %s)"
                            % (S * V, D, S * V, tuple(wcat.shape), tuple(bcat.shape)))
    lib = _lib.load()
    tok = torch.empty(B, S, dtype=torch.int64, device=out.device)
    top = torch.empty(B, S, 2, dtype=torch.float32, device=out.device)
    nbytes = lib.dagnn_heads_argmax_bytes(B, S, V)
    if nbytes == 0:
        raise DagnnHipError("heads_argmax: unsupported shape (B=%d, S=%d, V=%d)" % (B, S, V))
    work = arena.scratch(nbytes, out.device) if arena is not None else torch.empty(nbytes // 8, dtype=torch.int64, device=out.device)
    with _span("heads_argmax", out):
        check(lib.dagnn_heads_argmax(out.data_ptr(), out.stride(0), wcat.data_ptr(), wcat.stride(0), bcat.data_ptr(), B, D, S, V,
                                     tok.data_ptr(), top.data_ptr(), work.data_ptr(), work.numel() * 8, _stream(out)),
              "dagnn_heads_argmax")
    return tok, top


def heads_score(out: torch.Tensor, wcat: torch.Tensor, bcat: torch.Tensor, S: int, V: int, y: Optional[torch.Tensor] = None,
                k: int = 1, sums: Optional[torch.Tensor] = None, arena: Optional[GranuleArena] = None):
    """`dagnn_heads_score`: (tok [B, S, k] int64, logit [B, S, k], lse [B, S], nll [B, S] or None) of the S heads kept as one
    matrix `wcat` [S V, D] / `bcat` [S V] on the pooled vectors `out` [B, D], without the logits: the k best columns of every
    (graph, head) with their logits, the log-sum-exp, and with targets `y` [B, S] int64 the row losses.  `sums`: an
    `evaluate.SeqLoss`'s 16 device bytes (a float64 tensor of 2 elements: the running sum of row losses, and the row count as
    int64 bits), added to in place.  The per-tile partials live in `arena`'s scratch (a fresh tensor without one).  Nothing
    synchronises."""
    out = _rows(out, "pooled graph vectors")
    wcat, bcat = _rows(wcat, "head weights"), _dev(bcat, "head biases", torch.float32)
    B, D = out.shape
    k = int(k)
    if tuple(wcat.shape) != (S * V, D) or bcat.numel() != S * V or wcat.device != out.device or bcat.device != out.device:
        raise DagnnHipError("heads_score: heads of shape [%d, %d] / [%d] on the device of `out` needed (got %s / %s)"
                            % (S * V, D, S * V, tuple(wcat.shape), tuple(bcat.shape)))
    if not 1 <= k <= 8:
        raise DagnnHipError("heads_score: k must lie in 1..8 (got %d)" % k)
    if y is not None:
        y = _dev(y, "targets", torch.int64)
        if y.numel() != B * S or y.device != out.device:
            raise DagnnHipError("heads_score: targets [%d, %d] on the device of `out` needed (got %s)" % (B, S, tuple(y.shape)))
        y = y.reshape(B, S).contiguous()
    if sums is not None:
        if y is None:
            raise DagnnHipError("heads_score: `sums` accumulates row losses: targets needed")
        if sums.dtype != torch.float64 or sums.numel() != 2 or not sums.is_contiguous() or sums.device != out.device:
            raise DagnnHipError("heads_score: `sums` must be 2 contiguous float64 elements on the device of `out`")
    lib = _lib.load()
    tok = torch.empty(B, S, k, dtype=torch.int64, device=out.device)
    logit = torch.empty(B, S, k, dtype=torch.float32, device=out.device)
    lse = torch.empty(B, S, dtype=torch.float32, device=out.device)
    nll = torch.empty(B, S, dtype=torch.float32, device=out.device) if y is not None else None
    nbytes = lib.dagnn_heads_score_bytes(B, S, V, k)
    if nbytes == 0:
        raise DagnnHipError("heads_score: unsupported shape (B=%d, S=%d, V=%d)" % (B, S, V))
    work = arena.scratch(nbytes, out.device) if arena is not None else torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=out.device)
    with _span("heads_score", out):
        check(lib.dagnn_heads_score(out.data_ptr(), out.stride(0), wcat.data_ptr(), wcat.stride(0), bcat.data_ptr(), B, D, S, V,
                                    _ptr(y), k, tok.data_ptr(), logit.data_ptr(), lse.data_ptr(), _ptr(nll), _ptr(sums),
                                    work.data_ptr(), work.numel() * work.element_size(), _stream(out)), "dagnn_heads_score")
    return tok, logit, lse, nll


def rows_argmax(logits: torch.Tensor, S: int, V: int) -> torch.Tensor:
    """`dagnn_rows_argmax`: tok [B, S] int64 of `logits` [B, S V] (fp32, unit column stride, any row pitch), one launch."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        _dev(logits, "logits")   # (raises: no CPU path)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[1] != S * V:
        raise DagnnHipError("rows_argmax: fp32 logits [B, %d] needed (got %s %s)" % (S * V, logits.dtype, tuple(logits.shape)))
    if logits.stride(1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < S * V):
        logits = logits.contiguous()
    B = logits.shape[0]
    tok = torch.empty(B, S, dtype=torch.int64, device=logits.device)
    check(_lib.load().dagnn_rows_argmax(logits.data_ptr(), logits.stride(0) if B > 1 else S * V, B, S, V, tok.data_ptr(),
                                        _stream(logits)), "dagnn_rows_argmax")
    return tok


def seq_f1_counts(tok: torch.Tensor, eos_id: int, ref_ids: torch.Tensor, ref_extra: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`dagnn_seq_f1_counts`: counts [B, 4] int32 = (true_positive, n_pred, n_ref, len) per graph (into `out` when given: a
    contiguous int32 [B, 4] view whose start is 16-byte aligned).  Nothing synchronises."""
    tok = _dev(tok, "tok", torch.int64)
    ref_ids, ref_extra = _dev(ref_ids, "ref_ids", torch.int32), _dev(ref_extra, "ref_extra", torch.int32)
    if tok.dim() != 2 or ref_ids.dim() != 2 or ref_ids.shape[0] != tok.shape[0] or ref_extra.numel() != tok.shape[0] or \
            ref_ids.device != tok.device or ref_extra.device != tok.device:
        raise DagnnHipError("seq_f1_counts: tok [B, S], ref_ids [B, R] and ref_extra [B] on one device needed (got %s, %s, %s)"
                            % (tuple(tok.shape), tuple(ref_ids.shape), tuple(ref_extra.shape)))
    B, S = tok.shape
    if out is None:
        out = torch.empty(B, 4, dtype=torch.int32, device=tok.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B, 4) or not out.is_contiguous() or out.device != tok.device:
        raise DagnnHipError("seq_f1_counts: `out` must be a contiguous int32 [B, 4] tensor on tok's device")
    check(_lib.load().dagnn_seq_f1_counts(tok.data_ptr(), B, S, int(eos_id), ref_ids.data_ptr(), ref_ids.shape[1],
                                          ref_extra.data_ptr(), out.data_ptr(), _stream(tok)), "dagnn_seq_f1_counts")
    return out


def _ce_buffers(B: int, S: int, V: int, need_grad: bool, dev):
    """(d logits [B, S V] in rows pitched to a multiple of 4 floats - what the heads' weight-gradient product reads 16 bytes
    at a time - or None, row losses [B S], loss [1]) of one cross-entropy launch."""
    dl = torch.empty(B, (S * V + 3) // 4 * 4, dtype=torch.float32, device=dev)[:, :S * V] if need_grad else None
    return dl, torch.empty(B * S, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)


def _scale_rows(dl: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """`dl * g`, the backward of the four cross-entropy functions: out of place (`backward(retain_graph=True)` may run it
    again on the same `dl`), into rows of the same pitch."""
    out = torch.empty(dl.shape[0], dl.stride(0), dtype=dl.dtype, device=dl.device)[:, :dl.shape[1]]
    return torch.mul(dl, g, out=out)


def seq_ce(base: torch.Tensor, y: torch.Tensor, S: int, V: int, need_grad: bool):
    """`dagnn_seq_ce` (csrc/loss.hip): (loss [1], d loss / d logits [B, S V] in rows pitched to a multiple of 4 floats, or
    None) of fp32 GPU logits `base` [B, S V] with unit column stride and contiguous int64 targets `y` [B, S] on its device.
    One launch, nothing synchronises."""
    B = base.shape[0]
    dl, row, loss = _ce_buffers(B, S, V, need_grad, base.device)
    check(_lib.load().dagnn_seq_ce(base.data_ptr(), base.stride(0), y.data_ptr(), B, S, V, _ptr(dl),
                                   0 if dl is None else dl.stride(0), row.data_ptr(), loss.data_ptr(),
                                   _lp_counter(base).data_ptr(), _stream(base)), "dagnn_seq_ce")
    return loss, dl


def seq_ce_step(base: torch.Tensor, y: torch.Tensor, S: int, V: int, need_grad: bool, eos_id: int,
                ref_ids: Optional[torch.Tensor], ref_extra: Optional[torch.Tensor], counts: torch.Tensor, graph_offset: int,
                epoch_sum: torch.Tensor, epoch_steps: torch.Tensor):
    """`dagnn_seq_ce_step` (csrc/loss.hip): (loss [1], d loss / d logits [B, S V] in rows pitched to a multiple of 4
    floats or None, tok [B, S] int64) of fp32 GPU logits `base` [B, S V] and int64 targets `y` [B, S] - `seq_ce`'s bits, the
    same kernel - and in the same launch `epoch_sum` [1] float64 += loss, `epoch_steps` [1] int64 += 1 and, with `ref_ids`
    [B, R] int32
    (`ref_extra` [B] int32), the F1 counts of the B graphs into rows `graph_offset` .. of `counts` [capacity, 4] int32.
    Nothing synchronises."""
    if not isinstance(base, torch.Tensor) or not base.is_cuda:
        _dev(base, "logits")   # (raises: no CPU path)
    if base.dim() != 2 or base.dtype != torch.float32:
        raise DagnnHipError("seq_ce_step: fp32 logits [B, %d] needed (got %s %s)" % (S * V, base.dtype, tuple(base.shape)))
    if base.stride(1) != 1 or (base.shape[0] > 1 and base.stride(0) < S * V):
        base = base.contiguous()
    y = _dev(y, "targets", torch.int64)
    B = base.shape[0]
    dev = base.device
    if base.shape[1] != S * V or tuple(y.shape) != (B, S) or not y.is_contiguous() or y.device != dev:
        raise DagnnHipError("seq_ce_step: logits [B, %d] and contiguous int64 targets [B, %d] on one device needed (got %s, %s)"
                            % (S * V, S, tuple(base.shape), tuple(y.shape)))
    counts, epoch_sum, epoch_steps = _dev(counts, "counts", torch.int32), _dev(epoch_sum, "epoch_sum", torch.float64), \
        _dev(epoch_steps, "epoch_steps", torch.int64)
    if counts.dim() != 2 or counts.shape[1] != 4 or not counts.is_contiguous() or {counts.device, epoch_sum.device, epoch_steps.device} != {dev}:
        raise DagnnHipError("seq_ce_step: counts must be a contiguous int32 [capacity, 4] tensor, the epoch words on the logits' device")
    R = 1
    if ref_ids is not None:
        ref_ids = _dev(ref_ids, "ref_ids", torch.int32)
        if ref_ids.dim() != 2 or ref_ids.shape[0] != B or ref_ids.shape[1] < 1 or not ref_ids.is_contiguous() or ref_ids.device != dev:
            raise DagnnHipError("seq_ce_step: contiguous int32 ref_ids [B, R >= 1] on the logits' device needed (got %s)" % (tuple(ref_ids.shape),))
        R = ref_ids.shape[1]
        if ref_extra is not None:
            ref_extra = _dev(ref_extra, "ref_extra", torch.int32)
            if ref_extra.numel() != B or not ref_extra.is_contiguous() or ref_extra.device != dev:
                raise DagnnHipError("seq_ce_step: contiguous int32 ref_extra [B] on the logits' device needed")
    dl, row, loss = _ce_buffers(B, S, V, need_grad, dev)
    tok = torch.empty(B, S, dtype=torch.int64, device=dev)
    check(_lib.load().dagnn_seq_ce_step(base.data_ptr(), base.stride(0) if B > 1 else S * V, y.data_ptr(), B, S, V, _ptr(dl),
                                        0 if dl is None else dl.stride(0), row.data_ptr(), loss.data_ptr(), tok.data_ptr(),
                                        int(eos_id), _ptr(ref_ids), R, _ptr(ref_extra) if ref_ids is not None else None,
                                        counts.data_ptr(), counts.shape[0], int(graph_offset), epoch_sum.data_ptr(),
                                        epoch_steps.data_ptr(), _lp_counter(base).data_ptr(), _stream(base)), "dagnn_seq_ce_step")
    return loss, dl, tok


# ----------------------------------------------------------------------------- the LP task's tail (csrc/lp.hip)
_LP_KINDS = {torch.int64: _lib.LP_INT64, torch.float32: _lib.LP_FLOAT32, torch.float64: _lib.LP_FLOAT64}
_LP_WORDS = {}


def lp_target(targ: torch.Tensor, B: int, device) -> Tuple[torch.Tensor, int]:
    """(`targ` as a contiguous [B] tensor on `device`, its DAGNN_LP_* kind): int64 / float32 / float64 as they are, any other
    dtype as int64 (integers) or float32 (floats)."""
    if targ.numel() != B:
        raise DagnnHipError("LP targets: %d values for %d graphs" % (targ.numel(), B))
    if targ.dtype not in _LP_KINDS:
        targ = targ.to(torch.float32 if targ.is_floating_point() else torch.int64)
    if targ.device != device:
        targ = targ.to(device, non_blocking=True)
    return targ.reshape(B).contiguous(), _LP_KINDS[targ.dtype]


def _lp_counter(t: torch.Tensor) -> torch.Tensor:
    """The zeroed device word the last-workgroup-in kernels (csrc/loss.hip, lp.hip, predictor.hip) count on, one per (device,
    stream): launches on a stream are ordered and every kernel leaves the word zero, so one is enough for all of them."""
    key = (t.device.index, _stream(t))
    cnt = _LP_WORDS.get(key)
    if cnt is None:
        cnt = _LP_WORDS[key] = torch.zeros(1, dtype=torch.int32, device=t.device)
    return cnt


def graph_depth(layer: torch.Tensor, batch: torch.Tensor, num_graphs: int) -> torch.Tensor:
    """`dagnn_graph_depth`: [num_graphs] int64, the largest `layer` value among each graph's nodes (`batch` sorted; 0 for a
    graph without nodes).  One launch, nothing synchronises."""
    layer, batch = _dev(layer, "layer ids", torch.int64), _dev(batch, "batch", torch.int64)
    if layer.numel() != batch.numel() or layer.device != batch.device:
        raise DagnnHipError("graph_depth: layer ids and batch must have one entry per node on one device")
    out = torch.empty(int(num_graphs), dtype=torch.int64, device=layer.device)
    check(_lib.load().dagnn_graph_depth(layer.data_ptr(), batch.data_ptr(), layer.numel(), int(num_graphs), out.data_ptr(),
                                        _stream(layer)), "dagnn_graph_depth")
    return out


def class_ce(pred: torch.Tensor, targ: torch.Tensor, need_grad: bool):
    """`dagnn_class_ce` (csrc/loss.hip, the S = 1 instance of `seq_ce`'s kernel): (loss [1], d loss / d logits [B, C] in rows
    pitched to a multiple of 4 floats, or None) for fp32 GPU logits `pred` [B, C] with unit column stride.  One launch,
    nothing synchronises."""
    B, C = pred.shape
    dev = pred.device
    targ, kind = lp_target(targ, B, dev)
    dl, row, loss = _ce_buffers(B, 1, C, need_grad, dev)
    check(_lib.load().dagnn_class_ce(pred.data_ptr(), pred.stride(0) if B > 1 else C, targ.data_ptr(), kind, B, C, _ptr(dl),
                                     0 if dl is None else dl.stride(0), row.data_ptr(), loss.data_ptr(),
                                     _lp_counter(pred).data_ptr(), _stream(pred)), "dagnn_class_ce")
    return loss, dl


def class_ce_step(pred: torch.Tensor, targ: torch.Tensor, need_grad: bool, epoch_hits: torch.Tensor, epoch_sum: torch.Tensor,
                  epoch_steps: torch.Tensor):
    """`dagnn_class_ce_step` (csrc/loss.hip): `class_ce`'s (loss [1], d loss / d logits) - its bits, the same kernel - plus
    tok [B] int64
    (the row argmax) and, in the same launch, `epoch_hits` [2] int64 += (hits, labelled) by `dagnn_class_hits`' rules,
    `epoch_sum` [1] float64 += loss, `epoch_steps` [1] int64 += 1.  Nothing synchronises."""
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        _dev(pred, "logits")   # (raises: no CPU path)
    if pred.dim() != 2 or pred.dtype != torch.float32 or pred.shape[0] < 1 or pred.shape[1] < 1:
        raise DagnnHipError("class_ce_step: fp32 logits [B >= 1, C >= 1] needed (got %s %s)" % (pred.dtype, tuple(pred.shape)))
    if pred.stride(1) != 1 or (pred.shape[0] > 1 and pred.stride(0) < pred.shape[1]):
        pred = pred.contiguous()
    B, C = pred.shape
    dev = pred.device
    targ, kind = lp_target(targ, B, dev)
    epoch_hits, epoch_sum, epoch_steps = _dev(epoch_hits, "epoch_hits", torch.int64), _dev(epoch_sum, "epoch_sum", torch.float64), \
        _dev(epoch_steps, "epoch_steps", torch.int64)
    if epoch_hits.numel() != 2 or {epoch_hits.device, epoch_sum.device, epoch_steps.device} != {dev}:
        raise DagnnHipError("class_ce_step: epoch_hits [2] and the epoch words on the logits' device needed")
    dl, row, loss = _ce_buffers(B, 1, C, need_grad, dev)
    tok = torch.empty(B, dtype=torch.int64, device=dev)
    check(_lib.load().dagnn_class_ce_step(pred.data_ptr(), pred.stride(0) if B > 1 else C, targ.data_ptr(), kind, B, C, _ptr(dl),
                                          0 if dl is None else dl.stride(0), row.data_ptr(), loss.data_ptr(), tok.data_ptr(),
                                          epoch_hits.data_ptr(), epoch_sum.data_ptr(), epoch_steps.data_ptr(),
                                          _lp_counter(pred).data_ptr(), _stream(pred)), "dagnn_class_ce_step")
    return loss, dl, tok


def class_hits(pred: torch.Tensor, targ: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`dagnn_class_hits`: [2] int64 = (hits, labelled) of one batch.  `pred`: fp32 logits [B, C] (argmax fused) or int64
    tokens [B] / [B, 1].  One launch, nothing synchronises."""
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        _dev(pred, "predictions")   # (raises: no CPU path)
    lib = _lib.load()
    dev = pred.device
    if pred.is_floating_point():
        if pred.dim() != 2 or pred.dtype != torch.float32:
            raise DagnnHipError("class_hits: fp32 logits [B, C] needed (got %s %s)" % (pred.dtype, tuple(pred.shape)))
        B, C = pred.shape
        if pred.stride(1) != 1 or (B > 1 and pred.stride(0) < C):
            pred = pred.contiguous()
        logits, ld, tok = pred.data_ptr(), (pred.stride(0) if B > 1 else C), None
    else:
        if pred.dim() > 2 or (pred.dim() == 2 and pred.shape[1] != 1):
            raise DagnnHipError("class_hits: tokens [B] or [B, 1] needed (got %s)" % (tuple(pred.shape),))
        pred = _dev(pred.reshape(-1), "tokens", torch.int64)
        B, C = pred.shape[0], 0
        logits, ld, tok = None, 0, pred.data_ptr()
    targ, kind = lp_target(targ, B, dev)
    if out is None:
        out = torch.empty(2, dtype=torch.int64, device=dev)
    nbytes = lib.dagnn_class_hits_bytes(B, 1 if tok is None else 0)
    work = torch.empty(max(nbytes // 8, 2), dtype=torch.int64, device=dev)
    check(lib.dagnn_class_hits(logits, ld, tok, B, C, targ.data_ptr(), kind, work.data_ptr(), work.numel() * 8,
                               _lp_counter(pred).data_ptr(), out.data_ptr(), _stream(pred)), "dagnn_class_hits")
    return out


# ----------------------------------------------------------------------------- the D-VAE predictor (csrc/predictor.hip)
def _predictor_params(W1, b1, W2, b2, nz: int, dev):
    """The four parameters as they lie (contiguous fp32 on `dev`; nothing is derived or cached) and hs."""
    if W1.dim() != 2 or W1.shape[1] != nz:
        raise DagnnHipError("predictor: W1 [hs, nz=%d] needed (got %s)" % (nz, tuple(W1.shape)))
    hs = W1.shape[0]
    if not (1 <= nz <= _lib.PREDICTOR_MAX_NZ and 1 <= hs <= _lib.PREDICTOR_MAX_HS):
        raise DagnnHipError("predictor: 1 <= nz <= %d and 1 <= hs <= %d needed (got nz=%d, hs=%d)"
                            % (_lib.PREDICTOR_MAX_NZ, _lib.PREDICTOR_MAX_HS, nz, hs))
    if b1.numel() != hs or W2.numel() != hs or b2.numel() != 1:
        raise DagnnHipError("predictor: b1 [hs], W2 [1, hs], b2 [1] needed with hs = %d (got %s, %s, %s)"
                            % (hs, tuple(b1.shape), tuple(W2.shape), tuple(b2.shape)))
    out = []
    for t, what in ((W1, "W1"), (b1, "b1"), (W2, "W2"), (b2, "b2")):
        if not t.is_cuda or t.device != dev or t.dtype != torch.float32:
            raise DagnnHipError("predictor: %s must be fp32 on %s (got %s on %s)" % (what, dev, t.dtype, t.device))
        out.append(t.detach() if t.is_contiguous() else t.detach().contiguous())
    return out, hs


def _predictor_rows(x: torch.Tensor, what: str) -> torch.Tensor:
    """fp32 GPU matrix with unit column stride; a row pitch above the width (a view of a wider tensor) is kept."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        _dev(x, what)   # (raises: no CPU path)
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.dim() != 2 or x.shape[1] < 1:
        raise DagnnHipError("predictor: %s [rows, nz] needed (got %s)" % (what, tuple(x.shape)))
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def predictor_mse(mu: torch.Tensor, y: torch.Tensor, W1, b1, W2, b2, need_grads: bool, need_dmu: bool):
    """`dagnn_predictor_mse`: (y_pred [B], loss [1], (d W1, d b1, d W2, d b2) or None, d mu [B, nz] or None) of
    sum (W2 tanh(W1 mu + b1) + b2 - y)^2 for an upstream gradient of 1.  `mu` [B, nz] fp32 (row pitch kept), `y` [B] fp32
    on mu's device.  One launch, nothing synchronises."""
    mu = _predictor_rows(mu, "mu")
    B, nz = mu.shape
    dev = mu.device
    if B < 1:
        raise DagnnHipError("predictor_mse: no row")
    (W1, b1, W2, b2), hs = _predictor_params(W1, b1, W2, b2, nz, dev)
    y = _dev(y, "y", torch.float32)
    if y.numel() != B or y.device != dev:
        raise DagnnHipError("predictor_mse: y must hold one value per row of mu on its device (got %s for %d rows)"
                            % (tuple(y.shape), B))
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=dev)
    P = hs * nz + 2 * hs + 2 if need_grads else 1
    y_pred, out = torch.empty(B, **f32), torch.empty(P, **f32)
    dmu = torch.empty(B, nz, **f32) if (need_grads and need_dmu) else None
    nbytes = lib.dagnn_predictor_mse_bytes(B, nz, hs, 1 if need_grads else 0)
    work = torch.empty(max(nbytes // 4, 1), **f32)
    check(lib.dagnn_predictor_mse(mu.data_ptr(), mu.stride(0) if B > 1 else nz, y.data_ptr(), B, nz, hs, W1.data_ptr(),
                                  b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), y_pred.data_ptr(), out.data_ptr(), _ptr(dmu),
                                  work.data_ptr(), work.numel() * 4, _lp_counter(mu).data_ptr(), 1 if need_grads else 0,
                                  _stream(mu)), "dagnn_predictor_mse")
    if not need_grads:
        return y_pred, out, None, None
    n1 = hs * nz
    grads = (out[:n1].view(hs, nz), out[n1:n1 + hs], out[n1 + hs:n1 + 2 * hs].view(1, hs), out[P - 2:P - 1])
    return y_pred, out[P - 1:], grads, dmu


def predictor_forward(Z: torch.Tensor, W1, b1, W2, b2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`dagnn_predictor_forward`: pred [M] of the rows of Z [M, nz] (into `out` when given: a contiguous fp32 [M] view).  One
    launch, nothing synchronises."""
    Z = _predictor_rows(Z, "Z")
    M, nz = Z.shape
    (W1, b1, W2, b2), hs = _predictor_params(W1, b1, W2, b2, nz, Z.device)
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=Z.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (M,) or not out.is_contiguous() or out.device != Z.device:
        raise DagnnHipError("predictor_forward: `out` must be a contiguous fp32 [M] tensor on Z's device")
    if M:
        check(_lib.load().dagnn_predictor_forward(Z.data_ptr(), Z.stride(0) if M > 1 else nz, M, nz, hs, W1.data_ptr(),
                                                  b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), out.data_ptr(), _stream(Z)),
              "dagnn_predictor_forward")
    return out


def fit_sums(pred: torch.Tensor, y: torch.Tensor, mean: float, std: float) -> torch.Tensor:
    """`dagnn_fit_sums`: float64 [6] on the device = sum p, sum y, sum p^2, sum y^2, sum p y, sum (p - y)^2 with
    p = (-pred - mean) / std; `pred` [M] fp32, `y` [M] fp32 or float64 (anything else as float64).  One launch, nothing
    synchronises."""
    pred = _dev(pred.reshape(-1), "pred", torch.float32)
    M = pred.numel()
    y = y.reshape(-1)
    if y.dtype not in (torch.float32, torch.float64):
        y = y.to(torch.float64)
    y = _dev(y, "y")
    if M < 1 or y.numel() != M or y.device != pred.device:
        raise DagnnHipError("fit_sums: pred [M >= 1] and y [M] on one device needed (got %d and %d)" % (M, y.numel()))
    lib = _lib.load()
    out = torch.empty(6, dtype=torch.float64, device=pred.device)
    work = torch.empty(max(lib.dagnn_fit_sums_bytes(M) // 8, 6), dtype=torch.float64, device=pred.device)
    check(lib.dagnn_fit_sums(pred.data_ptr(), y.data_ptr(), 1 if y.dtype == torch.float64 else 0, M, float(mean), float(std),
                             out.data_ptr(), work.data_ptr(), work.numel() * 8, _lp_counter(pred).data_ptr(), _stream(pred)),
          "dagnn_fit_sums")
    return out


# ----------------------------------------------------------------------------- the graph store's batch (csrc/store.hip)
_STORE_SOURCES = ("node_ptr", "edge_ptr", "tok_ptr", "x", "depth", "layer_f", "layer_b", "src", "dst", "tok", "depth_max",
                  "y_arr", "ref_ids", "ref_extra")


def store_gather(packed: dict, table: torch.Tensor, B: int, N: int, E: int, layers: bool = True, llp: bool = True,
                 labels: bool = True, refs: bool = True) -> dict:
    """`dagnn_store_gather`: one batch of a packed graph store, every tensor freshly allocated, in ONE launch; nothing
    synchronises.  `packed`: the store's device arrays under the names of `dagnn_store_gather_args` (an absent or None
    optional array is NULL); `table`: device int64 [4, B + 1] - row 0 the graph ids (B used), rows 1-3 the node / AST-edge /
    next-token-edge offsets of the batch - the caller has checked the ids.  `layers`, `llp`, `labels`, `refs` switch the
    optional outputs (given only where the store has their source).  Returns the batch's attributes by name."""
    table = _dev(table, "store batch table", torch.int64)
    B, N, E = int(B), int(N), int(E)
    if table.dim() != 2 or table.shape[0] != 4 or table.shape[1] < B + 1 or B <= 0:
        raise DagnnHipError("store_gather: table int64 [4, >= B + 1] and B > 0 needed (got %s, B = %d)" % (tuple(table.shape), B))
    dev = table.device
    a = _lib.StoreGatherArgs()
    for k in _STORE_SOURCES:
        t = packed.get(k)
        if t is not None and (not t.is_cuda or t.device != dev or not t.is_contiguous()):
            raise DagnnHipError("store_gather: packed array %s must be contiguous on %s" % (k, dev))
        setattr(a, k, _ptr(t))
    y_arr, ref_ids = packed.get("y_arr"), packed.get("ref_ids")
    S = y_arr.shape[1] if (labels and y_arr is not None) else 0
    R = ref_ids.shape[1] if (refs and ref_ids is not None) else 0
    a.idx, a.offsets, a.ld_offsets = table.data_ptr(), table.data_ptr() + 8 * table.stride(0), table.stride(0)
    a.B, a.N, a.E, a.S, a.R = B, N, E, S, R
    i64 = dict(dtype=torch.int64, device=dev)
    out = {"x": torch.empty(N, 2, **i64), "node_depth": torch.empty(N, 1, **i64), "edge_index": torch.empty(2, E, **i64),
           "edge_attr": torch.empty(E, 2, dtype=torch.float32, device=dev), "batch": torch.empty(N, **i64),
           "ptr": torch.empty(B + 1, **i64), "_bi_layer_index0": torch.empty(N, **i64), "_bi_layer_index1": torch.empty(N, **i64)}
    if layers and packed.get("layer_f") is not None:
        out["_bi_layer_idx0"], out["_bi_layer_idx1"] = torch.empty(N, **i64), torch.empty(N, **i64)
    if llp and packed.get("depth_max") is not None:
        out["len_longest_path"] = torch.empty(B, dtype=torch.float32, device=dev)
    if S:
        out["y_arr"] = torch.empty(B, S, **i64)
    if R:
        out["ref_ids"] = torch.empty(B, R, dtype=torch.int32, device=dev)
        out["ref_extra"] = torch.empty(B, dtype=torch.int32, device=dev)
    for field, key in (("out_x", "x"), ("out_depth", "node_depth"), ("out_edge_index", "edge_index"), ("out_edge_attr", "edge_attr"),
                       ("out_batch", "batch"), ("out_ptr", "ptr"), ("out_index0", "_bi_layer_index0"),
                       ("out_index1", "_bi_layer_index1"), ("out_layer_f", "_bi_layer_idx0"), ("out_layer_b", "_bi_layer_idx1"),
                       ("out_llp", "len_longest_path"), ("out_y_arr", "y_arr"), ("out_ref_ids", "ref_ids"),
                       ("out_ref_extra", "ref_extra")):
        setattr(a, field, _ptr(out.get(key)))
    check(_lib.load().dagnn_store_gather(C.byref(a), _stream(table)), "dagnn_store_gather")
    return out


# ----------------------------------------------------------------------------- the D-VAE store (csrc/dvae_store.hip)
_DAG_STORE_SOURCES = ("types", "preds", "succs", "layer_f", "layer_b", "y")


def dag_store_layers(preds: torch.Tensor, succs: torch.Tensor):
    """`dagnn_dag_store_layers`: (layer_f, layer_b) int32 [M, n] of M dense graphs given as predecessor / successor masks
    int32 [M, n] (n <= 32, read as unsigned words).  One launch, nothing synchronises."""
    preds, succs = _dev(preds, "preds", torch.int32), _dev(succs, "succs", torch.int32)
    if preds.dim() != 2 or preds.shape != succs.shape or not 1 <= preds.shape[1] <= 32 or succs.device != preds.device:
        raise DagnnHipError("dag_store_layers: preds and succs int32 [M, n <= 32] on one device needed (got %s, %s)"
                            % (tuple(preds.shape), tuple(succs.shape)))
    lf, lb = torch.empty_like(preds), torch.empty_like(preds)
    check(_lib.load().dagnn_dag_store_layers(_ptr(preds), _ptr(succs), preds.shape[0], preds.shape[1], _ptr(lf), _ptr(lb),
                                             _stream(preds)), "dagnn_dag_store_layers")
    return lf, lb


def dag_store_gather(packed: dict, table: torch.Tensor, B: int, E: int, nvt: int, schedule: bool = True) -> dict:
    """`dagnn_dag_store_gather`: one batch of a packed D-VAE store, every tensor freshly allocated, in ONE launch; nothing
    synchronises.  `packed`: the store's device arrays under the names of `dagnn_dag_store_gather_args` (`y` may be absent);
    `table`: device int64 [2, B + 1] - row 0 the graph ids (B used), row 1 the batch's edge offsets - the caller has checked
    the ids.  `schedule` False leaves `types` / `preds` out.  Returns the batch's attributes by name."""
    table = _dev(table, "store batch table", torch.int64)
    B, E, nvt = int(B), int(E), int(nvt)
    if table.dim() != 2 or table.shape[0] != 2 or table.shape[1] < B + 1 or B <= 0:
        raise DagnnHipError("dag_store_gather: table int64 [2, >= B + 1] and B > 0 needed (got %s, B = %d)" % (tuple(table.shape), B))
    dev = table.device
    a = _lib.DagStoreGatherArgs()
    for k in _DAG_STORE_SOURCES:
        t = packed.get(k)
        if t is not None and (not t.is_cuda or t.device != dev or not t.is_contiguous()):
            raise DagnnHipError("dag_store_gather: packed array %s must be contiguous on %s" % (k, dev))
        setattr(a, k, _ptr(t))
    n = int(packed["types"].shape[1])
    N = B * n
    a.idx, a.offsets = table.data_ptr(), table.data_ptr() + 8 * table.stride(0)
    a.B, a.n, a.nvt, a.E = B, n, nvt, E
    i64 = dict(dtype=torch.int64, device=dev)
    out = {"x": torch.empty(N, nvt, dtype=torch.float32, device=dev), "edge_index": torch.empty(2, E, **i64),
           "bi_layer_index": torch.empty(2, 2, N, **i64), "batch": torch.empty(N, **i64), "ptr": torch.empty(B + 1, **i64)}
    if schedule:
        out["types"] = torch.empty(B, n, dtype=torch.int32, device=dev)
        out["preds"] = torch.empty(B, n, dtype=torch.int32, device=dev)
    if packed.get("y") is not None:
        out["y"] = torch.empty(B, dtype=torch.float32, device=dev)
    for field, key in (("out_x", "x"), ("out_edge_index", "edge_index"), ("out_bi_layer_index", "bi_layer_index"),
                       ("out_batch", "batch"), ("out_ptr", "ptr"), ("out_types", "types"), ("out_preds", "preds"), ("out_y", "y")):
        setattr(a, field, _ptr(out.get(key)))
    check(_lib.load().dagnn_dag_store_gather(C.byref(a), _stream(table)), "dagnn_dag_store_gather")
    return out


def bn_score(desc: "_lib.BnData", parents: torch.Tensor, valid: Optional[torch.Tensor] = None, stage: int = 0):
    """`dagnn_bn_score`: the BIC scores of M structures - `parents` int32 / uint32 [M, n_var] parent masks on the device of
    the packed table `desc` describes, `valid` None or int32 [M] - as (scores float64 [M], n_over int32 [1]) on that device.
    One launch, nothing synchronises.  stage: _lib.BN_STAGE_AUTO / _LDS / _GLOBAL."""
    if not isinstance(parents, torch.Tensor) or not parents.is_cuda or parents.dim() != 2 or parents.shape[1] != desc.n_var \
            or parents.dtype not in (torch.int32, torch.uint32):
        raise DagnnHipError("bn_score: parents must be a 32-bit integer [M, n_var=%d] tensor on the GPU" % desc.n_var)
    parents = parents if parents.is_contiguous() else parents.contiguous()
    M, dev = parents.shape[0], parents.device
    if valid is not None:
        valid = _dev(valid, "valid", torch.int32)
        if valid.numel() != M or valid.device != dev:
            raise DagnnHipError("bn_score: valid must hold one flag per structure on the parents' device")
    scores = torch.empty(M, dtype=torch.float64, device=dev)
    n_over = torch.zeros(1, dtype=torch.int32, device=dev)
    check(_lib.load().dagnn_bn_score(C.byref(desc), _ptr(parents), _ptr(valid), M, int(stage), _ptr(scores), _ptr(n_over),
                                     _stream(parents)), "dagnn_bn_score")
    return scores, n_over


def bn_rows_to_parents(types: torch.Tensor, preds: torch.Tensor, nv: torch.Tensor, nvt: int, start_type: int, end_type: int):
    """`dagnn_bn_rows_to_parents`: dense rows types / preds int32 [R, n], nv int32 [R] -> (parents int32 [R, nvt - 2] - the
    masks read as unsigned words -, valid int32 [R]).  One launch, nothing synchronises."""
    types, preds, nv = _dev(types, "types", torch.int32), _dev(preds, "preds", torch.int32), _dev(nv, "nv", torch.int32)
    if types.dim() != 2 or tuple(preds.shape) != tuple(types.shape) or nv.numel() != types.shape[0]:
        raise DagnnHipError("bn_rows_to_parents: types / preds [R, n] and nv [R] needed (got %s, %s, %s)"
                            % (tuple(types.shape), tuple(preds.shape), tuple(nv.shape)))
    R, n = types.shape
    parents = torch.empty(R, max(int(nvt) - 2, 0), dtype=torch.int32, device=types.device)
    valid = torch.empty(R, dtype=torch.int32, device=types.device)
    check(_lib.load().dagnn_bn_rows_to_parents(_ptr(types), _ptr(preds), _ptr(nv), R, n, int(nvt), int(start_type), int(end_type),
                                               _ptr(parents), _ptr(valid), _stream(types)), "dagnn_bn_rows_to_parents")
    return parents, valid


# ----------------------------------------------------------------------------- the sparse GP's grids (csrc/sgp.hip)
def sgp_project(X: torch.Tensor, zt: torch.Tensor, inv_ls: torch.Tensor, sf: float, Tt: Optional[torch.Tensor], Mt: int, split: int,
                a: Optional[torch.Tensor], U: Optional[torch.Tensor] = None, u_col0: int = 0, want_var0: bool = False,
                want_var1: bool = False):
    """`dagnn_sgp_project` over the rows of X [N, d] (fp32, a row pitch is read in place): (mean, var0, var1), each fp32 [N] or
    None - mean with `a`, var0 / var1 as asked; the columns u_col0.. of U = k(X, z) T^T go into `U` [N, >= Mt - u_col0] when
    given.  zt [d, M], inv_ls [d], Tt [M, >= Mt] (T transposed), a [M]: fp32 on X's device.  One launch, nothing synchronises."""
    X = _rows(X, "X")
    if X.dim() != 2:
        raise DagnnHipError("sgp_project: X must be [N, d] (got %s)" % (tuple(X.shape),))
    N, d = X.shape
    dev = X.device
    zt, inv_ls = _dev(zt, "zt", torch.float32), _dev(inv_ls, "inv_ls", torch.float32)
    M = zt.shape[1]
    if zt.dim() != 2 or zt.shape[0] != d or inv_ls.numel() != d or zt.device != dev or inv_ls.device != dev:
        raise DagnnHipError("sgp_project: zt [d, M] and inv_ls [d] on X's device needed")
    Mt, ld_t = int(Mt), 0
    if Mt > 0:
        Tt = _dev(Tt, "Tt", torch.float32)
        if Tt.dim() != 2 or Tt.shape[0] != M or Tt.shape[1] < Mt or Tt.device != dev:
            raise DagnnHipError("sgp_project: Tt must be [M=%d, >= Mt=%d] on X's device (got %s)" % (M, Mt, tuple(Tt.shape)))
        ld_t = Tt.shape[1]
    if a is not None:
        a = _dev(a, "a", torch.float32)
        if a.numel() != M or a.device != dev:
            raise DagnnHipError("sgp_project: a must hold M = %d values on X's device" % M)
    ld_u = 0
    if U is not None:
        if not U.is_cuda or U.device != dev or U.dtype != torch.float32 or U.dim() != 2 or U.shape[0] != N or U.stride(1) != 1 \
                or U.shape[1] < Mt - int(u_col0) or (N > 1 and U.stride(0) < U.shape[1]):
            raise DagnnHipError("sgp_project: U must be fp32 [N, >= Mt - u_col0] with contiguous rows on X's device")
        ld_u = U.stride(0) if N > 1 else U.shape[1]
    mean = torch.empty(N, dtype=torch.float32, device=dev) if a is not None else None
    var0 = torch.empty(N, dtype=torch.float32, device=dev) if want_var0 else None
    var1 = torch.empty(N, dtype=torch.float32, device=dev) if want_var1 else None
    check(_lib.load().dagnn_sgp_project(X.data_ptr(), X.stride(0) if N > 1 else d, N, d, M, zt.data_ptr(), M, inv_ls.data_ptr(), float(sf),
                                        _ptr(Tt) if Mt > 0 else None, ld_t, Mt, int(split), _ptr(a), _ptr(U), ld_u, int(u_col0),
                                        _ptr(var0), _ptr(var1), _ptr(mean), _stream(X)), "dagnn_sgp_project")
    return mean, var0, var1


def sgp_ei_step(mode: int, mean: torch.Tensor, r: torch.Tensor, incumbent: float = 0.0, update=None, want_keys: bool = False):
    """`dagnn_sgp_ei_step`: the argmin of the mean (mode _lib.SGP_ARGMIN_MEAN) or of -log EI (SGP_ARGMIN_EI) over the N rows -
    `mean`, `r` contiguous fp32 [N] on the GPU - as (result int64 [4] on the device: index, rows without a positive variance,
    the winning key's bits, 0; keys float64 [N] or None).  `update` = (X [N, d], inv_ls [d], sf, p [d], U [N, > Me], Me, c [Me],
    inv_delta) first appends the point p to the factor: column Me of U is written and `r` is lowered IN PLACE.  One launch,
    nothing synchronises."""
    for t, what in ((mean, "mean"), (r, "r")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
            raise DagnnHipError("sgp_ei_step: %s must be a contiguous fp32 [N] tensor on the GPU" % what)
    N, dev = mean.numel(), mean.device
    if N < 1 or r.numel() != N or r.device != dev:
        raise DagnnHipError("sgp_ei_step: mean and r must hold N >= 1 rows on one device")
    X = inv_ls = p = U = c = None
    ld_x = ld_u = d = Me = 0
    sf = inv_delta = 0.0
    if update is not None:
        X, inv_ls, sf, p, U, Me, c, inv_delta = update
        X = _rows(X, "X")
        d, Me = X.shape[1], int(Me)
        ok = X.dim() == 2 and X.shape[0] == N and X.device == dev
        for t, n in ((inv_ls, d), (p, d), (c, Me)):
            ok = ok and isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and \
                t.is_contiguous() and t.numel() >= n
        ok = ok and isinstance(U, torch.Tensor) and U.is_cuda and U.device == dev and U.dtype == torch.float32 and U.dim() == 2 \
            and U.shape[0] == N and U.stride(1) == 1 and U.shape[1] > Me and (N == 1 or U.stride(0) >= U.shape[1])
        if not ok:
            raise DagnnHipError("sgp_ei_step: update needs X [N, d], inv_ls [d], p [d], c [Me] and U [N, > Me] as fp32 on one GPU")
        ld_x, ld_u = (X.stride(0) if N > 1 else d), (U.stride(0) if N > 1 else U.shape[1])
    lib = _lib.load()
    result = torch.empty(4, dtype=torch.int64, device=dev)
    keys = torch.empty(N, dtype=torch.float64, device=dev) if want_keys else None
    work = torch.empty(max(lib.dagnn_sgp_ei_step_bytes(N) // 8, 4), dtype=torch.int64, device=dev)
    check(lib.dagnn_sgp_ei_step(int(mode), N, mean.data_ptr(), r.data_ptr(), float(incumbent), _ptr(X), ld_x, d, _ptr(inv_ls), float(sf),
                                _ptr(p), _ptr(U), ld_u, Me, _ptr(c), float(inv_delta), _ptr(keys), result.data_ptr(), work.data_ptr(),
                                work.numel() * 8, _lp_counter(mean).data_ptr(), _stream(mean)), "dagnn_sgp_ei_step")
    return result, keys


# ----------------------------------------------------------------------------- the sparse GP's refinement (csrc/sgp_refine.hip)
def _sgp_refine_args(what: str, mode: int, X: torch.Tensor, ze: torch.Tensor, zet, inv_ls: torch.Tensor, a: torch.Tensor, T, Me: int):
    """The shared checks of `sgp_refine_eval` / `sgp_refine_run`: float64 contiguous operands on X's GPU, shapes in range.
    `zet` [d, >= Me] is ze transposed (None: made here).  Returns (S, d, M, Me, ld_t, zet)."""
    if mode not in (_lib.SGP_REFINE_MEAN, _lib.SGP_REFINE_EI):
        raise ValueError("%s: mode must be SGP_REFINE_MEAN or SGP_REFINE_EI (got %r)" % (what, mode))
    for t, name in ((X, "X"), (ze, "ze"), (inv_ls, "inv_ls"), (a, "a")) + (((T, "T"),) if mode == _lib.SGP_REFINE_EI else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.device != X.device or not t.is_contiguous():
            raise DagnnHipError("%s: %s must be a contiguous float64 tensor on X's GPU: this path is HIP only" % (what, name))
    if X.dim() != 2 or ze.dim() != 2 or ze.shape[1] != X.shape[1] or inv_ls.numel() != X.shape[1]:
        raise ValueError("%s: X [S, d], ze [>= Me, d] and inv_ls [d] needed (got %s, %s, %s)"
                         % (what, tuple(X.shape), tuple(ze.shape), tuple(inv_ls.shape)))
    (S, d), M, Me = X.shape, a.numel(), int(Me)
    if not 1 <= S <= _lib.SGP_REFINE_MAX_STARTS or not 1 <= d <= _lib.SGP_MAX_D or not 1 <= M <= _lib.SGP_MAX_M \
            or not M <= Me <= min(M + _lib.SGP_MAX_Q, ze.shape[0]):
        raise ValueError("%s: 1 <= S <= %d, 1 <= d <= %d, 1 <= M <= %d and M <= Me <= min(M + %d, rows of ze) needed (got S = %d, "
                         "d = %d, M = %d, Me = %d, %d rows)" % (what, _lib.SGP_REFINE_MAX_STARTS, _lib.SGP_MAX_D, _lib.SGP_MAX_M,
                                                                _lib.SGP_MAX_Q, S, d, M, Me, ze.shape[0]))
    ld_t = 0
    if mode == _lib.SGP_REFINE_EI:
        if T.dim() != 2 or T.shape[0] < Me or T.shape[1] < Me:
            raise ValueError("%s: T must be [>= Me, >= Me] for Me = %d (got %s)" % (what, Me, tuple(T.shape)))
        ld_t = T.shape[1]
    if zet is None:
        zet = ze[:Me].t().contiguous()
    elif not isinstance(zet, torch.Tensor) or not zet.is_cuda or zet.dtype != torch.float64 or zet.device != X.device \
            or not zet.is_contiguous() or zet.dim() != 2 or zet.shape[0] != d or zet.shape[1] < Me:
        raise DagnnHipError("%s: zet must be a contiguous float64 [d = %d, >= Me = %d] tensor on X's GPU" % (what, d, Me))
    return S, d, M, Me, ld_t, zet


def _sgp_refine_work(S: int, d: int, Me: int, dev, work: Optional[torch.Tensor]) -> torch.Tensor:
    words = _lib.load().dagnn_sgp_refine_bytes(Me, d, S) // 8
    if work is None:
        return torch.empty(words, dtype=torch.float64, device=dev)
    if work.dtype != torch.float64 or work.device != dev or work.numel() < words or not work.is_contiguous():
        raise DagnnHipError("sgp_refine: work must hold %d float64 values on X's GPU" % words)
    return work


def sgp_refine_words(M: int, q: int, d: int, S: int) -> int:
    """The float64 values of the refinement's workspace for up to M + q expanded rows."""
    return _lib.load().dagnn_sgp_refine_bytes(int(M) + int(q), int(d), int(S)) // 8


def sgp_refine_eval(mode: int, X: torch.Tensor, ze: torch.Tensor, inv_ls: torch.Tensor, sf: float, a: torch.Tensor,
                    T: Optional[torch.Tensor] = None, Me: Optional[int] = None, tri: bool = False, incumbent: float = 0.0,
                    work: Optional[torch.Tensor] = None, zet: Optional[torch.Tensor] = None):
    """`dagnn_sgp_refine_eval`: the refinement's objective at the S rows of X [S, d] in float64 - (f [S], mean [S], v [S],
    d mean / dx [S, d], d v / dx [S, d]) over the first Me rows of ze (default: a.numel() = M) with T [>= Me, >= Me] (tri: lower
    triangular); mode SGP_REFINE_MEAN: f = mean, T unused; SGP_REFINE_EI: f = -log EI against `incumbent`.  Four launches,
    nothing synchronises."""
    S, d, M, Me, ld_t, zet = _sgp_refine_args("sgp_refine_eval", mode, X, ze, zet, inv_ls, a, T, a.numel() if Me is None else Me)
    work = _sgp_refine_work(S, d, Me, X.device, work)
    out = torch.empty(S, 4 + 2 * d, dtype=torch.float64, device=X.device)
    check(_lib.load().dagnn_sgp_refine_eval(int(mode), S, d, M, Me, X.data_ptr(), ze.data_ptr(), zet.data_ptr(), zet.shape[1], inv_ls.data_ptr(), float(sf),
                                            a.data_ptr(),
                                            _ptr(T) if ld_t else None, ld_t, int(bool(tri)), float(incumbent), out.data_ptr(),
                                            work.data_ptr(), work.numel() * 8, _stream(X)), "dagnn_sgp_refine_eval")
    return out[:, 0], out[:, 1], out[:, 2], out[:, 4:4 + d], out[:, 4 + d:]


def sgp_refine_run(mode: int, X0: torch.Tensor, lower: torch.Tensor, upper: torch.Tensor, ze: torch.Tensor, inv_ls: torch.Tensor,
                   sf: float, a: torch.Tensor, T: Optional[torch.Tensor] = None, Me: Optional[int] = None, tri: bool = False,
                   incumbent: float = 0.0, max_evals: int = 64, nstart: Optional[torch.Tensor] = None,
                   work: Optional[torch.Tensor] = None, want_points: bool = False, zet: Optional[torch.Tensor] = None):
    """`dagnn_sgp_refine_run`: the S rows of X0 [S, d] (clipped into [lower, upper], float64 [d] each) advanced in lock-step for
    `max_evals` evaluations on the objective of `sgp_refine_eval`; `nstart` (an int32 device word): the rows from it on are
    dead.  Returns float64 [2 + d + 3 S] on the device: the best start (-1: none), its objective, its point, then status,
    evaluations and objective per start - with `want_points` a pair of it and every start's accepted point [S, d] (NaN: dead).  1 + 3 max_evals + 1 launches (1 + max_evals + 1 for SGP_REFINE_MEAN), nothing synchronises."""
    S, d, M, Me, ld_t, zet = _sgp_refine_args("sgp_refine_run", mode, X0, ze, zet, inv_ls, a, T, a.numel() if Me is None else Me)
    for t, name in ((lower, "lower"), (upper, "upper")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.device != X0.device \
                or not t.is_contiguous() or t.numel() != d:
            raise DagnnHipError("sgp_refine_run: %s must hold d = %d float64 values on X0's GPU" % (name, d))
    if not 4 <= int(max_evals) <= 1024:
        raise ValueError("sgp_refine_run: 4 <= max_evals <= 1024 needed (got %d)" % max_evals)
    if nstart is not None and (not isinstance(nstart, torch.Tensor) or nstart.dtype != torch.int32 or nstart.device != X0.device
                               or nstart.numel() < 1):
        raise DagnnHipError("sgp_refine_run: nstart must be an int32 word on X0's GPU")
    work = _sgp_refine_work(S, d, Me, X0.device, work)
    out = torch.empty(2 + d + 3 * S, dtype=torch.float64, device=X0.device)
    xs = torch.empty(S, d, dtype=torch.float64, device=X0.device) if want_points else None
    check(_lib.load().dagnn_sgp_refine_run(int(mode), S, d, M, Me, X0.data_ptr(), _ptr(nstart), lower.data_ptr(), upper.data_ptr(),
                                           ze.data_ptr(), zet.data_ptr(), zet.shape[1], inv_ls.data_ptr(), float(sf), a.data_ptr(), _ptr(T) if ld_t else None, ld_t,
                                           int(bool(tri)), float(incumbent), int(max_evals), out.data_ptr(), _ptr(xs),
                                           work.data_ptr(), work.numel() * 8, _stream(X0)), "dagnn_sgp_refine_run")
    return (out, xs) if want_points else out


# ----------------------------------------------------------------------------- the sparse GP's training step (csrc/sgp_train.hip)
def sgp_energy_grad(X: torch.Tensor, y: torch.Tensor, params, n_points: int, fail: torch.Tensor, work: Optional[torch.Tensor] = None):
    """`dagnn_sgp_energy_grad`: (E [1], [g_lls, g_lsf, g_z, g_mParamPost, g_LParamPost, g_lvar_noise]) of the minibatch X [b, d],
    y [b] (float64 on the GPU, a row pitch of X is read in place) at `params` (the six float64 tensors of
    `SparseGP.get_params()`, read in place).  `fail`: an int32 device word that counts failed pivots (the caller zeroes and
    reads it); `work`: a float64 scratch tensor of at least `sgp_energy_grad_words(M, d, b)` values, allocated when None.  No
    synchronisation; M > 512 or d > 128 raises ValueError."""
    lls, lsf, z, mP, Lp, lvn = params
    for t, what in ((X, "X"), (y, "y"), (lls, "lls"), (lsf, "lsf"), (z, "z"), (mP, "mParamPost"), (Lp, "LParamPost"), (lvn, "lvar_noise")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.device != X.device:
            raise DagnnHipError("sgp_energy_grad: %s must be a float64 tensor on X's GPU: this path is HIP only" % what)
    if X.dim() != 2 or z.dim() != 2 or X.shape[1] != z.shape[1] or X.shape[0] < 1:
        raise ValueError("sgp_energy_grad: X [b >= 1, d] and z [M, d] needed (got %s, %s)" % (tuple(X.shape), tuple(z.shape)))
    (b, d), M = X.shape, z.shape[0]
    words = sgp_energy_grad_words(M, d, b)
    if X.stride(1) != 1 or (b > 1 and X.stride(0) < d):
        X = X.contiguous()
    y = y.reshape(-1)
    y = y if y.is_contiguous() else y.contiguous()
    if y.numel() != b or lls.numel() != d or lsf.numel() != 1 or lvn.numel() != 1 or mP.numel() != M or tuple(Lp.shape) != (M, M) \
            or not all(t.is_contiguous() for t in (lls, z, mP, Lp)):
        raise ValueError("sgp_energy_grad: y [b], lls [d], lsf [], z [M, d], mParamPost [M, 1], LParamPost [M, M], lvar_noise [] "
                         "contiguous needed")
    if fail.dtype != torch.int32 or not fail.is_cuda or fail.device != X.device or fail.numel() < 1:
        raise DagnnHipError("sgp_energy_grad: fail must be an int32 word on X's GPU")
    dev = X.device
    if work is None:
        work = torch.empty(words, dtype=torch.float64, device=dev)
    elif work.dtype != torch.float64 or work.device != dev or work.numel() < words or not work.is_contiguous():
        raise DagnnHipError("sgp_energy_grad: work must hold %d float64 values on X's GPU" % words)
    E = torch.empty(1, dtype=torch.float64, device=dev)
    grads = [torch.empty_like(p) for p in params]
    check(_lib.load().dagnn_sgp_energy_grad(X.data_ptr(), X.stride(0) if b > 1 else d, y.data_ptr(), b, M, d, float(n_points),
                                            lls.data_ptr(), lsf.data_ptr(), z.data_ptr(), mP.data_ptr(), Lp.data_ptr(), lvn.data_ptr(),
                                            E.data_ptr(), *[g.data_ptr() for g in grads], work.data_ptr(), work.numel() * 8,
                                            fail.data_ptr(), _stream(X)), "dagnn_sgp_energy_grad")
    return E, grads


def sgp_energy_grad_words(M: int, d: int, b: int) -> int:
    """The float64 values of `dagnn_sgp_energy_grad`'s workspace; ValueError for a shape the kernels do not take."""
    if not 1 <= int(M) <= _lib.SGP_MAX_M or not 1 <= int(d) <= _lib.SGP_MAX_D:
        raise ValueError("sgp_energy_grad: 1 <= M <= %d and 1 <= d <= %d needed (got M = %d, d = %d)"
                         % (_lib.SGP_MAX_M, _lib.SGP_MAX_D, M, d))
    nbytes = _lib.load().dagnn_sgp_energy_grad_bytes(int(M), int(d), int(b))
    if nbytes == 0:
        raise ValueError("sgp_energy_grad: 1 <= b <= 2^24 rows needed (got %d)" % b)
    return nbytes // 8
