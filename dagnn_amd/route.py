"""Which recurrence path a pass of `DAGNN` / the D-VAE encoders takes, decided once (DESIGN.md §4a″ has the table).

`before_plan` gives what the plan and schedule builders need - the padded width `Hp` and the dataflow kernel's group
count - from the model's shape alone; `with_plan` completes the `Route` once the batch's plan exists.  A forward pass
evaluates each once and hands the result on: `core.run_stack_lockstep` dispatches on `kind`, the backward pass reads
`reverse`.  `dataflow_only` is the question of the caller that can run on nothing else (`dvae._encode_fused`); `plain` is
the whole route of the `add` / `max` passes (`variants.run_plain_dataflow`, `variants.PlainRecurrence`).  The primitives
stay in `engine`; every flag is read there when the function runs."""
from typing import NamedTuple, Optional, Sequence

from . import engine

OFF = "DAGNN_AMD_DATAFLOW=0"
IDLE = "an empty batch, or a pass without a granule arena"
POLICY = "hidden size 512 with stacked layers: the tile kernel or, for a batch that is faster there, the per-layer launches"
QUIET = (OFF, IDLE, POLICY)   # reasons that are a choice, not a cliff: `core._warn_off_dataflow` says nothing
LIB = "the kernel does not apply to this shape"   # a 0 of `dagnn_dataflow_groups` (cell count, CUs), or a 32-bit limit


class Route(NamedTuple):
    Hp: int                        # padded width of a state row
    groups: int                    # groups of the dataflow kernel; 0: it does not run
    kind: Optional[str] = None     # "dataflow" | "tiles" | "launches+tiles" | "launches"; None before the plan
    tiles: int = 0                 # launches of the tile kernel (0 unless `kind` has tiles)
    split: Optional[Sequence[int]] = None   # "launches+tiles": per direction the first layer of the tile kernel's tail
    stat_rows: bool = False        # the forward launch writes the reverse sweep's static rows (training only)
    reverse: Optional[str] = None  # "dataflow" | "lockstep"; None: an evaluation pass
    why: Optional[str] = None      # None on the dataflow kernel, else the Python-side reason it was not taken


def _served(Hp: int, R: int, keys_hidden: bool, vid_nodes: int, edge_enc: bool) -> bool:
    """Widths the dataflow kernels exist for.  320 wide is `dagnn_dataflow_run_wide`'s shape only (the lean loaders): an edge
    encoder over exactly two edge features, hidden-state keys, no vertex-id key biases."""
    return Hp <= 256 or bool(Hp == 320 and edge_enc and R == 2 and keys_hidden and not vid_nodes)


def width(H: int, L: int, R: int, keys_hidden: bool, vid_nodes: int, edge_enc: bool):
    """(padded width, the cells take the dataflow kernel's weight layout) of a model with `L` stacked layers and `R` edge
    features; other models of the 320-wide kernel's width run on the per-layer launches."""
    Hp = engine.state_width(H, L, R, wide_ok=bool(edge_enc and keys_hidden and not vid_nodes))
    return Hp, bool(engine.DATAFLOW and (Hp <= 256 or engine.DF_WIDE) and _served(Hp, R, keys_hidden, vid_nodes, edge_enc))


def before_plan(device, H: int, L: int, ndirs: int, R: int, B: int, keys_hidden: bool = True, vid_nodes: int = 0,
                edge_enc: bool = False, training: bool = False, Hp: Optional[int] = None, active: bool = True) -> Route:
    """`Hp` and `groups`, what the plan's schedule is built for.  `keys_hidden`: the keys are hidden states, not the inputs
    (one static score per node, `*_x` aggregators); `Hp`: the width the cells already have; `active`: False for an empty
    batch or a pass without an arena.  A pass the kernel does not serve asks the library nothing."""
    if Hp is None:
        Hp = width(H, L, R, keys_hidden, vid_nodes, edge_enc)[0]
    served = active and _served(Hp, R, keys_hidden, vid_nodes, edge_enc)
    return Route(Hp, engine.dataflow_groups(device, ndirs, L, Hp, B, training=training) if served else 0)


def _rows32(N: int, Hp: int) -> bool:
    return N * 3 * Hp < (1 << 31)   # the dataflow kernels address their granule buffers with 32-bit row offsets


def dataflow_only(device, ndirs: int, L: int, Hp: int, B: int, N: int) -> int:
    """Groups of an evaluation pass that runs on the dataflow kernel at 256 wide at most or not at all; 0: not this path."""
    if N == 0 or Hp > 256 or not _rows32(N, Hp):
        return 0
    return engine.dataflow_groups(device, ndirs, L, Hp, B)


PLAIN_OFF = "DAGNN_AMD_VARIANT_DATAFLOW=0"
PLAIN_BACKEND = "variant_backend = 'hip': training passes of add / max take the lock-step sweep unless 'dataflow' is asked for"


def plain(device, backend: str, training: bool, agg: str, recurr: bool, agg_x: bool, schedule: str, wea: bool, R: int,
          H: int, L: int, ndirs: int, B: int, N: int, ok: bool = True, groups: Optional[int] = None,
          fits: Optional[bool] = None) -> Route:
    """The route of a pass of `agg` = `add` / `max` (AggConv, `variants.run_plain_dataflow` and its training twin): `kind`
    "dataflow" - the persistent kernel with a plain fold in its loaders - or "launches", the per-layer variant launches; a
    training pass that takes the kernel also takes the reverse dataflow sweep (`reverse`), or neither.  An evaluation pass
    takes the kernel under either HIP backend; a training pass only under `backend` "dataflow".  `wea`: the aggregator has an
    edge encoder, `R`: edge features of the batch's plan, `ok`: the model class shares one AggConv the way the kernel
    assumes.  `groups` / `fits`: what `dataflow_only` / `engine.bwd_dataflow_fits` answer for this device (asked here when
    None, and only once everything else holds).  `why`: None on the kernel, else the first condition that failed."""
    Hp = width(H, L, 0, True, 0, False)[0]
    stat_rows = False

    def off(why):
        return Route(Hp, 0, "launches", 0, None, False, "lockstep" if training else None, why)

    if not engine.DATAFLOW:
        return off(OFF)
    if not engine.VARIANT_DATAFLOW:
        return off(PLAIN_OFF)
    if training and backend != "dataflow":
        return off(PLAIN_BACKEND)
    if agg not in ("add", "max") or not ok:
        return off("aggregator %r is not a plain fold of one shared AggConv" % (agg,))
    if not recurr:
        return off("recurr=0: the kernel's cells are GRU cells")
    if agg_x:
        return off("agg_x: the aggregator reads the inputs, nothing couples the layers")
    if schedule != "lockstep":
        return off("schedule %r: the kernel runs on the lock-step schedule" % (schedule,))
    if R > 2 or (wea and R == 0):
        return off("the loaders fold at most two edge features (and an edge encoder needs the batch's)")
    if Hp > 256:
        return off("hidden size %d > 256: the plain loaders exist up to 256 wide" % Hp)
    if N == 0:
        return off(IDLE)
    if not _rows32(N, Hp):
        return off(LIB)
    if training:
        if not engine.BWD_DATAFLOW:
            return off("DAGNN_AMD_BWD_DATAFLOW=0")
        if fits is None:
            fits = engine.bwd_dataflow_fits(device, N, ndirs * L)
        if not fits:
            return off("the reverse dataflow sweep's records do not fit this device's memory budget")
        stat_rows = bool(engine.STAT_FWD and engine.lib_static_floats(N, Hp) * 4 < (1 << 32))   # a record: 32-bit offsets
    if groups is None:
        groups = engine.dataflow_groups(device, ndirs, L, Hp, B, training=training)
    if groups <= 0:
        return off(LIB)
    return Route(Hp, groups, "dataflow", 0, None, stat_rows, "dataflow" if training else None, None)


def with_plan(r: Route, device, plan, dirs: Sequence[int], L: int, N: int, keys_hidden: bool = True, active: bool = True,
              training: bool = False) -> Route:
    """The rest of the route `before_plan` began, with the same `keys_hidden` and `active`.  `plan` gives R and - only on
    the two `tiles_*` policies that read them - its layer row counts."""
    Hp, R = r.Hp, plan.R
    groups = r.groups if active and _rows32(N, Hp) else 0
    tiles, split = 0, None
    if groups == 0 and active and keys_hidden and N * engine.frontier_ld(Hp) * 4 < (1 << 31) - 16:
        tiles = engine.tiles_launches(device, len(dirs), L, Hp, R, N)   # wide states (512): csrc/tiles.hip
        if tiles > 0 and engine.tiles_batch_too_flat(plan, dirs):
            tiles = 0   # few wide layers: the launches' 32-row tiles win
        if tiles == 0 and engine.TILES == 1 and L >= 2:
            # a batch too large for the tile kernel alone: it takes the thin tail behind the launches, if there is one
            tail = engine._lib.load().dagnn_tiles_launches(engine._num_cus(device), len(dirs), L, Hp, R)
            split = engine.tiles_tail_split(plan, dirs) if tail > 0 else None
            tiles = tail if split is not None else 0
    kind = "launches+tiles" if split is not None else "tiles" if tiles > 0 else "dataflow" if groups > 0 else "launches"
    stat_rows, reverse = False, None
    if training:
        # the reverse dataflow sweep runs on the forward's schedule, so on its group count, and keeps a record per (cell, node)
        fits = bool(kind == "dataflow" and engine.BWD_DATAFLOW and engine.bwd_dataflow_fits(device, N, len(dirs) * L))
        reverse = "dataflow" if fits else "lockstep"
        stat_rows = bool(fits and engine.STAT_FWD and engine.lib_static_floats(N, Hp) * 4 < (1 << 32))   # a record: 32-bit offsets
    if kind == "dataflow":
        why = None
    elif not engine.DATAFLOW:
        why = OFF
    elif not active:
        why = IDLE
    elif Hp == 512 and engine.TILES == 1 and L >= 2:
        why = POLICY
    elif Hp == 320 and not engine.DF_WIDE:
        why = "DAGNN_AMD_DF_WIDE=0 keeps hidden sizes 257..320 off the dataflow kernel's 320-wide shape"
    elif Hp == 320:
        why = "hidden size 320 runs on the dataflow kernel only with exactly two edge features, hidden-state keys and no vertex-id key biases"
    elif Hp > 256:
        why = "hidden size %d > 256 (a 32-unit slice of the [3H, H] matrices no longer fits the register file)" % Hp
    else:
        why = LIB
    return Route(Hp, groups, kind, tiles, split, stat_rows, reverse, why)
