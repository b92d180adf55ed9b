"""BIC scores of Bayesian-network structures on a table of discrete samples, in HIP: the objective of the D-VAE's BN loops.

A BN graph's target y is the BIC score of its structure on a data table; the reference gets it from one R process per
structure (`Eval_BN.eval`, bayesian_optimization/evaluate_BN.py, which calls bnlearn's `score(net, data)`), in the BO loop
(bo.py:288-306) and - ahead of time - for the y column of its BN training file.  The score is counting, so here the table
lives on the device and `dagnn_bn_score` (csrc/bn_score.hip) scores any number of structures in one launch:

    data = BnData.from_samples(samples, device="cuda")                  # [S, n_var] integers, packed once
    scores, n_over = bn_scores(data, parents)                           # parents [M, n_var] masks: bit j of [m, i] = arc j -> i
    y = store_scores(data, store)[0]                                    # the y column of a BN DagStore
    strings, y = decode_and_score(z, model, data)                       # the BN body of a BO round
    BnEvaluator(data).eval("0 1 0 ...")                                 # drop-in for Eval_BN.eval (a float)

The score (bnlearn's default for discrete data, type "bic"), for S samples, node i with r_i values and parent set Pa_i:

    q_i      = product of r_j over j in Pa_i (1 without a parent; every configuration counts, observed or not)
    N_ijk    = samples with parent configuration j and x_i = k;   N_ij = sum over k of N_ijk
    family_i = sum over (j, k) with N_ijk > 0 of N_ijk (log N_ijk - log N_ij)  -  0.5 log(S) q_i (r_i - 1)
    score    = sum over i of family_i

in float64 after the integer counts.  A family's count table holds at most `TABLE_CELLS` cells (q_i r_i): a structure with a
larger family is not scored - NaN, counted in `n_over`.  Scores are bitwise repeatable: from run to run, under any
permutation of the samples, and whichever staging path (`stage`) ran.  `scores_host` is the module's numpy mirror; tables on
the CPU go through it, tables on the GPU never do.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, dvae, engine

__all__ = ["BnData", "BnEvaluator", "TABLE_CELLS", "MAX_VARS", "bn_scores", "score_dense", "store_scores", "score_strings",
           "decode_and_score", "scores_host", "parents_from_adj", "parents_from_string"]

TABLE_CELLS = _lib.BN_TABLE_CELLS   # DAGNN_BN_TABLE_CELLS: cells (q_i r_i) of the largest family that is scored
MAX_VARS = _lib.BN_MAX_VARS         # DAGNN_BN_MAX_VARS
_STAGES = {None: _lib.BN_STAGE_AUTO, "auto": _lib.BN_STAGE_AUTO, "lds": _lib.BN_STAGE_LDS, "global": _lib.BN_STAGE_GLOBAL}


class BnData(object):
    """A table of S samples of n_var discrete variables, packed for `dagnn_bn_score`: column-major, one byte per value,
    columns `ld` bytes apart (S rounded up to 16, zero padded), on `device`.  `samples` int64 [S, n_var] and `cards` stay on
    the host for the mirror and the checks."""

    def __init__(self, samples: np.ndarray, cards: np.ndarray, device):
        self.samples, self.cards = samples, cards
        self.S, self.n_var = int(samples.shape[0]), int(samples.shape[1])
        self.device = torch.device(device)
        self.ld = (self.S + 15) // 16 * 16
        cols = np.zeros((self.n_var, self.ld), dtype=np.uint8)
        cols[:, :self.S] = samples.T
        self.cols = torch.from_numpy(cols).to(self.device)
        self.desc = _lib.BnData()
        self.desc.cols, self.desc.ld, self.desc.S, self.desc.n_var = self.cols.data_ptr(), self.ld, self.S, self.n_var
        for i, r in enumerate(cards.tolist()):
            self.desc.cards[i] = int(r)

    @classmethod
    def from_samples(cls, samples, cards=None, device="cuda") -> "BnData":
        """`samples`: an [S, n_var] integer array (or tensor), variable i with values in [0, cards[i]); `cards` defaults to
        the column maximum + 1.  ValueError for a dtype that is not integer, a value outside its range, no sample, more than
        MAX_VARS variables or a cardinality above 255."""
        if isinstance(samples, torch.Tensor):
            samples = samples.detach().cpu().numpy()
        samples = np.asarray(samples)
        if samples.ndim != 2 or samples.shape[0] < 1 or samples.shape[1] < 1:
            raise ValueError("BnData: samples must be [S >= 1, n_var >= 1] (got %s)" % (samples.shape,))
        if samples.dtype.kind not in "iu":
            raise ValueError("BnData: samples must hold integers (got %s)" % samples.dtype)
        S, n_var = samples.shape
        if n_var > MAX_VARS:
            raise ValueError("BnData: at most %d variables (got %d)" % (MAX_VARS, n_var))
        if S >= 1 << 31:
            raise ValueError("BnData: fewer than 2^31 samples needed (got %d)" % S)
        samples = samples.astype(np.int64)
        if int(samples.min()) < 0:
            raise ValueError("BnData: a value is negative")
        if cards is None:
            cards = samples.max(axis=0) + 1
        cards = np.asarray(cards)
        if cards.dtype.kind not in "iu" or cards.reshape(-1).size != n_var:
            raise ValueError("BnData: cards must hold one integer per variable")
        cards = cards.reshape(-1).astype(np.int64)
        if int(cards.min()) < 1 or int(cards.max()) > 255:
            raise ValueError("BnData: cardinalities must lie in 1..255 (got %s)" % cards.tolist())
        if (samples >= cards[None, :]).any():
            s, i = (int(a[0]) for a in np.nonzero(samples >= cards[None, :]))
            raise ValueError("BnData: sample %d has x_%d = %d, outside [0, %d)" % (s, i, int(samples[s, i]), int(cards[i])))
        return cls(np.ascontiguousarray(samples), cards, device)

    @property
    def on_gpu(self) -> bool:
        return self.device.type == "cuda"

    def fits_lds(self) -> bool:
        """Whether the staged path is possible for this table (`dagnn_bn_stage_fits`)."""
        return _lib.load().dagnn_bn_stage_fits(self.desc) == 1


# --------------------------------------------------------------------------------- the host mirror
def scores_host(samples, cards, parents) -> np.ndarray:
    """The numpy mirror of `dagnn_bn_score` in float64: scores [M] of the parent masks `parents` [M, n_var] on `samples`
    [S, n_var] with cardinalities `cards`; NaN for a structure with a family beyond TABLE_CELLS."""
    return _scores_host(np.asarray(samples), np.asarray(cards), parents)[0]


def _scores_host(samples, cards, parents):
    X = np.asarray(samples, dtype=np.int64)
    r = np.asarray(cards, dtype=np.int64).reshape(-1)
    P = np.asarray(parents).astype(np.int64) & 0xFFFFFFFF
    S, n_var = X.shape
    if P.ndim != 2 or P.shape[1] != n_var:
        raise ValueError("scores_host: parents must be [M, n_var=%d] (got %s)" % (n_var, P.shape))
    out = np.empty(P.shape[0], dtype=np.float64)
    n_over = 0
    half_log_s = 0.5 * np.log(float(S))
    for m in range(P.shape[0]):
        pa = [[j for j in range(n_var) if P[m, i] >> j & 1] for i in range(n_var)]
        q = [int(np.prod([int(r[j]) for j in p], dtype=object)) if p else 1 for p in pa]
        if any(q[i] * int(r[i]) > TABLE_CELLS for i in range(n_var)):
            out[m] = np.nan
            n_over += 1
            continue
        total = 0.0
        for i in range(n_var):
            cfg = np.zeros(S, dtype=np.int64)
            mult = 1
            for j in pa[i]:
                cfg += X[:, j] * mult
                mult *= int(r[j])
            n = np.bincount(cfg * r[i] + X[:, i], minlength=q[i] * int(r[i])).reshape(q[i], int(r[i])).astype(np.float64)
            nij = n.sum(axis=1, keepdims=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.where(n > 0, n * (np.log(n) - np.log(nij)), 0.0)
            total += float(t.sum()) - half_log_s * q[i] * (int(r[i]) - 1)
        out[m] = total
    return out, n_over


# --------------------------------------------------------------------------------- masks in, scores out
def _stage(stage) -> int:
    if stage not in _STAGES:
        raise ValueError("stage must be None, 'lds' or 'global' (got %r)" % (stage,))
    return _STAGES[stage]


def _masks(data: BnData, parents, what: str) -> torch.Tensor:
    """parents as a 32-bit [M, n_var] tensor on the table's device (an array or a CPU tensor is copied once)."""
    if isinstance(parents, torch.Tensor):
        if parents.dtype not in (torch.int32, torch.uint32):
            raise ValueError("%s: parents must be uint32 (or int32 words) (got %s)" % (what, parents.dtype))
        t = parents
    else:
        a = np.asarray(parents)
        if a.dtype.kind not in "iu":
            raise ValueError("%s: parents must hold integers (got %s)" % (what, a.dtype))
        if a.size and (int(a.min()) < -(1 << 31) or int(a.max()) >= 1 << 32):
            raise ValueError("%s: parent masks must be 32-bit words" % what)
        t = torch.from_numpy((a.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    if t.dim() != 2 or t.shape[1] != data.n_var:
        raise ValueError("%s: parents must be [M, n_var=%d] (got %s)" % (what, data.n_var, tuple(t.shape)))
    return t.to(data.device)


def _scores_cpu(data: BnData, masks: torch.Tensor, valid: Optional[torch.Tensor]):
    p = masks.numpy().view(np.uint32) if masks.dtype == torch.int32 else masks.view(torch.int32).numpy().view(np.uint32)
    if valid is None:
        s, n_over = _scores_host(data.samples, data.cards, p)
    else:
        keep = valid.numpy() != 0
        s = np.full(p.shape[0], np.nan)
        s[keep], n_over = _scores_host(data.samples, data.cards, p[keep])
    return torch.from_numpy(s), torch.tensor([n_over], dtype=torch.int32)


def bn_scores(data: BnData, parents, stage=None):
    """(scores float64 [M], n_over int32 [1]) of M structures on `data`, both on the table's device, without synchronising.
    `parents`: uint32 [M, n_var] parent masks (bit j of parents[m, i]: the arc j -> i) - a tensor on the device (int32
    words are read as unsigned), or an array / CPU tensor that is copied once.  stage: None (LDS when the table fits),
    'lds' or 'global'.  A structure with a family beyond TABLE_CELLS cells scores NaN and counts in n_over.

    The masks of one structure must describe a DAG.  That is the caller's business: nothing here checks it, and a cyclic
    structure gets the number the formula gives."""
    st = _stage(stage)
    masks = _masks(data, parents, "bn_scores")
    if not data.on_gpu:
        return _scores_cpu(data, masks, None)
    return engine.bn_score(data.desc, masks, None, st)


def score_dense(data: BnData, types, preds, nv, nvt: int, start_type: int = 0, end_type: int = 1, stage=None):
    """Scores of dense decoder / `DagStore` rows - types / preds int32 [R, n] (preds as predecessor bitmasks), nv [R] - as
    (scores float64 [R], n_over int32 [1]): the first and last vertex are dropped, a middle vertex is the variable given
    by the rank of its type (`bn_adj_string`'s order).  A row that is invalid under `row_valid(..., data_type='BN')` scores
    NaN and does not count in n_over.  nvt - 2 must be the table's n_var.  Nothing synchronises."""
    if int(nvt) - 2 != data.n_var:
        raise ValueError("score_dense: nvt - 2 = %d middle types, but the table has %d variables" % (int(nvt) - 2, data.n_var))
    st = _stage(stage)
    if data.on_gpu:
        parents, valid = engine.bn_rows_to_parents(types, preds, nv, nvt, start_type, end_type)
        return engine.bn_score(data.desc, parents, valid, st)
    t, p, k = (np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a) for a in (types, preds, nv))
    masks, valid = rows_to_parents_host(t, p, k.reshape(-1), nvt, start_type, end_type)
    return _scores_cpu(data, torch.from_numpy(masks.view(np.int32)), torch.from_numpy(valid))


def rows_to_parents_host(types, preds, nv, nvt: int, start_type: int = 0, end_type: int = 1):
    """The numpy mirror of `dagnn_bn_rows_to_parents`: (parents uint32 [R, nvt - 2], valid int32 [R])."""
    R, n_var = types.shape[0], int(nvt) - 2
    parents, valid = np.zeros((R, n_var), dtype=np.uint32), np.zeros(R, dtype=np.int32)
    for g in range(R):
        if not dvae.row_valid(types[g], preds[g], nv[g], "BN", nvt, start_type, end_type):
            continue
        valid[g] = 1
        k = int(nv[g])
        rank = np.argsort(np.argsort([int(t) for t in types[g][1:k - 1]]))
        for v in range(1, k - 1):
            for u in range(1, v):
                if int(preds[g][v]) >> u & 1:
                    parents[g, rank[v - 1]] |= np.uint32(1 << int(rank[u - 1]))
    return parents, valid


def store_scores(data: BnData, store, idx=None, end_type: int = 1, stage=None):
    """(scores float64, n_over) of the graphs `idx` (host ids, any order, repeats allowed; None: all, in order) of a
    `DagStore` of BN graphs on the table's device, in one call of `score_dense`: the y column the reference's BN training
    file carries."""
    types, preds = store.arrays["types"], store.arrays["preds"]
    if idx is not None:
        ids = torch.from_numpy(store._ids(idx)).to(types.device)
        types, preds = types.index_select(0, ids), preds.index_select(0, ids)
    nv = torch.full((types.shape[0],), store.n, dtype=torch.int32, device=types.device)
    return score_dense(data, types, preds, nv, store.nvt, store.start_type, end_type, stage)


# --------------------------------------------------------------------------------- strings (Eval_BN.eval)
def parents_from_adj(adj: np.ndarray) -> np.ndarray:
    """Parent masks uint32 [n_var] of an adjacency matrix: adj[j, i] == 1 is the arc j -> i."""
    a = np.asarray(adj)
    n = a.shape[0]
    return np.array([sum(1 << j for j in range(n) if a[j, i]) for i in range(n)], dtype=np.uint32)


def _acyclic(adj: np.ndarray) -> bool:
    indeg = adj.sum(axis=0).astype(np.int64)
    ready = [i for i in range(adj.shape[0]) if indeg[i] == 0]
    seen = 0
    while ready:
        u = ready.pop()
        seen += 1
        for v in np.flatnonzero(adj[u]):
            indeg[v] -= 1
            if indeg[v] == 0:
                ready.append(int(v))
    return seen == adj.shape[0]


def parents_from_string(data: BnData, input_string: str) -> np.ndarray:
    """The reference's flat adjacency string (n_var^2 entries of 0 / 1 separated by blanks, row-major, entry [j, i] the
    arc j -> i) as parent masks.  ValueError for a wrong length, an entry outside {0, 1}, a cyclic matrix and a family
    beyond TABLE_CELLS cells."""
    if not isinstance(input_string, str):
        raise ValueError("BN string expected (got %s)" % type(input_string).__name__)
    toks = input_string.split()
    n = data.n_var
    if len(toks) != n * n:
        raise ValueError("a BN string for %d variables has %d entries (got %d)" % (n, n * n, len(toks)))
    if any(t not in ("0", "1") for t in toks):
        raise ValueError("a BN string holds only 0 and 1 (got %r)" % next(t for t in toks if t not in ("0", "1")))
    adj = np.array([int(t) for t in toks], dtype=np.int64).reshape(n, n)
    if not _acyclic(adj):
        raise ValueError("the adjacency matrix has a cycle")
    for i in range(n):
        cells = int(data.cards[i])
        for j in np.flatnonzero(adj[:, i]):
            cells *= int(data.cards[j])
        if cells > TABLE_CELLS:
            raise ValueError("node %d's family has %d cells, beyond the table capacity %d" % (i, cells, TABLE_CELLS))
    return parents_from_adj(adj)


def score_strings(data: BnData, strings: Sequence[Optional[str]]) -> list:
    """The scores of a list of BN strings as python floats, NaN where the entry is None.  Synchronises (the result is on the
    host), so every string is checked first: ValueError as `parents_from_string` raises it."""
    strings = list(strings)
    keep = [b for b, s in enumerate(strings) if s is not None]
    out = [float("nan")] * len(strings)
    if keep:
        masks = np.stack([parents_from_string(data, strings[b]) for b in keep])
        got = bn_scores(data, masks)[0].cpu().numpy()
        for b, v in zip(keep, got):
            out[b] = float(v)
    return out


class BnEvaluator(object):
    """Drop-in for the reference's `Eval_BN`: `eval(input_string)` is the BIC score of the structure on `data` as a float."""

    def __init__(self, data: BnData):
        self.data = data

    def eval(self, input_string: str) -> float:
        return score_strings(self.data, [input_string])[0]


# --------------------------------------------------------------------------------- the BN body of a BO round
def decode_and_score(latent_points, model, data: BnData, decode_attempts=500, n_nodes="variable", select="first", chunk=None,
                     draws=None):
    """The BN body of bo.py:289-306: `decode_from_latent_space(..., data_type='BN')` and the score of every decoded
    structure.  Returns (strings, scores): the strings exactly those of `decode_from_latent_space` for the same draws,
    scores a float64 numpy array [B], NaN where the string is None.  The scores are computed on the device from the picked
    rows and reach the host in the one copy (and synchronisation) `decode_from_latent_space` makes anyway."""
    if not data.on_gpu:
        raise engine.DagnnHipError("decode_and_score: the table must be on the GPU the model decodes on")
    if model.nvt - 2 != data.n_var:
        raise ValueError("decode_and_score: the model has %d middle types, the table %d variables" % (model.nvt - 2, data.n_var))

    def extra(d, sel, pick):
        ar = torch.arange(pick.shape[0], device=pick.device)
        scores = score_dense(data, d.types[pick, ar], d.preds[pick, ar], d.nv[pick, ar], model.nvt, model.START_TYPE,
                             model.END_TYPE)[0]
        nan = torch.full_like(scores, float("nan"))
        return torch.where(sel.pick < 0, nan, scores).view(torch.int32).view(-1, 2)

    strings, more = dvae._decode_and_pick(latent_points, model, decode_attempts, n_nodes, False, "BN", select, chunk, draws, extra)
    return strings, np.ascontiguousarray(more).view(np.float64).reshape(-1)
