"""Boosted search: pymilvus' Boost Ranker (`Function(..., FunctionType.RERANK, params={"reranker":
"boost", "filter": ..., "weight": ...})`, passed to `search(..., ranker=)`) as a value object, the
class weights it induces and the definition of the boosted ranking in numpy.

m <= 3 boosts (filter_i, weight_i) split the rows into 2^m classes: bit i of a row's class is set iff
the row passes filter_i.  W[c] is the product of the weights of c's set bits; with s the fp64
ranking score, boosted = W[class] * s, and rows rank by (boosted desc, s desc, row asc)."""
from __future__ import annotations

import math

import numpy as np

MAX_BOOSTS = 3   # RF_BOOST_MAX (include/ragfin.h)


def _check_weight(weight) -> float:
    if isinstance(weight, (bool, np.bool_)) or not isinstance(weight, (int, float, np.integer, np.floating)):
        raise ValueError(f"boost ranker: weight must be a real number > 0, got {weight!r}")
    w = float(weight)
    if not math.isfinite(w) or not w > 0.0:
        raise ValueError(f"boost ranker: weight must be finite and > 0, got {weight!r}")
    return w


class BoostRanker:
    """One boost: the rows `filter` selects (an expression in the store's grammar, never empty) have
    their score multiplied by `weight` (finite, > 0; below 1 demotes).  Several rankers multiply."""

    def __init__(self, filter: str, weight: float, name: str = "boost"):
        if not isinstance(filter, str) or not filter.strip():
            raise ValueError(f"boost ranker: filter must be a non-empty expression string, got {filter!r}")
        if not isinstance(name, str):
            raise ValueError(f"boost ranker: name must be a string, got {name!r}")
        self.filter = filter
        self.weight = _check_weight(weight)
        self.name = name

    @classmethod
    def from_params(cls, params: dict, name: str = "boost") -> "BoostRanker":
        """From Milvus' params dict {"reranker": "boost", "filter": ..., "weight": ...}."""
        if not isinstance(params, dict):
            raise ValueError(f"boost ranker: params must be a dict, got {type(params).__name__}")
        if params.get("reranker") != "boost":
            raise ValueError(f"boost ranker: reranker {params.get('reranker')!r} is not supported (only 'boost')")
        if "random_score" in params:
            raise ValueError("boost ranker: random_score is not supported (the ranking is exact and reproducible)")
        unknown = sorted(set(params) - {"reranker", "filter", "weight"})
        if unknown:
            raise ValueError(f"boost ranker: unknown params {unknown}")
        if "filter" not in params or "weight" not in params:
            raise ValueError("boost ranker: params need 'filter' and 'weight'")
        return cls(params["filter"], params["weight"], name)

    def __repr__(self):
        return f"BoostRanker({self.filter!r}, {self.weight!r})"


def check_rankers(ranker) -> list:
    """The `ranker` argument of a search -> a list of 1..MAX_BOOSTS BoostRanker."""
    boosts = list(ranker) if isinstance(ranker, (list, tuple)) else [ranker]
    if not 1 <= len(boosts) <= MAX_BOOSTS or not all(isinstance(b, BoostRanker) for b in boosts):
        raise ValueError(f"ranker must be a BoostRanker or a list of 1..{MAX_BOOSTS} of them")
    return boosts


def class_weights(boosts) -> list:
    """W[c] for c in [0, 2^m): the product of weight_i over the set bits i of c, i ascending, in
    Python floats; W[0] = 1.0.  A product that overflows or underflows raises ValueError."""
    weights = [b.weight if isinstance(b, BoostRanker) else _check_weight(b) for b in boosts]
    if not 1 <= len(weights) <= MAX_BOOSTS:
        raise ValueError(f"boost ranker: 1..{MAX_BOOSTS} boosts, got {len(weights)}")
    out = []
    for c in range(1 << len(weights)):
        w = 1.0
        for i, wi in enumerate(weights):
            if (c >> i) & 1:
                w = w * wi
        if not math.isfinite(w) or not w > 0.0:
            raise ValueError(f"boost ranker: the product of the weights of class {c:#b} is {w!r}; every class weight "
                             "must be finite and > 0")
        out.append(w)
    return out


def boost_reference(scores64, pass_mask, class_of_row, W, k: int):
    """The definition of the boosted ranking.  scores64: fp64 [B, N] ranking scores; pass_mask: bool
    [N] or None (every row takes part); class_of_row: int [N] in [0, len(W)); W: the class weights.
    -> (scores f32 [B, k], rows i64 [B, k], boosted f64 [B, k], base f64 [B, k]): per query the best k
    passing rows by (boosted desc, s desc, row asc), boosted = W[class] * s as one fp64
    multiplication; the tail is -inf / -1 / -inf / -inf."""
    s = np.asarray(scores64, dtype=np.float64)
    if s.ndim != 2:
        raise ValueError("boost_reference expects scores [B, N]")
    B, N = s.shape
    cls = np.asarray(class_of_row, dtype=np.int64).reshape(N)
    w = np.asarray(W, dtype=np.float64)[cls]
    rows = np.arange(N, dtype=np.int64) if pass_mask is None else np.flatnonzero(np.asarray(pass_mask, dtype=bool))
    scores = np.full((B, k), -np.inf, dtype=np.float32)
    ids = np.full((B, k), -1, dtype=np.int64)
    boosted = np.full((B, k), -np.inf, dtype=np.float64)
    base = np.full((B, k), -np.inf, dtype=np.float64)
    for b in range(B):
        sb = s[b, rows]
        bb = w[rows] * sb
        order = np.lexsort((rows, -sb, -bb))[:k]   # last key first: boosted desc, then s desc, then row asc
        n = order.size
        ids[b, :n] = rows[order]
        boosted[b, :n] = bb[order]
        base[b, :n] = sb[order]
        scores[b, :n] = bb[order].astype(np.float32)
    return scores, ids, boosted, base
