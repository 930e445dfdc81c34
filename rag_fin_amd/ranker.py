"""Boosted search: pymilvus' Boost Ranker (`Function(..., FunctionType.RERANK, params={"reranker":
"boost", "filter": ..., "weight": ...})`, passed to `search(..., ranker=)`) as a value object, the
class weights it induces and the definition of the boosted ranking in numpy.

m <= 3 boosts (filter_i, weight_i) split the rows into 2^m classes: bit i of a row's class is set iff
the row passes filter_i.  W[c] is the product of the weights of c's set bits; with s the fp64
ranking score, boosted = W[class] * s, and rows rank by (boosted desc, s desc, row asc).

Decay ranker (pymilvus' `params={"reranker": "decay", "function": "gauss" | "exp" | "linear", "origin": ...,
"scale": ..., "offset": ..., "decay": ...}` over a numeric field): every row has a weight of its own
in [0, 1] -- 1 within `offset` of `origin`, `decay` at distance offset + scale -- and rows rank by (w * s desc,
s desc, row asc).  `decay_weights_reference` defines the weight, bit for bit what rf_decay_weights computes on
the device, `decay_reference` the ranking."""
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


# ---- decay ranker -------------------------------------------------------------------------------------
DECAY_FUNCTIONS = ("gauss", "exp", "linear")   # the function codes of rf_decay_weights, in this order
_LN2 = np.float64(0.6931471805599453)
# 1/13!, 1/12!, ..., 1/1!, 1/0!: the Taylor coefficients of e^x, each a correctly rounded quotient
_EXP_COEFFS = tuple(np.float64(1.0) / np.float64(math.factorial(j)) for j in range(13, -1, -1))
EXP2_NEG_CUTOFF = 1100.0   # 2^-t is 0 from here on (the smallest subnormal is 2^-1074)


def _check_real(what: str, v) -> float:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"decay ranker: {what} must be a real number, got {v!r}")
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"decay ranker: {what} must be finite, got {v!r}")
    return v


class DecayRanker:
    """Scores decay with the distance of a numeric field's value from `origin`: the weight of a row is 1 within
    `offset` of the origin and falls to `decay` at distance offset + scale, along a bell curve ("gauss"), an
    exponential ("exp") or a straight line that reaches 0 ("linear").  `field` is primary_value or an INT64 /
    DOUBLE field of the collection (checked by the store that runs the search)."""

    def __init__(self, field: str, function: str, origin, scale, offset=0.0, decay=0.5, name: str = "decay"):
        if not isinstance(field, str) or not field.strip():
            raise ValueError(f"decay ranker: field must be a field name, got {field!r}")
        if not isinstance(function, str) or function.lower() not in DECAY_FUNCTIONS:
            raise ValueError(f"decay ranker: function must be one of {', '.join(DECAY_FUNCTIONS)}, got {function!r}")
        if not isinstance(name, str):
            raise ValueError(f"decay ranker: name must be a string, got {name!r}")
        self.field = field
        self.function = function.lower()
        self.origin = _check_real("origin", origin)
        self.scale = _check_real("scale", scale)
        self.offset = _check_real("offset", offset)
        self.decay = _check_real("decay", decay)
        if not self.scale > 0.0:
            raise ValueError(f"decay ranker: scale must be > 0, got {scale!r}")
        if not self.offset >= 0.0:
            raise ValueError(f"decay ranker: offset must be >= 0, got {offset!r}")
        if not 0.0 < self.decay < 1.0:
            raise ValueError(f"decay ranker: decay must lie strictly between 0 and 1, got {decay!r}")
        self.name = name
        # the one constant the device is handed beside origin / scale / offset: L = -log2(decay) for gauss and
        # exp (w = 2^(-L ...)), S = scale / (1 - decay) for linear (w = (S - d) / S)
        if self.function == "linear":
            self.shape = self.scale / (1.0 - self.decay)
            if not math.isfinite(self.shape):
                raise ValueError(f"decay ranker: scale / (1 - decay) overflows for scale = {scale!r}, decay = {decay!r}")
        else:
            self.shape = -math.log2(self.decay)
            if not self.shape > 0.0:   # (a decay that rounds to 1)
                raise ValueError(f"decay ranker: decay = {decay!r} is too close to 1")

    @property
    def function_code(self) -> int:
        return DECAY_FUNCTIONS.index(self.function)

    @classmethod
    def from_params(cls, params: dict, field: str, name: str = "decay") -> "DecayRanker":
        """From Milvus' params dict {"reranker": "decay", "function": ..., "origin": ..., "scale": ..., "offset":
        ..., "decay": ...} and the input field name of the Function."""
        if not isinstance(params, dict):
            raise ValueError(f"decay ranker: params must be a dict, got {type(params).__name__}")
        if params.get("reranker") != "decay":
            raise ValueError(f"decay ranker: reranker {params.get('reranker')!r} is not 'decay'")
        unknown = sorted(set(params) - {"reranker", "function", "origin", "scale", "offset", "decay"})
        if unknown:
            raise ValueError(f"decay ranker: unknown params {unknown}")
        missing = [key for key in ("function", "origin", "scale") if key not in params]
        if missing:
            raise ValueError(f"decay ranker: params need {missing}")
        return cls(field, params["function"], params["origin"], params["scale"], params.get("offset", 0.0),
                   params.get("decay", 0.5), name)

    def to_params(self) -> dict:
        return {"reranker": "decay", "function": self.function, "origin": self.origin, "scale": self.scale,
                "offset": self.offset, "decay": self.decay}

    def __repr__(self):
        return (f"DecayRanker({self.field!r}, {self.function!r}, origin={self.origin!r}, scale={self.scale!r}, "
                f"offset={self.offset!r}, decay={self.decay!r})")


def exp2_neg(t):
    """2^-t for float64 t >= 0, defined by its arithmetic so that numpy and the device give the same bits: 0
    unless t < 1100; else n = floor(t + 0.5), f = t - n (exact), x = -(f ln2), the degree-13 Taylor polynomial of
    e^x in Horner form (one multiplication, then one addition, each rounded), and ldexp(p, -n)."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        big = ~(t < EXP2_NEG_CUTOFF)   # also a NaN and +inf
        tt = np.where(big, 0.0, t)
        n = np.floor(tt + 0.5)
        x = -((tt - n) * _LN2)
        p = np.full_like(x, _EXP_COEFFS[0])
        for c in _EXP_COEFFS[1:]:
            p = p * x + c
        r = np.ldexp(p, -n.astype(np.int64))
    return np.where(big, 0.0, r)


def decay_weights_reference(values, ranker: DecayRanker):
    """The definition of the row weights: values int64 or float64 [N] -> float64 [N] in [0, 1].  v = float64(value)
    (an int64 rounds to nearest), d = max(0, |v - origin| - offset); gauss 2^-(L (d / scale)^2), exp
    2^-(L (d / scale)), linear max(0, (S - d) / S); a NaN value weighs 0.  Every operation is one IEEE fp64
    operation, in this order."""
    v = np.asarray(values)
    if v.dtype not in (np.dtype(np.int64), np.dtype(np.float64)):
        raise ValueError(f"decay_weights_reference expects int64 or float64 values, got {v.dtype}")
    v = v.astype(np.float64)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        e = np.abs(v - np.float64(ranker.origin)) - np.float64(ranker.offset)
        d = np.where(e > 0.0, e, 0.0)   # (a NaN lands on 0 and is overruled below)
        c = np.float64(ranker.shape)
        if ranker.function == "linear":
            u = (c - d) / c
            w = np.where(u > 0.0, u, 0.0)
        else:
            r = d / np.float64(ranker.scale)
            w = exp2_neg(c * (r * r) if ranker.function == "gauss" else c * r)
    return np.where(nan, 0.0, w)


def decay_reference(scores64, pass_mask, weights64, k: int):
    """The definition of the decayed ranking.  scores64: fp64 [B, N] ranking scores; pass_mask: bool [N] or None
    (every row takes part); weights64: fp64 [N] row weights.  -> (scores f32 [B, k], rows i64 [B, k], decayed f64
    [B, k], base f64 [B, k]), the shapes of boost_reference: per query the best k passing rows by (decayed desc,
    s desc, row asc), decayed = w[row] * s as one fp64 multiplication; the tail is -inf / -1 / -inf / -inf."""
    s = np.asarray(scores64, dtype=np.float64)
    if s.ndim != 2:
        raise ValueError("decay_reference expects scores [B, N]")
    B, N = s.shape
    w = np.asarray(weights64, dtype=np.float64).reshape(N)
    rows = np.arange(N, dtype=np.int64) if pass_mask is None else np.flatnonzero(np.asarray(pass_mask, dtype=bool))
    scores = np.full((B, k), -np.inf, dtype=np.float32)
    ids = np.full((B, k), -1, dtype=np.int64)
    decayed = np.full((B, k), -np.inf, dtype=np.float64)
    base = np.full((B, k), -np.inf, dtype=np.float64)
    for b in range(B):
        sb = s[b, rows]
        db = w[rows] * sb
        order = np.lexsort((rows, -sb, -db))[:k]   # last key first: decayed desc, then s desc, then row asc
        n = order.size
        ids[b, :n] = rows[order]
        decayed[b, :n] = db[order]
        base[b, :n] = sb[order]
        scores[b, :n] = db[order].astype(np.float32)
    return scores, ids, decayed, base
