"""pymilvus-shaped arguments of `CorpusStore.hybrid_search`: one `AnnSearchRequest` per arm (a dense
search of "embedding" or a BM25 search of "sparse") and the `RRFRanker` that fuses the arms' lists
by weighted reciprocal rank on the GPU (rf_fuse_rrf)."""
from __future__ import annotations

import math
import numbers

MAX_ARMS = 4   # RF_FUSE_MAX_ARMS (include/ragfin.h)


class AnnSearchRequest:
    """One arm of a hybrid search.  data: query vectors [B, dim] for anns_field "embedding", a list of
    B query strings for "sparse"; param: {"metric_type": "COSINE" | "IP"} / {"metric_type": "BM25"};
    limit: hits this arm contributes per query (1..64); expr: this arm's own filter."""

    def __init__(self, data, anns_field: str, param: dict | None = None, limit: int = 10, expr: str | None = None):
        if isinstance(limit, bool) or not isinstance(limit, numbers.Integral) or limit < 1:
            raise ValueError(f"AnnSearchRequest: limit must be an integer >= 1, got {limit!r}")
        if not isinstance(anns_field, str):
            raise ValueError(f"AnnSearchRequest: anns_field must be a string, got {anns_field!r}")
        if param is not None and not isinstance(param, dict):
            raise ValueError("AnnSearchRequest: param must be a dict")
        self.data = data
        self.anns_field = anns_field
        self.param = dict(param or {})
        self.limit = int(limit)
        self.expr = expr

    def __repr__(self):
        return f"AnnSearchRequest(anns_field={self.anns_field!r}, limit={self.limit}, expr={self.expr!r})"


class RRFRanker:
    """Weighted reciprocal-rank fusion: fused(d) = sum over the arms a that hold d of
    weights[a] / (k + rank_a(d)), rank 1-based.  k: the smoothing constant (Milvus' default 60);
    weights: one per arm in request order, finite and >= 0 (default: all 1.0)."""

    def __init__(self, k: float = 60, weights=None):
        if isinstance(k, bool) or not isinstance(k, numbers.Real) or not math.isfinite(float(k)) or float(k) <= 0:
            raise ValueError(f"RRFRanker: k must be a finite number > 0, got {k!r}")
        self.k = float(k)
        if weights is not None:
            weights = list(weights)
            for w in weights:
                if isinstance(w, bool) or not isinstance(w, numbers.Real) or not math.isfinite(float(w)) or float(w) < 0:
                    raise ValueError(f"RRFRanker: weights must be finite numbers >= 0, got {w!r}")
            weights = [float(w) for w in weights]
        self.weights = weights

    def arm_weights(self, n_arms: int) -> list[float]:
        if self.weights is None:
            return [1.0] * n_arms
        if len(self.weights) != n_arms:
            raise ValueError(f"RRFRanker: {len(self.weights)} weights for {n_arms} search requests")
        return list(self.weights)


class WeightedRanker:
    """Milvus' score-normalising ranker (atan of each arm's score) is not offered: it needs the arms'
    scores on one scale.  Weigh the arms by rank instead."""

    def __init__(self, *weights):
        raise NotImplementedError("WeightedRanker (score normalisation) is not supported; "
                                  "use RRFRanker(weights=...) to weigh the arms")
