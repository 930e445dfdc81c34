"""Adversarial corpora for the exactness margin of the search path.  TEST INFRASTRUCTURE ONLY
(same rules as oracle/search.py); plain numpy on the CPU.

Near-tie clusters: rows that the contract's float64 score separates and no float32
score can.  Take a unit query q, shrink `n_small` of its components by 2^-5, renormalise, round to
fp16.  Row 0 of the cluster is q itself; row j is q with ONE shrunk component moved one fp16 ulp
(np.nextafter on float16), alternately up and down.  A shrunk component is ~2^-9..2^-11, so its
ulp is ~2^-20 and one step moves the score (~1) by ~1e-9: a fraction of the 6e-8 spacing of
float32 there.  Past n_small + 1 rows a row steps TWO components.

Value-range corpora: finite fp16 far from the exponent of a unit row (subnormals, values at the
largest finite fp16, one dominant row, per-row scales, cancelling signs).
"""
from __future__ import annotations

import numpy as np

from . import search as osearch

SHRINK = np.float32(2.0 ** -5)
FP16_MAX = np.float16(65504.0)
FP16_MIN_NORMAL = 2.0 ** -14


def default_small(dim: int) -> int:
    """How many components near_tie_cluster shrinks: 96, or half the row below dim 192."""
    return min(96, dim // 2)


def near_tie_cluster(dim: int, m: int, seed: int, n_small: int | None = None):
    """-> (q fp16 [dim], rows fp16 [m, dim]).  rows[0] == q; rows[j] differs from q in one
    component (j <= n_small) or two (beyond) by one fp16 ulp."""
    n_small = default_small(dim) if n_small is None else n_small
    assert 2 <= n_small <= dim and 1 <= m <= 1 + n_small + n_small * (n_small - 1)
    rng = np.random.default_rng(seed)
    q = osearch.synth_unit_rows(1, dim, seed)[0].astype(np.float32)
    # random components among those below 2^-3 (then the smallest of the others): shrunk and
    # renormalised they stay below ~2^-7.5, where one fp16 ulp is at most 2^-18 -- so one step moves
    # the score by < 2.2e-8 and the whole cluster spans < 0.75 float32 spacings of a score near 1
    perm = rng.permutation(dim)
    key = np.maximum(np.abs(q[perm]), np.float32(0.125))
    small = np.sort(perm[np.argsort(key, kind="stable")[:n_small]])
    q[small] *= SHRINK
    q16 = osearch.l2_normalize_f32(q[None, :])[0].astype(np.float16)
    rows = np.repeat(q16[None, :], m, axis=0)
    up, down = np.float16(np.inf), np.float16(-np.inf)
    for j in range(1, m):
        t = j - 1
        if t < n_small:
            comps = (small[t],)
        else:               # two components: a, and the one (1 + round) places further on
            t -= n_small
            a, rnd = t % n_small, t // n_small
            comps = (small[a], small[(a + 1 + rnd) % n_small])
        for i in comps:
            rows[j, i] = np.nextafter(q16[i], up if j % 2 else down)
    return q16, rows


def embed_clusters(n: int, dim: int, seed: int, clusters, start: int = 5, stride: int = 37):
    """A synth_unit_rows corpus of n rows with the clusters' rows scattered through it, interleaved:
    row j of cluster c sits at start + (j * len(clusters) + c) * stride.  A stride that is no
    multiple of 32 crosses blocks and partitions.  -> (corpus fp16 [n, dim], positions: one int64
    array per cluster)."""
    c16 = osearch.synth_unit_rows(n, dim, seed)
    nc = len(clusters)
    pos = []
    for ci, rows in enumerate(clusters):
        p = start + (np.arange(rows.shape[0], dtype=np.int64) * nc + ci) * stride
        assert p[-1] < n, "the clusters do not fit: lower the stride"
        c16[p] = rows
        pos.append(p)
    assert len(np.unique(np.concatenate(pos))) == sum(len(p) for p in pos)
    return c16, pos


def scatter_stride(n: int, total_rows: int, start: int = 5) -> int:
    """The largest odd stride (no multiple of 32, so block boundaries are crossed at every phase)
    at which total_rows scattered rows fit into n."""
    s = (n - 1 - start) // max(1, total_rows - 1) if total_rows > 1 else 1
    s = max(1, min(s, 211))
    return s if s % 2 else s - 1 if s > 1 else 1


def f32_scores(q16: np.ndarray, c16: np.ndarray) -> np.ndarray:
    """What a float32 scoring sees: a float32 matmul of the widened fp16 values."""
    return np.asarray(q16, np.float16).astype(np.float32) @ np.asarray(c16, np.float16).astype(np.float32).T


# ---- the fp16 value range -----------------------------------------------------------------------
KINDS = ("unit", "tiny", "huge", "outlier", "mixed", "cancel")


def value_range(kind: str, n: int, dim: int, b: int, seed: int):
    """-> (corpus fp16 [n, dim], queries fp16 [b, dim]), all finite.
      unit     synth_unit_rows (the baseline)
      tiny     rows and queries scaled by 2^-10 (2^-11 below dim 128, where a unit row's
               components are ~2^-3 and 2^-10 would leave only ~38% of them below 2^-14): most
               components are fp16 subnormals
      huge     rows and queries scaled by 2^10, a few components of some set to +-65504
      outlier  unit rows and one row (n // 3) of norm ~2^13
      mixed    per-row and per-query scales 2^U[-12, 12]
      cancel   rows and queries alternate +-large components: scores near 0, |q||c| large"""
    rng = np.random.default_rng(seed)
    c = osearch.synth_unit_rows(n, dim, seed + 1).astype(np.float32)
    q = osearch.synth_unit_rows(b, dim, seed + 2).astype(np.float32)
    if kind == "unit":
        pass
    elif kind == "tiny":
        down = np.float32(2.0 ** (-10 if dim >= 128 else -11))
        c *= down
        q *= down
    elif kind == "huge":
        c *= np.float32(2.0 ** 10)
        q *= np.float32(2.0 ** 10)
        # 5% of the rows and half of the queries carry 8 extreme values among the same 16
        # components, so that they meet: scores reach 8 * 65504^2 = 3.4e10
        for x, share in ((c, 0.05), (q, 0.5)):
            for r in np.flatnonzero(rng.random(x.shape[0]) < share):
                hot = rng.choice(16, 8, replace=False) * (dim // 16)
                x[r, hot] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), 8) * np.float32(FP16_MAX)
    elif kind == "outlier":
        c[n // 3] *= np.float32(2.0 ** 13)
    elif kind == "mixed":
        c *= np.exp2(rng.uniform(-12, 12, (n, 1))).astype(np.float32)
        q *= np.exp2(rng.uniform(-12, 12, (b, 1))).astype(np.float32)
    elif kind == "cancel":
        # queries carry +-24 with period 2, rows +-48 in the same pattern with the second half of
        # the row negated (and either sign overall): the products are +1152 over the first half
        # and -1152 over the second, so the partial sums climb to 576 dim before they cancel, and
        # what is left comes from the unit parts
        alt = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0).astype(np.float32)
        half = np.where(np.arange(dim) < dim // 2, 1.0, -1.0).astype(np.float32)
        sign = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), (n, 1))
        c = np.float32(48.0) * sign * (alt * half)[None, :] + np.float32(8.0) * c
        q = np.float32(24.0) * alt[None, :] + np.float32(8.0) * q
    else:
        raise ValueError(kind)
    c16 = np.ascontiguousarray(c.astype(np.float16))
    q16 = np.ascontiguousarray(q.astype(np.float16))
    assert np.isfinite(c16).all() and np.isfinite(q16).all()
    return c16, q16


def flush_subnormals(x16: np.ndarray) -> np.ndarray:
    """fp16 with every subnormal replaced by a zero of its sign (what a flushing datapath reads)."""
    x = np.asarray(x16, np.float16).copy()
    sub = (np.abs(x.astype(np.float32)) < FP16_MIN_NORMAL) & (x != 0)
    x[sub] = np.copysign(np.float16(0), x[sub])
    return x


def subnormal_share(x16: np.ndarray) -> float:
    """The share of the non-zero components that are fp16 subnormals."""
    a = np.abs(np.asarray(x16, np.float16).astype(np.float32))
    nz = a > 0
    return float(((a < FP16_MIN_NORMAL) & nz).sum() / max(1, nz.sum()))
