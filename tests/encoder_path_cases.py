"""What tests/test_encoder_path_cases_cpu.py and tests/test_encoder_paths_gpu.py share: the batches that put every
GEMM path of the BERT forward (encode_enqueue, csrc/encoder.hip) at the token counts where the slot count B * T,
which selects the kernels, and the packed count M = sum(lens), which every kernel reads from device memory, diverge.

  path_of(B, T)          the kernel class a batch runs on, from the thresholds of launch_linear / encode_enqueue
  EDGE_CASES             packed-count edges: M at and next to the 64 / 128 / 256-token tile edges of each path
  BOUNDARY_CASES         dense batches on both sides of every slot threshold
  lens_with_total(...)   a lens vector of a given sum, zero elsewhere, its live rows scattered

The CPU test proves for every case the path, the packed count and the placement rules; the GPU test then runs them.
Nothing here needs a GPU."""
import functools

import numpy as np

from oracle import encoder as oenc

CFG = dict(oenc.MINILM_L6, layers=2, vocab_size=2000)   # two layers: k_post_block reads a QKV k_linear_dma wrote AND writes the next layer's
SEED = 29
SMALL_SLOTS, DMA_SLOTS, WIDE_SLOTS = 1024, 8192, 49152
PATHS = ("one_query", "small", "direct", "dma", "dma_wide")
TILE = {"direct": 64, "dma": 128, "dma_wide": 256}      # tokens of one workgroup of the path's (first) GEMM


def path_of(B: int, T: int) -> str:
    """The kernel class of a [B, T] batch: the fused single-query launch, k_linear_small + k_ln_rows, k_linear,
    k_linear_dma<0> + k_post_block, k_linear_dma<1> + k_post_block."""
    slots = B * T
    if B == 1 and T <= 32:
        return "one_query"
    if slots <= SMALL_SLOTS:
        return "small"
    if slots < DMA_SLOTS:
        return "direct"
    return "dma" if slots < WIDE_SLOTS else "dma_wide"


def lens_with_total(B: int, T: int, M: int, seed: int) -> np.ndarray:
    """int32 [B] with sum M, every entry in [0, T], zero outside the live rows.

    The live lengths: one row of length 1 (M >= 1); one row of length T once M >= T + 1; what is left is cut into
    max(min(3, left), ceil(left / (T - 1))) pieces of 1 .. T - 1 tokens.  The live rows: with three or more of them,
    row 0, row B // 2 and row B - 1 and then rows drawn at random; two live rows (M = T + 1 leaves no third) sit at
    row 0 and row B - 1; a single one sits at row B // 2, between empty rows on both sides.  Which length goes to
    which row is drawn from the seed."""
    assert B >= 3 and T >= 2 and 0 <= M <= B * T
    rng = np.random.default_rng(seed)
    lengths = []
    left = M
    if left >= 1:
        lengths.append(1)
        left -= 1
    if M >= T + 1:
        lengths.append(T)
        left -= T
    if left > 0:
        k = max(min(3, left), -(-left // (T - 1)))
        parts = np.full(k, 2 if left >= 2 * k and T > 2 else 1, dtype=np.int64)   # (no second row of one token)
        for _ in range(left - int(parts.sum())):                        # one token at a time to a piece that still has room
            room = np.flatnonzero(parts < T - 1)
            parts[rng.choice(room)] += 1
        lengths += parts.tolist()
    n = len(lengths)
    assert n <= B and sum(lengths) == M
    if n >= 3:
        first = [0, B // 2, B - 1]
        others = [r for r in rng.permutation(B).tolist() if r not in first]
        rows = first + others[:n - 3]
    elif n == 2:
        rows = [0, B - 1]
    else:
        rows = [B // 2][:n]
    lens = np.zeros(B, dtype=np.int32)
    if n:
        lens[rows] = rng.permutation(np.asarray(lengths, dtype=np.int32))
    return lens


def random_ids(B: int, T: int, seed: int, vocab: int = CFG["vocab_size"]) -> np.ndarray:
    """Random ids in [1, vocab) everywhere, padding included: what the padding holds must not matter."""
    return np.random.default_rng(seed).integers(1, vocab, (B, T)).astype(np.int32)


# ---- packed-count edges ---------------------------------------------------------------------------------------------
# path -> (B, T, the values of M)
EDGE_TABLE = {
    "direct": (40, 64, (0, 1, 63, 64, 65, 129)),
    "dma": (64, 128, (0, 1, 31, 32, 33, 127, 128, 129, 257)),
    "dma_wide": (384, 128, (0, 1, 127, 128, 129, 255, 256, 257, 513)),
}
EDGE_CASES = [(path, B, T, M) for path, (B, T, Ms) in EDGE_TABLE.items() for M in Ms]
WORKSPACE_CASES = [("direct", 40, 64, 65), ("dma", 64, 128, 129), ("dma_wide", 384, 128, 257)]


def edge_id(case) -> str:
    path, B, T, M = case
    return f"{path}_{B}x{T}_M{M}"


@functools.lru_cache(maxsize=None)
def edge_batch(path: str, B: int, T: int, M: int):
    """-> (ids int32 [B, T], lens int32 [B] of sum M, dense_lens int32 [B]): dense_lens gives every empty row a
    random positive length and leaves the live rows as they are.  Read-only."""
    seed = 1000 * PATHS.index(path) + M
    lens = lens_with_total(B, T, M, seed)
    ids = random_ids(B, T, seed + 500)
    dense = np.where(lens > 0, lens, np.random.default_rng(seed + 900).integers(1, T + 1, B)).astype(np.int32)
    for a in (ids, lens, dense):
        a.setflags(write=False)
    return ids, lens, dense


# ---- slot boundaries --------------------------------------------------------------------------------------------------
# (name, B, T, the path the shape must run on); consecutive pairs straddle one threshold
BOUNDARY_CASES = [
    ("small_32x32", 32, 32, "small"), ("direct_41x25", 41, 25, "direct"),
    ("direct_8191x1", 8191, 1, "direct"), ("dma_8192x1", 8192, 1, "dma"),
    ("dma_2137x23", 2137, 23, "dma"), ("wide_2048x24", 2048, 24, "dma_wide"),
]
BOUNDARY_PAIRS = [("small_32x32", "direct_41x25", SMALL_SLOTS + 1), ("direct_8191x1", "dma_8192x1", DMA_SLOTS),
                  ("dma_2137x23", "wide_2048x24", WIDE_SLOTS)]   # (below, above, the first slot count of the upper class)
N_PROBES, N_SHARED, N_EMPTY_T1 = 8, 16, 12


@functools.lru_cache(maxsize=None)
def boundary_batch(name: str):
    """-> (ids [B, T], lens [B], probes [8], shared [16] or None).  lens is dense, U[1, T]; the two T = 1 batches
    have a dozen rows of length 0.  probes are eight live rows compared with the oracle; shared are the rows that
    hold, in BOTH batches of the (8191 | 8192) and (49151 | 49152) pairs, the same sixteen sequences.  Read-only."""
    _, B, T, _ = next(c for c in BOUNDARY_CASES if c[0] == name)
    pair = next((p for p in BOUNDARY_PAIRS[1:] if name in p[:2]), None)
    rng = np.random.default_rng(B * 100 + T)
    lens = rng.integers(1, T + 1, B).astype(np.int32)
    ids = random_ids(B, T, B * 100 + T + 1)
    shared = None
    if pair is not None:
        # the same sixteen sequences at the same rows of both batches; their width is the narrower batch's
        Bmin = min(c[1] for c in BOUNDARY_CASES if c[0] in pair[:2])
        Tmin = min(c[2] for c in BOUNDARY_CASES if c[0] in pair[:2])
        srng = np.random.default_rng(BOUNDARY_PAIRS.index(pair))
        shared = np.sort(srng.choice(Bmin, N_SHARED, replace=False))
        s_ids = srng.integers(1, CFG["vocab_size"], (N_SHARED, Tmin)).astype(np.int32)
        s_lens = srng.integers(1, Tmin + 1, N_SHARED).astype(np.int32)
        s_lens[0], s_lens[1] = Tmin, 1
        ids[shared, :Tmin] = s_ids
        lens[shared] = s_lens
    if T == 1:
        free = np.setdiff1d(np.arange(B), shared)
        lens[rng.choice(free, N_EMPTY_T1, replace=False)] = 0
    live = np.flatnonzero(lens > 0)
    probes = np.sort(np.concatenate([live[[0, -1]], rng.choice(live[1:-1], N_PROBES - 2, replace=False)]))
    for a in (ids, lens, probes) + (() if shared is None else (shared,)):
        a.setflags(write=False)
    return ids, lens, probes, shared


# ---- the oracle -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights():
    """(fp32 weights, fp16-rounded weights) of CFG from SEED: both sides of a test from the seed alone."""
    w = oenc.random_weights(CFG, SEED)
    return w, oenc.round_weights_fp16(w)


def oracle_rows(ids, lens, rows) -> np.ndarray:
    """oracle.encoder.encode in float64 on the fp16-rounded weights, of the named rows only (a sequence's embedding
    does not depend on what else is in the batch) -> float64 [len(rows), 384]."""
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size == 0:
        return np.zeros((0, CFG["hidden"]))
    return oenc.encode(weights()[1], CFG, np.asarray(ids)[rows], np.asarray(lens)[rows])


@functools.lru_cache(maxsize=None)
def edge_oracle(path: str, B: int, T: int, M: int):
    """-> (live rows, their oracle embeddings), computed once per case and read-only."""
    ids, lens, _ = edge_batch(path, B, T, M)
    live = np.flatnonzero(lens > 0)
    want = oracle_rows(ids, lens, live)
    want.setflags(write=False)
    return live, want


# ---- the heads' batches -----------------------------------------------------------------------------------------------
HEAD_EDGE_LENS = (64, 1, 31, 32, 33)       # at rows 0, 9, 19, 29, 39 of the 40 x 64 batch
HEAD_EDGE_ROWS = (0, 9, 19, 29, 39)
HEAD_SEGS = (1, 31, 32, 33)                # the second segment's start, as tests/test_rerank_gpu.py SHAPES places it
HEAD_SPARSE = {0: 33, 31: 1, 63: 95}       # row -> length: three live rows, M = 129
HEAD_SPARSE_SEG = {0: 9, 31: 1, 63: 31}


@functools.lru_cache(maxsize=None)
def head_batch(kind: str, vocab: int):
    """The batches every head runs on -> a dict of read-only arrays.
      "direct"  40 x 64, ragged, the lengths 1, 31, 32, 33, 64 among the rows: ids, lens, seg
      "wide"    64 x 128 and 384 x 128 whose first 64 rows are those same rows: ids, lens, seg (the 384 rows; the
                first 64 are the narrow batch) and probes, eight rows among the last 64
      "sparse"  64 x 128 with three live rows summing to M = 129: ids, lens, seg, dense (the lengths of its dense twin)
    seg is the first token of the second segment of a pair (<= len), for the heads that take pairs."""
    if kind == "direct":
        B, T = 40, 64
        rng = np.random.default_rng(401)
        lens = rng.integers(1, T + 1, B).astype(np.int32)
        lens[list(HEAD_EDGE_ROWS)] = HEAD_EDGE_LENS
        seg = np.minimum(np.asarray(HEAD_SEGS, dtype=np.int32)[np.arange(B) % 4], lens)
        out = dict(ids=random_ids(B, T, 411, vocab), lens=lens, seg=seg)
    elif kind == "wide":
        B, T = 384, 128
        rng = np.random.default_rng(402)
        lens = rng.integers(1, T + 1, B).astype(np.int32)
        lens[0], lens[1], lens[63] = T, 1, 33
        probes = np.array([320, 329, 338, 347, 356, 365, 374, 383])
        lens[probes] = (1, 31, 32, 33, 64, 65, 127, T)
        seg = np.minimum(rng.integers(2, 30, B).astype(np.int32), lens)
        out = dict(ids=random_ids(B, T, 412, vocab), lens=lens, seg=seg, probes=probes)
    elif kind == "sparse":
        B, T = 64, 128
        lens = np.zeros(B, dtype=np.int32)
        seg = np.zeros(B, dtype=np.int32)
        for r, n in HEAD_SPARSE.items():
            lens[r], seg[r] = n, HEAD_SPARSE_SEG[r]
        rng = np.random.default_rng(403)
        dense = np.where(lens > 0, lens, rng.integers(1, T + 1, B)).astype(np.int32)
        dense_seg = np.where(lens > 0, seg, np.minimum(rng.integers(2, 30, B), dense)).astype(np.int32)
        out = dict(ids=random_ids(B, T, 413, vocab), lens=lens, seg=seg, dense=dense, dense_seg=dense_seg)
    else:
        raise KeyError(kind)
    for a in out.values():
        a.setflags(write=False)
    return out
