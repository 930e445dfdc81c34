"""The row filter's definition in numpy.  TEST INFRASTRUCTURE ONLY (same rules as oracle/search.py).

Two things the filter kernels (rag_fin_amd/csrc/filter.hip) must reproduce:

  run_ops / run_program   the postfix program of rf_filter_eval / rf_filter_eval_bitmaps
                          (include/ragfin.h, "filtered search"), one numpy array per stack entry.
                          Raw op tuples and raw word arrays in, a bool row mask out: nothing here
                          needs the expression compiler, and nothing here calls the library.
  plan                    how a filter buffer of n rows is cut into compaction tiles (plan_tiles in
                          filter.hip; RF_FILTER_MAX_TILES in rf_internal.h), which the device writes
                          into header word 3.

The opcodes are restated from include/ragfin.h so that this module imports nothing of the package;
tests/test_filter_programs_gpu.py holds them against rag_fin_amd._lib.
"""
from __future__ import annotations

import numpy as np

# include/ragfin.h, "filtered search"
FOP_CODESET, FOP_RANGE, FOP_ROWLIST, FOP_TRUE, FOP_FALSE, FOP_AND, FOP_OR, FOP_NOT, FOP_BITMAP = range(1, 10)
FRANGE_LO_INCL = 1
FRANGE_HI_INCL = 2
FILTER_MAX_OPS = 64
FILTER_MAX_DEPTH = 32
# rf_internal.h: "#define RF_FILTER_MAX_TILES 1024   // compaction tiles; a tile is 32 * rows_per_thread
# mask words"
FILTER_MAX_TILES = 1024
FILTER_HDR_WORDS = 4

LEAF_OPS = (FOP_CODESET, FOP_RANGE, FOP_ROWLIST, FOP_TRUE, FOP_FALSE, FOP_BITMAP)


def plan(n: int) -> tuple[int, int, int]:
    """(nblk, tile_words, n_tiles) of a filter buffer over n rows.

    include/ragfin.h: the mask has nblk = ceil(n / 32) words and header word 3 is n_tiles.
    rf_internal.h: at most RF_FILTER_MAX_TILES tiles, a tile a multiple of 32 mask words (one trip of
    a 16-wave workgroup of k_filter_eval, two words per wave).  So the tile is the smallest multiple
    of 32 words with which 1024 tiles cover the mask:
        tile_words = 32 * max(1, ceil(nblk / (32 * 1024))),  n_tiles = ceil(nblk / tile_words)
    tile_words is 32 up to n = 1 048 576; above 256 (k_filter_compact takes a second 256-word chunk)
    from n = 8 388 609; above 1024 (k_filter_copy strides) from n = 33 554 433."""
    nblk = (n + 31) // 32
    per = 32 * FILTER_MAX_TILES
    tile_words = 32 * max(1, (nblk + per - 1) // per)
    return nblk, tile_words, (nblk + tile_words - 1) // tile_words


def filter_bytes(n: int) -> int:
    """rf_filter_bytes: header, mask and block list (each nblk words, 16-byte aligned), then the
    per-tile counts {non-empty blocks, passing rows} of the compaction."""
    words = ((n + 31) // 32 * 4 + 15) // 16 * 16
    return 4 * FILTER_HDR_WORDS + 2 * words + 2 * 4 * FILTER_MAX_TILES


def resolve_bitmap_ops(ops, words_per_leaf: int) -> list:
    """A compiled program names the bitmap of text leaf l as (off = l, len = 0); the launch turns that
    into the leaf's word range (filter_expr.Program.ops_ctypes).  The same step on tuples."""
    return [(op, col, off * words_per_leaf, words_per_leaf, flags, lo, hi) if op == FOP_BITMAP
            else (op, col, off, ln, flags, lo, hi) for op, col, off, ln, flags, lo, hi in ops]


def run_ops(ops, code_sets, row_lists, bitmaps, codes, values, n: int) -> np.ndarray:
    """ops: tuples (op, column, off, len, flags, lo, hi); code_sets / row_lists / bitmaps: the uint32
    word arrays the leaves point into (None or empty when no leaf reads them); codes: {column index:
    int32 [n]}; values: fp64 [n] -> bool [n], row r of the mask."""
    cs = np.asarray(code_sets if code_sets is not None else [], dtype=np.uint32).reshape(-1)
    rl = np.asarray(row_lists if row_lists is not None else [], dtype=np.uint32).reshape(-1)
    bm = np.asarray(bitmaps if bitmaps is not None else [], dtype=np.uint32).reshape(-1)
    rows = np.arange(n, dtype=np.uint32)
    stack = []
    for op, col, off, ln, flags, lo, hi in ops:
        if op == FOP_AND:
            b, a = stack.pop(), stack.pop()
            stack.append(a & b)
        elif op == FOP_OR:
            b, a = stack.pop(), stack.pop()
            stack.append(a | b)
        elif op == FOP_NOT:
            stack.append(~stack.pop())
        elif op == FOP_CODESET:
            c = codes[col].astype(np.int64)
            ok = (c >= 0) & (c < 32 * ln)
            w = cs[off + np.clip(c >> 5, 0, max(ln - 1, 0))] if ln else np.zeros(n, np.uint32)
            stack.append(ok & (((w >> (c & 31).astype(np.uint32)) & 1) == 1))
        elif op == FOP_RANGE:
            with np.errstate(invalid="ignore"):
                a = values >= lo if flags & FRANGE_LO_INCL else values > lo
                b = values <= hi if flags & FRANGE_HI_INCL else values < hi
            stack.append(a & b)
        elif op == FOP_ROWLIST:
            stack.append(np.isin(rows, rl[off:off + ln]))
        elif op == FOP_BITMAP:
            # row r passes iff r >> 5 < len and bit r & 31 of bitmaps[off + (r >> 5)] is set
            word = (rows >> 5).astype(np.int64)
            ok = word < ln
            w = bm[off + np.minimum(word, max(ln - 1, 0))] if ln else np.zeros(n, np.uint32)
            stack.append(ok & (((w >> (rows & 31)) & 1) == 1))
        elif op == FOP_TRUE:
            stack.append(np.ones(n, bool))
        elif op == FOP_FALSE:
            stack.append(np.zeros(n, bool))
        else:
            raise AssertionError(op)
    assert len(stack) == 1
    return stack[0]


def run_program(prog, codes, values, n: int, bitmaps=None) -> np.ndarray:
    """run_ops of a compiled filter_expr.Program (its ops, code_sets and row_lists).  bitmaps: uint32
    [L, words_per_leaf], one row per text leaf, when the program has RF_FOP_BITMAP leaves."""
    ops = prog.ops
    if bitmaps is not None:
        bitmaps = np.asarray(bitmaps, dtype=np.uint32)
        ops = resolve_bitmap_ops(ops, bitmaps.shape[1])
    return run_ops(ops, prog.code_sets, prog.row_lists, bitmaps, codes, values, n)


def pack_rows(mask) -> np.ndarray:
    """bool [n] -> the uint32 mask words (bit r & 31 of word r >> 5 = row r; bits past n zero)."""
    mask = np.asarray(mask, dtype=bool)
    bits = np.zeros((mask.size + 31) // 32 * 32, dtype=np.uint8)
    bits[:mask.size] = mask
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


def popcount(words) -> int:
    return int(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)).sum(dtype=np.int64))
