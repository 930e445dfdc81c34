"""The condition that keeps tests/test_encoder_paths_gpu.py honest, checked without a GPU: every case of
tests/encoder_path_cases.py runs on the kernel class its table claims, holds exactly the packed count it claims,
places its live rows by the stated rules, and has a finite, unit-norm float64 oracle.  A case that quietly lands on
another path fails here instead of passing there."""
import os
import re

import numpy as np
import pytest

import encoder_path_cases as epc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thresholds_are_the_librarys():
    from rag_fin_amd.embedder import Embedder
    assert epc.SMALL_SLOTS == Embedder.SMALL_SLOTS == 1024
    with open(os.path.join(ROOT, "rag_fin_amd", "csrc", "encoder.hip")) as f:
        src = f.read()
    assert re.search(r"#define SM_MAX_TOK %d\b" % epc.SMALL_SLOTS, src)
    assert re.search(r"rf_knob_linear_dma && tokens >= %d\b" % epc.DMA_SLOTS, src)           # launch_linear: k_linear_dma
    assert re.search(r"rf_knob_post_block && tiles >= %d\b" % epc.DMA_SLOTS, src)            # encode_enqueue: k_post_block
    assert re.search(r"rf_knob_linear_dma == 1 && tokens >= %d\b" % epc.WIDE_SLOTS, src)     # the 256-token form


def test_path_of_at_every_threshold():
    assert epc.path_of(1, 32) == "one_query" and epc.path_of(1, 33) == "small" and epc.path_of(2, 16) == "small"
    assert epc.path_of(1024, 1) == "small" and epc.path_of(1025, 1) == "direct"
    assert epc.path_of(8191, 1) == "direct" and epc.path_of(8192, 1) == "dma"
    assert epc.path_of(49151, 1) == "dma" and epc.path_of(49152, 1) == "dma_wide"
    assert epc.path_of(40, 64) == "direct" and epc.path_of(64, 128) == "dma" and epc.path_of(384, 128) == "dma_wide"


def test_the_edge_table_is_the_issues():
    assert epc.EDGE_TABLE == {"direct": (40, 64, (0, 1, 63, 64, 65, 129)),
                              "dma": (64, 128, (0, 1, 31, 32, 33, 127, 128, 129, 257)),
                              "dma_wide": (384, 128, (0, 1, 127, 128, 129, 255, 256, 257, 513))}
    assert len(epc.EDGE_CASES) == 24
    for path, B, T, Ms in ((p,) + v for p, v in epc.EDGE_TABLE.items()):
        tile = epc.TILE[path]
        assert {tile - 1, tile, tile + 1} <= set(Ms) and {0, 1} <= set(Ms)      # both sides of the first tile edge
        assert any(M > tile + 1 and M % tile == 1 for M in Ms)                  # and one token into a later tile
    assert all(c in epc.EDGE_CASES for c in epc.WORKSPACE_CASES)
    assert [c[3] for c in epc.WORKSPACE_CASES] == [65, 129, 257]


@pytest.mark.parametrize("case", epc.EDGE_CASES, ids=epc.edge_id)
def test_edge_case_path_count_placement_and_oracle(case):
    path, B, T, M = case
    assert epc.path_of(B, T) == path
    ids, lens, dense = epc.edge_batch(*case)
    assert ids.shape == (B, T) and ids.dtype == np.int32 and ids.min() >= 1 and ids.max() < epc.CFG["vocab_size"]
    assert lens.shape == (B,) and lens.dtype == np.int32 and lens.min() >= 0 and lens.max() <= T
    assert int(lens.sum()) == M
    live = np.flatnonzero(lens > 0)
    if M >= 1:
        assert (lens == 1).sum() == 1                                           # one live row of one token
    if M >= T + 1:
        assert (lens == T).sum() == 1                                           # a live row of the full width
    else:
        assert lens.max() < T
    if len(live) >= 3:
        assert {0, B // 2, B - 1} <= set(live.tolist())
    elif len(live) == 2:
        assert M == T + 1 and live.tolist() == [0, B - 1]
    elif len(live) == 1:
        assert M == 1 and live.tolist() == [B // 2]
    assert len(live) >= 3 or M in (0, 1, T + 1)                                 # "once M allows it"
    assert len(live) < B or M == 0                                              # zero-length rows between live ones
    if len(live) >= 2:
        assert (lens[live[0]:live[-1]] == 0).any()
    # the dense twin: the same live rows, no empty row
    assert np.array_equal(dense[live], lens[live]) and dense.min() >= 1 and dense.max() <= T
    assert epc.path_of(B, T) == path and int(dense.sum()) > M
    rows, want = epc.edge_oracle(*case)
    assert np.array_equal(rows, live) and want.shape == (len(live), 384)
    assert np.isfinite(want).all()
    if len(live):
        assert np.abs(np.linalg.norm(want, axis=1) - 1).max() < 1e-12


def test_lens_with_total_over_a_sweep_of_totals():
    for B, T in ((40, 64), (64, 128), (384, 128), (7, 5)):
        for M in range(0, 3 * T + 3):
            lens = epc.lens_with_total(B, T, M, M)
            assert int(lens.sum()) == M and lens.min() >= 0 and lens.max() <= T, (B, T, M)
            assert (lens == 1).any() or M == 0, (B, T, M)
            assert (lens == T).any() or M < T + 1, (B, T, M)


@pytest.mark.parametrize("name", [c[0] for c in epc.BOUNDARY_CASES])
def test_boundary_case_path_lens_and_oracle(name):
    """The oracle of a dense boundary batch is evaluated on the rows the GPU test compares (eight probes and the
    sixteen shared sequences): the largest batch holds 25 k tokens, minutes of float64 on a CPU."""
    _, B, T, path = next(c for c in epc.BOUNDARY_CASES if c[0] == name)
    assert epc.path_of(B, T) == path
    ids, lens, probes, shared = epc.boundary_batch(name)
    assert ids.shape == (B, T) and lens.shape == (B,) and ids.min() >= 1 and ids.max() < epc.CFG["vocab_size"]
    if T == 1:
        assert (lens == 0).sum() == epc.N_EMPTY_T1 and set(lens.tolist()) == {0, 1}
    else:
        assert lens.min() >= 1 and lens.max() <= T and int(lens.sum()) > B * T // 4         # dense
    assert len(probes) == epc.N_PROBES == len(set(probes.tolist())) and (lens[probes] > 0).all()
    live = np.flatnonzero(lens > 0)
    assert probes[0] == live[0] and probes[-1] == live[-1]                      # the first and the last live row
    rows = probes if shared is None else np.concatenate([probes, shared])
    want = epc.oracle_rows(ids, lens, rows)
    assert np.isfinite(want).all() and np.abs(np.linalg.norm(want, axis=1) - 1).max() < 1e-12


@pytest.mark.parametrize("below,above,first_slot", epc.BOUNDARY_PAIRS)
def test_boundary_pairs_fall_on_different_sides(below, above, first_slot):
    lo = next(c for c in epc.BOUNDARY_CASES if c[0] == below)
    hi = next(c for c in epc.BOUNDARY_CASES if c[0] == above)
    assert lo[1] * lo[2] == first_slot - 1 and hi[1] * hi[2] == first_slot      # adjacent slot counts
    assert epc.path_of(lo[1], lo[2]) == lo[3] != hi[3] == epc.path_of(hi[1], hi[2])
    assert epc.PATHS.index(hi[3]) == epc.PATHS.index(lo[3]) + 1
    a, b = epc.boundary_batch(below), epc.boundary_batch(above)
    if first_slot == epc.SMALL_SLOTS + 1:
        assert a[3] is None and b[3] is None
        return
    # the shared sequences are the same rows, ids and lengths in both batches
    assert np.array_equal(a[3], b[3]) and len(a[3]) == epc.N_SHARED
    rows, Tmin = a[3], min(lo[2], hi[2])
    assert np.array_equal(a[1][rows], b[1][rows]) and (a[1][rows] >= 1).all() and a[1][rows].max() <= Tmin
    assert np.array_equal(a[0][rows, :Tmin], b[0][rows, :Tmin])


@pytest.mark.parametrize("vocab", [2000, 2005, 30522])
def test_the_heads_batches_are_on_the_paths_they_are_there_for(vocab):
    d, w, s = (epc.head_batch(k, vocab) for k in ("direct", "wide", "sparse"))
    for b in (d, w, s):
        assert b["ids"].min() >= 1 and b["ids"].max() < vocab and b["ids"].max() >= vocab - 50
        assert (b["seg"] <= b["lens"]).all() and (b["seg"] >= 0).all()
    assert epc.path_of(*d["ids"].shape) == "direct" and d["ids"].shape == (40, 64)
    assert {1, 31, 32, 33, 64} <= set(d["lens"].tolist()) and d["lens"].min() >= 1
    with_second = d["seg"][d["lens"] > d["seg"]]                    # pairs that do have a second segment
    assert set(epc.HEAD_SEGS) <= set(with_second.tolist())
    assert (d["seg"] == d["lens"]).any()                            # and one without
    assert w["ids"].shape == (384, 128) and epc.path_of(384, 128) == "dma_wide" and epc.path_of(64, 128) == "dma"
    assert len(w["probes"]) == 8 and w["probes"].min() >= 320 and w["probes"].max() == 383
    assert set(w["lens"][w["probes"]].tolist()) == {1, 31, 32, 33, 64, 65, 127, 128}
    assert w["lens"].min() >= 1 and w["lens"][0] == 128 and w["lens"][1] == 1
    assert s["ids"].shape == (64, 128) and epc.path_of(64, 128) == "dma"
    live = np.flatnonzero(s["lens"])
    assert live.tolist() == [0, 31, 63] and int(s["lens"].sum()) == 129
    assert np.array_equal(s["dense"][live], s["lens"][live]) and s["dense"].min() >= 1
    assert np.array_equal(s["dense_seg"][live], s["seg"][live]) and (s["dense_seg"] <= s["dense"]).all()
