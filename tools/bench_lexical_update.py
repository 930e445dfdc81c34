"""Lexical index maintenance against the whole rebuild it replaces, on one store in one process: the
1 M-row corpus of tools/bench_hybrid.py (seeded Zipf texts, 8..40 terms per row), 64 periods.

Measured, with and without token positions attached (a PHRASE_MATCH filter attaches them; with them the
first answer asked for is a BM25 search under a PHRASE_MATCH filter, so both routes need them), for
  add      16 new rows
  upsert   16 rows: 8 restated, 8 new
  delete   every row of one period (1 / 64 of the corpus)
the host-clock time from the mutation to the first BM25 answer:
  * update_s    the mutation, then the search: CorpusStore replays the mutation through
                SparseIndex.appended / .compacted (median of --repeats different mutations, after one
                unrecorded mutation of each kind has warmed the kernels)
  * rebuild_s   the same mutation's time plus a search on the same rows with the retained state
                discarded: lexical.build_postings (and build_positions) over every text -- what the
                store did before it kept its index up to date.  Taken once per case (it is seconds).
  * bits_equal  the device post_off / post_row / post_imp (and pos_off / pos) of the two routes are equal
Then the HIP-event time of every new entry point inside SparseIndex.appended / .compacted on the full
index (median of --repeats calls after a warm-up), with the bytes each one moves by its definition
(gathers counted once per posting) and the GB/s that gives.

    python tools/bench_lexical_update.py [--rows 1000000] [--repeats 3] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_hybrid import zipf_texts  # noqa: E402
from rag_fin_amd import lexical  # noqa: E402

DIM = 384
PERIODS = 64
BM25 = {"metric_type": "BM25"}
ENTRY_POINTS = ("rf_sparse_append", "rf_sparse_compact_plan", "rf_sparse_compact_apply", "rf_sparse_impacts")


class TimedLib:
    """The library with HIP events around the maintenance entry points (current stream)."""

    def __init__(self, lib, torch):
        self._lib, self._torch, self.events = lib, torch, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ENTRY_POINTS:
            return fn

        def timed(*args):
            a, b = self._torch.cuda.Event(enable_timing=True), self._torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            self.events.append((name, a, b))
            return rc
        return timed

    def take(self):
        self._torch.cuda.synchronize()
        out = [(n, a.elapsed_time(b)) for n, a, b in self.events]
        self.events = []
        return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lexical_update_bench.json"))
    args = ap.parse_args()
    from rag_fin_amd.store import CorpusStore, require_gpu
    dev = require_gpu("cuda:0")
    n = args.rows
    res = {"rows": n, "dim": DIM, "vocab": args.vocab, "periods": PERIODS, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(dev),
           "timing": "host clock from the mutation to the first BM25 answer (s); kernels: HIP events (ms)"}
    spare = 16 * 6 * (args.repeats + 2)
    texts = zipf_texts(n + spare, args.vocab, 11)
    store = CorpusStore("bench", dim=DIM, capacity=n + spare, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)

    def vectors(m):
        x = torch.randn((m, DIM), generator=gen, device=dev, dtype=torch.float32)
        return (x / x.norm(dim=1, keepdim=True)).half()

    def batch(keys, idx):
        m = len(keys)
        return [keys, [texts[i] for i in idx], vectors(m), [f"P{i % PERIODS:02d}" for i in idx], ["c"] * m, ["s"] * m, [0.0] * m]

    step = 1 << 18
    for s in range(0, n, step):
        idx = list(range(s, min(n, s + step)))
        store.insert(batch(idx, idx))
    store.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    queries = [" ".join(texts[r].split()[:5]) for r in (3, 1000, 70000 % n)]
    phrase = 'PHRASE_MATCH(text, "t00000 t00001")'
    next_row = [n]
    next_period = [0]

    def first_answer(expr):
        store.search(queries, "sparse", BM25, limit=10, expr=expr)   # (ends in a download: synchronised)

    def mutate(kind):
        if kind == "delete":
            p = next_period[0]
            next_period[0] += 1
            return lambda: store.delete(f'period == "P{p:02d}"')
        idx = list(range(next_row[0], next_row[0] + 16))
        next_row[0] += 16
        keys = list(idx)
        if kind == "upsert":
            keys[:8] = store.columns["id"][1000:1008]
        data = batch(keys, idx)
        return (lambda: store.insert(data)) if kind == "add" else (lambda: store.upsert(data))

    def arrays():
        sp = store._lexical.built[1]
        return [sp.post_off, sp.post_row, sp.post_imp] + list(sp.positions or ())

    t0 = time.perf_counter()
    first_answer(None)
    res["index_build_s"] = round(time.perf_counter() - t0, 2)
    postings = store._lexical.built[0]
    res["nnz"], res["terms"], res["avgdl"] = postings.nnz, postings.n_terms, round(postings.avgdl, 2)
    cases = {}
    for with_pos in (False, True):
        expr = phrase if with_pos else None
        if with_pos:
            t0 = time.perf_counter()
            first_answer(expr)
            res["positions_build_s"] = round(time.perf_counter() - t0, 2)
            res["positions"] = int(store._lexical.built[1].positions[1].numel())
        for kind in ("add", "upsert", "delete"):                       # warm-up: kernels loaded, allocator primed
            mutate(kind)()
            first_answer(expr)
        for kind in ("add", "upsert", "delete"):
            upd, mut = [], []
            for _ in range(args.repeats):
                fn = mutate(kind)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                first_answer(expr)
                upd.append(time.perf_counter() - t0)
                mut.append(t1 - t0)
                assert store._lexical.kept is not None and store._lexical.built[1].supports_update
            live = arrays()
            assert with_pos == (store._lexical.built[1].positions is not None)
            store._lexical.built = None
            store._lexical.forget()
            t0 = time.perf_counter()
            first_answer(expr)
            rebuild_search = time.perf_counter() - t0
            whole = arrays()
            equal = len(live) == len(whole) and all(a.shape == b.shape and bool(torch.equal(a, b)) for a, b in zip(live, whole))
            c = {"update_s": round(statistics.median(upd), 4), "update_s_all": [round(x, 4) for x in upd],
                 "mutation_s": round(statistics.median(mut), 4), "rebuild_search_s": round(rebuild_search, 2),
                 "rebuild_s": round(statistics.median(mut) + rebuild_search, 2), "bits_equal": equal,
                 "rows_after": store.num_entities}
            c["rebuild_over_update"] = round(c["rebuild_s"] / c["update_s"], 1)
            cases[f"{kind}{'_positions' if with_pos else ''}"] = c
            print(json.dumps({kind: c, "positions": with_pos}), flush=True)
    res["cases"] = cases

    # ---- the entry points on the full index, by HIP events -----------------------------------------------
    from rag_fin_amd import index as index_mod
    postings, sp = store._lexical.index()
    lib = TimedLib(sp.lib, torch)
    index_mod._lib.load_library = lambda: lib
    sp.lib = lib
    nnz, n_pos, n_rows = sp.nnz, int(sp.positions[1].numel()), sp.n_rows
    delta = lexical.count_terms(texts[next_row[0]:next_row[0] + 16])
    vocab, map_old, map_delta = lexical.merge_vocab(postings.vocab, postings.term_id, delta.vocab)
    post_off = lexical.merged_offsets(len(vocab), postings.post_off, map_old, delta.post_off, map_delta)
    dl = np.concatenate([postings.dl, delta.dl])
    keep = np.arange(n_rows) % PERIODS != PERIODS - 1
    row_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    times = {name: [] for name in ENTRY_POINTS}
    kept_nnz = kept_pos = 0
    for it in range(args.repeats + 1):
        sp.appended(delta, map_old, map_delta, post_off, dl, postings.k1, postings.b)
        new, _, _ = sp.compacted(row_map, postings.dl[keep], postings.k1, postings.b)
        kept_nnz, kept_pos = new.nnz, int(new.positions[1].numel())
        for i, (name, ms) in enumerate(lib.take()):
            if it and not (name == "rf_sparse_impacts" and i > 2):   # (the impacts of the append; the compaction's are fewer)
                times[name].append(ms)
    moved = {   # bytes by definition, positions attached: (row, tf) 8 B, pos_off 8 B, a position 4 B, dst 8 B, imp 4 B
        "rf_sparse_append": (nnz + delta.nnz) * (8 + 8 + 8 + 8) + (n_pos + int(delta.pos.size)) * 8,
        "rf_sparse_compact_plan": 2 * nnz * (4 + 4 + 16) + nnz * 16,
        "rf_sparse_compact_apply": nnz * (4 + 4 + 16 + 4 + 16) + kept_nnz * (8 + 8) + kept_pos * 8,
        "rf_sparse_impacts": (nnz + delta.nnz) * (4 + 4 + 4 + 4),
    }
    res["kernels"] = {name: {"ms": round(statistics.median(times[name]), 4), "bytes": int(moved[name]),
                             "gb_per_s": round(moved[name] / statistics.median(times[name]) / 1e6, 1)} for name in ENTRY_POINTS}
    res["kernels_on"] = {"nnz": nnz, "positions": n_pos, "rows": n_rows, "kept_nnz": kept_nnz}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
