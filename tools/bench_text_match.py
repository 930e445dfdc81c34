"""Keyword filters (TEXT_MATCH / PHRASE_MATCH in expr) on the corpus of tools/bench_hybrid.py, in one
process: 1 M rows x 384, Zipf texts over 50 000 terms.

Three leaves:
  match1   TEXT_MATCH(text, 't00020')                                          one term
  match3   TEXT_MATCH(text, 't00005 t00010 t00020', minimum_should_match=2)    three terms, two must match
  phrase3  PHRASE_MATCH(text, 't00000 t00001 t00002')                          the three commonest terms, adjacent
Measured for each, as the median over --steps calls of a host clock around a call that ends in a device
synchronisation (every shape warmed first):
  * filter_ms        CorpusStore.build_filter(expr): parse, compile, rf_text_match, rf_filter_eval_bitmaps
  * text_match_ms    SparseIndex.text_match of the compiled leaf alone (the two launches of rf_text_match)
  * host_route_ms    the only route before this: the row set in numpy over the Postings (lexical.
                     text_match_reference; the positions it reads for the phrase are NOT counted), written
                     out as `id in [...]`, then build_filter of that expression
  * period_ms        build_filter of `period == "..."` for the period value whose share of the rows is the
                     closest to the leaf's (period values cover 1/2, 1/4, ... of the rows)
  * dense_ms         CorpusStore.search("embedding", limit 10) under the keyword filter, under the period
                     filter and without a filter, B in {1, 64}; the three alternate
Also recorded: the one-off build and upload of the token positions the first PHRASE_MATCH needs
(`positions_build_s`), the rows each filter passes, and `equals_definition`: every bitmap compared with
lexical.text_match_reference, bit for bit.

    python tools/bench_text_match.py [--rows 1000000] [--steps 20] [--out FILE.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_hybrid import DIM, K, timed, zipf_texts  # noqa: E402
from rag_fin_amd import filter_expr, lexical  # noqa: E402

COS = {"metric_type": "COSINE"}
LEAVES = {
    "match1": "TEXT_MATCH(text, 't00020')",
    "match3": "TEXT_MATCH(text, 't00005 t00010 t00020', minimum_should_match=2)",
    "phrase3": "PHRASE_MATCH(text, 't00000 t00001 t00002')",
}
N_PERIODS = 14   # value j holds about 2^-(j + 1) of the rows


def period_column(n: int, seed: int) -> list[str]:
    rng = np.random.default_rng(seed)
    share = 0.5 ** np.arange(1, N_PERIODS + 1)
    share[-1] += 1.0 - share.sum()
    return [f"P{j:02d}" for j in rng.choice(N_PERIODS, size=n, p=share).tolist()]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_match_bench.json"))
    args = ap.parse_args()
    from rag_fin_amd.store import CorpusStore, filter_mask_bits, require_gpu
    dev = require_gpu("cuda:0")
    n = args.rows
    res = {"rows": n, "dim": DIM, "vocab": args.vocab, "k": K, "steps": args.steps,
           "device": torch.cuda.get_device_name(dev),
           "timing": "median wall ms of a call ending in a device synchronisation", "leaves": LEAVES}

    texts = zipf_texts(n, args.vocab, 11)
    periods = period_column(n, 13)
    store = CorpusStore("bench", dim=DIM, capacity=n, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    step = 1 << 18
    for s in range(0, n, step):
        m = min(step, n - s)
        x = torch.randn((m, DIM), generator=gen, device=dev, dtype=torch.float32)
        x = (x / x.norm(dim=1, keepdim=True)).half()
        store.add(list(range(s, s + m)), texts[s:s + m], x, periods[s:s + m], ["c"] * m, ["s"] * m, [0.0] * m)
    store.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    t0 = time.perf_counter()
    postings, sparse = store._lexical.index()
    torch.cuda.synchronize()
    res["postings_build_s"] = round(time.perf_counter() - t0, 2)
    res["nnz"] = postings.nnz
    t0 = time.perf_counter()
    store._lexical.text_index(filter_expr.text_leaves(filter_expr.parse(LEAVES["phrase3"])))   # builds and attaches the positions
    torch.cuda.synchronize()
    res["positions_build_s"] = round(time.perf_counter() - t0, 2)
    positions = lexical.build_positions(postings, texts)
    res["n_positions"] = int(positions[1].size)
    share = np.bincount([int(p[1:]) for p in periods], minlength=N_PERIODS) / n

    def sync(fn):
        def run():
            out = fn()
            torch.cuda.synchronize()
            return out
        return run

    queries = {}
    for B in (1, 64):
        qv = torch.randn((B, DIM), generator=gen, device=dev, dtype=torch.float32)
        queries[B] = (qv / qv.norm(dim=1, keepdim=True)).half()

    ok = True
    runs = {}
    for name, expr in LEAVES.items():
        prog = filter_expr.compile_expr(filter_expr.parse(expr), {}, {}, postings.term_id)
        want = lexical.text_match_reference(postings, positions, prog.text_leaves, n)
        got = sync(lambda: sparse.text_match(prog.text_leaves))().cpu().numpy().view(np.uint32)
        same = bool(np.array_equal(got[:, :want.shape[1]], want) and not got[:, want.shape[1]:].any())
        mask = filter_mask_bits(store.build_filter(expr), n)
        same = same and bool(np.array_equal(np.packbits(np.pad(mask, (0, -n % 32)), bitorder="little").view(np.uint32), want[0]))
        ok = ok and same
        passing = int(mask.sum())
        j = int(np.argmin(np.abs(share - passing / n)))
        period_expr = f'period == "P{j:02d}"'
        r = {"equals_definition": same, "rows_passing": passing, "period_expr": period_expr,
             "period_rows_passing": int(round(share[j] * n))}

        def host_route():
            bits = lexical.text_match_reference(postings, positions, prog.text_leaves, n)[0]
            rows = np.flatnonzero(np.unpackbits(bits.view(np.uint8), bitorder="little")[:n])
            out = store.build_filter("id in [" + ", ".join(map(str, rows.tolist())) + "]")
            torch.cuda.synchronize()
            return out

        r["filter_ms"] = timed(sync(lambda: store.build_filter(expr)), args.steps)
        r["text_match_ms"] = timed(sync(lambda: sparse.text_match(prog.text_leaves)), args.steps)
        r["period_ms"] = timed(sync(lambda: store.build_filter(period_expr)), args.steps)
        r["host_route_ms"] = timed(host_route, 3, warm=1)
        r["host_route_over_filter"] = r["host_route_ms"] / r["filter_ms"]
        r["filter_over_period"] = r["filter_ms"] / r["period_ms"]
        for B, qv in queries.items():
            arms = {"keyword": lambda: store.search(qv, "embedding", COS, limit=K, expr=expr),
                    "period": lambda: store.search(qv, "embedding", COS, limit=K, expr=period_expr),
                    "plain": lambda: store.search(qv, "embedding", COS, limit=K)}
            rounds = {a: [] for a in arms}
            for _ in range(3):                               # alternate, so that drift hits all three alike
                for a, fn in arms.items():
                    rounds[a].append(timed(fn, max(5, args.steps // 2)))
            for a, v in rounds.items():
                r[f"dense_{a}_B{B}_ms"] = round(statistics.median(v), 4)
        for key in ("filter_ms", "text_match_ms", "period_ms", "host_route_ms", "host_route_over_filter", "filter_over_period"):
            r[key] = round(r[key], 4)
        runs[name] = r
        print(json.dumps({name: r}), flush=True)
    res["equals_definition"] = ok
    res["runs"] = runs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
