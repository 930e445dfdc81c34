"""BM25 and hybrid search on one store, in one process: 1 M rows x 384, B in {1, 64}, k = 10,
fetch_k = 64.

Texts: seeded Zipf draws (p ~ 1 / rank over --vocab terms "t00000".."t49999", 8..40 terms per row;
the generator is zipf_texts below).  Vectors: seeded normal rows, L2-normalised, fp16.  Queries: the
first 3..8 terms of random rows, and random unit vectors.  Measured, each as the median over --steps
calls of a host clock around a call that ends in a device synchronisation (every shape warmed first):
  * bm25_gpu_ms       SparseIndex.search on a pre-encoded CSR batch (rf_sparse_search: scan + merge)
  * bm25_scipy_ms     the same scoring on the CPU: the impacts as a scipy.sparse CSR matrix
                      [rows, terms] times the batch's weight matrix, then the top k per query by
                      (score desc, row asc).  scipy sums in its own order, so its scores can differ
                      from the definition's in the last bit: `scipy_same_ids` counts the queries whose
                      id lists agree with the GPU's all the same.
  * dense_ms          CorpusStore.search("embedding"), limit k
  * bm25_store_ms     CorpusStore.search("sparse"), limit k (analysis and encoding of the query texts
                      included)
  * hybrid_ms         CorpusStore.hybrid_search: both arms at fetch_k, RRF, limit k
dense / bm25_store / hybrid rounds alternate.  Also recorded: the posting-list build on the host and
its upload (`index_build_s`, once), nnz, and the definition check of the first batch
(lexical.bm25_reference == GPU, bit for bit).

    python tools/bench_hybrid.py [--rows 1000000] [--steps 30] [--out FILE.json]
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

from rag_fin_amd import lexical  # noqa: E402

K = 10
FETCH_K = 64
DIM = 384
COS = {"metric_type": "COSINE"}
BM25 = {"metric_type": "BM25"}


def zipf_texts(n: int, vocab: int, seed: int) -> list[str]:
    """n rows of 8..40 terms drawn with p ~ 1 / rank from `vocab` terms."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    names = np.array([f"t{i:05d}" for i in range(vocab)])
    lens = rng.integers(8, 41, n)
    out, step = [], 1 << 16
    for s in range(0, n, step):
        ls = lens[s:s + step]
        draws = names[rng.choice(vocab, size=int(ls.sum()), p=p)]
        at = 0
        for ln in ls.tolist():
            out.append(" ".join(draws[at:at + ln]))
            at += ln
    return out


def timed(fn, steps: int, warm: int = 3) -> float:
    """Median wall time of fn() in ms; fn ends in a synchronisation."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def scipy_topk(matrix, postings, enc, k: int):
    """The scipy.sparse arm: scores = M @ W (W: terms x B weights), top k per query."""
    import scipy.sparse as sp
    q_off, q_term, q_weight = enc
    B = len(q_off) - 1
    cols = np.repeat(np.arange(B), np.diff(q_off))
    W = sp.csc_matrix((q_weight, (q_term, cols)), shape=(postings.n_terms, B), dtype=np.float32)
    S = (matrix @ W).tocsc()
    ids = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        rows, vals = S.indices[S.indptr[b]:S.indptr[b + 1]], S.data[S.indptr[b]:S.indptr[b + 1]]
        keep = vals > 0
        rows, vals = rows[keep], vals[keep]
        if rows.size > k:
            part = np.argpartition(-vals, k - 1)[:k]
            kth = vals[part].min()
            sel = vals >= kth                      # keeps every tie of the k-th score
            rows, vals = rows[sel], vals[sel]
        order = np.lexsort((rows, -vals.astype(np.float64)))[:k]
        ids[b, :order.size] = rows[order]
    return ids


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_bench.json"))
    args = ap.parse_args()
    from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
    from rag_fin_amd.store import CorpusStore, require_gpu
    dev = require_gpu("cuda:0")
    n = args.rows
    res = {"rows": n, "dim": DIM, "vocab": args.vocab, "k": K, "fetch_k": FETCH_K, "steps": args.steps,
           "device": torch.cuda.get_device_name(dev), "timing": "median wall ms of a call ending in a device synchronisation"}

    t0 = time.perf_counter()
    texts = zipf_texts(n, args.vocab, 11)
    res["text_gen_s"] = round(time.perf_counter() - t0, 2)
    store = CorpusStore("bench", dim=DIM, capacity=n, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    step = 1 << 18
    for s in range(0, n, step):
        m = min(step, n - s)
        x = torch.randn((m, DIM), generator=gen, device=dev, dtype=torch.float32)
        x = (x / x.norm(dim=1, keepdim=True)).half()
        store.add(list(range(s, s + m)), texts[s:s + m], x, ["p"] * m, ["c"] * m, ["s"] * m, [0.0] * m)
    store.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    t0 = time.perf_counter()
    postings, sparse = store._lexical.index()
    torch.cuda.synchronize()
    res["index_build_s"] = round(time.perf_counter() - t0, 2)
    res["nnz"], res["terms"], res["avgdl"] = postings.nnz, postings.n_terms, round(postings.avgdl, 2)

    import scipy.sparse as sp
    indptr = postings.post_off
    matrix = sp.csr_matrix(sp.csc_matrix((postings.post_imp, postings.post_row.astype(np.int32), indptr),
                                         shape=(n, postings.n_terms)))

    rng = np.random.default_rng(3)
    runs = {}
    for B in (1, 64):
        qtexts = [" ".join(texts[r].split()[:int(rng.integers(3, 9))]) for r in rng.integers(0, n, B).tolist()]
        qv = torch.randn((B, DIM), generator=gen, device=dev, dtype=torch.float32)
        qv = (qv / qv.norm(dim=1, keepdim=True)).half()
        enc = lexical.encode_queries(postings, qtexts)
        r = {"query_terms_mean": float(np.diff(enc[0]).mean())}

        def gpu():
            out = sparse.search(*enc, K)
            torch.cuda.synchronize()
            return out

        got = [t.cpu().numpy() for t in gpu()]
        ws, wi, we = lexical.bm25_reference(postings, *enc, K)
        r["equals_definition"] = bool(np.array_equal(got[1], wi) and got[0].tobytes() == ws.tobytes()
                                      and got[2].tobytes() == we.tobytes())
        r["bm25_gpu_ms"] = timed(gpu, args.steps)
        r["bm25_scipy_ms"] = timed(lambda: scipy_topk(matrix, postings, enc, K), max(3, args.steps // 10), warm=1)
        r["scipy_same_ids"] = int((scipy_topk(matrix, postings, enc, K) == got[1]).all(axis=1).sum())

        def dense():
            return store.search(qv, "embedding", COS, limit=K)

        def bm25_store():
            return store.search(qtexts, "sparse", BM25, limit=K)

        def hybrid():
            return store.hybrid_search([AnnSearchRequest(qv, "embedding", COS, limit=FETCH_K),
                                        AnnSearchRequest(qtexts, "sparse", BM25, limit=FETCH_K)], RRFRanker(), limit=K)

        rounds = {"dense_ms": [], "bm25_store_ms": [], "hybrid_ms": []}
        for _ in range(3):                               # alternate, so that drift hits all three alike
            for name, fn in (("dense_ms", dense), ("bm25_store_ms", bm25_store), ("hybrid_ms", hybrid)):
                rounds[name].append(timed(fn, max(5, args.steps // 3)))
        for name, v in rounds.items():
            r[name] = statistics.median(v)
            r[name + "_rounds"] = [round(x, 4) for x in v]
        h, d = hybrid(), dense()
        r["hybrid_lists_differing_from_dense"] = sum([x.row for x in a] != [x.row for x in b_] for a, b_ in zip(h, d))
        r["gpu_over_scipy"] = r["bm25_scipy_ms"] / r["bm25_gpu_ms"]
        r["hybrid_over_dense"] = r["hybrid_ms"] / r["dense_ms"]
        for key in ("bm25_gpu_ms", "bm25_scipy_ms", "gpu_over_scipy", "hybrid_over_dense", "dense_ms", "bm25_store_ms",
                    "hybrid_ms"):
            r[key] = round(r[key], 4)
        runs[f"B{B}"] = r
        print(json.dumps({f"B{B}": r}), flush=True)
    res["runs"] = runs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
