"""The first build of the lexical index: the host route (lexical.build_postings + build_positions, numpy)
against the device route (lexical.analyze_native + SparseIndex.from_tokens), in one process,
on the corpus of tools/bench_lexical_update.py (seeded Zipf texts, 8..40 terms per row) at 10 k, 100 k
and 1 M rows.

Per size, with and without token positions, the host-clock time from the texts to the first BM25 answer
(the answer ends in a download, so the clock stops on finished work):
  * host_s     build_postings (+ build_positions), the upload (SparseIndex), the search; median and
               every value of --repeats runs
  * device_s   analyze_native, from_tokens (with positions: count_tokens with positions), the search;
               median and every value of --repeats runs after one unrecorded warm-up run
  * stages     the device route taken apart, each stage ended by a synchronisation of its own (so their
               sum is a little above device_s): prepass (Python: join, ASCII test, UTF-8), native
               (rf_analyze and the copy-out), vocab (dictionary -> Python list), upload, plan, readback,
               apply, impacts (idf on the host + rf_sparse_impacts + the guard), term_id (the dict)
  * bits_equal vocab, post_off, post_row, post_tf, post_imp bits, dl, pos_off, pos of the two routes

    python tools/bench_lexical_build.py [--rows 10000,100000,1000000] [--repeats 3] [--out FILE.json]
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

K1, B = lexical.DEFAULT_K1, lexical.DEFAULT_B


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000,100000,1000000")
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lexical_build_bench.json"))
    args = ap.parse_args()
    from rag_fin_amd.index import SparseIndex, require_gpu
    dev = require_gpu("cuda:0")
    sizes = [int(x) for x in args.rows.split(",")]
    all_texts = zipf_texts(max(sizes), args.vocab, 11)
    res = {"vocab": args.vocab, "repeats": args.repeats, "device": torch.cuda.get_device_name(dev),
           "timing": "host clock from the texts to the first BM25 answer (s)", "sizes": {}}

    def answer(postings, sp, queries):
        q = lexical.encode_queries(postings, queries)
        scores, rows, _ = sp.search(*q, 10, want_exact=False)
        return scores.cpu().numpy(), rows.cpu().numpy()

    def host_route(texts, queries, positions):
        t0 = time.perf_counter()
        p = lexical.build_postings(texts, K1, B)
        sp = SparseIndex(p, dev)
        pos = None
        if positions:
            pos = lexical.build_positions(p, texts)
            sp.attach_positions(*pos)
        ans = answer(p, sp, queries)
        return time.perf_counter() - t0, p, pos, ans

    def device_route(texts, queries, positions, timing=None):
        t0 = time.perf_counter()
        vocab, tok, dl = lexical.analyze_native(texts, timing=timing)
        sp = SparseIndex.from_tokens(len(vocab), tok, dl, K1, B, dev, positions, timing)
        t1 = time.perf_counter()
        p = lexical.LivePostings(vocab, None, sp.host_post_off, dl, K1, B, sp.host_array)
        t2 = time.perf_counter()
        ans = answer(p, sp, queries)
        if timing is not None:
            for k, v in {"term_id_s": t2 - t1, "search_s": time.perf_counter() - t2}.items():
                timing[k] = timing.get(k, 0.0) + v   # (summed over the repeats, like from_tokens' stages)
        return time.perf_counter() - t0, p, sp, ans

    for n in sizes:
        texts = all_texts[:n]
        queries = [" ".join(texts[r].split()[:5]) for r in (3, 1000 % n, 70000 % n)]
        out = {}
        for positions in (False, True):
            reps = args.repeats
            host = [host_route(texts, queries, positions) for _ in range(reps)]
            _, hp, hpos, hans = host[-1]
            device_route(texts, queries, positions)                                   # warm-up
            runs = [device_route(texts, queries, positions) for _ in range(args.repeats)]
            stages: dict = {}
            staged = [device_route(texts, queries, positions, stages) for _ in range(args.repeats)]
            _, dp, sp, dans = runs[-1]
            equal = (dp.vocab == hp.vocab and np.array_equal(dp.post_off, hp.post_off) and np.array_equal(dp.dl, hp.dl)
                     and np.array_equal(dp.post_row, hp.post_row) and np.array_equal(dp.post_tf, hp.post_tf)
                     and np.array_equal(dp.post_imp.view(np.uint32), hp.post_imp.view(np.uint32))
                     and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(hans, dans)))
            if positions:
                equal = equal and np.array_equal(sp.positions[0].cpu().numpy(), hpos[0]) and \
                    np.array_equal(sp.positions[1].cpu().numpy().view(np.uint32), hpos[1])
            hs, ds = [h[0] for h in host], [r[0] for r in runs]
            c = {"host_s": round(statistics.median(hs), 4), "host_s_all": [round(x, 4) for x in hs],
                 "device_s": round(statistics.median(ds), 4), "device_s_all": [round(x, 4) for x in ds],
                 "staged_s_all": [round(s[0], 4) for s in staged],
                 "stages_s": {k: round(v / args.repeats, 5) for k, v in sorted(stages.items())},
                 "bits_equal": bool(equal), "nnz": hp.nnz, "terms": hp.n_terms, "tokens": int(hp.dl.sum())}
            c["host_over_device"] = round(c["host_s"] / c["device_s"], 2)
            out["positions" if positions else "postings"] = c
            print(json.dumps({"rows": n, "positions": positions, **c}), flush=True)
            del host, runs, staged, hp, hpos, dp, sp
        res["sizes"][str(n)] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
