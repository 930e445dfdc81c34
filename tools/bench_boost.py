"""Boosted search (CorpusStore.search(ranker=...)) against what it replaces, at 1 M x 384, k = 10, in one
process.

Store: 1 M synth rows; `period` dealt in 8 contiguous runs (a corpus ingested quarter by quarter),
`chunk_type` row % 4, `statement_type` (row // 4) % 2, `primary_value` row % 1000.  Cases: B in
{1, 8, 64} x m in {1, 2, 3} boosts (the latest period x 1.5, one chunk type x 1.2, one statement type
x 0.8) x with / without a base expr (`primary_value < 500`).  Per case, wall-clock milliseconds with a
device synchronisation at the end of every call (both routes download their hits), warm-up first:
  boosted    one search(ranker=...) call
  plain      one search(expr=base) call of the same B and k -- the unit the boosted call is counted in
  emulation  the client-side route: one search(expr=base AND class) per (query, non-empty class) at
             limit k, the hits re-weighted and merged in numpy
and the split of one boosted call between its stages (filter builds, class masks + class filter
buffers, sweeps, merge + download; each stage synchronised, so the parts add up to more than the call).

    python tools/bench_boost.py [--rows 1000000] [--steps 10] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import search as osearch  # noqa: E402
from rag_fin_amd.ranker import BoostRanker, class_weights  # noqa: E402
from rag_fin_amd.store import CorpusStore  # noqa: E402

COS = {"metric_type": "COSINE"}
BS = [1, 8, 64]
BOOSTS = [('period == "P7"', 1.5), ('chunk_type == "c0"', 1.2), ('statement_type == "s1"', 0.8)]
BASE = "primary_value < 500"


def wall(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def class_exprs(boosts, base):
    """One expression per class c: base AND, for each boost, its filter or the negation of it."""
    out = []
    for c in range(1 << len(boosts)):
        terms = [f"({f})" if (c >> i) & 1 else f"not ({f})" for i, (f, _) in enumerate(boosts)]
        out.append(" and ".join(([f"({base})"] if base else []) + terms))
    return out


def emulate(st, q, k, boosts, base, live):
    """The route without the feature: a filtered search per (query, non-empty class), merged on the host."""
    W = class_weights([w for _, w in boosts])
    exprs = class_exprs(boosts, base)
    out = []
    for b in range(q.shape[0]):
        cand = []
        for c in live:
            for h in st.search(q[b:b + 1], "embedding", COS, k, expr=exprs[c])[0]:
                cand.append((-(W[c] * h.score), -h.score, h.row))
        out.append([r for _, _, r in sorted(cand)[:k]])
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boost_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d, k = a.rows, a.dim, a.topk
    r = np.arange(n)
    st = CorpusStore("boost_bench", dim=d, capacity=n, device=dev)
    chunk = 1 << 18
    for lo in range(0, n, chunk):   # (chunked: the fp16 rows of a chunk go to the device and are dropped)
        rr = r[lo:lo + chunk]
        rows = osearch.synth_unit_rows(rr.size, d, 11 + lo)
        st.add([f"k{i}" for i in rr], ["t"] * rr.size, torch.from_numpy(rows).to(dev),
               [f"P{i}" for i in rr * 8 // n], [f"c{i}" for i in rr % 4], [f"s{i}" for i in (rr // 4) % 2],
               (rr % 1000).astype(np.float64).tolist())
    qall = torch.from_numpy(osearch.synth_unit_rows(max(BS), d, 6)).to(dev)
    res = {"rows": n, "dim": d, "topk": k, "steps": a.steps, "cases": []}
    for base in (None, BASE):
        for B in BS:
            q = qall[:B].contiguous()
            plain_ms = wall(lambda: st.search(q, "embedding", COS, k, expr=base), a.steps, a.warmup)
            for m in (1, 2, 3):
                boosts = BOOSTS[:m]
                rankers = [BoostRanker(f, w) for f, w in boosts]

                def boosted():
                    return st.search(q, "embedding", COS, k, expr=base, ranker=rankers)

                boosted_ms = wall(boosted, a.steps, a.warmup)
                split = {}
                for _ in range(a.steps):
                    st._search_boosted(q, "embedding", COS, k, base, None, None, None, None, None, rankers, timing=split)
                sweeps, classes = split.pop("sweeps"), split.pop("classes")
                split = {key: v / a.steps for key, v in split.items()}
                live = [c for c, e in enumerate(class_exprs(boosts, base)) if st.filter_rows(e).size]
                emu_steps = max(1, min(a.steps, 256 // (B * len(live))))
                emulation_ms = wall(lambda: emulate(st, q, k, boosts, base, live), emu_steps, 1)
                same = [[h.row for h in hits] for hits in boosted()] == emulate(st, q, k, boosts, base, live)
                row = {"B": B, "m": m, "base_expr": base, "classes": classes, "sweeps": sweeps,
                       "boosted_ms": boosted_ms, "plain_ms": plain_ms, "emulation_ms": emulation_ms,
                       "boosted_over_plain": boosted_ms / plain_ms, "emulation_over_boosted": emulation_ms / boosted_ms,
                       "split_ms": split, "emulation_steps": emu_steps, "ids_equal_emulation": bool(same)}
                res["cases"].append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
