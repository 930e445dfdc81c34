"""Per-query filters against the routes that exist without them, at 1 M x 384, k = 10, B = 64, in one
process.

Filters: G in {1, 4, 16, 64} `period`-style sets that partition the rows, the 64 queries dealt
evenly over them, in two layouts -- contiguous (set g = rows [g n / G, (g + 1) n / G): a corpus
inserted period by period) and interleaved (row r in set r mod G).  Three routes on the same index,
alternated round by round and timed with device events (warm-up first; the median of the rounds):
  multi       rf_search_multi_filtered: one call, one sweep over the union
  per_filter  one rf_search_filtered per distinct filter with that filter's queries (the best route
              without per-query filters)
  per_query   one rf_search_filtered per query (what a server does that cannot coalesce them)
Also: a plain unfiltered 64-query step, the share of queries the multi call flags, and the time of
rf_multi_filter_build.  The gate of the change: at G = 4 interleaved, multi < 0.5 x per_filter.

    python tools/bench_multi_filter.py [--rows 1000000] [--rounds 7] [--steps 10] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import search as osearch  # noqa: E402
from rag_fin_amd import _lib  # noqa: E402
from rag_fin_amd.index import GpuIndex, MultiFilter  # noqa: E402
from tools.bench_filtered import filter_from_mask, timed  # noqa: E402

GS = [1, 4, 16, 64]
LAYOUTS = ["contiguous", "interleaved"]


def masks_of(layout, G, n):
    r = np.arange(n)
    if layout == "contiguous":
        return [(r * G // n) == g for g in range(G)]
    return [r % G == g for g in range(G)]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_filter_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d, B, k = a.rows, a.dim, a.batch, a.topk
    lib = _lib.load_library()
    ix = GpuIndex(d, n, dev)
    ix.add(torch.from_numpy(osearch.synth_unit_rows(n, d, 11)).to(dev))
    q = torch.from_numpy(osearch.synth_unit_rows(B, d, 6)).to(dev)
    out = ix._outputs(B, k, True)
    one = ix._outputs(1, k, True)
    plain_ms = timed(lambda: ix.search_raw(q, k, want_exact=True, out=out), a.rounds * a.steps, a.warmup)
    res = {"rows": n, "dim": d, "batch": B, "topk": k, "rounds": a.rounds, "steps_per_round": a.steps,
           "plain_unfiltered_ms": plain_ms, "configs": []}
    print(f"plain unfiltered step: {plain_ms:.4f} ms", flush=True)
    for layout in LAYOUTS:
        for G in GS:
            if G == 1 and layout == "interleaved":
                continue   # one filter that passes every row: the same as contiguous
            masks = masks_of(layout, G, n)
            qf = [b % G for b in range(B)]
            filters = [filter_from_mask(m, dev) for m in masks]
            mf = MultiFilter(filters, qf, n, dev)
            torch.cuda.synchronize()
            ptrs = (c_void_p * G)(*[c_void_p(f.data_ptr()) for f in filters])
            build_ms = timed(lambda: _lib.check(lib.rf_multi_filter_build(ptrs, G, n, c_void_p(mf.buf.data_ptr()),
                                                                          _lib.current_stream_ptr())),
                             a.steps, a.warmup)
            flags = ix.search_raw(q, k, want_exact=True, filt=mf)[3]
            flagged = int((flags != 0).sum())
            groups = [(q[torch.tensor([b for b in range(B) if qf[b] == g], device=dev)].contiguous(), filters[g])
                      for g in range(G)]
            outs = [ix._outputs(qs.shape[0], k, True) for qs, _ in groups]
            singles = [(q[b:b + 1].contiguous(), filters[qf[b]]) for b in range(B)]

            def multi():
                ix.search_raw(q, k, want_exact=True, out=out, filt=mf)

            def per_filter():
                for (qs, f), o in zip(groups, outs):
                    ix.search_raw(qs, k, want_exact=True, out=o, filt=f)

            def per_query():
                for qs, f in singles:
                    ix.search_raw(qs, k, want_exact=True, out=one, filt=f)

            routes = {"multi": multi, "per_filter": per_filter, "per_query": per_query}
            for fn in routes.values():
                timed(fn, a.warmup, 0)
            samples = {name: [] for name in routes}
            for _ in range(a.rounds):   # the routes alternate
                for name, fn in routes.items():
                    samples[name].append(timed(fn, a.steps, 0))
            row = {"layout": layout, "G": G, "build_ms": build_ms, "flagged_queries": flagged,
                   "flagged_share": flagged / B,
                   **{name + "_ms": statistics.median(v) for name, v in samples.items()},
                   **{name + "_ms_min_max": [min(v), max(v)] for name, v in samples.items()}}
            row["per_filter_over_multi"] = row["per_filter_ms"] / row["multi_ms"]
            row["per_query_over_multi"] = row["per_query_ms"] / row["multi_ms"]
            res["configs"].append(row)
            print(json.dumps(row), flush=True)
            del mf, filters, groups, singles
    g4 = next(r for r in res["configs"] if r["layout"] == "interleaved" and r["G"] == 4)
    res["gate"] = {"what": "G = 4, interleaved, B = 64: multi_ms < 0.5 * per_filter_ms", "multi_ms": g4["multi_ms"],
                   "per_filter_ms": g4["per_filter_ms"], "holds": bool(g4["multi_ms"] < 0.5 * g4["per_filter_ms"])}
    print(json.dumps(res["gate"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if res["gate"]["holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
