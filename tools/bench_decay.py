"""Decayed search (CorpusStore.search(ranker=DecayRanker(...))) against what stands beside it, at 1 M x 384,
k = 10, B = 1 and 64, in one process.

Store: 1 M synth rows with an INT64 `fiscal_year` field (row % 23 years) and `primary_value` row % 1000; the
decay is a gauss over fiscal_year, the expr `primary_value < 500` (half of the rows, every block).  Per B, wall
-clock milliseconds with a device synchronisation at the end of every call, warm-up first:
  weights    rf_decay_weights alone over the int64 column (device time per call, by events around a run of calls)
  decayed    GpuIndex.search(filt=, weights=): the weighted sweep with the filter of the expr
  filtered   GpuIndex.search(filt=): the existing filtered sweep of the same filter -- the unit the decayed
             step is counted in
  decayed_nofilter / plain    the same pair without a filter (the plain side is rf_search: the shadow-first chain at 1 M rows)
  store_decayed / store_filtered    the whole store calls (expression build, weights, sweep, download, hits)
  emulation  what a user has without the feature: every score to the host (rf_debug_scores), the weights and the
             top k in numpy

    python tools/bench_decay.py [--rows 1000000] [--steps 20] [--out FILE.json]
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
from rag_fin_amd.index import decay_weights  # noqa: E402
from rag_fin_amd.ranker import DecayRanker, decay_weights_reference  # noqa: E402
from rag_fin_amd.schema import DataType, FieldSchema  # noqa: E402
from rag_fin_amd.store import CorpusStore  # noqa: E402

COS = {"metric_type": "COSINE"}
BS = [1, 64]
EXPR = "primary_value < 500"


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


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decay_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d, k = a.rows, a.dim, a.topk
    r = np.arange(n)
    st = CorpusStore("decay_bench", dim=d, capacity=n, device=dev, fields=[FieldSchema("fiscal_year", DataType.INT64)])
    chunk = 1 << 18
    for lo in range(0, n, chunk):   # (chunked: the fp16 rows of a chunk go to the device and are dropped)
        rr = r[lo:lo + chunk]
        rows = osearch.synth_unit_rows(rr.size, d, 11 + lo)
        st.add([f"k{i}" for i in rr], ["t"] * rr.size, torch.from_numpy(rows).to(dev), ["P"] * rr.size, ["c"] * rr.size,
               ["s"] * rr.size, (rr % 1000).astype(np.float64).tolist(), extra={"fiscal_year": (2002 + rr % 23).tolist()})
    ranker = DecayRanker("fiscal_year", "gauss", 2024, 3, offset=1)
    ix = st.index
    filt = st.build_filter(EXPR)
    column = st._decay_column(st._check_decay_field("fiscal_year"))
    weights = decay_weights(column, ranker)
    w64_host = decay_weights_reference(np.asarray(st.columns["fiscal_year"], dtype=np.int64), ranker)
    assert np.array_equal(weights[1].cpu().numpy().view(np.int64), w64_host.view(np.int64))
    passing = np.asarray(st.columns["primary_value"]) < 500

    # rf_decay_weights alone: device time per call
    calls = 50
    for _ in range(3):
        decay_weights(column, ranker)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        decay_weights(column, ranker)
    e1.record()
    torch.cuda.synchronize()
    weights_ms = e0.elapsed_time(e1) / calls
    res = {"rows": n, "dim": d, "topk": k, "steps": a.steps, "expr": EXPR, "passing_rows": int(passing.sum()),
           "ranker": ranker.to_params(), "weights_ms": weights_ms,
           "weights_gb_per_s": n * 20 / weights_ms / 1e6, "cases": []}
    print(json.dumps({"weights_ms": weights_ms}), flush=True)

    qall = torch.from_numpy(osearch.synth_unit_rows(max(BS), d, 6)).to(dev)
    for B in BS:
        q = qall[:B].contiguous()

        def emulate():
            s = ix.debug_scores(q).cpu().numpy().astype(np.float64)   # every score to the host
            dec = np.where(passing, w64_host * s, -np.inf)
            top = np.argpartition(-dec, k, axis=1)[:, :k]
            return np.take_along_axis(top, np.argsort(-np.take_along_axis(dec, top, 1), axis=1, kind="stable"), 1)

        row = {
            "B": B,
            "decayed_ms": wall(lambda: ix.search(q, k, filt=filt, weights=weights), a.steps, a.warmup),
            "filtered_ms": wall(lambda: ix.search(q, k, filt=filt), a.steps, a.warmup),
            "decayed_nofilter_ms": wall(lambda: ix.search(q, k, weights=weights), a.steps, a.warmup),
            "plain_ms": wall(lambda: ix.search(q, k), a.steps, a.warmup),
            "store_decayed_ms": wall(lambda: st.search(q, "embedding", COS, k, expr=EXPR, ranker=ranker), a.steps, a.warmup),
            "store_filtered_ms": wall(lambda: st.search(q, "embedding", COS, k, expr=EXPR), a.steps, a.warmup),
            "emulation_ms": wall(emulate, max(1, a.steps // 10), 1),
        }
        split = {}
        for _ in range(a.steps):
            st._search_decayed(q, "embedding", COS, k, EXPR, None, None, None, None, None, ranker, timing=split)
        row["store_split_ms"] = {key: v / a.steps for key, v in split.items()}
        row["decayed_over_filtered"] = row["decayed_ms"] / row["filtered_ms"]
        row["decayed_nofilter_over_plain"] = row["decayed_nofilter_ms"] / row["plain_ms"]
        row["store_decayed_over_store_filtered"] = row["store_decayed_ms"] / row["store_filtered_ms"]
        row["emulation_over_store_decayed"] = row["emulation_ms"] / row["store_decayed_ms"]
        # (the emulation ranks MFMA fp32 scores: the same rows wherever no two decayed scores lie within eps)
        got = [[h.row for h in hits] for hits in st.search(q, "embedding", COS, k, expr=EXPR, ranker=ranker)]
        row["rows_equal_emulation"] = sum(a_ == b_ for a_, b_ in zip(got, emulate().tolist())) / B
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
