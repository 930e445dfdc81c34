"""Metric aggregations (CorpusStore.facets(..., metrics=), query(expr, ["sum(f)"])) beside the same calls without
metrics and against the route a user had before -- query(expr, output_fields=[field, metric]) + math.fsum per bucket
on the host -- at 1 M rows in one process.

Store: 1 M synth rows; `bank` (VARCHAR) 16 values, `tags` (ARRAY VARCHAR) 4 M elements over 64 tags, `doc` (VARCHAR)
1 M distinct values; the metrics primary_value, `weight`, `amount` (DOUBLE, magnitudes from 1e-3 to 1e12, both signs)
and `year` (INT64).  Filters:
  half    row parity: about half of the rows, every block passes
  blocks  row < n / 100: about 1 % of the blocks
Arms, interleaved round after round in an order drawn anew for every round (seeded); per arm the median of the wall
clock with a device synchronisation at the end (every arm ends in a download), and of the time between two HIP events:
  counts/<filter>   facets(["bank"], expr)                                      the call without metrics
  stats1/<filter>   facets(["bank"], expr, metrics=["primary_value"])            16 slots x 1 metric: LDS records
  stats4/<filter>   the same with 4 metrics                                      16 x 4 = 64 records: the LDS bound
  tags0/<filter>, tags1/<filter>    facets(["tags"], expr) without and with metrics=["primary_value"]
  doc0/<filter>, doc1/<filter>      facets(["doc"], expr, limit=1000) without and with 1 metric: 1 000 records, the
                                    global-atomic path
  count/<filter>    query(expr, ["count(*)"])
  sum/<filter>      query(expr, ["sum(primary_value)"])                          the one-slot group alone
Once each (it takes seconds): host/<filter>, query(expr, ["bank", "primary_value"]) + math.fsum per bucket, whose sums
the device's must equal bit for bit.

    python tools/bench_facet_stats.py [--rows 1000000] [--rounds 20] [--warmup 3] [--out profiles/facet_stats_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import search as osearch  # noqa: E402
from rag_fin_amd.schema import DataType, FieldSchema  # noqa: E402
from rag_fin_amd.store import CorpusStore  # noqa: E402
from tools.bench_facets import summary, timed  # noqa: E402

TAGS = [f"t{i}" for i in range(64)]
FIELDS = [FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=8),
          FieldSchema("bank", DataType.VARCHAR), FieldSchema("doc", DataType.VARCHAR), FieldSchema("row", DataType.INT64),
          FieldSchema("parity", DataType.INT64), FieldSchema("weight", DataType.DOUBLE), FieldSchema("amount", DataType.DOUBLE),
          FieldSchema("year", DataType.INT64)]
METRICS = ["primary_value", "weight", "amount", "year"]


def build_store(n, d, device):
    import torch
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 9, size=n)
    flat = rng.integers(64, size=int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)])
    values = {name: (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 13, size=n)).tolist()
              for name in ("primary_value", "weight", "amount")}
    st = CorpusStore("bench", dim=d, capacity=n, device=device, fields=FIELDS)
    step = 1 << 17
    for s in range(0, n, step):
        e = min(n, s + step)
        rows = list(range(s, e))
        st.add(rows, [""] * (e - s), torch.from_numpy(osearch.synth_unit_rows(e - s, d, 100 + s // step)).to(device),
               [f"P{r * 8 // n}" for r in rows], [f"c{r % 4}" for r in rows], [f"s{(r // 4) % 2}" for r in rows],
               values["primary_value"][s:e],
               extra={"tags": [[TAGS[c] for c in flat[off[r]:off[r + 1]]] for r in rows],
                      "bank": [f"bank{(r * 7) % 16}" for r in rows], "doc": [f"doc{r}" for r in rows], "row": rows,
                      "parity": [r % 2 for r in rows], "weight": values["weight"][s:e], "amount": values["amount"][s:e],
                      "year": [2000 + (r * 13) % 25 for r in rows]})
    return st


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    n = args.rows
    st = build_store(n, args.dim, device)
    exprs = {"half": "parity == 0", "blocks": f"row < {n // 100}"}
    arms = {}
    for name, expr in exprs.items():
        arms[f"counts/{name}"] = lambda e=expr: st.facets(["bank"], expr=e)
        arms[f"stats1/{name}"] = lambda e=expr: st.facets(["bank"], expr=e, metrics=["primary_value"])
        arms[f"stats4/{name}"] = lambda e=expr: st.facets(["bank"], expr=e, metrics=METRICS)
        arms[f"tags0/{name}"] = lambda e=expr: st.facets(["tags"], expr=e)
        arms[f"tags1/{name}"] = lambda e=expr: st.facets(["tags"], expr=e, metrics=["primary_value"])
        arms[f"doc0/{name}"] = lambda e=expr: st.facets(["doc"], expr=e, limit=1000)
        arms[f"doc1/{name}"] = lambda e=expr: st.facets(["doc"], expr=e, limit=1000, metrics=["primary_value"])
        arms[f"count/{name}"] = lambda e=expr: st.query(e, output_fields=["count(*)"])
        arms[f"sum/{name}"] = lambda e=expr: st.query(e, output_fields=["sum(primary_value)"])
    ev = {k: [] for k in arms}
    wall = {k: [] for k in arms}
    last = {}
    shuffle = np.random.default_rng(0)
    for r in range(args.warmup + args.rounds):
        for name in shuffle.permutation(list(arms)).tolist():
            e, w, out = timed(arms[name])
            if r >= args.warmup:
                ev[name].append(e)
                wall[name].append(w)
            last[name] = out
    host, checks = {}, {}
    for name, expr in exprs.items():
        t = time.perf_counter()
        groups: dict = {}
        for rec in st.query(expr, output_fields=["bank", "primary_value"]):
            groups.setdefault(rec["bank"], []).append(rec["primary_value"])
        sums = {k: math.fsum(v) for k, v in groups.items()}
        host[name] = (time.perf_counter() - t) * 1e3
        got = last[f"stats1/{name}"]
        for b in got["facets"]["bank"]["buckets"]:   # the device's sums are math.fsum's, bit for bit
            assert bits(b["metrics"]["primary_value"]["sum"]) == bits(sums[b["value"]] + 0.0), (name, b["value"])
            assert b["metrics"]["primary_value"]["count"] == len(groups[b["value"]]) == b["count"]
        total = math.fsum(v for vs in groups.values() for v in vs)
        assert bits(got["metrics"]["primary_value"]["sum"]) == bits(total + 0.0) == \
            bits(last[f"sum/{name}"][0]["sum(primary_value)"]), name
        assert last[f"stats4/{name}"]["facets"]["bank"]["buckets"][0]["metrics"]["primary_value"] == \
            got["facets"]["bank"]["buckets"][0]["metrics"]["primary_value"]
        checks[name] = got["count"]
    med = {k: summary(v)["median"] for k, v in wall.items()}
    result = {
        "bench": "facet_stats", "rows": n, "dim": args.dim, "rounds": args.rounds, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "bank_values": 16, "distinct_tags": len(TAGS), "doc_values": n,
        "metrics": METRICS, "passing_rows": checks,
        "wall_ms": {k: summary(v) for k, v in wall.items()}, "event_ms": {k: summary(v) for k, v in ev.items()},
        "host_query_fsum_ms": host,
        "ratio_stats1_over_counts": {k: med[f"stats1/{k}"] / med[f"counts/{k}"] for k in exprs},
        "ratio_stats4_over_counts": {k: med[f"stats4/{k}"] / med[f"counts/{k}"] for k in exprs},
        "ratio_tags1_over_tags0": {k: med[f"tags1/{k}"] / med[f"tags0/{k}"] for k in exprs},
        "ratio_doc1_over_doc0": {k: med[f"doc1/{k}"] / med[f"doc0/{k}"] for k in exprs},
        "ratio_sum_over_count": {k: med[f"sum/{k}"] / med[f"count/{k}"] for k in exprs},
        "ratio_host_over_stats1": {k: host[k] / med[f"stats1/{k}"] for k in exprs},
    }
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "facet_stats", "rows": n, "wall_ms": {k: round(v, 4) for k, v in med.items()},
                      "host_query_fsum_ms": {k: round(v, 1) for k, v in host.items()},
                      "ratio_stats1_over_counts": {k: round(v, 2) for k, v in result["ratio_stats1_over_counts"].items()},
                      "ratio_host_over_stats1": {k: round(v, 1) for k, v in result["ratio_host_over_stats1"].items()}}))


if __name__ == "__main__":
    main()
