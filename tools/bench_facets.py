"""Faceted counts (CorpusStore.facets, query(..., ["count(*)"])) against the filter build alone and against the route a
user had before -- query(expr, output_fields=[field]) + collections.Counter on the host -- at 1 M rows in one process.

Store: 1 M synth rows; `tags` (ARRAY VARCHAR) holds 4 M elements over 64 tags (a row's length uniform in 0..8), `bank`
(VARCHAR) 16 values, `doc` (VARCHAR) 1 M distinct values, `row` (INT64) the row number.  Filters:
  half    row parity: about half of the rows, every block passes
  blocks  row < n / 100: about 1 % of the blocks
Arms, interleaved round after round in an order drawn anew for every round (seeded); per arm the median of the wall
clock with a device synchronisation at the end (every arm ends in a download), and of the time between two HIP events:
  facets/<filter>        facets(["bank", "tags", "doc"], expr, ranges={"primary_value": 3 ranges}): filter build included
  filter/<filter>        build_filter(expr) alone
  facets_small/<filter>  facets(["bank", "tags"], expr): without the 1 M-value dictionary
  count/<filter>         query(expr, output_fields=["count(*)"])
Once each (they take seconds): host/<filter>, Counter over query(expr, output_fields=["bank"]), and len(query(expr)).

    python tools/bench_facets.py [--rows 1000000] [--rounds 20] [--warmup 3] [--out profiles/facets_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import search as osearch  # noqa: E402
from rag_fin_amd.schema import DataType, FieldSchema  # noqa: E402
from rag_fin_amd.store import CorpusStore  # noqa: E402

TAGS = [f"t{i}" for i in range(64)]
FIELDS = [FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=8),
          FieldSchema("bank", DataType.VARCHAR), FieldSchema("doc", DataType.VARCHAR), FieldSchema("row", DataType.INT64),
          FieldSchema("parity", DataType.INT64)]


def build_store(n, d, device):
    import torch
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 9, size=n)
    flat = rng.integers(64, size=int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)])
    st = CorpusStore("bench", dim=d, capacity=n, device=device, fields=FIELDS)
    step = 1 << 17
    for s in range(0, n, step):
        e = min(n, s + step)
        rows = list(range(s, e))
        st.add(rows, [""] * (e - s), torch.from_numpy(osearch.synth_unit_rows(e - s, d, 100 + s // step)).to(device),
               [f"P{r * 8 // n}" for r in rows], [f"c{r % 4}" for r in rows], [f"s{(r // 4) % 2}" for r in rows],
               [float(r % 2000) for r in rows],
               extra={"tags": [[TAGS[c] for c in flat[off[r]:off[r + 1]]] for r in rows],
                      "bank": [f"bank{(r * 7) % 16}" for r in rows], "doc": [f"doc{r}" for r in rows], "row": rows,
                      "parity": [r % 2 for r in rows]})
    return st, int(flat.size)


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t) * 1e3, out


def summary(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90)),
            "min": float(xs.min()), "n": int(xs.size)}


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
    st, elements = build_store(n, args.dim, device)
    exprs = {"half": "parity == 0", "blocks": f"row < {n // 100}"}
    ranges = {"primary_value": [(None, 500), (500, 1500), (1500, None)]}
    arms = {}
    for name, expr in exprs.items():
        arms[f"facets/{name}"] = lambda e=expr: st.facets(["bank", "tags", "doc"], expr=e, ranges=ranges)
        arms[f"facets_small/{name}"] = lambda e=expr: st.facets(["bank", "tags"], expr=e)
        arms[f"filter/{name}"] = lambda e=expr: st.build_filter(e)
        arms[f"count/{name}"] = lambda e=expr: st.query(e, output_fields=["count(*)"])
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
    host, host_len, checks = {}, {}, {}
    for name, expr in exprs.items():
        t = time.perf_counter()
        counts = Counter(rec["bank"] for rec in st.query(expr, output_fields=["bank"]))
        host[name] = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        n_pass = len(st.query(expr))
        host_len[name] = (time.perf_counter() - t) * 1e3
        got = last[f"facets/{name}"]
        assert got["count"] == n_pass == last[f"count/{name}"][0]["count(*)"], (name, got["count"], n_pass)
        # (the definition's order, count descending then value ascending: most_common cuts a tie by first-seen order)
        want = sorted(counts.items(), key=lambda vc: (-vc[1], vc[0]))[:10]
        assert [(b["value"], b["count"]) for b in got["facets"]["bank"]["buckets"]] == want, name
        checks[name] = n_pass
    med = {k: summary(v)["median"] for k, v in wall.items()}
    result = {
        "bench": "facets", "rows": n, "dim": args.dim, "rounds": args.rounds, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "array_elements": elements, "distinct_tags": len(TAGS),
        "bank_values": 16, "doc_values": n, "passing_rows": checks,
        "wall_ms": {k: summary(v) for k, v in wall.items()}, "event_ms": {k: summary(v) for k, v in ev.items()},
        "host_query_counter_ms": host, "host_len_query_ms": host_len,
        "ratio_host_over_facets": {k: host[k] / med[f"facets/{k}"] for k in exprs},
        "ratio_host_over_facets_small": {k: host[k] / med[f"facets_small/{k}"] for k in exprs},
        "ratio_facets_over_filter": {k: med[f"facets/{k}"] / med[f"filter/{k}"] for k in exprs},
        "ratio_facets_small_over_filter": {k: med[f"facets_small/{k}"] / med[f"filter/{k}"] for k in exprs},
        "ratio_len_query_over_count": {k: host_len[k] / med[f"count/{k}"] for k in exprs},
    }
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "facets", "rows": n, "wall_ms": {k: round(v, 4) for k, v in med.items()},
                      "host_query_counter_ms": {k: round(v, 1) for k, v in host.items()},
                      "ratio_host_over_facets": {k: round(v, 1) for k, v in result["ratio_host_over_facets"].items()},
                      "ratio_facets_over_filter": {k: round(v, 2) for k, v in result["ratio_facets_over_filter"].items()}}))


if __name__ == "__main__":
    main()
