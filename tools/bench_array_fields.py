"""Filters over ARRAY fields (FieldSchema(..., DataType.ARRAY, ...)) against the same selection on a declared VARCHAR
field and against the host route, at 1 M x 384 in one process.

Store: 1 M synth rows and 64 distinct tags t0 .. t63.  Two VARCHAR ARRAY fields hold 4 M elements each:
  tags_u  uniform: a row's length is uniform in 0..8, its tags uniform over the 64
  tags_s  skewed: the same 4 M elements in 1 000 rows of 4 000 elements each (every 1 000th row), all other rows empty
and `bank` (VARCHAR) is "t7" exactly on the rows whose tags_u holds "t7", so `bank == "t7"` and
ARRAY_CONTAINS(tags_u, "t7") select the same rows (asserted) and the search steps behind them see the same filter.
Filter-build arms, each one CorpusStore.build_filter call (parse, compile, the small uploads, the kernels) except
the host one:
  contains/array    ARRAY_CONTAINS(tags_u, "t7")          contains/scalar   bank == "t7"
  contains/host     the mask in numpy over the host CSR (flat codes == code, rows by bincount), packed, uploaded
                    and compacted by rf_filter_from_mask -- the route the device leaf replaces
  all3              ARRAY_CONTAINS_ALL(tags_u, [3 tags])
  any1000           ARRAY_CONTAINS_ANY(tags_u, [1 000 strings]), 16 of them tags (the others are dropped against
                    the field's dictionary at compile time: a field of 64 distinct tags has no more needles)
  contains_skewed   ARRAY_CONTAINS(tags_s, "t7")
  length            ARRAY_LENGTH(tags_u) >= 4             elem0             tags_u[0] == "t7"
The arms run interleaved, round after round, in an order drawn anew for every round (seeded); per arm the median over
the rounds of the time between two HIP events on the stream around the call, and of the wall clock with a device
synchronisation at the end (the host arm is mostly host work, which events do not see).  Then one filtered search
step (B = 64, k = 10) behind the array and the scalar buffer of `contains`, interleaved in the same way.

    python tools/bench_array_fields.py [--rows 1000000] [--rounds 40] [--warmup 5] [--out FILE.json]
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
from rag_fin_amd.index import filter_from_mask  # noqa: E402
from rag_fin_amd.schema import DataType, FieldSchema  # noqa: E402
from rag_fin_amd.store import CorpusStore  # noqa: E402

TAGS = [f"t{i}" for i in range(64)]
LONG = 4000   # elements of a long row of the skewed field
FIELDS = [FieldSchema("tags_u", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=8),
          FieldSchema("tags_s", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=4096),
          FieldSchema("bank", DataType.VARCHAR)]


def build_store(n, d, device):
    """-> (store, lengths of tags_u int64 [n], its flat codes int64 [sum])."""
    import torch
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 9, size=n)
    flat = rng.integers(64, size=int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)])
    every = max(1, n // max(1, flat.size // LONG))   # a long row every `every` rows holds the same elements, LONG at a time
    st = CorpusStore("bench", dim=d, capacity=n, device=device, fields=FIELDS)
    step = 1 << 17
    for s in range(0, n, step):
        e = min(n, s + step)
        rows = list(range(s, e))
        tags_u = [[TAGS[c] for c in flat[off[r]:off[r + 1]]] for r in rows]
        tags_s = [[TAGS[c] for c in flat[(r // every) * LONG:(r // every + 1) * LONG]] if r % every == 0 else [] for r in rows]
        bank = ["t7" if "t7" in t else "t8" for t in tags_u]
        st.add(rows, [""] * (e - s), torch.from_numpy(osearch.synth_unit_rows(e - s, d, 100 + s // step)).to(device),
               [f"P{r * 8 // n}" for r in rows], [f"c{r % 4}" for r in rows], [f"s{(r // 4) % 2}" for r in rows],
               [float(r % 1000) for r in rows], extra={"tags_u": tags_u, "tags_s": tags_s, "bank": bank})
    return st, lens, flat


def timed(fn):
    """(milliseconds between two events on the stream around fn, wall milliseconds with a sync at the end, fn())."""
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
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    n = args.rows
    st, lens, flat = build_store(n, args.dim, device)
    row_of = np.repeat(np.arange(n), lens)
    any1000 = [f"x{i}" for i in range(984)] + TAGS[:16]
    exprs = {"contains/array": 'ARRAY_CONTAINS(tags_u, "t7")', "contains/scalar": 'bank == "t7"',
             "all3": 'ARRAY_CONTAINS_ALL(tags_u, ["t7", "t8", "t9"])',
             "any1000": "ARRAY_CONTAINS_ANY(tags_u, [" + ", ".join(f'"{t}"' for t in any1000) + "])",
             "contains_skewed": 'ARRAY_CONTAINS(tags_s, "t7")', "length": "ARRAY_LENGTH(tags_u) >= 4",
             "elem0": 'tags_u[0] == "t7"'}

    def host_route():
        mask = np.bincount(row_of[flat == 7], minlength=n) > 0
        bits = np.packbits(np.pad(mask, (0, -n % 32)), bitorder="little")
        return filter_from_mask(torch.from_numpy(bits.view(np.int32)).to(device), n)

    arms = {name: (lambda e=expr: st.build_filter(e)) for name, expr in exprs.items()}
    arms["contains/host"] = host_route
    ev = {k: [] for k in arms}
    wall = {k: [] for k in arms}
    passing = {}
    shuffle = np.random.default_rng(0)
    for r in range(args.warmup + args.rounds):
        for name in shuffle.permutation(list(arms)).tolist():
            e, w, buf = timed(arms[name])
            if r >= args.warmup:
                ev[name].append(e)
                wall[name].append(w)
            passing[name] = int(buf[4:8].cpu().numpy().view(np.uint32)[0])
    assert passing["contains/array"] == passing["contains/scalar"] == passing["contains/host"] > 0, passing
    assert passing["length"] == int((lens >= 4).sum()) and 0 < passing["contains_skewed"] <= -(-n // 1000), passing

    q = torch.from_numpy(osearch.synth_unit_rows(64, args.dim, 7)).to(device)
    bufs = {"array": st.build_filter(exprs["contains/array"]), "scalar": st.build_filter(exprs["contains/scalar"])}
    step = {k: [] for k in bufs}
    for r in range(args.warmup + args.rounds):
        for name, buf in bufs.items():
            e, _, _ = timed(lambda: st.index.search(q, 10, filt=buf))
            if r >= args.warmup:
                step[name].append(e)
    med = {k: summary(v)["median"] for k, v in ev.items()}
    result = {
        "bench": "array_fields", "rows": n, "dim": args.dim, "rounds": args.rounds, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "elements": int(flat.size), "distinct_tags": len(TAGS),
        "long_rows": int(sum(1 for r in st.columns["tags_s"] if r)), "long_row_elements": LONG,
        "filter_build_event_ms": {k: summary(v) for k, v in ev.items()},
        "filter_build_wall_ms": {k: summary(v) for k, v in wall.items()},
        "passing_rows": passing,
        "ratio_array_over_scalar": med["contains/array"] / med["contains/scalar"],
        "ratio_skewed_over_uniform": med["contains_skewed"] / med["contains/array"],
        "ratio_host_wall_over_array_wall": summary(wall["contains/host"])["median"] / summary(wall["contains/array"])["median"],
        "search_step_event_ms": {k: summary(v) for k, v in step.items()}, "search_B": 64, "search_k": 10,
    }
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "array_fields", "rows": n,
                      "filter_build_event_ms": {k: round(v, 4) for k, v in med.items()},
                      "ratio_array_over_scalar": round(result["ratio_array_over_scalar"], 3),
                      "ratio_skewed_over_uniform": round(result["ratio_skewed_over_uniform"], 3),
                      "search_step_event_ms": {k: round(summary(v)["median"], 4) for k, v in step.items()}}))


if __name__ == "__main__":
    main()
