"""Filters over user-defined scalar fields (CorpusStore(fields=...)) against the built-in column they stand
beside, at 1 M x 384 in one process.

Store: 1 M synth rows; `period` dealt in 8 contiguous runs (a corpus ingested quarter by quarter), an extra
VARCHAR field `period2` holding a copy of it, an extra INT64 field `fiscal_year` (row % 4000), an extra BOOL
field `audited` (row % 2) and an extra DOUBLE field `weight` (row % 1000).  Filter-build arms, each one
CorpusStore.build_filter call (parse, compile, the small uploads, the kernels) except (f):
  a  builtin_period     period == "P3"                      the built-in column: the yardstick
  b  extra_varchar      period2 == "P3"                     the same predicate on the extra copy
  c  int64_interval     fiscal_year >= 2000                 one inclusive int64 interval
  d  int64_in_1000      fiscal_year in [1000 values]        binary search in a sorted set
  e  sixteen_leaves     16 leaves over the four extra fields joined by and / or
  f  host_mask          the route (b) replaces: the mask of the host column in numpy, packed, uploaded and
                        compacted by rf_filter_from_mask
The arms run interleaved, round after round; per arm the median over the rounds of the time between two HIP
events on the stream around the call (and of the wall clock with a device synchronisation at the end: (f) is
mostly host work, which events do not see).  Then one filtered search step (B = 64, k = 10) behind the
buffers of (a) and (b), interleaved in the same way; the two buffers are bit-identical
(tests/test_extra_fields_gpu.py), so the two medians can differ only by the run-to-run spread, which is
reported beside them (the 10th and 90th percentile of (a)).

    python tools/bench_extra_fields.py [--rows 1000000] [--rounds 40] [--warmup 5] [--out FILE.json]
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

FIELDS = [FieldSchema("period2", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64),
          FieldSchema("audited", DataType.BOOL), FieldSchema("weight", DataType.DOUBLE)]

SIXTEEN = ('(period2 == "P3" or period2 == "P4" or period2 > "P6" or period2 like "P0%") and '
           '(fiscal_year >= 100 and fiscal_year < 3900 and fiscal_year != 2000 and fiscal_year not in [1, 2, 3]) and '
           '(audited == true or audited != false or weight > 10 or weight <= 990) and '
           '(weight != 500 and fiscal_year in [5, 6, 7, 2001] or period2 != "P1" or fiscal_year <= 3000)')


def build_store(n, d, device):
    import torch
    st = CorpusStore("bench", dim=d, capacity=n, device=device, fields=FIELDS)
    step = 1 << 17
    for s in range(0, n, step):
        e = min(n, s + step)
        rows = list(range(s, e))
        per = [f"P{r * 8 // n}" for r in rows]
        st.add(rows, [""] * (e - s), torch.from_numpy(osearch.synth_unit_rows(e - s, d, 100 + s // step)).to(device), per,
               [f"c{r % 4}" for r in rows], [f"s{(r // 4) % 2}" for r in rows], [float(r % 1000) for r in rows],
               extra={"period2": per, "fiscal_year": [r % 4000 for r in rows], "audited": [r % 2 == 0 for r in rows],
                      "weight": [float(r % 1000) for r in rows]})
    return st


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
    st = build_store(n, args.dim, device)
    period_host = np.array(st.columns["period2"])
    in_1000 = "fiscal_year in [" + ", ".join(str(3 * i + 1) for i in range(1000)) + "]"

    def host_mask():
        bits = np.packbits(np.pad(period_host == "P3", (0, -n % 32)), bitorder="little")
        return filter_from_mask(torch.from_numpy(bits.view(np.int32)).to(device), n)

    arms = {
        "a_builtin_period": lambda: st.build_filter('period == "P3"'),
        "b_extra_varchar": lambda: st.build_filter('period2 == "P3"'),
        "c_int64_interval": lambda: st.build_filter("fiscal_year >= 2000"),
        "d_int64_in_1000": lambda: st.build_filter(in_1000),
        "e_sixteen_leaves": lambda: st.build_filter(SIXTEEN),
        "f_host_mask": host_mask,
    }
    ev = {k: [] for k in arms}
    wall = {k: [] for k in arms}
    passing = {}
    for r in range(args.warmup + args.rounds):
        for name, fn in arms.items():       # interleaved: one call of every arm per round
            e, w, buf = timed(fn)
            if r >= args.warmup:
                ev[name].append(e)
                wall[name].append(w)
            passing[name] = int(buf[4:8].cpu().numpy().view(np.uint32)[0])
    assert passing["a_builtin_period"] == passing["b_extra_varchar"] == passing["f_host_mask"]

    q = torch.from_numpy(osearch.synth_unit_rows(64, args.dim, 7)).to(device)
    bufs = {"a_builtin_period": st.build_filter('period == "P3"'), "b_extra_varchar": st.build_filter('period2 == "P3"')}

    def written(buf):
        """The words of a filter buffer the device wrote: header, mask, and the block list up to its count."""
        w = buf.cpu().numpy().view(np.uint32)
        nblk = (n + 31) // 32
        stride = (nblk * 4 + 15) // 16 * 4
        return np.concatenate([w[:4 + nblk], w[4 + stride:4 + stride + int(w[2])]])

    same = bool(np.array_equal(written(bufs["a_builtin_period"]), written(bufs["b_extra_varchar"])))
    step = {k: [] for k in bufs}
    for r in range(args.warmup + args.rounds):
        for name, buf in bufs.items():
            e, _, _ = timed(lambda: st.index.search(q, 10, filt=buf))
            if r >= args.warmup:
                step[name].append(e)
    leaves = {k: len(st_prog_leaves(st, e)) for k, e in (("b_extra_varchar", 'period2 == "P3"'), ("c_int64_interval", "fiscal_year >= 2000"),
                                                      ("d_int64_in_1000", in_1000), ("e_sixteen_leaves", SIXTEEN))}
    result = {
        "bench": "extra_fields", "rows": n, "dim": args.dim, "rounds": args.rounds, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "filter_build_event_ms": {k: summary(v) for k, v in ev.items()},
        "filter_build_wall_ms": {k: summary(v) for k, v in wall.items()},
        "passing_rows": passing, "column_leaves": leaves,
        "search_step_event_ms": {k: summary(v) for k, v in step.items()},
        "search_filters_bit_identical": same, "search_B": 64, "search_k": 10,
    }
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "extra_fields", "rows": n,
                      "filter_build_event_ms": {k: round(summary(v)["median"], 4) for k, v in ev.items()},
                      "search_step_event_ms": {k: round(summary(v)["median"], 4) for k, v in step.items()}}))


def st_prog_leaves(st, expr):
    """The column leaves an expression compiles to on this store."""
    from rag_fin_amd import filter_expr
    node = filter_expr.parse(expr, st.analyzer, st.schema)
    dicts = {name: c.dict for (name, coded), c in (st._xcols or {}).items() if coded}
    return filter_expr.compile_expr(node, st._dcols.dicts, st._pk_row, None, st.schema, dicts).column_leaves


if __name__ == "__main__":
    main()
