"""Filters over dynamic fields (CorpusStore(enable_dynamic_field=True)) against the same predicates on declared
fields of the matching type and against the host route, at 1 M x 384 in one process.

Store: 1 M synth rows; `period` dealt in 8 contiguous runs; declared fields period2 (VARCHAR, a copy of period),
fiscal_year (INT64, row % 4000), audited (BOOL, row % 2) and weight (DOUBLE, row % 1000); and the dynamic keys
d_period, d_year, d_audited and d_weight holding the same values, so a predicate selects the same rows on either
side (asserted).  A dynamic leaf reads a tag byte and 8 payload bytes per row (9 bytes) where a coded declared
column reads 4 and an INT64 / DOUBLE one 8.  Filter-build arms, each one CorpusStore.build_filter call (parse,
compile, the small uploads, the kernels) except the host ones:
  str_eq      X == "P3"                      declared period2 | dynamic d_period | host
  int_range   X >= 2000                      declared fiscal_year | dynamic d_year | host
  in_1000     X in [1000 values]             declared fiscal_year | dynamic d_year | host
  sixteen     16 comparisons over the four fields joined by and / or   declared | dynamic | host
host: the route the device leaves replace -- the mask of the host columns in numpy, packed, uploaded and
compacted by rf_filter_from_mask.
The arms run interleaved, round after round, in an order drawn anew for every round (seeded, so that no arm always
follows the same neighbour); per arm the median over the rounds of the time between two HIP events on the stream around the call, and of the wall clock with a device synchronisation at the end (the host arms are
mostly host work, which events do not see).  Then one filtered search step (B = 64, k = 10) behind the declared
and the dynamic buffer of str_eq, interleaved in the same way; the buffers' written words are compared, so the two
medians can differ only by the run-to-run spread, which is reported beside them (p10 / p90).

    python tools/bench_dynamic_fields.py [--rows 1000000] [--rounds 40] [--warmup 5] [--out FILE.json]
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
from rag_fin_amd import filter_expr  # noqa: E402
from rag_fin_amd.index import filter_from_mask  # noqa: E402
from rag_fin_amd.schema import DataType, FieldSchema  # noqa: E402
from rag_fin_amd.store import CorpusStore  # noqa: E402

FIELDS = [FieldSchema("period2", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64),
          FieldSchema("audited", DataType.BOOL), FieldSchema("weight", DataType.DOUBLE)]
DYNAMIC = {"period2": "d_period", "fiscal_year": "d_year", "audited": "d_audited", "weight": "d_weight"}

SIXTEEN = ('(period2 == "P3" or period2 == "P4" or period2 > "P6" or period2 like "P0%") and '
           '(fiscal_year >= 100 and fiscal_year < 3900 and fiscal_year != 2000 and fiscal_year not in [1, 2, 3]) and '
           '(audited == true or audited != false or weight > 10 or weight <= 990) and '
           '(weight != 500 and fiscal_year in [5, 6, 7, 2001] or period2 != "P1" or fiscal_year <= 3000)')


def on_dynamic(expr: str) -> str:
    for name, key in DYNAMIC.items():
        expr = expr.replace(name, key)
    return expr


def sixteen_host(c):
    p, y, a, w = c["period2"], c["fiscal_year"], c["audited"], c["weight"]
    return (((p == "P3") | (p == "P4") | (p > "P6") | np.char.startswith(p, "P0")) &
            ((y >= 100) & (y < 3900) & (y != 2000) & ~np.isin(y, [1, 2, 3])) &
            (a | a | (w > 10) | (w <= 990)) &
            ((w != 500) & np.isin(y, [5, 6, 7, 2001]) | (p != "P1") | (y <= 3000)))


def build_store(n, d, device):
    import torch
    st = CorpusStore("bench", dim=d, capacity=n, device=device, fields=FIELDS, enable_dynamic_field=True)
    step = 1 << 17
    for s in range(0, n, step):
        e = min(n, s + step)
        rows = list(range(s, e))
        per = [f"P{r * 8 // n}" for r in rows]
        own = {"period2": per, "fiscal_year": [r % 4000 for r in rows], "audited": [r % 2 == 0 for r in rows],
               "weight": [float(r % 1000) for r in rows]}
        st.add(rows, [""] * (e - s), torch.from_numpy(osearch.synth_unit_rows(e - s, d, 100 + s // step)).to(device), per,
               [f"c{r % 4}" for r in rows], [f"s{(r // 4) % 2}" for r in rows], [float(r % 1000) for r in rows],
               extra=dict(own, **{DYNAMIC[f]: col for f, col in own.items()}))
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
    host = {"period2": np.array(st.columns["period2"]), "fiscal_year": np.array(st.columns["fiscal_year"], dtype=np.int64),
            "audited": np.array(st.columns["audited"]), "weight": np.array(st.columns["weight"])}
    values = [3 * i + 1 for i in range(1000)]
    exprs = {"str_eq": 'period2 == "P3"', "int_range": "fiscal_year >= 2000",
             "in_1000": "fiscal_year in [" + ", ".join(map(str, values)) + "]", "sixteen": SIXTEEN}
    masks = {"str_eq": lambda: host["period2"] == "P3", "int_range": lambda: host["fiscal_year"] >= 2000,
             "in_1000": lambda: np.isin(host["fiscal_year"], values), "sixteen": lambda: sixteen_host(host)}

    def host_route(mask):
        bits = np.packbits(np.pad(mask(), (0, -n % 32)), bitorder="little")
        return filter_from_mask(torch.from_numpy(bits.view(np.int32)).to(device), n)

    arms = {}
    for name, expr in exprs.items():
        arms[name + "/declared"] = lambda e=expr: st.build_filter(e)
        arms[name + "/dynamic"] = lambda e=on_dynamic(expr): st.build_filter(e)
        arms[name + "/host"] = lambda m=masks[name]: host_route(m)
    ev = {k: [] for k in arms}
    wall = {k: [] for k in arms}
    passing = {}
    shuffle = np.random.default_rng(0)
    for r in range(args.warmup + args.rounds):
        # interleaved: one call of every arm per round, in an order drawn anew for every round (seeded), so that no
        # arm always runs behind the same neighbour (a 9 ms host arm leaves the device idle before the next call)
        for name in shuffle.permutation(list(arms)).tolist():
            e, w, buf = timed(arms[name])
            if r >= args.warmup:
                ev[name].append(e)
                wall[name].append(w)
            passing[name] = int(buf[4:8].cpu().numpy().view(np.uint32)[0])
    for name in exprs:
        assert passing[name + "/declared"] == passing[name + "/dynamic"] == passing[name + "/host"], (name, passing)

    q = torch.from_numpy(osearch.synth_unit_rows(64, args.dim, 7)).to(device)
    bufs = {"declared": st.build_filter(exprs["str_eq"]), "dynamic": st.build_filter(on_dynamic(exprs["str_eq"]))}

    def written(buf):
        """The words of a filter buffer the device wrote: header, mask, and the block list up to its count."""
        w = buf.cpu().numpy().view(np.uint32)
        nblk = (n + 31) // 32
        stride = (nblk * 4 + 15) // 16 * 4
        return np.concatenate([w[:4 + nblk], w[4 + stride:4 + stride + int(w[2])]])

    same = bool(np.array_equal(written(bufs["declared"]), written(bufs["dynamic"])))
    step = {k: [] for k in bufs}
    for r in range(args.warmup + args.rounds):
        for name, buf in bufs.items():
            e, _, _ = timed(lambda: st.index.search(q, 10, filt=buf))
            if r >= args.warmup:
                step[name].append(e)
    result = {
        "bench": "dynamic_fields", "rows": n, "dim": args.dim, "rounds": args.rounds, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "filter_build_event_ms": {k: summary(v) for k, v in ev.items()},
        "filter_build_wall_ms": {k: summary(v) for k, v in wall.items()},
        "passing_rows": passing, "leaves": {name: leaves_of(st, expr) for name, expr in exprs.items()},
        "search_step_event_ms": {k: summary(v) for k, v in step.items()},
        "search_filters_bit_identical": same, "search_B": 64, "search_k": 10,
    }
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "dynamic_fields", "rows": n,
                      "filter_build_event_ms": {k: round(summary(v)["median"], 4) for k, v in ev.items()},
                      "search_step_event_ms": {k: round(summary(v)["median"], 4) for k, v in step.items()}}))


def leaves_of(st, expr):
    """How many column leaves the declared form and how many dynamic leaves the dynamic form compile to."""
    dicts = {name: c.dict for (name, coded), c in (st._xcols or {}).items() if coded}
    dyn = {key: c.dict for key, c in (st._dyncols or {}).items()}
    out = {}
    for side, e in (("declared", expr), ("dynamic", on_dynamic(expr))):
        prog = filter_expr.compile_expr(filter_expr.parse(e, st.analyzer, st.schema, True), st._dcols.dicts, st._pk_row,
                                        None, st.schema, dicts, dyn)
        out[side] = len(prog.column_leaves) + len(prog.dynamic_leaves)
    return out


if __name__ == "__main__":
    main()
