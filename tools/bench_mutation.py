"""Cost of CorpusStore.delete at 1 M x 384: device time of rf_index_compact, the host bookkeeping,
and the first search after the delete next to a fresh index of the survivors.

Cases: 1 % of the rows at random, a contiguous 1/8, 50 % at random.  Per case:
  * compact_device_ms: rf_index_compact alone (keep list already on the device), HIP events,
    median of --repeats runs, each on a freshly loaded index; with the bytes it moves
    (gather read + scratch write, tile read + write, norm read: 5 x n_keep x dim x 2) and the
    rate over the device time;
  * store delete (expression on the device columns): wall time of the whole call, split into the
    row mask (build_filter + download), the index compaction (upload of the keep list + the
    kernels, synchronised) and the host bookkeeping (columns, pk map, filter mirror);
  * the first rf_search (B = 64, k = 10) after the delete and the median of the next --steps,
    against the same on a fresh GpuIndex of the survivors.

    python tools/bench_mutation.py [--rows 1000000] [--repeats 5] [--steps 50] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import search as osearch  # noqa: E402
from rag_fin_amd import _lib  # noqa: E402
from rag_fin_amd.store import CorpusStore, GpuIndex  # noqa: E402

CASES = {"rand1pct": 'primary_value < 0.01', "contig8": 'chunk_type == "part3"', "rand50pct": 'primary_value < 0.5'}


def columns(n, rng):
    pv = rng.random(n)
    return pv, [f"part{i * 8 // n}" for i in range(n)]


def first_and_steady(ix, q, k, steps):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda.synchronize()
    ev[0].record()
    ix.search_raw(q, k)
    ev[1].record()
    for _ in range(5):
        ix.search_raw(q, k)
    ev[2].record()
    for _ in range(steps):
        ix.search_raw(q, k)
    ev[3].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]) / steps


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the results as one JSON file here")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d, k = a.rows, a.dim, 10
    lib = _lib.load_library()
    c16 = torch.from_numpy(osearch.synth_unit_rows(n, d, 1234)).to(dev)
    q = torch.from_numpy(osearch.synth_unit_rows(64, d, 99)).to(dev)
    rng = np.random.default_rng(0)
    pv, parts = columns(n, rng)
    ids = [f"c{i}" for i in range(n)]
    out = {"rows": n, "dim": d, "window_rows": GpuIndex.COMPACT_WINDOW_ROWS, "cases": []}
    ix = GpuIndex(d, n, dev)
    for name, expr in CASES.items():
        mask = (pv < 0.01) if name == "rand1pct" else (pv < 0.5) if name == "rand50pct" else \
            np.array([p == "part3" for p in parts])
        keep = np.flatnonzero(~mask)
        keep_d = torch.from_numpy(keep).to(dev)
        w = GpuIndex.COMPACT_WINDOW_ROWS
        scratch = torch.empty(w * d * 2, dtype=torch.uint8, device=dev)
        # (1) the kernels alone
        dev_ms = []
        for _ in range(a.repeats):
            ix.reset()
            ix.add(c16)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            with torch.cuda.device(dev):
                _lib.check(lib.rf_index_compact(ix.handle, c_void_p(keep_d.data_ptr()), keep.size,
                                                c_void_p(scratch.data_ptr()), scratch.numel(), _lib.current_stream_ptr()))
            ev[1].record()
            torch.cuda.synchronize()
            dev_ms.append(ev[0].elapsed_time(ev[1]))
        moved = 5 * keep.size * d * 2
        ms = float(np.median(dev_ms))
        # (2) the store's delete, split into its parts
        st = CorpusStore("bench", dim=d, capacity=n, device=dev)
        st.insert([list(ids), ["t"] * n, c16, ["Q1_FY2024"] * n, parts, ["s"] * n, pv.tolist()])
        st.build_filter('period == "Q1_FY2024"')      # the device column mirror exists, as after a filtered search
        torch.cuda.synchronize()
        parts_ms = {}

        def timed(label, fn):
            def run(*args, **kw):
                torch.cuda.synchronize()
                t = time.perf_counter()
                r = fn(*args, **kw)
                torch.cuda.synchronize()
                parts_ms[label] = (time.perf_counter() - t) * 1e3
                return r
            return run
        st._match_mask = timed("mask", st._match_mask)
        st.index.compact = timed("compact", st.index.compact)
        t0 = time.perf_counter()
        res = st.delete(expr)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        assert res.delete_count == int(mask.sum()) and st.num_entities == keep.size
        # (3) first search after the delete vs a fresh index of the survivors
        first_del, steady_del = first_and_steady(st.index, q, k, a.steps)
        fresh = GpuIndex(d, keep.size, dev)
        fresh.add(c16[keep_d].contiguous())
        first_fresh, steady_fresh = first_and_steady(fresh, q, k, a.steps)
        row = {"case": name, "expr": expr, "n_deleted": int(mask.sum()), "n_keep": int(keep.size),
               "compact_device_ms": round(ms, 4), "compact_device_ms_spread": [round(min(dev_ms), 4), round(max(dev_ms), 4)],
               "compact_bytes_moved": moved, "compact_gb_per_s": round(moved / (ms * 1e-3) / 1e9, 1),
               "store_delete_ms": round(total, 2), "store_mask_ms": round(parts_ms["mask"], 2),
               "store_compact_ms": round(parts_ms["compact"], 2),
               "store_host_bookkeeping_ms": round(total - parts_ms["mask"] - parts_ms["compact"], 2),
               "first_search_ms_after_delete": round(first_del, 4), "first_search_ms_fresh": round(first_fresh, 4),
               "steady_search_ms_after_delete": round(steady_del, 4), "steady_search_ms_fresh": round(steady_fresh, 4)}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
        del st, fresh
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
