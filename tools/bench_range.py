"""Range search against plain search on one index, interleaved in one process: 1 M x 384 random
unit rows, k = 10, B in {1, 64}.

Per B, pipelined as bench.py does (4 lanes: own stream and workspace each, bare enqueues), the
variants alternating round by round, median of the rounds:
  plain       rf_search (the yardstick: the code path of a search without range parameters)
  all_rows    rf_search_range with the band (-inf, +inf]: what the band form itself costs (no sample
              fold: the emit reads the sampled 1/16 of the corpus again; the clip's compares)
  top         a band of ~100 rows per query at the top of the ranking
  low         a band of the same width well below the top (around rank 5 000): every block holds
              rows above the ceiling
  empty       a band above every score
The bounds come from the fp32 scores of the batch on the device (medians over the queries of the
scores at those ranks).  Writes one JSON (default profiles/range_bench.json) and prints it.

    python tools/bench_range.py [--rows 1000000] [--steps 40] [--rounds 5] [--out FILE.json]
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
from rag_fin_amd.store import GpuIndex  # noqa: E402

K = 10
LANES = 4
INF = float("inf")


def pipelined(enqueue, steps, warm, sync):
    for i in range(warm):
        enqueue(i)
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        enqueue(i)
    sync()
    return (time.perf_counter() - t0) / steps


def rank_scores(q, c16, ranks, dev):
    """Median over the queries of the fp32 score at each of `ranks` (1 = best)."""
    import torch
    top = max(ranks)
    best = None
    for s in range(0, c16.shape[0], 1 << 18):
        sc = q.float() @ torch.from_numpy(c16[s:s + (1 << 18)]).to(dev).float().T
        best = sc if best is None else torch.cat([best, sc], 1)
        best = best.topk(min(top, best.shape[1]), dim=1).values
    return {r: float(best[:, r - 1].median()) for r in ranks}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    d = 384
    c16 = osearch.synth_unit_rows(a.rows, d, 1234)
    qall = osearch.synth_unit_rows(64, d, 99)
    ix = GpuIndex(d, a.rows, dev)
    for s in range(0, a.rows, 1 << 18):
        ix.add(torch.from_numpy(c16[s:s + (1 << 18)]).to(dev))
    torch.cuda.synchronize()
    out = {"rows": a.rows, "dim": d, "k": K, "lanes": LANES, "steps": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(dev), "cases": []}
    for B in (1, 64):
        q = torch.from_numpy(np.ascontiguousarray(qall[:B])).to(dev)
        at = rank_scores(q, c16, (100, 5000, 5100), dev)
        bands = {"all_rows": (-INF, INF), "top": (at[100], INF), "low": (at[5100], at[5000]), "empty": (0.99, INF)}
        lanes = []
        for i in range(LANES):
            st = torch.cuda.Stream(device=dev)
            o = (torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
                 torch.empty((B, K), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
            lanes.append((st, ix.new_workspace(), o))

        def enq(band):
            def step(i):
                st, ws, o = lanes[i % LANES]
                tail = (c_void_p(o[0].data_ptr()), c_void_p(o[1].data_ptr()), c_void_p(o[2].data_ptr()),
                        c_void_p(o[3].data_ptr()), c_void_p(ws.data_ptr()), ix.workspace_bytes, c_void_p(st.cuda_stream))
                if band is None:
                    rc = lib.rf_search(ix.handle, c_void_p(q.data_ptr()), B, K, 0, *tail)
                else:
                    rc = lib.rf_search_range(ix.handle, None, c_void_p(q.data_ptr()), B, K, 0, band[0], band[1], *tail)
                if rc:
                    _lib.check(rc)
            return step

        variants = {"plain": enq(None), **{name: enq(b) for name, b in bands.items()}}
        times = {name: [] for name in variants}
        for _ in range(a.rounds):   # alternate: device drift hits every variant alike
            for name, fn in variants.items():
                times[name].append(pipelined(fn, a.steps, 2 * LANES, torch.cuda.synchronize))
        med = {name: float(np.median(t)) for name, t in times.items()}
        # what each band returns (hits per query) and whether the fused path proved it
        hits, flagged = {}, {}
        for name, b in bands.items():
            _, ids, _, flags = ix.search_raw(q, K, band=b)
            torch.cuda.synchronize()
            hits[name] = float((ids >= 0).sum(1).float().mean())
            flagged[name] = int((flags != 0).sum())
        case = {"B": B, "bands": {n_: list(b) for n_, b in bands.items()},
                "ms_step": {n_: round(t * 1e3, 4) for n_, t in med.items()},
                "ms_step_min": {n_: round(min(t) * 1e3, 4) for n_, t in times.items()},
                "ratio_to_plain": {n_: round(med[n_] / med["plain"], 3) for n_ in bands},
                "hits_per_query": hits, "flagged": flagged}
        out["cases"].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
