"""Paged search against plain search on one index, interleaved in one process: 1 M x 384 random unit
rows, B in {1, 64}.

Per B, the variants alternating round by round, median of the rounds:
  plain         (a) one rf_search step, k = 64 (the yardstick: the first page of any paged search)
  after_D       (b) one rf_search_after page of 64 hits behind depth D = 64, 1 000 and 10 000 (the
                bound of every query is its own hit of rank D)
  large_1000    (c) GpuIndex.search_large at k = 1 000: the fused first page + 15 search-after pages
  old_1000      (d) the same k = 1 000 by the route before rf_search_after existed: the fused first
                page, then _exhaustive(after=...) page by page, walked here in the tool
  offset_960    (e) CorpusStore.search(offset=960, limit=40), hit lists and all
(a) and (b) are pipelined as bench.py does (4 lanes: own stream and workspace each, bare enqueues);
(c), (d) and (e) are whole calls with their host synchronisations, one after the other.  The stage
times of the first sweep (HIP events; rf_search_profile / rf_search_after_profile) are recorded per
depth as well.  Writes one JSON (default profiles/paging_bench.json) and prints it.

    python tools/bench_paging.py [--rows 1000000] [--steps 40] [--rounds 5] [--out FILE.json]
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
from rag_fin_amd.store import CorpusStore  # noqa: E402

K = 64
LANES = 4
DEPTHS = (64, 1_000, 10_000)
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


def whole_calls(call, reps, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    sync()
    return (time.perf_counter() - t0) / reps


def old_route(ix, q, k):
    """search_large as it was before rf_search_after: every page after the first through the exhaustive kernel."""
    import torch
    page = _lib.RF_MAX_K
    s0, i0, e0 = ix.search(q, page, 0, want_exact=True)
    ids, exacts = [i0], [e0]
    last_s, last_i = e0[:, -1].contiguous(), i0[:, -1].contiguous()
    got = page
    while got < k and bool((last_i >= 0).any()):
        bs = torch.where(last_i >= 0, last_s, torch.full_like(last_s, -INF))
        bi = torch.where(last_i >= 0, last_i, torch.full_like(last_i, 2 ** 62))
        with ix._lock:
            _, i, e = ix._exhaustive(q, page, 0, True, None, after=(bs, bi))
        ids.append(i)
        exacts.append(e)
        last_s, last_i = e[:, -1].contiguous(), i[:, -1].contiguous()
        got += page
    return torch.cat(ids, 1)[:, :k], torch.cat(exacts, 1)[:, :k]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paging_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    d = 384
    c16 = osearch.synth_unit_rows(a.rows, d, 1234)
    qall = osearch.synth_unit_rows(64, d, 99)
    st = CorpusStore("paging", dim=d, capacity=a.rows, device=dev, metric_type="IP")
    for s in range(0, a.rows, 1 << 18):
        e = min(a.rows, s + (1 << 18))
        n = e - s
        st.add(list(range(s, e)), [""] * n, torch.from_numpy(c16[s:e]).to(dev), ["Q1"] * n, ["t"] * n, ["s"] * n, [0.0] * n)
    ix = st.index
    torch.cuda.synchronize()
    depths = tuple(D for D in DEPTHS if D + K <= a.rows)
    out = {"rows": a.rows, "dim": d, "page": K, "lanes": LANES, "steps": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(dev), "cases": []}
    for B in (1, 64):
        q = torch.from_numpy(np.ascontiguousarray(qall[:B])).to(dev)
        # the bounds: every query's own hit of rank D, from one long walk
        ids_all, exact_all = ix.search_large(q, max(depths) + K, want_exact=True)[1:]
        bounds = {D: (exact_all[:, D - 1].contiguous(), ids_all[:, D - 1].contiguous()) for D in depths}
        lanes = []
        for i in range(LANES):
            stream = torch.cuda.Stream(device=dev)
            o = (torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
                 torch.empty((B, K), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
            lanes.append((stream, ix.new_workspace(), o))

        def enq(bound):
            def step(i):
                stream, ws, o = lanes[i % LANES]
                tail = (c_void_p(o[0].data_ptr()), c_void_p(o[1].data_ptr()), c_void_p(o[2].data_ptr()),
                        c_void_p(o[3].data_ptr()), c_void_p(ws.data_ptr()), ix.workspace_bytes, c_void_p(stream.cuda_stream))
                if bound is None:
                    rc = lib.rf_search(ix.handle, c_void_p(q.data_ptr()), B, K, 0, *tail)
                else:
                    rc = lib.rf_search_after(ix.handle, None, c_void_p(q.data_ptr()), B, K, 0, -INF, INF,
                                             c_void_p(bound[0].data_ptr()), c_void_p(bound[1].data_ptr()), *tail)
                if rc:
                    _lib.check(rc)
            return step

        sync = torch.cuda.synchronize
        param = {"metric_type": "IP"}
        # the old route reads the corpus once per query and page in fp64: time one call first and
        # size its repetitions by it
        t_old = whole_calls(lambda: old_route(ix, q, 1000), 1, sync)
        reps_old = max(1, min(a.steps // 8, int(2.0 / max(t_old, 1e-3))))
        variants = {"plain": lambda: pipelined(enq(None), a.steps, 2 * LANES, sync)}
        for D in depths:
            variants[f"after_{D}"] = (lambda b: lambda: pipelined(enq(b), a.steps, 2 * LANES, sync))(bounds[D])
        variants["large_1000"] = lambda: whole_calls(lambda: ix.search_large(q, 1000), max(1, a.steps // 4), sync)
        variants["old_1000"] = lambda: whole_calls(lambda: old_route(ix, q, 1000), reps_old, sync)
        variants["offset_960"] = lambda: whole_calls(lambda: st.search(q, "embedding", param, limit=40, offset=960),
                                                     max(1, a.steps // 4), sync)
        for fn in variants.values():   # warm every path once (lazy allocations, pinned buffers)
            fn()
        times = {name: [] for name in variants}
        for _ in range(a.rounds):   # alternate: device drift hits every variant alike
            for name, fn in variants.items():
                times[name].append(fn())
        med = {name: float(np.median(t)) for name, t in times.items()}
        # the two k = 1 000 routes agree, and what the pages return
        ids_new, exact_new = ix.search_large(q, 1000, want_exact=True)[1:]
        ids_old, exact_old = old_route(ix, q, 1000)
        same = bool(torch.equal(ids_new, ids_old) and torch.equal(exact_new, exact_old))
        flagged, stages = {}, {"plain": {k_: round(v, 4) for k_, v in ix.search_profile(q, K).items()}}
        for D in depths:
            _, ids, _, flags = ix.search_after_raw(q, K, bounds[D])
            sync()
            if not bool(flags.any()):   # a page the sweep proved is the walk's
                assert torch.equal(ids, ids_all[:, D:D + K]), f"page behind depth {D} differs from the walk"
            flagged[f"after_{D}"] = int((flags != 0).sum())
            stages[f"after_{D}"] = {k_: round(v, 4) for k_, v in ix.search_after_profile(q, K, bounds[D]).items()}
        case = {"B": B, "ms": {n_: round(t * 1e3, 4) for n_, t in med.items()},
                "ms_min": {n_: round(min(t) * 1e3, 4) for n_, t in times.items()},
                "page_to_plain": {f"after_{D}": round(med[f"after_{D}"] / med["plain"], 3) for D in depths},
                "old_to_new_1000": round(med["old_1000"] / med["large_1000"], 2),
                "old_1000_reps": reps_old, "routes_agree": same, "flagged": flagged, "stage_ms_first_sweep": stages}
        out["cases"].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
