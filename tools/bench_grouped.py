"""Grouping search against the plain search and against its host-side emulation, one process.

    python tools/bench_grouped.py [--rows 1000000] [--dim 384] [--rounds 30] [--out profiles/grouped_bench.json]

Per (B, n_codes, limit, coding) with group_size 1, interleaved A/B/C rounds after a warm-up, medians
of the per-call wall time with one stream synchronisation per call:
  plain     rf_search with k = limit (the kernel of the plain path, same process)
  grouped   rf_search_grouped
  emulated  what a host writes without the argument: one rf_search_filtered (k = group_size) per
            code over a prepared "code == g" filter, then a host merge of the per-group bests
and the per-stage HIP-event times of one grouped sweep (rf_search_grouped_profile)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "grouped_bench.json"))
    a = ap.parse_args()
    import torch
    from rag_fin_amd import _lib
    from rag_fin_amd.store import GpuIndex, mask_words, _ptr
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    ix = GpuIndex(a.dim, a.rows, dev)
    for s0 in range(0, a.rows, 1 << 18):
        m = min(1 << 18, a.rows - s0)
        ix.add(torch.nn.functional.normalize(torch.randn(m, a.dim, generator=g, device=dev), dim=1).half())
    rows = torch.arange(a.rows, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    results = []
    for B in (1, 64):
        q = torch.nn.functional.normalize(torch.randn(B, a.dim, generator=g, device=dev), dim=1).half()
        for G, limit in ((4, 4), (16, 8), (64, 10)):
            for kind in ("interleaved", "contiguous"):
                codes = (rows % G if kind == "interleaved" else torch.clamp(rows * G // a.rows, max=G - 1)).to(torch.int32)
                group = (codes.contiguous(), G, limit, 1)
                filters = []
                for c in range(G):
                    buf = torch.empty(ix.lib.rf_filter_bytes(a.rows), dtype=torch.uint8, device=dev)
                    _lib.check(ix.lib.rf_filter_from_mask(_ptr(mask_words(codes == c)), a.rows, _ptr(buf),
                                                          _lib.current_stream_ptr()))
                    filters.append(buf)

                def plain():
                    ix.search_raw(q, limit)

                def grouped():
                    return ix.search_raw(q, limit, group=group)

                def emulated():
                    per = [ix.search_raw(q, 1, want_exact=True, filt=f) for f in filters]
                    ex = torch.cat([p[2] for p in per], 1).cpu().numpy()
                    ids = torch.cat([p[1] for p in per], 1).cpu().numpy()
                    return [np.lexsort((ids[b], -ex[b]))[:limit] for b in range(B)]

                flags = int(grouped()[3].abs().sum())
                t = {"plain": [], "grouped": [], "emulated": []}
                for r in range(a.warmup + a.rounds):
                    for name, fn in (("plain", plain), ("grouped", grouped), ("emulated", emulated)):
                        ms = timed(fn)
                        if r >= a.warmup:
                            t[name].append(ms)
                stages = ix.search_grouped_profile(q, group)
                rec = {"B": B, "n_codes": G, "limit": limit, "coding": kind, "flagged_queries": flags,
                       **{f"{k}_ms": round(statistics.median(v), 4) for k, v in t.items()},
                       **{f"{k}_min_ms": round(min(v), 4) for k, v in t.items()},
                       "stages_ms": {k: round(float(v), 4) for k, v in stages.items()}}
                results.append(rec)
                print(json.dumps(rec), flush=True)
                del filters
    out = {"rows": a.rows, "dim": a.dim, "rounds": a.rounds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
