"""Diversified search (MMR) against plain search and against the client-side emulation, on one
index in one process: 1 M x 384 clustered unit rows, fetch_k = 64, k = 10, lambda = 0.5, B in {1, 64}.

Per B, the variants alternating round by round, median of the rounds; every call ends on the host
(search_host: one synchronisation), as a serving call does:
  plain     search_host(limit = fetch_k): the candidate search alone (the yardstick)
  mmr       search_host(limit = k, mmr = (fetch_k, lambda)): the candidate search + rf_mmr_select
  client    what a client does without the stage (LangChain's max_marginal_relevance_search):
            search_host(limit = fetch_k), fetch the fetch_k vectors of every query back by row
            (get_rows + download), the MMR loop in numpy float32
and, on the device alone (HIP events around bare enqueues on one stream, no download):
  dev_plain rf_search(k = fetch_k)        dev_mmr   the same + rf_mmr_select
next to the merge stage of that search as rf_search_profile reports it.
Writes one JSON (default profiles/mmr_bench.json) and prints it.

    python tools/bench_mmr.py [--rows 1000000] [--steps 30] [--rounds 5] [--out FILE.json]
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

from rag_fin_amd.store import GpuIndex  # noqa: E402

FETCH_K, K, LAM = 64, 10, 0.5


def clustered_rows(n, dim, n_centres, seed, spread, centres=None):
    rng = np.random.default_rng(seed)
    if centres is None:
        centres = rng.standard_normal((n_centres, dim)).astype(np.float32)
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    out = np.empty((n, dim), dtype=np.float16)
    for s in range(0, n, 1 << 16):
        m = min(1 << 16, n - s)
        x = centres[rng.integers(0, centres.shape[0], m)] + spread * rng.standard_normal((m, dim)).astype(np.float32) / np.sqrt(dim)
        out[s:s + m] = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)
    return out, centres


def numpy_mmr(scores, vecs, k, lam):
    """The client's loop (float32, as LangChain's): scores [F], vecs [F, dim] -> picked indices."""
    sim = vecs @ vecs.T
    picks = [int(np.argmax(scores))]
    m = sim[:, picks[0]].copy()
    while len(picks) < min(k, scores.shape[0]):
        v = lam * scores - (1.0 - lam) * m
        v[picks] = -np.inf
        j = int(np.argmax(v))
        picks.append(j)
        m = np.maximum(m, sim[:, j])
    return picks


def timed(fn, steps, warm=3):
    for _ in range(warm):
        fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d = 384
    c16, centres = clustered_rows(a.rows, d, max(2, a.rows // 50), 1234, 0.15)
    qall, _ = clustered_rows(64, d, 0, 99, 0.6, centres)
    ix = GpuIndex(d, a.rows, dev)
    for s in range(0, a.rows, 1 << 18):
        ix.add(torch.from_numpy(c16[s:s + (1 << 18)]).to(dev))
    torch.cuda.synchronize()
    out = {"rows": a.rows, "dim": d, "fetch_k": FETCH_K, "k": K, "lambda": LAM, "steps": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(dev), "cases": []}
    for B in (1, 64):
        q = torch.from_numpy(np.ascontiguousarray(qall[:B])).to(dev)

        def plain():
            return ix.search_host(q, FETCH_K)

        def mmr():
            return ix.search_host(q, K, mmr=(FETCH_K, LAM))

        def client():
            scores, rows = ix.search_host(q, FETCH_K)
            vecs = ix.get_rows(np.maximum(rows, 0).reshape(-1)).float().cpu().numpy().reshape(B, FETCH_K, d)
            return [rows[b][numpy_mmr(scores[b], vecs[b], K, LAM)] for b in range(B)]

        def device_ms(with_mmr):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for i in range(3 + a.steps):
                if i == 3:
                    e0.record()
                ix.search_raw(q, K if with_mmr else FETCH_K, want_exact=True, mmr=(FETCH_K, LAM) if with_mmr else None)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps

        variants = {"plain": plain, "mmr": mmr, "client": client}
        times = {name: [] for name in variants}
        dev_times = {"dev_plain": [], "dev_mmr": []}
        for _ in range(a.rounds):   # alternate: device drift hits every variant alike
            for name, fn in variants.items():
                times[name].append(timed(fn, a.steps) * 1e3)
            dev_times["dev_plain"].append(device_ms(False))
            dev_times["dev_mmr"].append(device_ms(True))
        med = {name: float(np.median(t)) for name, t in {**times, **dev_times}.items()}
        stages = ix.search_profile(q, FETCH_K)
        got, want = mmr()[1], plain()[1][:, :K]
        case = {"B": B, "ms_call": {n_: round(t, 4) for n_, t in med.items()},
                "ms_call_min": {n_: round(min(t), 4) for n_, t in {**times, **dev_times}.items()},
                "mmr_minus_plain_ms": round(med["mmr"] - med["plain"], 4),
                "dev_mmr_minus_dev_plain_ms": round(med["dev_mmr"] - med["dev_plain"], 4),
                "client_over_mmr": round(med["client"] / med["mmr"], 3),
                "merge_stage_ms": round(float(stages["merge"]), 4),
                "stages_ms": {n_: round(float(v), 4) for n_, v in stages.items()},
                "queries_whose_list_differs_from_plain": int((got != want).any(axis=1).sum())}
        out["cases"].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
