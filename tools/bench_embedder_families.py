"""Sentence-embedder families on the MI355X: time per call of rf_encode_sentences for every pooling mode (through
Embedder.encode_ids on device-resident ids) beside rf_encode at the same (B, T) in the same process -- one 16-token
query, 64 and 256 chunks of 128 tokens -- and, for the query, the whole Embedder.encode_query call of a CLS model
with a query prompt (host tokenisation, upload, forward, download) beside today's Embedder.encode.

rf_encode replays a cached hipGraph at query size; rf_encode_sentences always launches its kernels one by one, so
the 1 x 16 ratio is the price of a model family other than all-MiniLM's for a single query.

One process, one GPU; every shape is warmed up, then the device calls are timed in alternation -- device events
around `iters` back-to-back calls, `reps` windows each, interleaved so that drift hits all alike; the whole calls
are timed by the wall clock around a synchronised call.  The median and the spread over the windows are reported.
Ratios are recorded, not asserted.

    python tools/bench_embedder_families.py [--layers 6] [--out profiles/embedder_families_bench.json]
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

SHAPES = [("query_1x16", 1, 16), ("chunks_64x128", 64, 128), ("chunks_256x128", 256, 128)]
MODES = ("mean", "cls", "max", "mean_sqrt_len")


def gpu_ms_interleaved(fns: dict, iters: int, reps: int) -> dict:
    """name -> (median, min, max) ms per call; the windows of the callables alternate."""
    import torch
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / iters)
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in out.items()}


def wall_ms(fn, reps: int):
    import torch
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embedder_families_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_embedder_families needs the GPU: a CPU run says nothing about these times")
    from rag_fin_amd.embedder import MINILM_L6, Embedder, random_weights
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    dev = torch.device("cuda:0")
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "query", ":"] + [f"w{i}" for i in range(3000)]   # one token per word
    tok = WordPieceTokenizer(vocab)
    cfg = dict(MINILM_L6, layers=args.layers, vocab_size=len(vocab))
    w = random_weights(cfg, 1)
    plain = Embedder(w, cfg, tokenizer=tok, device=dev)
    fam = {m: Embedder(w, cfg, tokenizer=tok, device=dev, pooling=m, normalize=True) for m in MODES}
    fam["cls"]._set_ends("cls", True, {"query": "query: "})
    rng = np.random.default_rng(0)
    rows = []
    for name, B, T in SHAPES:
        lens = rng.integers(int(0.85 * T), T + 1, B).astype(np.int32)
        lens[0] = T
        ids = rng.integers(7, len(vocab), (B, T)).astype(np.int32)
        d_ids, d_lens = (torch.as_tensor(a).to(dev) for a in (ids, lens))
        d_skip = torch.zeros(B, dtype=torch.int32, device=dev)
        fns = {"rf_encode": lambda: plain.encode_ids(d_ids, d_lens)}
        for m in MODES:   # (mean + normalise reaches rf_encode_sentences through a skip of zeros)
            fns[m] = (lambda e, kw: lambda: e.encode_ids(d_ids, d_lens, **kw))(fam[m], {"skip": d_skip} if m == "mean" else {})
        iters = max(8, int(40_000 / (B * T)) * 4)
        t = gpu_ms_interleaved(fns, iters, args.reps)
        row = dict(layers=args.layers, shape=name, B=B, T=T, token_slots=B * T, tokens=int(lens.sum()), iters=iters,
                   rf_encode_ms=t["rf_encode"][0], rf_encode_ms_min_max=t["rf_encode"][1:])
        for m in MODES:
            row[f"sentences_{m}_ms"] = t[m][0]
            row[f"sentences_{m}_ms_min_max"] = t[m][1:]
            row[f"sentences_{m}_over_rf_encode"] = t[m][0] / t["rf_encode"][0]
        if B == 1:
            text = " ".join(f"w{k}" for k in rng.integers(0, 3000, T - 4))      # [CLS] query : ... [SEP] = 16 tokens
            assert len(tok.encode("query: " + text, 256)) == T
            today = " ".join(f"w{k}" for k in rng.integers(0, 3000, T - 2))
            q = wall_ms(lambda: fam["cls"].encode_query([text]), 5 * args.reps)
            e = wall_ms(lambda: plain.encode([today]), 5 * args.reps)
            row.update(encode_query_cls_ms=q[0], encode_query_cls_ms_min_max=q[1:], encode_ms=e[0],
                       encode_ms_min_max=e[1:], encode_query_over_encode=q[0] / e[0])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(tool="tools/bench_embedder_families.py", device=torch.cuda.get_device_name(0),
               note="rf_encode / sentences_<mode>: ms per call of Embedder.encode_ids on device-resident ids (fp16 "
                    "output), device events around back-to-back calls, windows interleaved; at query size both go "
                    "through the embedder's fixed staging buffers and rf_encode replays its cached hipGraph while "
                    "rf_encode_sentences launches kernel by kernel; encode_query_cls / encode: wall-clock ms of the "
                    "whole call on one 16-token query (tokenisation on the host, upload, forward, download), a CLS "
                    "model with the prompt 'query: ' beside the mean-pooled embedder of before",
               shapes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
