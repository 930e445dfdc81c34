"""Cross-encoder reranking on the MI355X: time per call of CrossEncoder.score_ids (rf_score_pairs) at the
shapes a "retrieve fetch_k, rerank, keep top_k" stage runs, beside Embedder.encode_ids (rf_encode) at the same
(B, T) -- the same layers between other first and last kernels -- and beside transformers'
BertForSequenceClassification on the host CPU (fp32, the library's defaults).

One process; every shape is warmed up, then timed with device events around `iters` back-to-back calls on
device-resident inputs (so the figure is the forward, not the upload), repeated `reps` times; the median and
the spread over the repeats are reported.  Ratios are recorded, not asserted.

    python tools/bench_rerank.py [--layers 6] [--out profiles/rerank_bench.json]
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

SHAPES = [("rerank_20x290", 20, 290), ("rerank_64x290", 64, 290), ("batch_64x128", 64, 128), ("batch_226x290", 226, 290)]


def gpu_ms(fn, iters, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rerank needs the GPU: a CPU run says nothing about these times")
    from rag_fin_amd.embedder import MINILM_L6
    from rag_fin_amd.reranker import CrossEncoder
    dev = torch.device("cuda:0")
    cfg = dict(MINILM_L6, layers=args.layers)
    ce = CrossEncoder.from_random(cfg, seed=1, device=dev)
    import transformers
    hc = transformers.BertConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"],
                                 num_attention_heads=cfg["heads"], intermediate_size=cfg["intermediate"],
                                 max_position_embeddings=cfg["max_position"], type_vocab_size=2, num_labels=1)
    cpu_model = transformers.BertForSequenceClassification(hc).eval()
    rng = np.random.default_rng(0)
    rows = []
    for name, B, T in SHAPES:
        # a reranking batch: one ~12-token query against passages that fill most of the row
        lens = rng.integers(int(0.85 * T), T + 1, B).astype(np.int32)
        lens[0] = T
        seg = np.full(B, 14, dtype=np.int32)
        ids = rng.integers(1000, cfg["vocab_size"], (B, T)).astype(np.int32)
        d_ids, d_lens, d_seg = (torch.as_tensor(a).to(dev) for a in (ids, lens, seg))
        iters = max(4, int(40_000 / (B * T)) * 4)
        score = gpu_ms(lambda: ce.score_ids(d_ids, d_lens, d_seg), iters, args.reps)
        embed = gpu_ms(lambda: ce.encoder.encode_ids(d_ids, d_lens), iters, args.reps)
        pos = np.arange(T)[None, :]
        feed = dict(input_ids=torch.as_tensor(ids.astype(np.int64)),
                    attention_mask=torch.as_tensor((pos < lens[:, None]).astype(np.int64)),
                    token_type_ids=torch.as_tensor((pos >= seg[:, None]).astype(np.int64)))
        cpu = []
        with torch.no_grad():
            cpu_model(**feed)
            for _ in range(args.cpu_reps):
                t0 = time.perf_counter()
                cpu_model(**feed)
                cpu.append((time.perf_counter() - t0) * 1e3)
        row = dict(shape=name, B=B, T=T, token_slots=B * T, tokens=int(lens.sum()), iters=iters,
                   score_pairs_ms=score[0], score_pairs_ms_min_max=score[1:], encode_ids_ms=embed[0],
                   encode_ids_ms_min_max=embed[1:], score_over_encode=score[0] / embed[0],
                   pairs_per_s=B / score[0] * 1e3, torch_cpu_ms=float(np.median(cpu)),
                   torch_cpu_over_score=float(np.median(cpu)) / score[0])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(tool="tools/bench_rerank.py", device=torch.cuda.get_device_name(0), layers=args.layers,
               torch_cpu_threads=torch.get_num_threads(),
               note="score_pairs / encode_ids: ms per call, device events around back-to-back calls on device-resident "
                    "inputs (each call allocates its workspace from the caching allocator); torch_cpu: "
                    "BertForSequenceClassification fp32 on the host, same shapes, random weights of its own",
               shapes=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
