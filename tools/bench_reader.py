"""Extractive reading on the MI355X: time per call of ExtractiveReader.span_ids (rf_answer_spans) at the shapes an
answer step runs -- the top 3, 20 or 64 retrieved chunks of about 290 tokens behind one question -- beside
CrossEncoder.score_ids (rf_score_pairs) at the same (B, T): the same layers behind the same embedding launch,
closed by the classification head instead of the span kernel, so the difference is what the reader's closing
launch adds.  A third column times span_ids with n_best = 1: the kernel's logits and log-sum-exp phases with one
selection round instead of sixteen, which splits the kernel's share between its phases.  Beside them
transformers' BertForQuestionAnswering on the host CPU (fp32, the library's defaults) followed by the numpy
decode (rag_fin_amd.reader.span_reference).

One process, one GPU; every shape is warmed up, then the three calls are timed in alternation -- device events
around `iters` back-to-back calls on device-resident inputs, `reps` windows each, interleaved so that drift hits
all three alike; the median and the spread over the windows are reported.  Ratios are recorded, not asserted.

    python tools/bench_reader.py [--layers 6 12] [--out profiles/reader_bench.json]
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

SHAPES = [("answer_3x290", 3, 290), ("answer_20x290", 20, 290), ("answer_64x290", 64, 290)]
MAX_ANSWER_LEN, N_BEST = 30, 16


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, nargs="+", default=[6, 12])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reader_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_reader needs the GPU: a CPU run says nothing about these times")
    import transformers
    from rag_fin_amd.embedder import MINILM_L6, random_weights
    from rag_fin_amd.reader import ExtractiveReader, random_qa_head, span_reference
    from rag_fin_amd.reranker import CrossEncoder, random_pair_head
    dev = torch.device("cuda:0")
    rows = []
    for layers in args.layers:
        cfg = dict(MINILM_L6, layers=layers)
        w = random_weights(cfg, 1)
        rd = ExtractiveReader(w, random_qa_head(cfg["hidden"], 1), cfg, device=dev, max_answer_len=MAX_ANSWER_LEN)
        ce = CrossEncoder(w, random_pair_head(cfg["hidden"], 1), cfg, device=dev)
        hc = transformers.BertConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden"], num_hidden_layers=layers,
                                     num_attention_heads=cfg["heads"], intermediate_size=cfg["intermediate"],
                                     max_position_embeddings=cfg["max_position"], type_vocab_size=2)
        cpu_model = transformers.BertForQuestionAnswering(hc).eval()
        rng = np.random.default_rng(0)
        for name, B, T in SHAPES:
            # one ~12-token question against chunks that fill most of the row
            lens = rng.integers(int(0.85 * T), T + 1, B).astype(np.int32)
            lens[0] = T
            seg = np.full(B, 14, dtype=np.int32)
            ids = rng.integers(1000, cfg["vocab_size"], (B, T)).astype(np.int32)
            d_ids, d_lens, d_seg = (torch.as_tensor(a).to(dev) for a in (ids, lens, seg))
            iters = max(8, int(40_000 / (B * T)) * 4)
            t = gpu_ms_interleaved({
                "answer": lambda: rd.span_ids(d_ids, d_lens, d_seg, MAX_ANSWER_LEN, N_BEST),
                "score": lambda: ce.score_ids(d_ids, d_lens, d_seg),
                "answer1": lambda: rd.span_ids(d_ids, d_lens, d_seg, MAX_ANSWER_LEN, 1),
            }, iters, args.reps)
            pos = np.arange(T)[None, :]
            feed = dict(input_ids=torch.as_tensor(ids.astype(np.int64)),
                        attention_mask=torch.as_tensor((pos < lens[:, None]).astype(np.int64)),
                        token_type_ids=torch.as_tensor((pos >= seg[:, None]).astype(np.int64)))
            cpu = []
            with torch.no_grad():
                cpu_model(**feed)
                for _ in range(args.cpu_reps):
                    t0 = time.perf_counter()
                    out = cpu_model(**feed)
                    s, e = out.start_logits.numpy(), out.end_logits.numpy()
                    for b in range(B):
                        span_reference(s[b], e[b], seg[b], lens[b], MAX_ANSWER_LEN, N_BEST)
                    cpu.append((time.perf_counter() - t0) * 1e3)
            row = dict(layers=layers, shape=name, B=B, T=T, token_slots=B * T, tokens=int(lens.sum()), iters=iters,
                       answer_spans_ms=t["answer"][0], answer_spans_ms_min_max=t["answer"][1:],
                       score_pairs_ms=t["score"][0], score_pairs_ms_min_max=t["score"][1:],
                       answer_spans_n_best_1_ms=t["answer1"][0], answer_spans_n_best_1_ms_min_max=t["answer1"][1:],
                       answer_minus_score_us=(t["answer"][0] - t["score"][0]) * 1e3,
                       answer_over_score=t["answer"][0] / t["score"][0],
                       fifteen_rounds_us=(t["answer"][0] - t["answer1"][0]) * 1e3,
                       pairs_per_s=B / t["answer"][0] * 1e3, torch_cpu_ms=float(np.median(cpu)),
                       torch_cpu_over_answer=float(np.median(cpu)) / t["answer"][0])
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = dict(tool="tools/bench_reader.py", device=torch.cuda.get_device_name(0), max_answer_len=MAX_ANSWER_LEN,
               n_best=N_BEST, torch_cpu_threads=torch.get_num_threads(),
               note="answer_spans / score_pairs / answer_spans_n_best_1: ms per call, device events around back-to-back "
                    "calls on device-resident inputs, windows of the three interleaved (each call allocates its "
                    "workspace and outputs from the caching allocator); answer_minus_score_us: what the span kernel "
                    "costs beyond the classification head; fifteen_rounds_us: what the selection rounds 2..16 cost; "
                    "torch_cpu: BertForQuestionAnswering fp32 on the host + the numpy decode, same shapes, random "
                    "weights of its own",
               shapes=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
