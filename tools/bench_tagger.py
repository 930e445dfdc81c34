"""Entity tagging on the MI355X: time per call of TokenClassifier.predict (host tokenisation, rf_tag_logits,
rf_group_entities, one download, the dicts) at the shapes tagging runs -- one 16-token query, 20 and 64 chunks of
128 tokens -- beside its device part alone (tag_ids + group on device-resident ids), the embedder's forward
(Embedder.encode_ids, rf_encode) at the same (B, T) in the same process, and rf_group_entities alone on those
logits.  Beside them the `transformers` token-classification pipeline on the host CPU (fp32, the library's
defaults, the same texts, random weights of its own).

One process, one GPU; every shape is warmed up, then the device calls are timed in alternation -- device events
around `iters` back-to-back calls, `reps` windows each, interleaved so that drift hits all alike; predict is timed
by the wall clock around a synchronised call.  The median and the spread over the windows are reported.  Ratios
are recorded, not asserted.

    python tools/bench_tagger.py [--layers 6] [--out profiles/tagger_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("query_1x16", 1, 16), ("chunks_20x128", 20, 128), ("chunks_64x128", 64, 128)]
LABELS = ["O", "B-PER", "I-PER", "B-ORG", "I-ORG", "B-LOC", "I-LOC", "B-MISC", "I-MISC"]


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
    ap.add_argument("--layers", type=int, nargs="+", default=[6])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tagger_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tagger needs the GPU: a CPU run says nothing about these times")
    import transformers
    from rag_fin_amd.embedder import MINILM_L6, random_weights
    from rag_fin_amd.tagger import TokenClassifier, random_tag_head
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    dev = torch.device("cuda:0")
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(3000)]   # one token per word
    tok = WordPieceTokenizer(vocab)
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "vocab.txt"), "w") as f:
        f.write("\n".join(vocab) + "\n")
    rows = []
    for layers in args.layers:
        cfg = dict(MINILM_L6, layers=layers, vocab_size=len(vocab))
        tc = TokenClassifier(random_weights(cfg, 1), random_tag_head(cfg["hidden"], len(LABELS), 1, head_scale=0.1),
                             LABELS, cfg, tokenizer=tok, device=dev)
        hc = transformers.BertConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden"], num_hidden_layers=layers,
                                     num_attention_heads=cfg["heads"], intermediate_size=cfg["intermediate"],
                                     max_position_embeddings=cfg["max_position"], type_vocab_size=2,
                                     num_labels=len(LABELS), id2label=dict(enumerate(LABELS)),
                                     label2id={n: i for i, n in enumerate(LABELS)})
        cpu_model = transformers.BertForTokenClassification(hc).eval()
        with torch.no_grad():
            cpu_model.classifier.weight.mul_(20.0)       # labels that vary, as a trained head's do
        pipe = transformers.TokenClassificationPipeline(model=cpu_model, tokenizer=transformers.BertTokenizerFast(
            os.path.join(tmp, "vocab.txt"), do_lower_case=True), aggregation_strategy="simple")
        rng = np.random.default_rng(0)
        for name, B, T in SHAPES:
            lens = rng.integers(int(0.85 * T), T + 1, B).astype(np.int32)
            lens[0] = T
            texts = [" ".join(f"w{k}" for k in rng.integers(0, 3000, n - 2)) for n in lens]
            ids, lens2, _ = tc._rows(texts)
            assert np.array_equal(lens, lens2) and ids.shape == (B, T)
            d_ids, d_lens = (torch.as_tensor(a).to(dev) for a in (ids, lens))
            logits = tc.tag_ids(d_ids, d_lens)
            iters = max(8, int(40_000 / (B * T)) * 4)
            t = gpu_ms_interleaved({
                "tag": lambda: tc.group(tc.tag_ids(d_ids, d_lens), d_lens, None, 0, 0),
                "embed": lambda: tc.encoder.encode_ids(d_ids, d_lens),
                "group": lambda: tc.group(logits, d_lens, None, 0, 0),
            }, iters, args.reps)
            p = wall_ms(lambda: tc.predict(texts), args.reps)
            groups = sum(len(r) for r in tc.predict(texts))
            cpu = []
            pipe(texts, batch_size=B)
            for _ in range(args.cpu_reps):
                t0 = time.perf_counter()
                pipe(texts, batch_size=B)
                cpu.append((time.perf_counter() - t0) * 1e3)
            row = dict(layers=layers, shape=name, B=B, T=T, token_slots=B * T, tokens=int(lens.sum()), iters=iters,
                       groups=groups, predict_ms=p[0], predict_ms_min_max=p[1:],
                       tag_device_ms=t["tag"][0], tag_device_ms_min_max=t["tag"][1:],
                       embed_ms=t["embed"][0], embed_ms_min_max=t["embed"][1:],
                       group_entities_ms=t["group"][0], group_entities_ms_min_max=t["group"][1:],
                       tag_over_embed=t["tag"][0] / t["embed"][0], predict_over_embed=p[0] / t["embed"][0],
                       texts_per_s=B / p[0] * 1e3, pipeline_cpu_ms=float(np.median(cpu)),
                       pipeline_cpu_over_predict=float(np.median(cpu)) / p[0])
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = dict(tool="tools/bench_tagger.py", device=torch.cuda.get_device_name(0), labels=len(LABELS),
               torch_cpu_threads=torch.get_num_threads(),
               note="predict: wall-clock ms per call of TokenClassifier.predict(texts) (tokenisation on the host, "
                    "rf_tag_logits, rf_group_entities, one download, the dicts); tag_device / embed / group_entities: "
                    "ms per call, device events around back-to-back calls on device-resident inputs, windows "
                    "interleaved (each call allocates its workspace and outputs from the caching allocator); "
                    "group_entities includes the upload of the label tables' arguments; pipeline_cpu: transformers' "
                    "TokenClassificationPipeline, fp32 on the host, the same texts, random weights of its own",
               shapes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
