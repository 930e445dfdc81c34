"""Learned sparse search on the MI355X: time per call of SparseEncoder.encode_ids + sparsify (rf_encode_terms +
rf_sparsify_terms) at a query's shape and at two ingest shapes, beside Embedder.encode_ids (rf_encode) at the
same (B, T) in the same process -- the head's cost in units of an embedder forward -- and beside transformers'
BertForMaskedLM + log1p(relu) + masked max on the host CPU (fp32, the library's defaults); then a learned-sparse
search (rf_sparse_search over transposed rows) of 100 k rows of seeded random CSR, ~120 non-zeros per row at
V = 30 522, at B = 1 and B = 64, beside scipy.sparse on the host.

One process; every shape is warmed up, then timed with device events around `iters` back-to-back calls on
device-resident inputs (so the figure is the forward, not the upload), repeated `reps` times; the median and the
spread over the repeats are reported.  Ratios are recorded, not asserted.  The head's time is the DIFFERENCE of
the two forwards (they differ in the closing launches only: k_mlm_transform + k_mlm_decode_max against
k_pool_norm), and the decoder's rate is its 2 * tokens * 384 * V operations over that difference: a lower bound
of the GEMM kernel's own rate, not a kernel time.

    python tools/bench_sparse_encode.py [--layers 6] [--out profiles/sparse_encoder_bench.json]
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

SHAPES = [("query_1x16", 1, 16, True), ("ingest_64x128", 64, 128, True), ("ingest_256x128", 256, 128, False)]
PEAK_F16_FLOPS = 2.5e15   # dense fp16 matrix peak of the MI355X


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


def host_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def bench_encode(args, dev):
    import torch
    import transformers
    from rag_fin_amd.embedder import MINILM_L6
    from rag_fin_amd.sparse_encoder import SparseEncoder
    cfg = dict(MINILM_L6, layers=args.layers)
    V = cfg["vocab_size"]
    enc = SparseEncoder.from_random(cfg, seed=1, device=dev)
    hc = transformers.BertConfig(vocab_size=V, hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"],
                                 num_attention_heads=cfg["heads"], intermediate_size=cfg["intermediate"],
                                 max_position_embeddings=cfg["max_position"], type_vocab_size=2)
    cpu_model = transformers.BertForMaskedLM(hc).eval()
    rng = np.random.default_rng(0)
    rows = []
    for name, B, T, with_cpu in SHAPES:
        lens = rng.integers(max(1, int(0.6 * T)), T + 1, B).astype(np.int32)
        lens[0] = T
        ids = rng.integers(1000, V, (B, T)).astype(np.int32)
        d_ids, d_lens = torch.as_tensor(ids).to(dev), torch.as_tensor(lens).to(dev)
        iters = max(4, int(40_000 / (B * T)) * 4)
        max_terms = enc.query_max_terms if B == 1 else enc.max_terms
        terms = gpu_ms(lambda: enc.encode_ids(d_ids, d_lens), iters, args.reps)
        both = gpu_ms(lambda: enc.sparsify(enc.encode_ids(d_ids, d_lens), max_terms), iters, args.reps)
        embed = gpu_ms(lambda: enc.encoder.encode_ids(d_ids, d_lens), iters, args.reps)
        tokens = int(lens.sum())
        head_ms = terms[0] - embed[0]
        dec_flop = 2.0 * tokens * cfg["hidden"] * V
        row = dict(shape=name, B=B, T=T, token_slots=B * T, tokens=tokens, iters=iters, max_terms=max_terms,
                   encode_terms_ms=terms[0], encode_terms_ms_min_max=terms[1:],
                   encode_terms_plus_sparsify_ms=both[0], encode_terms_plus_sparsify_ms_min_max=both[1:],
                   encode_ids_ms=embed[0], encode_ids_ms_min_max=embed[1:], terms_over_encode=terms[0] / embed[0],
                   head_ms_by_difference=head_ms, decoder_gflop=dec_flop / 1e9,
                   decoder_tflops_lower_bound=dec_flop / (head_ms * 1e-3) / 1e12 if head_ms > 0 else None,
                   decoder_share_of_peak_lower_bound=dec_flop / (head_ms * 1e-3) / PEAK_F16_FLOPS if head_ms > 0 else None,
                   rows_per_s=B / both[0] * 1e3)
        if with_cpu:
            pos = np.arange(T)[None, :]
            att = torch.as_tensor((pos < lens[:, None]).astype(np.int64))
            feed = dict(input_ids=torch.as_tensor(ids.astype(np.int64)), attention_mask=att)

            def cpu_forward():
                with torch.no_grad():
                    logits = cpu_model(**feed).logits
                    return torch.max(torch.log1p(torch.relu(logits)) * att[:, :, None], dim=1).values
            row["torch_cpu_ms"] = host_ms(cpu_forward, args.cpu_reps)
            row["torch_cpu_over_gpu"] = row["torch_cpu_ms"] / both[0]
        else:
            row["torch_cpu_ms"] = None   # not measured: the [256, 128, 30522] fp32 logits alone are 4 GB on the host
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_search(args, dev):
    from scipy.sparse import csr_array
    from rag_fin_amd.index import SparseIndex
    from rag_fin_amd.sparse_encoder import TermPostings
    N, V, per_row, q_terms, k = args.rows, 30522, 120, 40, 10
    rng = np.random.default_rng(3)
    # ~120 distinct terms per row, drawn with a skew (a few hundred terms are frequent, as in a SPLADE corpus)
    draw = lambda *shape: np.minimum((rng.pareto(1.1, shape) * 40).astype(np.int32), V - 1)   # noqa: E731
    cand = np.sort(draw(N, 2 * per_row + 20), axis=1)
    first = np.ones(cand.shape, dtype=bool)
    first[:, 1:] = cand[:, 1:] != cand[:, :-1]
    keep = first & (np.cumsum(first, axis=1) <= per_row)
    idx = cand[keep]                                    # row after row, ascending within a row
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    data = rng.uniform(0.05, 2.5, idx.size).astype(np.float32)
    docs = csr_array((data, idx, indptr), shape=(N, V))
    sp = SparseIndex(TermPostings.from_csr(docs), dev)
    docs_t = docs.T.tocsr()
    rows = []
    for B in (1, 64):
        q_idx = np.stack([np.sort(rng.choice(np.unique(draw(4000)), q_terms, replace=False)) for _ in range(B)])
        q_off = (np.arange(B + 1) * q_terms).astype(np.int32)
        q_w = rng.uniform(0.1, 2.0, B * q_terms).astype(np.float32)
        d = (q_off, q_idx.reshape(-1).astype(np.int32), q_w)   # host arrays: the upload of a query batch is part of a search
        iters = 50 if B == 1 else 8
        gpu = gpu_ms(lambda: sp.search(d[0], d[1], d[2], k, want_exact=False), iters, args.reps)
        q = csr_array((q_w, q_idx.reshape(-1), q_off.astype(np.int64)), shape=(B, V))

        def cpu_search():
            s = (q @ docs_t).toarray()
            top = np.argpartition(-s, k, axis=1)[:, :k]
            return np.take_along_axis(top, np.argsort(-np.take_along_axis(s, top, 1), axis=1), 1)
        cpu = host_ms(cpu_search, args.cpu_reps)
        got = sp.search(d[0], d[1], d[2], k, want_exact=False)[1].cpu().numpy()
        s = (q @ docs_t).toarray()
        best = np.sort(s, axis=1)[:, ::-1][:, :k]
        agree = float(np.mean(np.abs(np.take_along_axis(s, got, 1) - best) <= 1e-4 * np.abs(best)))
        row = dict(B=B, rows=N, nnz=int(idx.size), query_terms=q_terms, k=k, iters=iters, sparse_search_ms=gpu[0],
                   sparse_search_ms_min_max=gpu[1:], queries_per_s=B / gpu[0] * 1e3, scipy_cpu_ms=cpu,
                   scipy_cpu_over_gpu=cpu / gpu[0], top_k_scores_agree_with_scipy=agree)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_encoder_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_encode needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    res = dict(tool="tools/bench_sparse_encode.py", device=torch.cuda.get_device_name(0), layers=args.layers,
               torch_cpu_threads=torch.get_num_threads(),
               note="ms per call, device events around back-to-back calls on device-resident inputs (each call "
                    "allocates its outputs and workspace from the caching allocator); head_ms_by_difference = "
                    "encode_terms - encode_ids (the forwards differ in their closing launches only); the decoder "
                    "figures divide the decoder GEMM's operations by that difference: lower bounds, not kernel "
                    "times; torch_cpu: BertForMaskedLM fp32 + log1p(relu) + masked max on the host, same shapes, "
                    "random weights of its own; scipy_cpu: (queries @ rows^T).toarray() + argpartition",
               encode=bench_encode(args, dev), search=bench_search(args, dev))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
