"""Late interaction on the MI355X, in one process:
  * ColBERT.encode_ids (rf_encode_tokens) beside Embedder.encode_ids (rf_encode) at the same (B, T): a 16-token
    query, 64 x 128 and 256 x 128;
  * candidate-mode MaxSim (the rerank path) of 64 / 256 / 1000 rows per query at B = 1 and B = 64, beside the
    cross-encoder (rf_score_pairs) scoring as many (query, chunk) pairs of 128 tokens;
  * all-rows MaxSim + rf_maxsim_topk (the search path) over 100 k rows x ~100 tokens x D = 96 at B = 1 and B = 64;
  * a torch-CPU einsum MaxSim over the same padded field as the host baseline.

Every shape is warmed up, then timed with device events around `iters` back-to-back calls on device-resident
inputs, repeated `reps` times; the median and the spread are reported.  Each MaxSim call is also reported against
its two bounds: the MFMA-issue bound -- tiles x D/16 x 32 cycles on one SIMD (v_mfma_f32_32x32x16_f16 issues
back to back at 32 cycles), spread over 256 CUs x 4 SIMDs at 2.4 GHz -- and the bytes it has to read against
8 TB/s of HBM.  Ratios are recorded, not asserted.

    python tools/bench_late_interaction.py [--layers 6] [--out profiles/late_interaction_bench.json]
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

SHAPES = [("query_1x16", 1, 16), ("ingest_64x128", 64, 128), ("ingest_256x128", 256, 128)]
SIMDS, CLOCK_HZ, HBM_BPS = 256 * 4, 2.4e9, 8e12
DIM = 96


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


def bounds(tiles_per_query_sum, dim, doc_bytes, ms):
    """tiles: 32-token document tiles times queries they meet.  -> the MFMA-issue bound and the HBM bound in ms
    and the call's time as a multiple of each."""
    mfma_ms = tiles_per_query_sum * (dim // 16) * 32 / SIMDS / CLOCK_HZ * 1e3
    hbm_ms = doc_bytes / HBM_BPS * 1e3
    return dict(mfma_issue_bound_ms=mfma_ms, fraction_of_mfma_issue_bound=mfma_ms / ms, hbm_bound_ms=hbm_ms,
                fraction_of_hbm_bound=hbm_ms / ms, field_bytes_read_once=int(doc_bytes))


def bench_encode(args, dev):
    import torch
    from rag_fin_amd.embedder import MINILM_L6
    from rag_fin_amd.late_interaction import ColBERT
    cfg = dict(MINILM_L6, layers=args.layers)
    col = ColBERT.from_random(cfg, seed=1, dim=DIM, device=dev)
    rng = np.random.default_rng(0)
    rows = []
    for name, B, T in SHAPES:
        lens = rng.integers(max(1, int(0.6 * T)), T + 1, B).astype(np.int32)
        lens[0] = T
        ids = rng.integers(1000, cfg["vocab_size"], (B, T)).astype(np.int32)
        d_ids, d_lens = torch.as_tensor(ids).to(dev), torch.as_tensor(lens).to(dev)
        iters = max(4, int(40_000 / (B * T)) * 4)
        tok = gpu_ms(lambda: col.encode_ids(d_ids, d_lens), iters, args.reps)
        emb = gpu_ms(lambda: col.encoder.encode_ids(d_ids, d_lens), iters, args.reps)
        row = dict(shape=name, B=B, T=T, tokens=int(lens.sum()), dim=DIM, iters=iters, encode_tokens_ms=tok[0],
                   encode_tokens_ms_min_max=tok[1:], encode_ids_ms=emb[0], encode_ids_ms_min_max=emb[1:],
                   tokens_over_encode=tok[0] / emb[0], head_ms_by_difference=tok[0] - emb[0])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows, cfg


def make_field(n_rows, dev, seed=3):
    import torch
    from rag_fin_amd.late_interaction import TokenField
    rng = np.random.default_rng(seed)
    counts = rng.integers(60, 141, n_rows)                   # ~100 tokens per row
    f = TokenField(DIM, dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    vec = torch.randn((int(counts.sum()), DIM), generator=g, device=dev)
    vec = torch.nn.functional.normalize(vec, dim=1).half()
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    f.vec, f.off, f.off_host = vec, torch.from_numpy(off).to(dev), off
    return f, counts


def make_queries(B, dev, seed=4):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn((B, 32, DIM), generator=g), dim=2).half().to(dev)
    return q, torch.full((B,), 32, dtype=torch.int32, device=dev)


def bench_rerank(args, dev, field, counts, cfg):
    import torch
    from rag_fin_amd.late_interaction import maxsim
    from rag_fin_amd.reranker import CrossEncoder
    ce = CrossEncoder.from_random(cfg, seed=2, device=dev)
    rng = np.random.default_rng(5)
    rows = []
    for B in (1, 64):
        q = make_queries(B, dev)
        for C in (64, 256, 1000):
            cand = rng.integers(0, field.n_rows, (B, C)).astype(np.int64)
            c_off = torch.arange(B + 1, dtype=torch.int64, device=dev) * C
            c_row = torch.from_numpy(cand.reshape(-1)).to(dev)
            iters = 50 if B * C <= 4096 else 10
            t = gpu_ms(lambda: maxsim(field, q, (c_off, c_row)), iters, args.reps)
            tiles = int(((counts[cand] + 31) // 32).sum())
            row = dict(mode="candidates", B=B, candidates=C, pairs=B * C, dim=DIM, iters=iters, maxsim_ms=t[0],
                       maxsim_ms_min_max=t[1:], pairs_per_s=B * C / t[0] * 1e3,
                       **bounds(tiles, DIM, int(counts[cand].sum()) * DIM * 2, t[0]))
            if B * C <= 4096:   # the cross-encoder at the same candidate count: (query, chunk) pairs of 128 tokens
                n = B * C
                ids = torch.from_numpy(rng.integers(1000, cfg["vocab_size"], (n, 128)).astype(np.int32)).to(dev)
                lens = torch.full((n,), 128, dtype=torch.int32, device=dev)
                seg = torch.full((n,), 18, dtype=torch.int32, device=dev)
                ct = gpu_ms(lambda: ce.score_ids(ids, lens, seg), 2, max(2, args.reps // 2))
                row.update(cross_encoder_ms=ct[0], cross_encoder_over_maxsim=ct[0] / t[0])
            else:
                row.update(cross_encoder_ms=None)   # not measured: 16 384 and 64 000 pairs of 128 tokens in one call
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_search(args, dev, field, counts):
    import torch
    from rag_fin_amd.late_interaction import maxsim
    rows = []
    tiles_row = int(((counts + 31) // 32).sum())
    pad = int(counts.max())
    n_cpu = min(args.cpu_rows, field.n_rows)               # the host baseline runs over the first rows only
    off = field.off_host
    host = torch.zeros((n_cpu, pad, DIM), dtype=torch.float32)
    hv = field.vec[:int(off[n_cpu])].float().cpu()
    valid = torch.zeros((n_cpu, pad), dtype=torch.bool)
    for r in range(n_cpu):
        host[r, :counts[r]] = hv[off[r]:off[r + 1]]
        valid[r, :counts[r]] = True
    for B in (1, 64):
        q = make_queries(B, dev)
        iters = 20 if B == 1 else 4
        t = gpu_ms(lambda: maxsim(field, q), iters, args.reps)
        both = gpu_ms(lambda: field.search(q, 10), iters, args.reps)
        row = dict(mode="all_rows", B=B, rows=field.n_rows, tokens=field.n_tok, dim=DIM, k=10, iters=iters,
                   maxsim_ms=t[0], maxsim_ms_min_max=t[1:], maxsim_plus_topk_ms=both[0],
                   maxsim_plus_topk_ms_min_max=both[1:], queries_per_s=B / both[0] * 1e3,
                   **bounds(tiles_row * B, DIM, field.n_tok * DIM * 2, t[0]))
        qh = q[0].float().cpu()[:min(B, args.cpu_queries)]

        def cpu_maxsim():
            s = torch.einsum("bid,rjd->brij", qh, host)
            s = s.masked_fill(~valid[None, :, None, :], float("-inf"))
            return s.max(dim=3).values.sum(dim=2)
        cpu = host_ms(cpu_maxsim, args.cpu_reps) / qh.shape[0] * B * (field.n_rows / n_cpu)   # scaled to the call
        got = maxsim(field, q)[:qh.shape[0], :n_cpu].cpu()
        row.update(torch_cpu_einsum_ms=cpu, torch_cpu_queries_timed=int(qh.shape[0]), torch_cpu_rows_timed=n_cpu,
                   torch_cpu_over_gpu=cpu / t[0],
                   max_abs_difference_to_torch_cpu=float((got - cpu_maxsim()).abs().max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "late_interaction_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--cpu-queries", type=int, default=1)
    ap.add_argument("--cpu-rows", type=int, default=10_000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_late_interaction needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    encode, cfg = bench_encode(args, dev)
    field, counts = make_field(args.rows, dev)
    res = dict(tool="tools/bench_late_interaction.py", device=torch.cuda.get_device_name(0), layers=args.layers,
               torch_cpu_threads=torch.get_num_threads(),
               note="ms per call, device events around back-to-back calls on device-resident inputs (each call "
                    "allocates its outputs from the caching allocator); mfma_issue_bound = 32-token tiles met by "
                    "queries x D/16 x 32 cycles over 1024 SIMDs at 2.4 GHz; hbm_bound = the vectors of the rows a "
                    "call touches, read once, over 8 TB/s; fraction_of_* = bound / measured; cross_encoder: "
                    "rf_score_pairs over as many pairs of 128 tokens, random weights; torch_cpu_einsum: fp32 einsum "
                    "+ masked max + sum over the field padded to its longest row, timed for torch_cpu_queries_timed "
                    "queries over the first torch_cpu_rows_timed rows and scaled to the call",
               encode=encode, rerank=bench_rerank(args, dev, field, counts, cfg),
               search=bench_search(args, dev, field, counts))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
