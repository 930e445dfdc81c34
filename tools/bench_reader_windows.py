"""Sliding windows of the extractive reader on the MI355X: what reading long contexts costs, and where.

1 and 8 contexts of 2 k and 16 k tokens behind a 12-token question, max_length 384, doc_stride 128 (windows of
369 context tokens every 241), six layers, random weights.  Per shape, ms per call of
  whole       ExtractiveReader.stitch_ids: the windows' forward in its buckets + rf_stitch_spans
  forward     ExtractiveReader.window_logits: the forward of the windows alone
  stitch      ExtractiveReader.stitch_logits on logits that are there: the three launches + the upload of the window
              table, the workspace and the outputs from the caching allocator
  launches    rf_stitch_spans itself through ctypes, tables, workspace and outputs already on the device
and the route a client has without it: download the [W, T, 2] logits and run stitch_reference (numpy) per context.

One process, one GPU, device-resident ids; every shape is warmed up, then the four calls are timed in alternation
-- device events around `iters` back-to-back calls, `reps` windows each, interleaved so that drift hits all alike
(tools/bench_reader.py's scheme); the median and the spread are reported.  The client route is timed with a host
clock around download + decode.  Ratios are recorded, not asserted.

    python tools/bench_reader_windows.py [--out profiles/reader_windows_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_reader import gpu_ms_interleaved  # noqa: E402

SHAPES = [("1x2k", 1, 2048), ("8x2k", 8, 2048), ("1x16k", 1, 16384), ("8x16k", 8, 16384)]
MAX_LENGTH, DOC_STRIDE, QUESTION_TOKENS, LAYERS = 384, 128, 12, 6
MAX_ANSWER_LEN, N_BEST = 30, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reader_windows_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_reader_windows needs the GPU: a CPU run says nothing about these times")
    from rag_fin_amd import _lib
    from rag_fin_amd.embedder import MINILM_L6, random_weights
    from rag_fin_amd.reader import ExtractiveReader, plan_windows, random_qa_head, stitch_reference
    dev = torch.device("cuda:0")
    cfg = dict(MINILM_L6, layers=LAYERS)
    rd = ExtractiveReader(random_weights(cfg, 1), random_qa_head(cfg["hidden"], 1, head_scale=0.1), cfg, device=dev,
                          max_length=MAX_LENGTH, max_answer_len=MAX_ANSWER_LEN)
    lib, p = rd.lib, ctypes.c_void_p
    seg, room = QUESTION_TOKENS + 2, MAX_LENGTH - QUESTION_TOKENS - 3
    rng = np.random.default_rng(0)
    rows = []
    for name, C, L in SHAPES:
        plan = plan_windows(L, room, DOC_STRIDE)
        windows = np.array([(f, n, seg) for _ in range(C) for f, n in plan], dtype=np.int32)
        ctx_win = (np.arange(C + 1) * len(plan)).astype(np.int32)
        W = len(windows)
        lens = (windows[:, 1] + seg + 1).astype(np.int32)
        d_ids = torch.as_tensor(rng.integers(1000, cfg["vocab_size"], (W, MAX_LENGTH)).astype(np.int32)).to(dev)
        logits = rd.window_logits(d_ids, lens, windows[:, 2])
        # the raw call's arguments, resident
        win4 = np.zeros((W, 4), dtype=np.int32)
        win4[:, :3] = windows
        d_win, d_ctx = torch.as_tensor(win4).to(dev), torch.as_tensor(ctx_win).to(dev)
        out = torch.empty(C * (N_BEST + 1) * 3, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.rf_stitch_workspace_bytes(W, C, L), dtype=torch.uint8, device=dev)

        def launches():
            _lib.check(lib.rf_stitch_spans(p(logits.data_ptr()), W, MAX_LENGTH, p(d_win.data_ptr()), p(d_ctx.data_ptr()), C,
                                           MAX_ANSWER_LEN, N_BEST, p(out.data_ptr()), p(out.data_ptr() + 4 * C * N_BEST * 3),
                                           p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr()))

        iters = max(4, int(400_000 / (W * MAX_LENGTH)))
        t = gpu_ms_interleaved({
            "whole": lambda: rd.stitch_ids(d_ids, lens, windows, ctx_win, MAX_ANSWER_LEN, N_BEST),
            "forward": lambda: rd.window_logits(d_ids, lens, windows[:, 2]),
            "stitch": lambda: rd.stitch_logits(logits, windows, ctx_win, MAX_ANSWER_LEN, N_BEST),
            "launches": launches,
        }, iters, args.reps)
        # the results must not differ between the routes timed
        a = rd.stitch_logits(logits, windows, ctx_win, MAX_ANSWER_LEN, N_BEST).cpu()
        launches()
        assert np.array_equal(a.packed.numpy(), out.cpu().numpy())
        client, host_spans = [], None
        for _ in range(args.cpu_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = logits.cpu().numpy()
            host_spans = [stitch_reference(host[ctx_win[c]:ctx_win[c + 1]], windows[ctx_win[c]:ctx_win[c + 1]],
                                           MAX_ANSWER_LEN, N_BEST) for c in range(C)]
            client.append((time.perf_counter() - t0) * 1e3)
        assert all([tuple(s) for s in a.spans.numpy()[c]] == [(i, j) for i, j, _ in host_spans[c][0]] for c in range(C))
        row = dict(shape=name, contexts=C, context_tokens=L, windows=W, T=MAX_LENGTH, token_slots=W * MAX_LENGTH,
                   selection_tiles=C * ((L + 511) // 512), iters=iters,
                   whole_ms=t["whole"][0], whole_ms_min_max=t["whole"][1:],
                   forward_ms=t["forward"][0], forward_ms_min_max=t["forward"][1:],
                   stitch_ms=t["stitch"][0], stitch_ms_min_max=t["stitch"][1:],
                   stitch_launches_ms=t["launches"][0], stitch_launches_ms_min_max=t["launches"][1:],
                   client_numpy_ms=float(np.median(client)),
                   stitch_over_forward=t["stitch"][0] / t["forward"][0],
                   launches_over_forward=t["launches"][0] / t["forward"][0],
                   whole_over_forward=t["whole"][0] / t["forward"][0],
                   client_numpy_over_stitch=float(np.median(client)) / t["stitch"][0])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(tool="tools/bench_reader_windows.py", device=torch.cuda.get_device_name(0), layers=LAYERS,
               max_length=MAX_LENGTH, doc_stride=DOC_STRIDE, question_tokens=QUESTION_TOKENS,
               max_answer_len=MAX_ANSWER_LEN, n_best=N_BEST,
               note="ms per call, device events around back-to-back calls on device-resident ids, windows of the four "
                    "calls interleaved, median (min, max) over the windows.  whole = stitch_ids; forward = "
                    "window_logits (buckets of 65536 token slots, each bucket's logits copied into the one buffer); "
                    "stitch = stitch_logits (window table upload + allocations + three launches); stitch_launches = "
                    "rf_stitch_spans alone; client_numpy = download of the logits + stitch_reference per context, "
                    "host clock",
               shapes=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
