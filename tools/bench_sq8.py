"""FLAT against SQ8 on one index, interleaved in one process: 1 M x 384, k = 10, B in {1, 64, 256}.

Data sets: random unit vectors, a clustered mixture (1 024 centres), and the encoder's embeddings of
oracle/synth_text.py texts under the trained-like weights (oracle.encoder.trained_like_weights;
dominant channels show up there if the weights produce them; --text-rows of them, the encoder set
being the slow one to make).  Per data set and B:
  * QPS of rf_search and rf_search_sq8, pipelined as bench.py does (4 lanes: own stream and
    workspace each, bare enqueues), FLAT and SQ8 rounds alternating, median of the rounds;
  * per-stage times of the first 64-query sweep (HIP events: rf_search_profile /
    rf_search_sq8_profile);
  * candidates per query and |R| (the rescoring set {score >= k-th candidate - 2 eps}) of both
    paths, read from the workspace (rf_debug_workspace_offset: runs on the experiments build,
    RAGFIN_LIB=exp, set below before the library loads);
  * queries SQ8 flags and how many of those FLAT flags too (fallback to the exhaustive kernel);
  * max over rows and queries of |a~ - a| / delta_q (rf_debug_scores_sq8 against fp64 scores).

    python tools/bench_sq8.py [--rows 1000000] [--text-rows 262144] [--steps 40] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from ctypes import c_void_p

import numpy as np

os.environ.setdefault("RAGFIN_LIB", "exp")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import search as osearch  # noqa: E402
from rag_fin_amd import _lib  # noqa: E402
from rag_fin_amd.store import GpuIndex  # noqa: E402

K = 10
LANES = 4


def clustered(n, d, seed, centers=1024, spread=0.05):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32)
    out = np.empty((n, d), dtype=np.float16)
    for s in range(0, n, 1 << 17):
        m = min(1 << 17, n - s)
        x = c[rng.integers(0, centers, m)] + spread * rng.standard_normal((m, d)).astype(np.float32)
        out[s:s + m] = osearch.l2_normalize_f32(x).astype(np.float16)
    return out


def encoder_rows(n, seed, dev):
    import torch
    from oracle import encoder as oenc, synth_text
    from rag_fin_amd.embedder import Embedder
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    cfg = dict(oenc.MINILM_L6)
    tok = WordPieceTokenizer(synth_text.vocab_for(size=cfg["vocab_size"]))
    emb = Embedder(oenc.trained_like_weights(cfg, 23), cfg, tokenizer=tok, device=dev)
    texts = synth_text.retemplated_texts(n, seed)
    ids, lens = tok.batch_native(texts, 256)
    out = torch.empty((n, cfg["hidden"]), dtype=torch.float16, device=dev)
    order = np.argsort(lens, kind="stable")
    i = 0
    while i < n:
        j = i
        while j < n and (j - i + 1) * int(lens[order[j]]) <= 65536:
            j += 1
        j = max(j, i + 1)
        idx = order[i:j]
        T = int(lens[idx].max())
        out[torch.as_tensor(idx, device=dev)] = emb.encode_ids(
            torch.from_numpy(np.ascontiguousarray(ids[idx, :T])).to(dev), torch.from_numpy(lens[idx]).to(dev))
        i = j
    torch.cuda.synchronize()
    return out.cpu().numpy()


def pipelined(enqueue, steps, warm, sync):
    for i in range(warm):
        enqueue(i)
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        enqueue(i)
    sync()
    return (time.perf_counter() - t0) / steps


def workspace_stats(lib, ws, B):
    """candidates per query and |R| from the workspace the last search left (counters kept)."""
    import torch
    off_cnt = lib.rf_debug_workspace_offset(b"cand_cnt")
    off_cand = lib.rf_debug_workspace_offset(b"cand")
    off_eps = lib.rf_debug_workspace_offset(b"eps")
    cnt = ws[off_cnt:off_cnt + 64 * 8 * 4].view(torch.int32).view(64, 8).cpu().numpy()
    cand = ws[off_cand:off_cand + 64 * 8 * 2048 * 8].view(torch.float32).view(64, 8, 2048, 2).cpu().numpy()
    eps = ws[off_eps:off_eps + 64 * 4].view(torch.float32).cpu().numpy()
    ncand, nr = [], []
    for q in range(min(B, 64)):
        sc = np.concatenate([cand[q, s, :min(int(cnt[q, s]), 2048), 1] for s in range(8)])
        ncand.append(int(cnt[q].sum()))
        if sc.size >= K:
            kth = np.sort(sc)[-K]
            nr.append(int((sc >= np.float32(kth) - np.float32(2) * eps[q]).sum()))
        else:
            nr.append(int(sc.size))
    return ncand, nr


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--text-rows", type=int, default=262_144)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", default="random,clustered,encoder")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    d = 384
    out = {"k": K, "lanes": LANES, "steps": a.steps, "library": os.path.basename(_lib.library_path()), "sets": []}
    for name in a.sets.split(","):
        t0 = time.perf_counter()
        if name == "random":
            c16 = osearch.synth_unit_rows(a.rows, d, 1234)
            qall = osearch.synth_unit_rows(256, d, 99)
        elif name == "clustered":
            x = clustered(a.rows + 256, d, 7)
            c16, qall = x[:a.rows], x[a.rows:]
        else:
            x = encoder_rows(a.text_rows + 256, 11, dev)
            c16, qall = x[:a.text_rows], x[a.text_rows:]
        n = c16.shape[0]
        ix = GpuIndex(d, n, dev)
        for s in range(0, n, 1 << 18):
            ix.add(torch.from_numpy(c16[s:s + (1 << 18)]).to(dev))
        ix.enable_sq8()
        torch.cuda.synchronize()
        # the quantization view: how the row scales spread (a dominant channel shows as large e_r)
        _, sc, er = ix.get_rows_sq8(np.arange(0, n, max(1, n // 65536), dtype=np.int64))
        er = er.cpu().numpy()
        entry = {"set": name, "rows": n, "build_s": round(time.perf_counter() - t0, 1),
                 "e_r_mean": float(er.mean()), "e_r_max": float(er.max()), "cases": []}
        for B in (1, 64, 256):
            q = torch.from_numpy(np.ascontiguousarray(qall[:B])).to(dev)
            lanes = []
            for i in range(LANES):
                st = torch.cuda.Stream(device=dev)
                ws = ix.new_workspace()
                o = (torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
                     torch.empty((B, K), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
                lanes.append((st, ws, o))

            def enq(fn, wsb):
                def step(i):
                    st, ws, o = lanes[i % LANES]
                    rc = fn(ix.handle, c_void_p(q.data_ptr()), B, K, 0, c_void_p(o[0].data_ptr()), c_void_p(o[1].data_ptr()),
                            c_void_p(o[2].data_ptr()), c_void_p(o[3].data_ptr()), c_void_p(ws.data_ptr()), wsb,
                            c_void_p(st.cuda_stream))
                    if rc:
                        _lib.check(rc)
                return step

            flat = enq(lib.rf_search, ix.workspace_bytes)
            sq8 = enq(lib.rf_search_sq8, ix.sq8_workspace_bytes)
            tf, ts = [], []
            for _ in range(a.rounds):   # alternate: device drift hits both alike
                tf.append(pipelined(flat, a.steps, 2 * LANES, torch.cuda.synchronize))
                ts.append(pipelined(sq8, a.steps, 2 * LANES, torch.cuda.synchronize))
            tf, ts = float(np.median(tf)), float(np.median(ts))
            # stage times of the first sweep (median of 5)
            pf = [ix.search_profile(q, K) for _ in range(5)]
            ps = [ix.search_sq8_profile(q, K) for _ in range(5)]
            stages_f = {k_: round(float(np.median([p[k_] for p in pf])) * 1e3, 2) for k_ in pf[0]}
            stages_s = {k_: round(float(np.median([p[k_] for p in ps])) * 1e3, 2) for k_ in ps[0]}
            # candidates / |R| of the first sweep, both paths (the merge leaves its counters)
            q64 = q[:64].contiguous()
            _lib.check(lib.rf_set_tuning(b"fold_dbg", 2))
            ws = ix.new_workspace()
            ix.search_raw(q64, K, workspace=ws)
            torch.cuda.synchronize()
            cf, rf = workspace_stats(lib, ws, B)
            ws = ix.new_workspace()
            _, _, _, f8 = ix.search_raw(q64, K, workspace=ws, sq8=True)
            torch.cuda.synchronize()
            cs, rs = workspace_stats(lib, ws, B)
            _lib.check(lib.rf_set_tuning(b"fold_dbg", 0))
            # flags over the whole batch, and how many of them FLAT flags too
            _, _, _, f8 = ix.search_raw(q, K, sq8=True)
            _, _, _, f0 = ix.search_raw(q, K)
            torch.cuda.synchronize()
            f8 = f8.cpu().numpy() != 0
            f0 = f0.cpu().numpy() != 0
            # what the fallback adds: the flagged queries through FLAT rf_search (one batch, serial)
            t_fb = 0.0
            if f8.any():
                qb = q[torch.from_numpy(np.flatnonzero(f8)).to(dev)].contiguous()
                t_fb = pipelined(lambda i: ix.search_raw(qb, K), 10, 3, torch.cuda.synchronize)
            # |a~ - a| / delta_q over every row, for up to 64 queries (fp64 scores on the device)
            at, delta = ix.debug_scores_sq8(q64)
            worst = 0.0
            cd = None
            for s in range(0, n, 1 << 18):
                cd = torch.from_numpy(c16[s:s + (1 << 18)]).to(dev).double()
                ex = q64.double() @ cd.T
                r = ((at[:, s:s + cd.shape[0]].double() - ex).abs() / delta.double().clamp_min(1e-30)[:, None]).max()
                worst = max(worst, float(r))
            del at, cd
            case = {"B": B, "qps_flat": round(B / tf), "qps_sq8": round(B / ts), "speedup": round(tf / ts, 3),
                    "ms_step_flat": round(tf * 1e3, 4), "ms_step_sq8": round(ts * 1e3, 4),
                    "ms_fallback_flat_serial": round(t_fb * 1e3, 4),
                    "speedup_with_fallback": round(tf / (ts + t_fb), 3),
                    "stages_us_flat": stages_f, "stages_us_sq8": stages_s,
                    "cand_per_query_flat": float(np.mean(cf)), "cand_per_query_sq8": float(np.mean(cs)),
                    "cand_max_sq8": int(np.max(cs)), "R_mean_flat": float(np.mean(rf)), "R_mean_sq8": float(np.mean(rs)),
                    "R_max_sq8": int(np.max(rs)), "sq8_flagged": int(f8.sum()), "fallback_exhaustive": int((f8 & f0).sum()),
                    "flat_flagged": int(f0.sum()), "delta_mean": float(delta.double().mean()),
                    "max_err_over_delta": round(worst, 4)}
            entry["cases"].append(case)
            print(json.dumps({"set": name, **case}), flush=True)
        out["sets"].append(entry)
        del ix
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
