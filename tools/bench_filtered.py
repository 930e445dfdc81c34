"""Filtered vs unfiltered search at 1 M x 384, k = 10, B in {1, 64}, in one process.

Per selectivity: the filter is built once (rf_filter_from_mask), then filtered and unfiltered
rf_search steps alternate, each timed with device events (warm-up first).  Reports ms per step,
the bytes the masked sweep streams (n_pass_blocks * 32 * dim * 2) and the rate achieved over the
filtered step time; and the time of rf_filter_eval (a one-leaf and a mixed program over the
device columns of 1 M rows).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats`.

    python tools/bench_filtered.py [--rows 1000000] [--steps 50] [--warmup 10] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import search as osearch  # noqa: E402
from rag_fin_amd import _lib, filter_expr  # noqa: E402
from rag_fin_amd.store import GpuIndex, eval_filter  # noqa: E402

KINDS = ["all", "contig8", "rr8", "contig64", "rand0.1"]


def selection(kind, n, rng):
    m = np.zeros(n, dtype=bool)
    if kind == "all":
        m[:] = True
    elif kind == "contig8":
        m[3 * n // 8:4 * n // 8] = True
    elif kind == "contig64":
        m[n // 2:n // 2 + n // 64] = True
    elif kind == "rr8":
        m[3::8] = True
    elif kind == "rand0.1":
        m[rng.random(n) < 0.001] = True
    return m


def filter_from_mask(mask, device):
    import torch
    lib = _lib.load_library()
    n = mask.size
    bits = np.zeros((n + 31) // 32 * 32, dtype=bool)
    bits[:n] = mask
    words = np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.int32)
    w = torch.from_numpy(words.copy()).to(device)
    buf = torch.empty(lib.rf_filter_bytes(n), dtype=torch.uint8, device=device)
    _lib.check(lib.rf_filter_from_mask(c_void_p(w.data_ptr()), n, c_void_p(buf.data_ptr()), _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    return buf


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="filtered / unfiltered alternations per case")
    ap.add_argument("--out", default=None, help="also write the results as one JSON file here")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d, k = a.rows, a.dim, 10
    c16 = osearch.synth_unit_rows(n, d, 1234)
    ix = GpuIndex(d, n, dev)
    ix.add(torch.from_numpy(c16).to(dev))
    del c16
    rng = np.random.default_rng(0)
    out = {"rows": n, "dim": d, "k": k, "steps": a.steps, "cases": []}
    for B in (1, 64):
        q = torch.from_numpy(osearch.synth_unit_rows(B, d, 99)).to(dev)
        bufs = (torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int64, device=dev),
                None, torch.empty((B,), dtype=torch.int32, device=dev))
        for kind in KINDS:
            filt = filter_from_mask(selection(kind, n, rng), dev)
            hdr = filt[:16].cpu().numpy().view(np.uint32)
            unf, fil = [], []
            for _ in range(a.rounds):   # alternate: drift of the device hits both sides alike
                unf.append(timed(lambda: ix.search_raw(q, k, out=bufs), a.steps, a.warmup))
                fil.append(timed(lambda: ix.search_raw(q, k, out=bufs, filt=filt), a.steps, a.warmup))
            ms_u, ms_f = float(np.median(unf)), float(np.median(fil))
            streamed = int(hdr[2]) * 32 * d * 2
            row = {"B": B, "selectivity": kind, "n_pass_rows": int(hdr[1]), "n_pass_blocks": int(hdr[2]),
                   "ms_unfiltered": round(ms_u, 4), "ms_filtered": round(ms_f, 4),
                   "ratio": round(ms_f / ms_u, 3), "bytes_streamed": streamed,
                   "gb_per_s_filtered_step": round(streamed / (ms_f * 1e-3) / 1e9, 1),
                   "ms_spread_filtered": [round(min(fil), 4), round(max(fil), 4)]}
            out["cases"].append(row)
            print(json.dumps(row), flush=True)
    # rf_filter_eval over device columns of n rows (20 bytes per row: three int32 codes + fp64)
    periods = [f"Q{i}_FY2024" for i in range(1, 5)]
    dicts = {"period": periods, "chunk_type": ["balance_sheet", "key_ratios", "segment", "pl"],
             "statement_type": ["consolidated", "standalone"]}
    cols = [torch.from_numpy(rng.integers(len(dicts[f]), size=n).astype(np.int32)).to(dev)
            for f in ("period", "chunk_type", "statement_type")]
    cols.append(torch.from_numpy(rng.normal(size=n)).to(dev))
    for expr in ['period == "Q1_FY2024"',
                 'period in ["Q1_FY2024", "Q3_FY2024"] and primary_value > 0 and statement_type != "standalone"']:
        prog = filter_expr.compile_expr(expr, dicts, {})
        ms = timed(lambda: eval_filter(dev, prog, cols, n), a.steps, a.warmup)
        row = {"rf_filter_eval": expr, "rows": n, "ms_per_call_incl_host": round(ms, 4)}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
