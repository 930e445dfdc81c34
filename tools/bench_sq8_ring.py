#!/usr/bin/env python3
"""A/B of the register-ring depth of the dim-384 int8 emit sweep, k_sq8_emit<12, R, JB>, in ONE process:
R = 12 (the whole block), 6 (what the product dispatches) and 4 -- the depths that divide the 12
fragments of a block (a ring of 8 does not).  Interleaved rounds on the experiments build
(rf_set_tuning sq8_ring12); per depth the emit stage of rf_search_sq8_profile (HIP events, one batch in
flight) as median / min / max over the rounds' medians, and the pipelined step with --lanes batches
in flight through rf_search on a shadow-first index (wall clock).  Every variant's answer is compared
with the first one's.

  python tools/bench_sq8_ring.py > profiles/flat_shadow_emit_ab.txt"""
import argparse
import os
import sys
import time
from ctypes import c_void_p

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("RAGFIN_LIB", "exp")   # rf_set_tuning lives in the experiments build only


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rings", default="12,6,4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="profiled sweeps per round and depth")
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--steps", type=int, default=400, help="pipelined steps per round and depth")
    args = ap.parse_args()
    import torch
    from oracle import search as osearch
    from rag_fin_amd import _lib
    from rag_fin_amd.store import GpuIndex
    dev = torch.device("cuda:0")
    dim, k, B = 384, 10, args.batch
    ix = GpuIndex(dim, args.rows, dev, shadow=True)
    c16 = osearch.synth_unit_rows(args.rows, dim, 1234)
    for s in range(0, args.rows, 1 << 18):
        ix.add(torch.from_numpy(c16[s:s + (1 << 18)]).to(dev))
    ix.enable_sq8()
    q = torch.from_numpy(osearch.synth_unit_rows(B, dim, 5678)).to(dev)
    lib = _lib.load_library()
    rings = [int(x) for x in args.rings.split(",")]
    lanes = [(torch.cuda.Stream(dev), ix.new_workspace(),
              (torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int64, device=dev),
               torch.empty((B, k), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)))
             for _ in range(args.lanes)]
    emit = {r: [] for r in rings}
    step = {r: [] for r in rings}
    ref = None
    torch.cuda.synchronize()
    for rnd in range(args.rounds + 1):            # round 0 warms every variant up and is dropped
        for r in rings:
            _lib.check(lib.rf_set_tuning(b"sq8_ring12", r))
            ms = [ix.search_sq8_profile(q, k)["emit"] for _ in range(args.reps)]
            out = ix.search_raw(q, k, want_exact=True)
            torch.cuda.synchronize()
            if ref is None:
                ref = [t.clone() for t in out]
            same = all(torch.equal(a, b) for a, b in zip(out, ref))
            assert same and not out[3].any(), f"ring {r}: answers differ from ring {rings[0]}'s, or flags set"
            t0 = time.perf_counter()
            for i in range(args.steps):
                st, ws, o = lanes[i % args.lanes]
                ix.enqueue_search(q.data_ptr(), B, k, 0, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                  o[3].data_ptr(), ws.data_ptr(), c_void_p(st.cuda_stream))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            if rnd:
                emit[r].append(float(np.median(ms)) * 1e3)
                step[r].append(dt * 1e6)
    _lib.check(lib.rf_set_tuning(b"sq8_ring12", 6))
    print(f"k_sq8_emit<12, R, 2> at {args.rows} x 384, B = {B}, k = {k}: {args.rounds} interleaved rounds, "
          f"{args.reps} profiled sweeps and {args.steps} pipelined steps ({args.lanes} in flight) per round and depth")
    print("ring | emit us, one in flight: median (min - max) | step us, pipelined: median (min - max)")
    for r in rings:
        e, s = emit[r], step[r]
        print(f"{r:4d} | {np.median(e):7.2f} ({min(e):.2f} - {max(e):.2f}) | {np.median(s):7.2f} ({min(s):.2f} - {max(s):.2f})")


if __name__ == "__main__":
    main()
