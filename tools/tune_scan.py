#!/usr/bin/env python3
"""A/B tuning of the scan pipeline in ONE process (interleaved rounds, medians):
ring depth x emit workgroups per CU x sample blocks per wave, via
rf_set_tuning.  Stage times come from rf_search_profile (HIP events).

--fold-ab: the sample fold on and off (rf_set_tuning sample_fold), interleaved; per variant the
stage times, the serial step and the pipelined step of bench.py's headline (4 batches in flight,
one stream + workspace each, wall clock), plus how many sample waves the fold rescans."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("RAGFIN_LIB", "exp")   # the experiments build: rf_set_tuning and the diagnostic hooks live there only


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rings", default="6,8,12,24")
    ap.add_argument("--wgs", default="2,3")
    ap.add_argument("--bpw", default="1,2")
    ap.add_argument("--fold-ab", action="store_true", help="A/B the sample fold instead (see the docstring)")
    ap.add_argument("--lanes", type=int, default=4, help="--fold-ab: batches in flight")
    ap.add_argument("--steps", type=int, default=400, help="--fold-ab: pipelined steps per round")
    ap.add_argument("--fold-run", type=int, choices=[0, 1], default=None,
                    help="only run --steps pipelined steps with sample_fold set to this (a workload for rocprofv3)")
    args = ap.parse_args()
    import torch
    from rag_fin_amd import _lib
    from rag_fin_amd.store import GpuIndex
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1234)
    c = torch.randn((args.rows, args.dim), generator=gen, device=dev)
    c = (c / c.norm(dim=1, keepdim=True)).half()
    q = torch.randn((args.batch, args.dim), generator=gen, device=dev)
    q = (q / q.norm(dim=1, keepdim=True)).half()
    ix = GpuIndex(args.dim, args.rows, dev)
    ix.add(c)
    lib = _lib.load_library()
    if args.fold_ab or args.fold_run is not None:
        return fold_ab(args, ix, q, lib)
    configs = list(itertools.product([int(x) for x in args.rings.split(",")], [int(x) for x in args.wgs.split(",")],
                                     [int(x) for x in args.bpw.split(",")]))
    res = {cfg: [] for cfg in configs}
    flags_bad = {cfg: 0 for cfg in configs}

    def apply(cfg):
        ring, wgs, bpw = cfg
        for k, v in (("ring24", ring), ("emit_wgs_per_cu", wgs), ("sample_bpw", bpw)):
            _lib.check(lib.rf_set_tuning(k.encode(), v))

    for cfg in configs:  # warm every variant (first launch loads code, sets LDS attributes)
        apply(cfg)
        for _ in range(3):
            ix.search_profile(q, 10)
    for rnd in range(args.rounds):
        for cfg in configs:
            apply(cfg)
            stages = [ix.search_profile(q, 10) for _ in range(args.reps)]
            res[cfg].append({k: float(np.median([s[k] for s in stages])) for k in stages[0]})
            _, _, _, f = ix.search_raw(q, 10)
            flags_bad[cfg] += int(f.abs().sum().item())
    print("ring wgs bpw | sample thr emit merge | total (us, median of round medians)")
    rows = []
    for cfg in configs:
        med = {k: float(np.median([r[k] for r in res[cfg]])) * 1e3 for k in res[cfg][0]}
        tot = sum(med.values())
        rows.append((tot, cfg, med))
    for tot, cfg, med in sorted(rows):
        print("%4d %3d %3d | %6.1f %5.1f %6.1f %5.1f | %6.1f  flags=%d" %
              (*cfg, med["sample"], med["threshold"], med["emit"], med["merge"], tot, flags_bad[cfg]))
    print(json.dumps({"best": {"ring24": rows and sorted(rows)[0][1][0]}}))


def fold_ab(args, ix, q, lib):
    import time
    from ctypes import c_void_p
    import torch
    from rag_fin_amd import _lib
    B, k = q.shape[0], 10
    lanes = []
    for _ in range(args.lanes):
        st = torch.cuda.Stream()
        o = (torch.empty((B, k), dtype=torch.float32, device=q.device), torch.empty((B, k), dtype=torch.int64, device=q.device),
             torch.empty((B, k), dtype=torch.float64, device=q.device), torch.empty((B,), dtype=torch.int32, device=q.device))
        ws = ix.new_workspace()
        lanes.append((o, (q.data_ptr(), B, k, 0, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                          ws.data_ptr(), c_void_p(st.cuda_stream)), ws, st))

    def timed(n_lanes, steps):
        for i in range(2 * n_lanes):
            ix.enqueue_search(*lanes[i % n_lanes][1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            ix.enqueue_search(*lanes[i % n_lanes][1])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    if args.fold_run is not None:
        _lib.check(lib.rf_set_tuning(b"sample_fold", args.fold_run))
        dt = timed(args.lanes, args.steps)
        print(json.dumps({"sample_fold": args.fold_run, "steps": args.steps, "pipelined_us": round(dt * 1e6, 2)}))
        return
    variants = [0, 1]
    res = {v: {"pipelined": [], "serial": [], "stages": []} for v in variants}
    outs = {}
    for v in variants:   # warm each variant; keep its outputs for the parity check
        _lib.check(lib.rf_set_tuning(b"sample_fold", v))
        timed(args.lanes, 20)
        s, i, e, f = ix.search_raw(q, k, want_exact=True)
        torch.cuda.synchronize()
        outs[v] = (s.clone(), i.clone(), e.clone(), int(f.abs().sum().item()))
    for rnd in range(args.rounds):
        for v in (variants if rnd % 2 == 0 else variants[::-1]):
            _lib.check(lib.rf_set_tuning(b"sample_fold", v))
            res[v]["pipelined"].append(timed(args.lanes, args.steps))
            res[v]["serial"].append(timed(1, args.steps // 2))
            st = [ix.search_profile(q, k) for _ in range(args.reps)]
            res[v]["stages"].append({n: float(np.median([x[n] for x in st])) for n in st[0]})
    # rescans of the fold at this shape (workspace of the last search_profile)
    _lib.check(lib.rf_set_tuning(b"sample_fold", 1))
    ix.search_profile(q, k)
    off_m = lib.rf_debug_workspace_offset(b"rmask")
    off_r = lib.rf_debug_workspace_offset(b"rcnt")
    rmask = ix.workspace[off_m:off_m + 2048 * 8].view(torch.int64).cpu().numpy()
    rcnt = int(ix.workspace[off_r:off_r + 4].view(torch.int32).cpu().item())
    same = all(torch.equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and outs[0][3] == outs[1][3] == 0
    out = {"rows": args.rows, "dim": args.dim, "batch": B, "lanes": args.lanes, "rounds": args.rounds,
           "outputs_identical_and_flags_clean": bool(same),
           "rescan": {"marked_sample_waves": int((rmask != 0).sum()), "rescanned_blocks": rcnt,
                      "marked_query_bits": int(sum(bin(int(x) & (2**64 - 1)).count("1") for x in rmask if x))}}
    for v in variants:
        pl = float(np.median(res[v]["pipelined"])) * 1e6
        se = float(np.median(res[v]["serial"])) * 1e6
        stg = {n: round(float(np.median([r[n] for r in res[v]["stages"]])) * 1e3, 2) for n in res[v]["stages"][0]}
        out["fold_%d" % v] = {"pipelined_us": round(pl, 2), "qps": round(B / pl * 1e6, 1), "serial_us": round(se, 2),
                              "stages_us": stg, "pipelined_rounds_us": [round(x * 1e6, 2) for x in res[v]["pipelined"]]}
        print("fold=%d: pipelined %.1f us (%.0f QPS)  serial %.1f us  stages %s" % (v, pl, B / pl * 1e6, se, stg))
    out["pipelined_gain"] = round(out["fold_0"]["pipelined_us"] / out["fold_1"]["pipelined_us"] - 1.0, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
