"""The sample fold of the 64-query sweep: the sample pass keeps, per lane, its
query's best row and second best score; k_threshold appends the rows of complete lists and marks
the sample waves whose lists are not; the emit sweep skips the sampled blocks except those of
marked waves.  Bar: the candidate sets the merge sees are the ones of the unfolded sweep, so ids,
ranks and scores equal the oracle's bit for bit and no flag is raised.

The knob tests run the experiments build (rf_set_tuning) in a child process of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle, search as osearch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def search_checked(ix, q16, c16, k, device):
    import torch
    scores, ids, exact, flags = ix.search_raw(torch.from_numpy(q16).to(device), k, want_exact=True)
    torch.cuda.synchronize()
    assert int(flags.abs().sum()) == 0, f"flags set: {flags.cpu().numpy()}"
    os_, oi = c_oracle.search(q16, c16, k)
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, oi), f"ids differ at {np.argwhere(ids != oi)[:5]}"
    assert np.array_equal(exact.cpu().numpy(), os_)
    assert np.array_equal(scores.cpu().numpy(), os_.astype(np.float32))


def make_index(c16, device):
    import torch
    from rag_fin_amd.store import GpuIndex
    ix = GpuIndex(c16.shape[1], c16.shape[0], device)
    ix.add(torch.from_numpy(c16).to(device))
    return ix


@pytest.mark.parametrize("n,d,b,k", [
    (8193, 384, 8, 10),      # first sample-path size: one block outside the sample
    (20011, 384, 64, 10),
    (30000, 128, 7, 64),     # max k: many incomplete lists
    (50000, 768, 64, 10),    # 8-wave kernel
    (65541, 384, 33, 10),    # ragged last block, JB = 2 with a partial second query block
    (70001, 256, 20, 5),     # ragged last block, JB = 1
])
def test_fold_parity_with_oracle(gpu_device, n, d, b, k):
    c = osearch.synth_unit_rows(n, d, 4321)
    q = osearch.synth_unit_rows(b, d, 8765)
    search_checked(make_index(c, gpu_device), q, c, k, gpu_device)


def test_fold_parity_1m_batch64(gpu_device):
    """The headline shape: all 64 queries against the on-device fp64 exhaustive kernel, 4 of them
    against the C oracle as well."""
    import torch
    c = osearch.synth_unit_rows(1_000_000, 384, 1234)
    q = osearch.synth_unit_rows(64, 384, 5678)
    ix = make_index(c, gpu_device)
    qd = torch.from_numpy(q).to(gpu_device)
    s, i, e, f = ix.search_raw(qd, 10, want_exact=True)
    s2, i2, e2 = ix.search_exhaustive(qd, 10, want_exact=True)
    torch.cuda.synchronize()
    assert int(f.abs().sum()) == 0
    assert torch.equal(i, i2) and torch.equal(e, e2) and torch.equal(s, s2)
    os_, oi = c_oracle.search(q[:4], c, 10)
    assert np.array_equal(i[:4].cpu().numpy(), oi) and np.array_equal(e[:4].cpu().numpy(), os_)


def test_duplicate_rows_in_sample_blocks(gpu_device):
    """Copies of the queries fill sampled blocks (block 0 is always sampled) and their neighbours:
    every lane there holds two equal best scores, so its list is incomplete and the wave is
    rescanned for that query; the ties rank by row id as in the oracle."""
    n, d, b, k = 60000, 384, 16, 20
    c = osearch.synth_unit_rows(n, d, 99)
    q = osearch.synth_unit_rows(b, d, 98)
    nblk = (n + 31) // 32
    n_work = max(nblk // 16, 256)
    bs = nblk // n_work
    for j in range(b):
        # rows of a sampled block of a wave of its own (blocks j * bs), and of the next block
        for base in (32 * j * bs, 32 * (j * bs + 1)):
            c[base + 3 * (j % 5): base + 3 * (j % 5) + 6] = q[j]
    search_checked(make_index(c, gpu_device), q, c, k, gpu_device)


_KNOB_CHILD = r"""
import json, sys
import numpy as np, torch
from oracle import search as osearch
from rag_fin_amd import _lib
from rag_fin_amd.store import GpuIndex
lib = _lib.load_library()
dev = torch.device("cuda:0")
out = {}
for (n, d, b, k) in json.loads(sys.argv[1]):
    c = osearch.synth_unit_rows(n, d, 1357)
    q = torch.from_numpy(osearch.synth_unit_rows(b, d, 2468)).to(dev)
    ix = GpuIndex(d, n, dev)
    ix.add(torch.from_numpy(c).to(dev))
    off_cnt = lib.rf_debug_workspace_offset(b"cand_cnt")
    off_cand = lib.rf_debug_workspace_offset(b"cand")
    off_rmask = lib.rf_debug_workspace_offset(b"rmask")
    off_rcnt = lib.rf_debug_workspace_offset(b"rcnt")
    runs = {}
    for fold, dbg in ((0, 2), (1, 2), (1, 3)):   # bit 1: the merge leaves the counters; bit 0: force rescans
        _lib.check(lib.rf_set_tuning(b"sample_fold", fold))
        _lib.check(lib.rf_set_tuning(b"fold_dbg", dbg))
        s, i, e, f = ix.search_raw(q, k, want_exact=True)
        torch.cuda.synchronize()
        ws = ix.workspace
        cnt = ws[off_cnt:off_cnt + 64 * 8 * 4].view(torch.int32).view(64, 8).cpu().numpy()
        cand = ws[off_cand:off_cand + 64 * 8 * 2048 * 8].view(torch.int32).view(64, 8, 2048, 2).cpu().numpy()
        sets = []
        for qi in range(b):
            ent = np.concatenate([cand[qi, sh, :cnt[qi, sh]] for sh in range(8)])
            sets.append(sorted(map(tuple, ent.tolist())))
        rmask = ws[off_rmask:off_rmask + 2048 * 8].view(torch.int64).cpu().numpy()
        rcnt = int(ws[off_rcnt:off_rcnt + 4].view(torch.int32).cpu().item())
        runs["%d_%d" % (fold, dbg)] = dict(
            ids=i.cpu().numpy().tolist(), exact=e.cpu().numpy().tolist(), scores=s.cpu().numpy().tolist(),
            flags=f.cpu().numpy().tolist(), counts=[len(x) for x in sets], sets=sets,
            marked_waves=int((rmask != 0).sum()) if fold else 0, rescan_blocks=rcnt if fold else 0)
    _lib.check(lib.rf_set_tuning(b"sample_fold", 1))
    _lib.check(lib.rf_set_tuning(b"fold_dbg", 0))
    out["%d_%d_%d_%d" % (n, d, b, k)] = runs
print("RESULT " + json.dumps(out))
"""


def test_fold_knob_keeps_candidates_and_results(gpu_device):
    """Experiments build, one child process: with the fold off, on, and on with every list forced
    incomplete, each query's candidate set (rows and MFMA score bits, read from the workspace) and
    every output are identical."""
    shapes = [(20011, 384, 64, 10), (30000, 128, 7, 64), (50000, 768, 40, 10), (200_000, 384, 64, 10)]
    env = dict(os.environ, RAGFIN_LIB="exp")
    r = subprocess.run([sys.executable, "-c", _KNOB_CHILD, json.dumps(shapes)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    for shape, runs in res.items():
        base = runs["0_2"]
        assert not any(base["flags"]), shape
        assert min(base["counts"]) > 0, shape
        for name in ("1_2", "1_3"):
            run = runs[name]
            for key in ("ids", "exact", "scores", "flags", "counts", "sets"):
                assert run[key] == base[key], (shape, name, key)
        # forced: every sampled block is swept again
        assert runs["1_3"]["rescan_blocks"] > 0, shape
        print(shape, "marked sample waves", runs["1_2"]["marked_waves"], "rescanned blocks", runs["1_2"]["rescan_blocks"])
